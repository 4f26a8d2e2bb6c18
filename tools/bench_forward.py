"""Forward-pass benchmark (cluster routes on the device).

Table: C4's generator at a reduced shape (--filters 4M, --topics 2M), C4's
subscriber rows, and a route-node table of --nodes remote nodes: every filter
has its local route and a route to each remote node with probability --p.
One batch is matched once on the device (EGM_MODE_ROUTES); then the compact
fan-out and the forward pass run --steps times each over that match result,
timed with HIP events through egm_set_timing (egm_get_timing /
egm_get_forward_timing), means after --warmup launches.

    python tools/bench_forward.py [--filters 4000000] [--topics 2000000] [--nodes 8] [--p 0.1]
One JSON line on stdout, also written to --out (profiles/forward.json).

--fanout-only times the compact fan-out alone: for a library without the
forward pass (EGM_LIB=<an older build>), to compare the fan-out of two builds
in one session.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=4_000_000)
    ap.add_argument("--topics", type=int, default=2_000_000)
    ap.add_argument("--nodes", type=int, default=8)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fanout-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward.json"))
    a = ap.parse_args()
    import torch
    from emqx_amd import _lib as L
    from emqx_amd import synth
    from emqx_amd.engine import GpuMatcher

    seed = synth.SEED_BASE + synth.CONFIG_INDEX["c4"]
    t0 = time.time()
    f, t = synth.config("c4", n_filters=a.filters, n_topics=a.topics)
    gm = GpuMatcher(0)
    gm.build(f.blob, f.off)
    srow, ssubs = synth.subscribers(f.n, lam=1.0, p_big=0.001, n_big=2000, p_share=0.1, groups=64, seed=seed)
    gm.subs_build(srow, ssubs)
    rng = np.random.default_rng(seed)
    masks = np.ones(f.n, dtype=np.uint64)                      # node 0: the local route
    for k in range(1, a.nodes + 1):
        masks |= (rng.random(f.n) < a.p).astype(np.uint64) << np.uint64(k)
    if not a.fanout_only:
        gm.routes_build(masks, 0)
    print(f"tables built in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)

    dev = torch.device("cuda:0")
    n, nbytes = t.n, int(t.off[-1])
    s = torch.cuda.current_stream().cuda_stream
    d_blob = torch.from_numpy(t.blob).to(dev)
    d_off = torch.from_numpy(t.off.view(np.int32)).to(dev)
    d_row = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    cap = max(4 * n, 1 << 20)
    for _ in range(3):
        d_ids = torch.zeros(cap, dtype=torch.int32, device=dev)
        gm.match_device(d_blob.data_ptr(), nbytes, d_off.data_ptr(), n, L.EGM_MODE_ROUTES, s, d_row.data_ptr(),
                        d_ids.data_ptr(), cap)
        torch.cuda.synchronize()
        st = gm.last_stats()
        if not st["overflow"]:
            break
        cap = int(st["n_ids"] * 1.25) + 1024
    entries = int(d_row[n].item())
    assert not st["overflow"] and not st["errors"], st

    d_drow = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_pos = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
    d_sub = torch.zeros(1024, dtype=torch.int32, device=dev)

    def fan(fcap):
        gm.fanout_device_compact(d_row.data_ptr(), d_ids.data_ptr(), cap, n, s, d_drow.data_ptr(), d_pos.data_ptr(),
                                 d_sub.data_ptr(), fcap)
        torch.cuda.synchronize()

    fan(1024)   # sizes the delivery buffer
    deliveries = gm.last_fanout()["deliveries"]
    fcap = deliveries + 1024
    d_sub = torch.zeros(fcap, dtype=torch.int32, device=dev)
    out = {"bench": "forward", "filters": f.n, "topics": n, "nodes": a.nodes, "p": a.p, "match_entries": entries,
           "deliveries": deliveries, "steps": a.steps, "lib": os.path.basename(L.LIB_PATH)}

    if not a.fanout_only:
        d_nrow = torch.zeros(L.EGM_ROUTE_MAX_NODES + 1, dtype=torch.int64, device=dev)
        d_ef = torch.zeros(entries + 1, dtype=torch.int32, device=dev)
        d_tf = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        d_ft = torch.zeros(1024, dtype=torch.int32, device=dev)
        d_ff = torch.zeros(1024, dtype=torch.int32, device=dev)

        def fwd(wcap):
            gm.forward_device(d_row.data_ptr(), d_ids.data_ptr(), cap, n, s, d_nrow.data_ptr(), d_ft.data_ptr(),
                              d_ff.data_ptr(), wcap, d_ef.data_ptr(), d_tf.data_ptr())
            torch.cuda.synchronize()

        fwd(1024)   # sizes the lists
        forwards = gm.last_forward()["forwards"]
        wcap = forwards + 1024
        d_ft = torch.zeros(wcap, dtype=torch.int32, device=dev)
        d_ff = torch.zeros(wcap, dtype=torch.int32, device=dev)
        for _ in range(a.warmup):
            fwd(wcap)
        assert gm.last_forward() == {"forwards": forwards, "overflow": 0}
        assert int(d_tf[:n].sum().item()) == forwards == int(d_nrow[-1].item())
        gm.set_timing(True)
        b = gm.forward_timing()
        for _ in range(a.steps):
            fwd(wcap)
        e = gm.forward_timing()
        gm.set_timing(False)
        ms = (e["forward_ms"] - b["forward_ms"]) / max(1, e["forward_launches"] - b["forward_launches"])
        n_tiles = (n + 63) // 64
        model = 2 * 12 * entries + 8 * forwards + 4 * (a.nodes + 1) * n_tiles
        out.update({"forwards": forwards, "forward_ms": round(ms, 4), "forward_model_bytes": model,
                    "forward_model_gbps": round(model / ms / 1e6, 1)})

    for _ in range(a.warmup):
        fan(fcap)
    assert gm.last_fanout() == {"deliveries": deliveries, "overflow": 0}
    gm.set_timing(True)
    b = gm.get_timing()
    for _ in range(a.steps):
        fan(fcap)
    e = gm.get_timing()
    out["fanout_compact_ms"] = round((e["fanout_ms"] - b["fanout_ms"]) /
                                     max(1, e["fanout_launches"] - b["fanout_launches"]), 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    gm.close()


if __name__ == "__main__":
    main()
