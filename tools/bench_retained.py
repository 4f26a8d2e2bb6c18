"""Retained reverse-match benchmark.

Store: M retained topics (the C2 topic generator, wildcard-free); queries: a
batch of N subscription filters (the C2 filter generator, all wildcard:
'+' p=.15, last-level '#' p=.5).  A step = egm_rstore_match on the whole batch
through the host API (filters uploaded, rows of message ids returned), i.e.
emqx_retainer_mnesia:match_messages/1 for N subscriptions at once.

CPU baseline: oracle/retainer_scan.cpp — the reference's dirty_select, a scan
of every record per filter — on `--cpu-threads` threads over a bounded sample
of the filters; its counts are checked against the GPU rows.

    python tools/bench_retained.py [--topics 1000000] [--filters 100000]
One JSON line on stdout.

--churn K measures the live store instead, in one process on
the same store: the time of egm_rstore_rebuild; then, with the overlay holding
0, 256, 1024, 4096 and 16384 topics, the match of the filter batch, the commit
of K puts (half on topics of the image, half new) and the match after it; and
the same K puts committed with the overlay cap at 0, where a commit is a
rebuild.  One JSON line on stdout (bench "retained_live").

--delete F measures delete_message/2 with a wildcard filter on
two stores of the same topics in one process: F filters (generated C2
filters and first-word prefixes `w/#`, picked by their match counts to span
small and large deletes) are deleted one by one, on one store by
egm_rstore_delete_matching and on the other by the sequence the mirror used
before that call existed -- egm_rstore_match at now = 0, one egm_rstore_delete
per matched topic, egm_rstore_commit -- alternating which goes first.  Both
must drop the same ids.  One JSON line on stdout (bench "retained_delete"),
also written to profiles/retained_delete.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--topics", type=int, default=1_000_000)
    ap.add_argument("--filters", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--churn", type=int, default=0, metavar="K",
                    help="measure rebuild, incremental commit of K changes and match against the overlay")
    ap.add_argument("--delete", type=int, default=0, metavar="F",
                    help="time F wildcard deletes: the device call against match + per-topic delete + commit")
    a = ap.parse_args()
    from emqx_amd import _lib as L
    from emqx_amd import synth
    from emqx_amd.engine import pack_strings
    from emqx_amd.retainer import RetainedStore
    from oracle.cpp import OracleRetained

    c = synth.CONFIGS["c2"]
    seed = synth.SEED_BASE + synth.CONFIG_INDEX["c2"]
    t0 = time.time()
    flt = synth.filters(a.filters, c["dmin"], c["dmax"], c["wc"], c["p_plus"], c["p_hash"], seed=seed)
    tp = synth.topics(int(a.topics * 1.05), flt, c["dmin"], c["dmax"], seed=seed + 17)
    topics = [x for x in dict.fromkeys(tp.to_list()) if b"+" not in x.split(b"/") and b"#" not in x.split(b"/")]
    topics = topics[: a.topics]
    print(f"generated {len(topics)} topics, {flt.n} filters in {time.time() - t0:.1f}s", file=sys.stderr,
          flush=True)

    if a.delete:
        delete_bench(a, topics, flt)
        return

    rs = RetainedStore(0)
    lib, h = rs.lib, rs.h
    t0 = time.time()
    for i, t in enumerate(topics):
        lib.egm_rstore_put(h, t, len(t), i, 0)
    rs.commit()
    build_s = time.time() - t0
    print(f"store built in {build_s:.1f}s", file=sys.stderr, flush=True)

    import ctypes as C
    fb, fo = flt.blob, flt.off
    n = flt.n

    def step():
        res = C.POINTER(L.egm_result)()
        rc = lib.egm_rstore_match(h, C.c_void_p(fb.ctypes.data), C.c_void_p(fo.ctypes.data), n, 0,
                                  L.EGM_RMODE_MATCH, C.byref(res))
        assert rc == 0, rc
        r = res.contents
        tot = int(r.n_ids)
        counts = np.ctypeslib.as_array(r.counts, shape=(n,)).copy()
        lib.egm_result_free(res)
        return tot, counts

    if a.churn:
        churn(a, rs, step, topics, flt, build_s)
        rs.close()
        return

    step()
    ts = []
    for _ in range(a.steps):
        t1 = time.perf_counter()
        tot, counts = step()
        ts.append(time.perf_counter() - t1)
    ms = 1e3 * float(np.median(ts))

    # CPU: full-table scan per filter over a bounded sample
    o = OracleRetained()
    tb, to = pack_strings(topics)
    o.put(tb, to, np.arange(len(topics), dtype=np.uint32), np.zeros(len(topics), dtype=np.uint64))
    k = 16
    while True:
        sb, so = pack_strings([flt[i] for i in range(k)])
        t1 = time.perf_counter()
        ctot, ccounts = o.match_counts(sb, so, 0, 0, threads=a.cpu_threads)
        dt = time.perf_counter() - t1
        if dt > a.cpu_seconds / 4 or k >= n:
            break
        k = min(n, k * 4)
    assert np.array_equal(ccounts, counts[:k]), "CPU scan and GPU rows disagree"
    out = {
        "bench": "retained_match", "metric": "subscription filters matched/sec against the retained store",
        "value": n / (ms / 1e3), "unit": "filters/s", "ms_per_batch": ms, "ids_per_s": tot / (ms / 1e3),
        "config": {"workload": "c2-shaped", "stored_topics": len(topics), "filters_per_batch": n,
                   "matched_ids_per_batch": tot, "path": "host API: H2D filters, match, D2H rows"},
        "cpu_baseline": {"value": k / dt, "unit": "filters/s", "cores": a.cpu_threads, "kind": "port",
                         "sample": f"{k} filters, full-table scan each (oracle/retainer_scan.cpp)"},
        "store_build_s": build_s,
    }
    print(json.dumps(out))
    rs.close()


OVERLAY_SIZES = (0, 256, 1024, 4096, 16384)


def churn(a, rs, step, topics, flt, build_s):
    """The live store: rebuild, incremental commits and overlay matches (--churn)."""
    from emqx_amd import synth

    lib, h = rs.lib, rs.h
    K = a.churn
    c = synth.CONFIGS["c2"]
    seed = synth.SEED_BASE + synth.CONFIG_INDEX["c2"]
    have = set(topics)
    need = max(OVERLAY_SIZES) + 8 * K
    extra = synth.topics(2 * need + 1000, flt, c["dmin"], c["dmax"], seed=seed + 18)   # shaped like the stored ones
    pool = [x for x in dict.fromkeys(extra.to_list())
            if x not in have and b"+" not in x.split(b"/") and b"#" not in x.split(b"/")]
    assert len(pool) >= need, (len(pool), need)
    next_id = [len(topics)]
    rng = np.random.default_rng(5)

    def put(t):
        assert lib.egm_rstore_put(h, t, len(t), next_id[0], 0) == 0
        next_id[0] += 1

    def timed(fn, reps=1):
        ts = []
        for _ in range(reps):
            t1 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t1)
        return 1e3 * float(np.median(ts)), r

    def changes():
        """K puts: half on topics of the image, half new; returns the new ones."""
        new = [pool.pop() for _ in range(K - K // 2)]
        for i in rng.choice(len(topics), K // 2, replace=False):
            put(topics[int(i)])
        for t in new:
            put(t)
        return new

    step()                                    # warm: code objects, workspace
    rebuild_ms, _ = timed(rs.rebuild, 2)
    rows = []
    rs.set_overlay_cap(1 << 20)               # the sizes below are set by hand
    overlay = []
    for size in OVERLAY_SIZES:
        while len(overlay) < size:
            overlay.append(pool.pop())
            put(overlay[-1])
        rs.commit()
        st = rs.last_commit() if size else {"rebuilt": 0, "overlay_topics": 0}
        assert st["rebuilt"] == 0 and st["overlay_topics"] == size, st
        step()
        match_ms, (tot, _) = timed(step, a.steps)
        new = changes()
        commit_ms, _ = timed(rs.commit)
        st = rs.last_commit()
        assert st["rebuilt"] == 0 and st["patched"] == K // 2 and st["overlay_topics"] == size + len(new), st
        after_ms, (tot2, _) = timed(step)
        assert tot2 >= tot, (tot, tot2)       # topics were added, none removed
        for t in new:                         # back to `size` overlay topics
            assert lib.egm_rstore_delete(h, t, len(t)) == 0
        rows.append({"overlay_topics": size, "match_ms": match_ms, "commit_ms": commit_ms,
                     "match_after_commit_ms": after_ms, "h2d_bytes": st["h2d_bytes"], "matched_ids": tot})
        print(f"overlay {size}: match {match_ms:.2f} ms, commit of {K} {commit_ms:.3f} ms, "
              f"match after {after_ms:.2f} ms", file=sys.stderr, flush=True)
    # cap 0: the same kind of change, committed by a rebuild
    rs.set_overlay_cap(0)
    rs.rebuild()
    changes()
    full_ms, _ = timed(rs.commit)
    st = rs.last_commit()
    assert st["rebuilt"] == 1, st
    full_after_ms, _ = timed(step)
    inc_ms = rows[0]["commit_ms"]
    out = {
        "bench": "retained_live", "metric": "commit of K changes to the retained store, incremental vs rebuild",
        "value": full_ms / inc_ms, "unit": "x (cap-0 commit time / incremental commit time, overlay 0)",
        "config": {"workload": "c2-shaped", "stored_topics": len(topics), "filters_per_batch": a.filters,
                   "changes_per_commit": K, "mix": "half puts on image topics, half new topics"},
        "rebuild_ms": rebuild_ms, "store_build_s": build_s, "by_overlay_size": rows,
        "cap0": {"commit_ms": full_ms, "match_after_commit_ms": full_after_ms, "h2d_bytes": st["h2d_bytes"]},
        "match_ratio_4096_vs_0": rows[3]["match_ms"] / rows[0]["match_ms"],
        "incremental_commit_faster": bool(max(r["commit_ms"] for r in rows) < full_ms),
    }
    print(json.dumps(out))
    assert out["incremental_commit_faster"], "the incremental commit is not faster than the cap-0 commit"


def delete_bench(a, topics, flt):
    """Wildcard deletes: one device call against the match / per-topic delete / commit sequence (--delete)."""
    import ctypes as C
    from collections import Counter

    from emqx_amd import _lib as L
    from emqx_amd.engine import pack_strings
    from emqx_amd.retainer import RetainedStore

    stores = [RetainedStore(0), RetainedStore(0)]      # [0]: the device call, [1]: the comparison leg
    lib = stores[0].lib
    t0 = time.time()
    for rs in stores:
        for i, t in enumerate(topics):
            lib.egm_rstore_put(rs.h, t, len(t), i, 0)
        rs.rebuild()
    build_s = (time.time() - t0) / 2
    print(f"two stores built, {build_s:.1f}s each", file=sys.stderr, flush=True)

    def match_ids(rs, f):
        blob, off = pack_strings([f])
        res = C.POINTER(L.egm_result)()
        rc = lib.egm_rstore_match(rs.h, C.c_void_p(blob.ctypes.data), C.c_void_p(off.ctypes.data), 1, 0,
                                  L.EGM_RMODE_MATCH, C.byref(res))
        assert rc == 0, rc
        nid = int(res.contents.n_ids)
        ids = np.ctypeslib.as_array(res.contents.ids, shape=(nid,)).copy() if nid else np.zeros(0, np.uint32)
        lib.egm_result_free(res)
        return ids

    def device_delete(rs, f):
        blob, off = pack_strings([f])
        ids, n = L._u32p(), C.c_uint64()
        rc = lib.egm_rstore_delete_matching(rs.h, C.c_void_p(blob.ctypes.data), C.c_void_p(off.ctypes.data), 1,
                                            C.byref(ids), C.byref(n))
        assert rc == 0, rc
        out = np.ctypeslib.as_array(ids, shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint32)
        lib.egm_result_free(ids)
        return out

    def host_delete(rs, f):
        ids = match_ids(rs, f)
        for i in ids.tolist():                         # ids are positions in `topics`
            t = topics[i]
            lib.egm_rstore_delete(rs.h, t, len(t))
        rs.commit()
        return ids

    # candidates and their sizes on the untouched store
    firsts = Counter(t.split(b"/", 1)[0] for t in topics)
    cands = [w + b"/#" for w, _ in firsts.most_common(64)] + [flt[i] for i in range(min(flt.n, 4096))]
    cands = list(dict.fromkeys(cands))
    blob, off = pack_strings(cands)
    res = C.POINTER(L.egm_result)()
    assert lib.egm_rstore_match(stores[0].h, C.c_void_p(blob.ctypes.data), C.c_void_p(off.ctypes.data), len(cands), 0,
                                L.EGM_RMODE_MATCH, C.byref(res)) == 0
    counts = np.ctypeslib.as_array(res.contents.counts, shape=(len(cands),)).copy()
    lib.egm_result_free(res)
    order = [int(i) for i in np.argsort(-counts.astype(np.int64), kind="stable") if counts[i] > 0]
    F = min(a.delete, len(order))
    # the largest, then an even spread over the rest; under 45 % of the store in all, so that no
    # commit inside the timed calls is a rebuild by the tombstone rule
    top, budget = [], int(0.45 * len(topics))
    for i in order:
        if len(top) < (F + 1) // 2 and counts[i] <= budget // 2:   # half of what is left: several large ones fit
            top.append(i)
            budget -= int(counts[i])
    budget //= max(1, F - len(top))
    rest = [i for i in order if i not in top and counts[i] <= budget]
    pick = top + [rest[(k * len(rest)) // (F - len(top))] for k in range(F - len(top) if rest else 0)]
    pick = list(dict.fromkeys(pick))
    warm = next(i for i in reversed(order) if i not in pick)
    for rs, fn in ((stores[0], device_delete), (stores[1], host_delete)):   # code objects, workspace
        fn(rs, cands[warm])

    rows = []
    for k, ci in enumerate(pick):
        f = cands[ci]
        legs = [("device_ms", stores[0], device_delete), ("host_ms", stores[1], host_delete)]
        if k % 2:
            legs.reverse()
        row = {"filter": f.decode(errors="replace"), "matched_on_full_store": int(counts[ci])}
        got = {}
        for name, rs, fn in legs:
            t1 = time.perf_counter()
            got[name] = fn(rs, f)                      # both end synchronised (readback / commit)
            row[name] = 1e3 * (time.perf_counter() - t1)
        assert np.array_equal(np.sort(got["device_ms"]), np.sort(got["host_ms"])), f
        row["ids_deleted"] = int(len(got["device_ms"]))
        rows.append(row)
        print(f"{row['filter']}: {row['ids_deleted']} ids, device {row['device_ms']:.3f} ms, "
              f"match+delete+commit {row['host_ms']:.3f} ms", file=sys.stderr, flush=True)
    assert stores[0].size() == stores[1].size()
    big = [r for r in rows if r["ids_deleted"] >= 10_000]
    dev, host = sum(r["device_ms"] for r in rows), sum(r["host_ms"] for r in rows)
    out = {
        "bench": "retained_delete", "metric": "wildcard delete_message: match + per-topic delete + commit over one "
                                              "egm_rstore_delete_matching call, summed over the filters",
        "value": host / dev, "unit": "x",
        "config": {"workload": "c2-shaped", "stored_topics": len(topics), "filters": len(rows),
                   "timing": "host clock around calls that end in a stream synchronise; one sample per filter "
                             "(a delete cannot be repeated), legs alternate, one process"},
        "device_ms_total": dev, "host_ms_total": host, "ids_deleted_total": sum(r["ids_deleted"] for r in rows),
        "deletes_of_10k_or_more": {"n": len(big), "device_ms": sum(r["device_ms"] for r in big),
                                   "host_ms": sum(r["host_ms"] for r in big),
                                   "device_faster_in_all": bool(all(r["device_ms"] < r["host_ms"] for r in big))},
        "store_build_s": build_s, "by_filter": rows,
    }
    line = json.dumps(out)
    print(line)
    prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    with open(os.path.join(prof, "retained_delete.json"), "w") as fh:
        fh.write(line + "\n")
    for rs in stores:
        rs.close()


if __name__ == "__main__":
    main()
