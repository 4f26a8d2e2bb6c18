"""Cluster routes on the device (egm_routes_*, egm_forward_*): the forward arm
of emqx_broker:do_route/2 (emqx_broker.erl:242-247, 262-280) over the
route-node table, and cleanup_routes/1 (emqx_router_helper.erl:137-146).

* the device's per-node lists equal the node entries of the oracle's
  aggre(match_routes(T)), and Broker(device_forward=True) returns what the
  host loop returns (with and without device_dispatch);
* hand-built match CSRs and masks at the tile, wave and slot edges, element for
  element (order included) against a numpy restatement;
* capacity overflow, deltas / commits / streams, the node drop, argument errors.
"""
import random

import numpy as np
import pytest

from emqx_amd import _lib as L
from emqx_amd.broker import Broker
from emqx_amd.engine import GpuMatcher, MatchResult
from oracle import trie_ref as R
from tests.test_capi_cpu import rand_filter, rand_topic

pytestmark = pytest.mark.gpu
CAP = 1 << 19
SENTINEL = 0xABABABAB
LOCAL = L.FWD_LOCAL
NODES = L.EGM_ROUTE_MAX_NODES


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view({4: np.int32, 8: np.int64}[np.dtype(dt).itemsize])
                            ).to(torch.device("cuda:0"))


def _host(t, dt):
    return t.cpu().numpy().view(dt)


def forward(gm, mrow, mids, cap=CAP, stream=None, sync=True, mids_len=None):
    """egm_forward_device on a host-built match CSR; every output is filled
    with SENTINEL on the launch stream first.  Returns the host copies (after
    a sync) or, sync=False, a function that does."""
    import torch
    n, nids = len(mrow) - 1, len(mids)
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        t_mrow, t_mids = _dev(mrow, np.uint64), _dev(np.append(mids, 0), np.uint32)
        t_nrow = _dev(np.full(NODES + 2, SENTINEL), np.uint64)
        t_topic = _dev(np.full(cap + 64, SENTINEL), np.uint32)
        t_fid = _dev(np.full(cap + 64, SENTINEL), np.uint32)
        t_ef = _dev(np.full(nids + 1, SENTINEL), np.uint32)
        t_tf = _dev(np.full(n + 1, SENTINEL), np.uint32)
    gm.forward_device(t_mrow.data_ptr(), t_mids.data_ptr(), nids if mids_len is None else mids_len, n, s.cuda_stream,
                      t_nrow.data_ptr(), t_topic.data_ptr(), t_fid.data_ptr(), cap, t_ef.data_ptr(), t_tf.data_ptr())

    def read():
        s.synchronize()
        keep = (t_mrow, t_mids)   # alive until the kernels have run
        del keep
        return {"nrow": _host(t_nrow, np.uint64), "topic": _host(t_topic, np.uint32), "fid": _host(t_fid, np.uint32),
                "efwd": _host(t_ef, np.uint32), "tfwd": _host(t_tf, np.uint32)}

    return read() if sync else read


def slots_of(n):
    """Device slots of a table built from n masks (the header's rule)."""
    return n + n // 4 + 4096


def popcount(x):
    x = x.astype(np.uint64)
    return np.array([bin(int(v)).count("1") for v in x], dtype=np.uint32) if len(x) else np.zeros(0, np.uint32)


def model(mrow, mids, masks, self_node):
    """The forward pass restated: node_row, the pair lists, entry_fwd, topic_fwd."""
    mrow, mids = np.asarray(mrow, dtype=np.int64), np.asarray(mids, dtype=np.int64)
    masks = np.asarray(masks, dtype=np.uint64)
    n = len(mrow) - 1
    m = np.zeros(len(mids), dtype=np.uint64)
    ok = mids < len(masks)
    m[ok] = masks[mids[ok]]
    selfbit = np.uint64(1 << self_node)
    remote = m & ~selfbit
    pc = popcount(remote)
    efwd = pc | np.where(m & selfbit, np.uint32(LOCAL), np.uint32(0)).astype(np.uint32)
    row_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(mrow))
    tfwd = np.bincount(row_of, weights=pc, minlength=n).astype(np.uint32) if n else np.zeros(0, np.uint32)
    nrow, topic, fid = [0], [], []
    for k in range(NODES):
        sel = ((remote >> np.uint64(k)) & np.uint64(1)).astype(bool)
        topic.append(row_of[sel])
        fid.append(mids[sel])
        nrow.append(nrow[-1] + int(sel.sum()))
    return (np.array(nrow, dtype=np.uint64), np.concatenate(topic).astype(np.uint32),
            np.concatenate(fid).astype(np.uint32), efwd, tfwd)


def check(gm, mrow, mids, masks, self_node, cap=CAP):
    nrow, topic, fid, efwd, tfwd = model(mrow, mids, masks, self_node)
    got = forward(gm, mrow, mids, cap)
    tot = len(topic)
    assert gm.last_forward() == {"forwards": tot, "overflow": 0}
    assert np.array_equal(got["nrow"][:NODES + 1], nrow) and got["nrow"][NODES + 1] == SENTINEL
    assert np.array_equal(got["topic"][:tot], topic) and np.all(got["topic"][tot:] == SENTINEL)
    assert np.array_equal(got["fid"][:tot], fid) and np.all(got["fid"][tot:] == SENTINEL)
    assert np.array_equal(got["efwd"][:len(mids)], efwd) and got["efwd"][len(mids)] == SENTINEL
    assert np.array_equal(got["tfwd"][:len(mrow) - 1], tfwd) and got["tfwd"][len(mrow) - 1] == SENTINEL
    assert nrow[self_node] == nrow[self_node + 1]                  # the local node's row is empty
    return tot


# ---------------------------------------------------------------- 1. parity ----
REMOTES = ["n1", "n2", "n3", "n4"]     # + "local": 5 nodes


def _scenario(device_forward, device_dispatch):
    """test_gpu_dispatch._scenario's shape plus 0-3 remote dests per filter."""
    rng = random.Random(17)
    br = Broker(shared_strategy="hash_clientid", device_dispatch=device_dispatch, device_forward=device_forward)
    o = R.Router()
    fl = list(dict.fromkeys(rand_filter(rng) for _ in range(120)))
    sid = 0
    for f in fl:
        for dst in rng.sample(REMOTES, rng.randint(0, 3)):
            br.router.do_add_route(f, dst)
            o.do_add_route(f, ("node", dst))
        if rng.random() < 0.8:
            for _ in range(rng.randint(1, 3)):
                br.subscribe(f, sid, clientid=b"c%d" % sid)
                sid += 1
            o.do_add_route(f, ("node", "local"))
        if rng.random() < 0.2:
            g = b"g%d" % rng.randint(0, 2)
            for _ in range(rng.randint(1, 5)):
                br.subscribe(b"$share/" + g + b"/" + f, sid)
                sid += 1
            o.do_add_route(f, ("group", g))
    for x in rng.sample(range(sid), sid // 4):
        br.kill(x)
    topics = [rand_topic(rng) for _ in range(300)]
    clients = [b"pub%d" % rng.randint(0, 40) for _ in topics]
    return br, o, topics, clients


def _canon(lists):
    return [sorted(x, key=repr) for x in lists]


@pytest.mark.parametrize("device_dispatch", [False, True])
def test_device_forwards_equal_the_oracle_and_the_host_loop(device_dispatch):
    host, o, topics, clients = _scenario(False, device_dispatch)
    devb = _scenario(True, device_dispatch)[0]
    # A: the device lists against aggre(match_routes(T))
    r = devb.router
    res = r.match_filters_batch(topics)
    f = r.m.forward(res)
    got = [set() for _ in topics]
    for nid, name in enumerate(r.node_names):
        for j in range(int(f["node_row"][nid]), int(f["node_row"][nid + 1])):
            pair = (r.filter_of(int(f["fid"][j])), name)
            assert pair not in got[int(f["topic"][j])]              # once per {To, Node}
            got[int(f["topic"][j])].add(pair)
    assert int(f["node_row"][-1]) == len(f["topic"]) > 100
    n_local = 0
    for k, t in enumerate(topics):
        nodes = [(to, d[1]) for to, d in R.aggre(o.match_routes(t)) if d[0] == "node"]
        assert got[k] == {x for x in nodes if x[1] != "local"}, t
        assert int(f["topic_fwd"][k]) == len(got[k])
        for i in range(int(res.row_ptr[k]), int(res.row_ptr[k + 1])):
            flt = r.filter_of(int(res.ids[i]))
            assert bool(f["entry_fwd"][i] & LOCAL) == ((flt, "local") in nodes)
            n_local += (flt, "local") in nodes
    assert n_local > 50
    # B: the broker with device_forward against the host loop (an entry's routes as a set: aggre/1 usorts)
    assert _canon(devb.publish_batch(topics, clients)) == _canon(host.publish_batch(topics, clients))
    assert sum(1 for dl in devb.publish_batch(topics, clients) for x in dl if x[0] == "node") > 100
    assert _canon(devb.publish_result_batch(topics, clients)) == _canon(host.publish_result_batch(topics, clients))
    assert devb.metrics == host.metrics and host.metrics["messages.forward"] > 100
    # route churn goes in as deltas, a lost node through cleanup_routes
    for b in (host, devb):
        fl = sorted(b.router.routes)
        b.router.do_add_route(fl[0], "n5")
        b.router.do_delete_route(next(f for f in fl if "n1" in b.router.routes[f]), "n1")
        gone = b.router.cleanup_routes("n2")
        b.gone = sorted(gone)
    assert devb.gone == host.gone and len(host.gone) > 0
    assert devb.router.m.routes_last_commit()["rebuilt"] is False
    assert _canon(devb.publish_result_batch(topics, clients)) == _canon(host.publish_result_batch(topics, clients))
    assert _canon(devb.publish_batch(topics, clients)) == _canon(host.publish_batch(topics, clients))
    assert devb.metrics == host.metrics
    assert not any(x[2] == "n2" for dl in devb.publish_batch(topics, clients) for x in dl if x[0] == "node")


# ------------------------------------------------------- 2. boundary shapes ----
N_MASKS = 40
ALL = (1 << 64) - 1


def shape_masks(rng):
    """Filter 0: mask 0; 1: all 64 bits; 2: only node 63; 3: only node 0; 4: nodes 0 and 63; the rest random."""
    m = [0, ALL, 1 << 63, 1, (1 << 63) | 1]
    while len(m) < N_MASKS:
        m.append(int(rng.integers(0, 2 ** 63)) << int(rng.integers(0, 2)) if rng.random() < 0.8 else 0)
    return np.array(m, dtype=np.uint64)


def shape_ids(rng, total):
    """Filter ids of `total` entries: the table's, the last slot, the first id past the slots, one far past."""
    s = slots_of(N_MASKS)
    pool = np.concatenate([np.arange(N_MASKS), [s - 1, s, s + 5, 0xFFFFFFEF]]).astype(np.uint32)
    ids = pool[rng.integers(0, len(pool), total)]
    ids[:min(total, len(pool))] = pool[:min(total, len(pool))]
    return ids


def csr_rows(total, rows):
    """`rows` rows over `total` entries, the first and last row empty and an empty row at every tile edge."""
    sizes = np.zeros(rows, dtype=np.int64)
    fill = [k for k in range(1, rows - 1) if k % 64 not in (0, 63)]
    for j in range(total):
        sizes[fill[j % len(fill)]] += 1
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


@pytest.fixture(scope="module", params=[0, 63])
def table(request):
    rng = np.random.default_rng(5)
    masks = shape_masks(rng)
    gm = GpuMatcher(0)
    gm.routes_build(masks, request.param)
    yield gm, masks, request.param
    gm.close()


@pytest.mark.parametrize("total", [0, 1, 63, 64, 65, 4097])
def test_entry_counts_at_the_wave_edges(table, total):
    gm, masks, self_node = table
    rng = np.random.default_rng(total)
    mids = shape_ids(rng, total)
    check(gm, np.array([0, total], dtype=np.uint64), mids, masks, self_node)         # one row
    tot = check(gm, csr_rows(total, 70), mids, masks, self_node)                     # two tiles
    assert tot > 0 or total < 2


@pytest.mark.parametrize("rows", [63, 64, 65, 129])
def test_row_counts_at_the_tile_edges(table, rows):
    gm, masks, self_node = table
    rng = np.random.default_rng(rows)
    total = 3 * rows + 7
    assert check(gm, csr_rows(total, rows), shape_ids(rng, total), masks, self_node) > rows
    check(gm, np.zeros(rows + 1, dtype=np.uint64), np.zeros(0, np.uint32), masks, self_node)   # every row empty


def test_long_rows_inside_a_tile(table):
    gm, masks, self_node = table
    rng = np.random.default_rng(9)
    sizes = [0, 3, 200, 0, 1, 5000, 2, 0] + [1] * 60 + [0, 7]
    mrow = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    total = int(mrow[-1])
    assert check(gm, mrow, shape_ids(rng, total), masks, self_node) > 5000
    check(gm, mrow, np.full(total, 1, dtype=np.uint32), masks, self_node)            # every entry: all 64 bits
    check(gm, mrow, np.full(total, 2, dtype=np.uint32), masks, self_node)            # every entry: only node 63
    check(gm, mrow, np.full(total, 0, dtype=np.uint32), masks, self_node)            # every entry: mask 0


# ------------------------------------------------------------- 3. overflow ----
def test_capacity_overflow_writes_no_list(table):
    gm, masks, self_node = table
    rng = np.random.default_rng(3)
    mrow, mids = csr_rows(300, 130), shape_ids(rng, 300)
    nrow, topic, fid, efwd, tfwd = model(mrow, mids, masks, self_node)
    total = len(topic)
    got = forward(gm, mrow, mids, cap=total - 1)
    assert gm.last_forward() == {"forwards": total, "overflow": 1}
    assert np.all(got["topic"] == SENTINEL) and np.all(got["fid"] == SENTINEL)
    assert np.array_equal(got["nrow"][:NODES + 1], nrow)
    assert np.array_equal(got["efwd"][:300], efwd) and np.array_equal(got["tfwd"][:len(tfwd)], tfwd)
    assert check(gm, mrow, mids, masks, self_node, cap=total) == total
    # a match row total past the id buffer is refused before any kernel reads the ids
    with pytest.raises(L.EgmError) as e:
        forward(gm, mrow, mids, mids_len=299)
    assert e.value.code == L.EGM_E_OVERFLOW


def test_host_form_retries_on_capacity(table):
    """egm_forward_batch (its first guess is ids + 1024 forwards)."""
    gm, masks, self_node = table
    mids = np.full(60, 1, dtype=np.uint32)           # 60 entries x 63 remote nodes
    mrow = np.array([0, 0, 25, 60], dtype=np.uint64)
    nrow, topic, fid, efwd, tfwd = model(mrow, mids, masks, self_node)
    assert len(topic) == 60 * 63 > 60 + 1024
    f = gm.forward(MatchResult(mrow, mids, np.zeros(3, np.uint8), 0, 0, 0, 0))
    assert np.array_equal(f["node_row"], nrow) and np.array_equal(f["topic"], topic) and np.array_equal(f["fid"], fid)
    assert np.array_equal(f["entry_fwd"], efwd) and np.array_equal(f["topic_fwd"], tfwd)
    assert gm.last_forward() == {"forwards": len(topic), "overflow": 0}


# --------------------------------------------------- 4. deltas and streams ----
def one_row_per_entry(mids):
    return np.arange(len(mids) + 1, dtype=np.uint64), np.asarray(mids, dtype=np.uint32)


def test_route_deltas_commits_and_streams():
    import torch
    gm = GpuMatcher(0)
    masks = np.zeros(8, dtype=np.uint64)
    masks[1], masks[2] = 0b0110, 0b0001
    gm.routes_build(masks, 0)
    want = masks.copy()
    ids = np.arange(8, dtype=np.uint32)

    def now(extra=0):
        return check(gm, *one_row_per_entry(np.append(ids, extra)), want, 0)

    assert now() == 2
    gm.routes_apply_delta(add=[(3, 5), (1, 2), (1, 3)])            # (1, 2) is present already: nothing
    assert now() == 2                                               # staged, not committed
    want[3] |= 1 << 5
    want[1] |= 1 << 3
    gm.routes_commit()
    assert gm.routes_last_commit() == {"patched": 2, "rebuilt": False} and now() == 4
    gm.routes_apply_delta(add=[(4, 0)], delete=[(1, 1), (7, 9), (100000, 1)])     # absent pairs do nothing
    want[4] |= 1
    want[1] &= ~np.uint64(2)
    gm.routes_commit()
    # the copy written now lacked the first commit's masks (1 and 3) as well: 1, 3 and 4
    assert gm.routes_last_commit() == {"patched": 3, "rebuilt": False} and now() == 3
    gm.routes_commit()                                              # nothing staged: the other copy catches up
    assert gm.routes_last_commit() == {"patched": 2, "rebuilt": False} and now() == 3
    with pytest.raises(L.EgmError) as e:                            # a pair in both lists: nothing applied
        gm.routes_apply_delta(add=[(5, 1), (3, 5)], delete=[(3, 5)])
    assert e.value.code == L.EGM_E_INVAL
    for bad in ([(1, 64)], [(0xFFFFFFF0, 1)], [(slots_of(8) + (1 << 22), 1)]):
        with pytest.raises(L.EgmError) as e:
            gm.routes_apply_delta(add=bad)
        assert e.value.code == L.EGM_E_INVAL
    with pytest.raises(L.EgmError) as e:
        gm.routes_apply_delta(delete=[(1, 64)])
    assert e.value.code == L.EGM_E_INVAL
    gm.routes_commit()
    assert now() == 3
    # a pass queued on a side stream before a commit returns the old epoch's lists
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    mrow, mids = one_row_per_entry(ids)
    old = model(mrow, mids, want, 0)
    pending = forward(gm, mrow, mids, stream=side, sync=False)
    gm.routes_apply_delta(add=[(6, 7)], delete=[(1, 2)])
    gm.routes_commit()
    got = pending()
    assert np.array_equal(got["nrow"][:NODES + 1], old[0]) and np.array_equal(got["topic"][:len(old[1])], old[1])
    assert np.array_equal(got["fid"][:len(old[2])], old[2]) and np.array_equal(got["efwd"][:8], old[3])
    torch.cuda.synchronize()
    want[6] |= 1 << 7
    want[1] &= ~np.uint64(4)
    assert now() == 3
    # a filter id past the slots: one full upload, then patches again
    big = slots_of(8) + 10
    gm.routes_apply_delta(add=[(big, 2), (2, 3)])
    want = np.concatenate([want, np.zeros(big + 1 - 8, dtype=np.uint64)])
    want[big] |= 4
    want[2] |= 8
    gm.routes_commit()
    assert gm.routes_last_commit()["rebuilt"] is True
    assert now(big) == 5
    gm.routes_apply_delta(delete=[(big, 2)], add=[(big + 1, 1)])
    want = np.append(want, np.uint64(2))
    want[big] = 0
    gm.routes_commit()
    assert gm.routes_last_commit() == {"patched": 2, "rebuilt": False}
    ids = np.append(ids, [big, big + 1]).astype(np.uint32)
    assert now() == 5
    gm.close()


# ------------------------------------------------------------ 5. drop_node ----
@pytest.mark.parametrize("n", [0, 1, 64, 65, 10000])
def test_drop_node(n):
    """Masks: bit 3 in half of them, and in half of them random bits below 62
    besides — so a quarter holds node 3 alone; self node 1."""
    rng = np.random.default_rng(n + 1)
    masks = (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(3)) | \
        (rng.integers(0, 2, n, dtype=np.uint64) * rng.integers(0, 2 ** 62, n, dtype=np.uint64))
    gm = GpuMatcher(0)
    gm.routes_build(masks, 1)
    mrow, mids = one_row_per_entry(np.arange(n + 2, dtype=np.uint32))
    assert len(gm.routes_drop_node(63)) == 0                          # nobody routes to node 63
    check(gm, mrow, mids, masks, 1)
    emptied = gm.routes_drop_node(3)
    want = np.flatnonzero(masks == np.uint64(8)).astype(np.uint32)
    assert np.array_equal(emptied, want) and (n < 64 or len(want) > n // 8)
    after = masks & ~np.uint64(8)
    nrow = model(mrow, mids, after, 1)[0]
    assert nrow[3] == nrow[4]
    check(gm, mrow, mids, after, 1)                                   # the other bits are untouched
    assert len(gm.routes_drop_node(3)) == 0                           # absent now
    check(gm, mrow, mids, after, 1)
    if n:   # the copy a drop did not rewrite gets it before the next commit's patches
        gm.routes_apply_delta(add=[(0, 3)])
        gm.routes_commit()
        after[0] |= np.uint64(8)
        check(gm, mrow, mids, after, 1)
        gm.routes_commit()
        check(gm, mrow, mids, after, 1)
    gm.close()


# ------------------------------------------------- 6. states and arguments ----
def test_states_and_argument_errors():
    import torch
    gm = GpuMatcher(0)
    mrow, mids = one_row_per_entry([0, 1])
    with pytest.raises(L.EgmError) as e:                   # before egm_routes_build
        forward(gm, mrow, mids)
    assert e.value.code == L.EGM_E_STATE
    for call in (lambda: gm.routes_apply_delta(add=[(0, 1)]), gm.routes_commit, lambda: gm.routes_drop_node(1),
                 gm.last_forward, lambda: gm.forward(MatchResult(mrow, mids, np.zeros(2, np.uint8), 0, 0, 0, 0))):
        with pytest.raises(L.EgmError) as e:
            call()
        assert e.value.code == L.EGM_E_STATE
    with pytest.raises(L.EgmError) as e:                   # self node >= 64
        gm.routes_build(np.zeros(2, np.uint64), 64)
    assert e.value.code == L.EGM_E_INVAL
    gm.routes_build(np.array([2, 1], dtype=np.uint64), 0)
    with pytest.raises(L.EgmError) as e:
        gm.routes_drop_node(64)
    assert e.value.code == L.EGM_E_INVAL
    t = _dev(np.zeros(80), np.uint64)
    p = t.data_ptr()
    lib, ctx = gm.lib, gm.ctx
    assert lib.egm_forward_device(ctx, None, p, 0, 0, None, p, p, p, 0, None, None) == L.EGM_E_INVAL
    assert lib.egm_forward_device(ctx, p, p, 0, 0, None, None, p, p, 0, None, None) == L.EGM_E_INVAL
    assert lib.egm_forward_device(ctx, p, p, 0, 0, None, p, None, p, 0, None, None) == L.EGM_E_INVAL
    assert lib.egm_forward_device(ctx, p, p, 0, 0, None, p, p, None, 0, None, None) == L.EGM_E_INVAL
    assert lib.egm_routes_drop_node(ctx, 1, None, None) == L.EGM_E_INVAL
    assert lib.egm_forward_device(ctx, p, p, 0, 0, None, p, p, p, 0, None, None) == L.EGM_OK   # the count arrays are optional
    torch.cuda.synchronize()
    assert gm.last_forward() == {"forwards": 0, "overflow": 0}
    assert check(gm, mrow, mids, np.array([2, 1], dtype=np.uint64), 0) == 1
    gm.close()
