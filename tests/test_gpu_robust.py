"""Failure behaviour of the C-ABI and the heavy path's no-overflow
guarantee, on the GPU.

* a delta or build with an invalid id changes nothing (the reference's route
  changes are all-or-nothing mnesia transactions, emqx_router.erl:252-303);
* a commit that fails after taking the staged changes publishes them with the
  next commit (EGM_DEBUG_FAIL_COMMIT);
* device batches on different streams share the context's workspaces safely;
* a fan-out into too small a buffer reports its overflow (egm_last_fanout);
* no legal topic (<= 65 535 bytes, emqx_topic.erl:45, 99-100) overflows: a
  7 000-level chain set and a 2^14-wide combination set, against the oracle.
"""
import numpy as np
import pytest

from emqx_amd import _lib as L
from emqx_amd import synth
from emqx_amd.engine import GpuMatcher
from oracle import trie_ref as R
from oracle.cpp import OracleTrie, canonical

pytestmark = pytest.mark.gpu
DEBUG_FAIL_COMMIT = 2


@pytest.fixture(scope="module")
def gm():
    m = GpuMatcher(0)
    yield m
    m.close()


def sets(res):
    return [sorted(res.row(i).tolist()) for i in range(len(res.row_ptr) - 1)]


def test_invalid_delta_changes_nothing(gm):
    gm.build_strings([b"a/+", b"b/#"], ids=[10, 11])
    topics = [b"a/x", b"b/y/z", b"c/d"]
    before = sets(gm.match_strings(topics))
    with pytest.raises(L.EgmError):   # id 10 is taken by a/+: the whole delta is refused
        gm.apply(inserts=[b"c/+", b"d/+"], insert_ids=[12, 10], deletes=[b"a/+"])
    with pytest.raises(L.EgmError):   # the same new id twice
        gm.apply(inserts=[b"c/+", b"d/+"], insert_ids=[13, 13])
    gm.commit()
    assert sets(gm.match_strings(topics)) == before
    assert gm.filter_id(b"c/+") is None
    with pytest.raises(L.EgmError):   # a failed build leaves the old table
        gm.build_strings([b"x/#", b"y/#"], ids=[1, 1])
    assert sets(gm.match_strings(topics)) == before
    gm.apply(inserts=[b"c/+"], insert_ids=[12])   # a valid delta still goes through
    gm.commit()
    assert sets(gm.match_strings(topics))[2] == [12]


def test_failed_commit_keeps_its_changes(gm):
    f, t = synth.config("c0", n_filters=6_000, n_topics=20_000)
    fl = f.to_list()
    gm.build(f.blob, f.off)
    gm.apply(deletes=fl[:2000])
    gm.set_debug(DEBUG_FAIL_COMMIT)
    with pytest.raises(L.EgmError):
        gm.commit()
    gm.set_debug(0)
    gm.apply(deletes=fl[2000:2500])
    gm.commit()                      # publishes both deltas
    res = gm.match(t.blob, t.off, L.EGM_MODE_ROUTES)
    o = OracleTrie(True, L.EGM_MODE_ROUTES)
    o.add(f.blob, f.off)
    from emqx_amd.engine import pack_strings
    o.remove(*pack_strings(fl[:2500]))
    row, ids = o.match(t.blob, t.off, threads=8)
    assert np.array_equal(res.row_ptr, row)
    assert np.array_equal(canonical(res.row_ptr, res.ids), canonical(row, ids))


def test_batches_on_two_streams(gm):
    import torch
    f, t = synth.config("c0", n_topics=60_000)
    gm.build(f.blob, f.off)
    want = gm.match(t.blob, t.off, L.EGM_MODE_ROUTES)
    dev = torch.device("cuda:0")
    d_blob = torch.from_numpy(t.blob).to(dev)
    d_off = torch.from_numpy(t.off.view(np.int32)).to(dev)
    n, cap = t.n, len(want.ids) + 1024
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    # the outputs are zeroed on torch's stream before any match is launched: the
    # side streams do not wait for that stream, so a zero-fill still queued there
    # could land after a match wrote its rows (a race of the test, not the library)
    bufs = [(torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(cap, dtype=torch.int32, device=dev))
            for _ in range(4)]
    torch.cuda.synchronize()
    outs = []
    for s, (r, i) in zip((s1, s2, s1, s2), bufs):   # back to back on alternating streams, no host sync in between
        gm.match_device(d_blob.data_ptr(), int(t.off[-1]), d_off.data_ptr(), n, L.EGM_MODE_ROUTES,
                        s.cuda_stream, r.data_ptr(), i.data_ptr(), cap)
        outs.append((s, r, i))
    torch.cuda.synchronize()
    for s, r, i in outs:
        row = r.cpu().numpy().view(np.uint64)
        ids = i.cpu().numpy().view(np.uint32)[: len(want.ids)]
        assert np.array_equal(row, want.row_ptr)
        assert np.array_equal(canonical(row, ids), canonical(want.row_ptr, want.ids))


def test_fanout_overflow_is_reported(gm):
    import torch
    f, t = synth.config("c1", n_filters=20_000, n_topics=5_000)
    gm.build(f.blob, f.off)
    srow, subs = synth.subscribers(f.n, p_big=0.01, n_big=500, p_share=0.1)
    gm.subs_build(srow, subs)
    host = gm.match(t.blob, t.off, L.EGM_MODE_ROUTES)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    mrow = torch.from_numpy(host.row_ptr.view(np.int64)).to(dev)
    mids = torch.from_numpy(host.ids.view(np.int32)).to(dev)
    n = t.n
    drow = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    fid = torch.zeros(100, dtype=torch.int32, device=dev)
    sub = torch.zeros(100, dtype=torch.int32, device=dev)
    gm.fanout_device(mrow.data_ptr(), mids.data_ptr(), len(host.ids), n, s, drow.data_ptr(), fid.data_ptr(),
                     sub.data_ptr(), 100)
    st = gm.last_fanout()
    total = int(sum(int(srow[x + 1] - srow[x]) for x in host.ids.tolist()))
    assert st["deliveries"] == total > 100 and st["overflow"] == 1
    fid = torch.zeros(total, dtype=torch.int32, device=dev)
    sub = torch.zeros(total, dtype=torch.int32, device=dev)
    gm.fanout_device(mrow.data_ptr(), mids.data_ptr(), len(host.ids), n, s, drow.data_ptr(), fid.data_ptr(),
                     sub.data_ptr(), total)
    assert gm.last_fanout() == {"deliveries": total, "overflow": 0}


def test_no_overflow_7000_level_chains(gm):
    """Topics of 7 000 levels (far deeper than the LDS walk takes: k_heavy with
    its HBM stack) against filter chains that keep a literal and a '+'
    alternative pending at every level, plus the long-topic edge of 65 535
    bytes."""
    D = 7000
    deep = [b"l%d" % (i % 7) for i in range(D)]
    filters = [b"/".join(deep), b"/".join(deep[:-1]) + b"/+", b"/".join([b"+"] * D),
               b"/".join(b"+" if i % 2 else deep[i] for i in range(D)),
               b"/".join(deep[:3500]) + b"/#", b"#", b"l0/#"]
    topics = [b"/".join(deep), b"/".join(deep[:-1]) + b"/zz", b"/".join(deep[:3500]), b"x" * 65_535,
              b"/" * 65_534, b"l0/l1"]
    gm.build_strings(filters)
    for mode in (L.EGM_MODE_TRIE, L.EGM_MODE_ROUTES):
        res = gm.match_strings(topics, mode)
        assert res.n_error == 0
        for i, tp in enumerate(topics):
            want = R.trie_semantics(tp, filters) if mode == 0 else R.routes_semantics(tp, filters)
            got = sorted(filters[x] for x in res.row(i).tolist())
            assert got == sorted(want), (mode, i)


def test_no_overflow_2_14_wide_frontier(gm):
    """Every filter of depth 14 over {'+', 'k<l>'}: the matching topic's
    frontier holds 2^14 states; the light walk narrows to depth-first instead
    of overflowing, and the heavy path (forced) agrees."""
    D = 14
    filters = [b"/".join(b"+" if (m >> l) & 1 else b"k%d" % l for l in range(D)) for m in range(1 << D)]
    filters += [b"#"]
    gm.build_strings(filters)
    topics = [b"/".join(b"k%d" % l for l in range(D)), b"/".join(b"k%d" % l for l in range(D - 1)) + b"/q"] + \
        [b"k0/zz"] * 100
    res = gm.match_strings(topics, L.EGM_MODE_TRIE)
    assert res.n_error == 0
    assert gm.walk_counters()["bounded"] > 0   # the frontier outgrew the LDS stack: depth-first pops
    got = sets(res)
    assert len(got[0]) == (1 << D) - 1 + 1   # all but the all-literal filter, + '#'
    assert len(got[1]) == (1 << (D - 1)) + 1  # last level must be '+', + '#'
    gm.set_debug(1)
    try:
        hv = gm.match_strings(topics, L.EGM_MODE_TRIE)
    finally:
        gm.set_debug(0)
    assert hv.n_error == 0 and sets(hv) == got
    for i in (0, 1):
        assert sorted(filters[x] for x in got[i]) == sorted(R.trie_semantics(topics[i], filters))


def test_pipeline_submit_wait(gm):
    """egm_match_submit / egm_match_wait: batches staged in pinned memory and
    overlapped, results equal to one-by-one matching (itself checked against
    the C++ oracle, emqx_router.erl:129-141), the caller's buffers
    reusable as soon as submit returns, and the ticket limit enforced."""
    f, t = synth.config("c0", n_topics=60_000)
    gm.build(f.blob, f.off)
    parts = [t.subset(np.arange(a, b)) for a, b in ((0, 20_000), (20_000, 20_001), (20_001, 20_001),
                                                      (20_001, 60_000))]
    want = [gm.match(p.blob, p.off, L.EGM_MODE_ROUTES) for p in parts]
    # the one-by-one results themselves against the pinned oracle (VERDICT r2:
    # the pipeline must not only agree with the library's own batch call)
    o = OracleTrie(True, L.EGM_MODE_ROUTES)
    o.add(f.blob, f.off)
    for p, w in zip(parts, want):
        orow, oids = o.match(p.blob, p.off, threads=4)
        assert np.array_equal(w.row_ptr, orow)
        assert np.array_equal(canonical(w.row_ptr, w.ids), canonical(orow, oids))
    tickets = []
    for p in parts:
        blob, off = p.blob.copy(), p.off.copy()
        tickets.append(gm.submit(blob, off, L.EGM_MODE_ROUTES))
        blob[:] = 0   # the library staged its own copy
        off[:] = 0
    for tk, w in zip(tickets, want):
        got = gm.wait(tk)
        assert np.array_equal(got.row_ptr, w.row_ptr)
        assert np.array_equal(canonical(got.row_ptr, got.ids), canonical(w.row_ptr, w.ids))
        assert np.array_equal(got.flags, w.flags)
    # results held by the caller block their slots: at most 8 outstanding
    import ctypes as C
    held = []
    for _ in range(8):
        tk = gm.submit(parts[0].blob, parts[0].off, L.EGM_MODE_ROUTES)
        r = C.POINTER(L.egm_result)()
        assert gm.lib.egm_match_wait(gm.ctx, tk, C.byref(r)) == 0
        held.append(r)
    with pytest.raises(L.EgmError):
        gm.submit(parts[0].blob, parts[0].off, L.EGM_MODE_ROUTES)
    for r in held:
        gm.lib.egm_result_free(r)
    again = gm.wait(gm.submit(parts[3].blob, parts[3].off, L.EGM_MODE_ROUTES))
    assert np.array_equal(again.row_ptr, want[3].row_ptr)


def test_pipeline_deep_in_flight_exact(gm):
    """Round 4's copier thread (results moved by SDMA copies sized from the
    device's id total, egm_pipe.cpp copier_main): 4-6 batches in flight on a
    fresh context — its first batches overflow their slots' id room and are
    rerun — of C2-shaped topics (~50 ids per topic), every result equal to the
    one-by-one device match, itself checked against the C++ oracle on a sample."""
    f, t = synth.config("c2", n_filters=300_000, n_topics=240_000)
    m = GpuMatcher(0)
    try:
        m.build(f.blob, f.off)
        parts = [t.subset(np.arange(k * 30_000, (k + 1) * 30_000)) for k in range(8)]
        want = [m.match(p.blob, p.off, L.EGM_MODE_ROUTES) for p in parts]
        assert int(want[0].row_ptr[-1]) > 15 * 30_000   # a sizeable result per batch (~21 ids per topic)
        o = OracleTrie(True, L.EGM_MODE_ROUTES)
        o.add(f.blob, f.off)
        sub = parts[5].subset(np.arange(0, 3_000))
        orow, oids = o.match(sub.blob, sub.off, threads=4)
        w5 = m.match(sub.blob, sub.off, L.EGM_MODE_ROUTES)
        assert np.array_equal(w5.row_ptr, orow)
        assert np.array_equal(canonical(w5.row_ptr, w5.ids), canonical(orow, oids))
        m2 = GpuMatcher(0)   # fresh pipeline slots: the first batches rerun with more id room
        try:
            m2.build(f.blob, f.off)
            from collections import deque
            for depth in (4, 6):
                inflight, k = deque(), 0
                for r in range(2 * len(parts)):
                    j = r % len(parts)
                    inflight.append((j, m2.submit(parts[j].blob, parts[j].off, L.EGM_MODE_ROUTES)))
                    while len(inflight) >= depth or (r == 2 * len(parts) - 1 and inflight):
                        jj, tk = inflight.popleft()
                        got = m2.wait(tk)
                        assert np.array_equal(got.row_ptr, want[jj].row_ptr), (depth, jj)
                        assert np.array_equal(canonical(got.row_ptr, got.ids),
                                              canonical(want[jj].row_ptr, want[jj].ids)), (depth, jj)
                        assert np.array_equal(got.flags, want[jj].flags)
                        k += 1
                assert k == 2 * len(parts)
        finally:
            m2.close()
    finally:
        m.close()


def test_pipeline_packed_results_exact(gm):
    """EGM_RESULT_PACKED (round 6, egm_pack.hip): batches past the small-batch
    size come back as u32 rows + 3-byte ids, several in flight, every one equal
    to the plain form; a small batch, and a table whose filter ids reach 2^24,
    come back plain (id_bytes 4) — equal too."""
    f, t = synth.config("c2", n_filters=200_000, n_topics=120_000)
    gm.build(f.blob, f.off)
    parts = [t.subset(np.arange(k * 30_000, (k + 1) * 30_000)) for k in range(4)]
    want = [gm.match(p.blob, p.off, L.EGM_MODE_ROUTES) for p in parts]
    assert want[0].id_bytes == 4 and int(want[0].row_ptr[-1]) > 5 * 30_000
    from collections import deque
    inflight = deque()
    for r in range(8):
        j = r % 4
        inflight.append((j, gm.submit(parts[j].blob, parts[j].off, L.EGM_MODE_ROUTES | L.EGM_RESULT_PACKED)))
        while len(inflight) >= 3 or (r == 7 and inflight):
            jj, tk = inflight.popleft()
            got = gm.wait(tk)
            assert got.id_bytes == 3
            assert np.array_equal(got.row_ptr, want[jj].row_ptr)
            assert np.array_equal(got.ids, want[jj].ids)   # the same device rows, only narrowed
            assert np.array_equal(got.flags, want[jj].flags)
    small = t.subset(np.arange(0, 4_096))
    ws = gm.match(small.blob, small.off, L.EGM_MODE_ROUTES)
    gs = gm.wait(gm.submit(small.blob, small.off, L.EGM_MODE_ROUTES | L.EGM_RESULT_PACKED))
    assert gs.id_bytes == 4 and np.array_equal(gs.row_ptr, ws.row_ptr)
    assert np.array_equal(canonical(gs.row_ptr, gs.ids), canonical(ws.row_ptr, ws.ids))
    # filter ids past 24 bits: the plain form
    ids = np.arange(f.n, dtype=np.uint32) + np.uint32((1 << 24) - 1000)
    gm.build(f.blob, f.off, ids)
    wl = gm.match(parts[0].blob, parts[0].off, L.EGM_MODE_ROUTES)
    gl = gm.wait(gm.submit(parts[0].blob, parts[0].off, L.EGM_MODE_ROUTES | L.EGM_RESULT_PACKED))
    assert gl.id_bytes == 4 and int(wl.ids.max()) >= (1 << 24) - 1000
    assert np.array_equal(gl.row_ptr, wl.row_ptr)
    assert np.array_equal(canonical(gl.row_ptr, gl.ids), canonical(wl.row_ptr, wl.ids))


def test_pipeline_tickets_are_generational_and_cancellable(gm):
    """a ticket carries a generation (a stale or repeated ticket is
    refused, never answered with another batch's result) and can be given up
    with egm_match_cancel (its slot is reclaimed once the batch finished)."""
    f, t = synth.config("c0", n_topics=30_000)
    gm.build(f.blob, f.off)
    a, b = t.subset(np.arange(0, 10_000)), t.subset(np.arange(10_000, 30_000))
    o = OracleTrie(True, L.EGM_MODE_ROUTES)
    o.add(f.blob, f.off)
    t1 = gm.submit(a.blob, a.off, L.EGM_MODE_ROUTES)
    r1 = gm.wait(t1)
    row, ids = o.match(a.blob, a.off, threads=4)
    assert np.array_equal(r1.row_ptr, row) and np.array_equal(canonical(r1.row_ptr, r1.ids), canonical(row, ids))
    with pytest.raises(L.EgmError) as e:
        gm.wait(t1)                         # waited already
    assert e.value.code == L.EGM_E_STATE
    t2 = gm.submit(b.blob, b.off, L.EGM_MODE_ROUTES)   # same slot, next generation
    assert (t2 & 0xFFFF) == (t1 & 0xFFFF) and t2 != t1
    with pytest.raises(L.EgmError):
        gm.wait(t1)                         # stale: must not return t2's rows
    r2 = gm.wait(t2)
    row, ids = o.match(b.blob, b.off, threads=4)
    assert np.array_equal(r2.row_ptr, row) and np.array_equal(canonical(r2.row_ptr, r2.ids), canonical(row, ids))
    # 8 abandoned tickets: cancelled, their slots come back (the 8-ticket limit would refuse otherwise)
    for _round in range(3):
        tks = [gm.submit(a.blob, a.off, L.EGM_MODE_ROUTES) for _ in range(8)]
        for tk in tks:
            gm.cancel(tk)
        with pytest.raises(L.EgmError):
            gm.wait(tks[0])                 # a cancelled ticket has no result
    r3 = gm.wait(gm.submit(a.blob, a.off, L.EGM_MODE_ROUTES))
    assert np.array_equal(r3.row_ptr, r1.row_ptr)


def test_cancel_never_blocks_on_a_busy_context(gm):
    """egm_match_cancel (the NIF ticket destructor, a normal
    scheduler) must not wait for the context lock a bulk build holds for
    seconds: it is queued and applied by the next pipeline call."""
    import threading
    import time
    f, t = synth.config("c0", n_topics=10_000)
    gm.build(f.blob, f.off)
    tk = gm.submit(t.blob, t.off, L.EGM_MODE_TRIE)
    big, _ = synth.config("c1", n_filters=1_000_000, n_topics=1)
    th = threading.Thread(target=lambda: gm.build(big.blob, big.off))
    th.start()
    time.sleep(0.3)                      # the build holds the context lock now
    t0 = time.monotonic()
    gm.cancel(tk)                        # queued: returns at once
    dt = time.monotonic() - t0
    busy = th.is_alive()
    th.join(timeout=300)
    assert dt < 0.1, f"cancel blocked {dt:.3f} s"
    with pytest.raises(L.EgmError) as e:
        gm.wait(tk)                      # the queued cancel was applied: no result
    assert e.value.code == L.EGM_E_STATE
    gm.build(f.blob, f.off)
    r = gm.wait(gm.submit(t.blob, t.off, L.EGM_MODE_TRIE))   # the slot came back
    assert len(r.row_ptr) == t.n + 1
    print(f"cancel took {dt * 1e3:.2f} ms while the build {'was' if busy else 'was not'} running")


def test_match_batch_many_threads_never_pipeline_full(gm):
    """more than 8 concurrent egm_match_batch callers (dirty
    schedulers) queue for pipeline slots instead of failing, also while the
    caller holds 8 unreleased ticket results; every row equals the oracle's."""
    import ctypes as C
    import threading
    f, t = synth.config("c0", n_topics=48_000)
    gm.build(f.blob, f.off)
    parts = [t.subset(np.arange(k * 2_000, (k + 1) * 2_000)) for k in range(24)]
    o = OracleTrie(True, L.EGM_MODE_ROUTES)
    o.add(f.blob, f.off)
    want = [o.match(p.blob, p.off, threads=2) for p in parts]
    held = []
    for _ in range(8):   # the 8 tickets of egm_match_submit, results not released
        r = C.POINTER(L.egm_result)()
        tk = gm.submit(parts[0].blob, parts[0].off, L.EGM_MODE_ROUTES)
        assert gm.lib.egm_match_wait(gm.ctx, tk, C.byref(r)) == 0
        held.append(r)
    errors, got = [], [None] * len(parts)

    def worker(k):
        try:
            for _ in range(3):
                got[k] = gm.match(parts[k].blob, parts[k].off, L.EGM_MODE_ROUTES)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(k,)) for k in range(len(parts))]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    for r in held:
        gm.lib.egm_result_free(r)
    assert not errors, errors[:3]
    for g, (row, ids) in zip(got, want):
        assert np.array_equal(g.row_ptr, row)
        assert np.array_equal(canonical(g.row_ptr, g.ids), canonical(row, ids))


def test_walk_guard_trip_is_a_device_error_not_overflow(gm):
    """a tripped walk guard (a kernel invariant failed) is
    EGM_E_DEVICE from wait/batch and from egm_last_stats, reported in its own
    bits (egm_last_guard), never as the capacity `overflow` a caller would
    answer with a bigger buffer."""
    import torch
    f, t = synth.config("c0", n_topics=20_000)
    gm.build(f.blob, f.off)
    good = gm.match(t.blob, t.off, L.EGM_MODE_ROUTES)
    gm.set_debug(L.EGM_DEBUG_FORCE_GUARD)
    try:
        with pytest.raises(L.EgmError) as e:
            gm.match(t.blob, t.off, L.EGM_MODE_ROUTES)
        assert e.value.code == L.EGM_E_DEVICE and "guard" in str(e.value)
        dev = torch.device("cuda:0")
        d_blob = torch.from_numpy(t.blob).to(dev)
        d_off = torch.from_numpy(t.off.view(np.int32)).to(dev)
        d_row = torch.zeros(t.n + 1, dtype=torch.int64, device=dev)
        d_ids = torch.zeros(64 * t.n, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        gm.match_device(d_blob.data_ptr(), int(t.off[-1]), d_off.data_ptr(), t.n, L.EGM_MODE_ROUTES, s,
                        d_row.data_ptr(), d_ids.data_ptr(), 64 * t.n)
        torch.cuda.synchronize()
        with pytest.raises(L.EgmError) as e:
            gm.last_stats()
        assert e.value.code == L.EGM_E_DEVICE
        assert gm.last_guard() & L.EGM_GUARD_LOOP
    finally:
        gm.set_debug(0)
    again = gm.match(t.blob, t.off, L.EGM_MODE_ROUTES)
    assert gm.last_guard() == 0 and gm.last_stats()["overflow"] == 0
    assert np.array_equal(again.row_ptr, good.row_ptr)
