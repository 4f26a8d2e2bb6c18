"""GPU parity: the HIP path through the C-ABI vs the pinned oracle.

Bit-exact set equality per topic (ids sorted within each row — the reference's
own suites compare with lists:sort).  Small cases against the Python
restatement, config-sized cases against the C++ restatement, full sizes through
size-independent properties (shard union, determinism, sampled oracle rows).
"""
import random

import numpy as np
import pytest

from emqx_amd import _lib as L
from emqx_amd import synth
from emqx_amd.engine import GpuMatcher, pack_strings
from oracle import trie_ref as R
from oracle.cpp import OracleTrie, canonical
from tests.kat import b, load
from tests.test_capi_cpu import rand_filter, rand_topic

pytestmark = pytest.mark.gpu

MODES = [L.EGM_MODE_TRIE, L.EGM_MODE_ROUTES]


@pytest.fixture(scope="module")
def gm():
    m = GpuMatcher(0)
    yield m
    m.close()


def sets_of(res, names=None):
    out = []
    for i in range(len(res.row_ptr) - 1):
        r = res.row(i)
        assert len(r) == len(set(r.tolist())), "duplicate ids in a row"
        out.append(sorted(names[int(x)] for x in r) if names is not None else sorted(r.tolist()))
    return out


@pytest.mark.parametrize("mode", MODES)
def test_reference_kats(gm, mode):
    K = load()
    for case in K["trie_cases"]:
        gm.build_strings([])
        live = {}
        nxt = 0
        for op in case["ops"]:
            if op[0] == "insert":
                f = b(op[1])
                if f not in live.values():
                    gm.apply(inserts=[f], insert_ids=[nxt])
                    live[nxt] = f
                    nxt += 1
                gm.commit()
            elif op[0] == "delete":
                f = b(op[1])
                gm.apply(deletes=[f])
                for k in [k for k, v in live.items() if v == f]:
                    del live[k]
                gm.commit()
            elif op[0] == "assert_empty":
                assert gm.empty() is op[1]
        if not case["queries"]:
            continue
        res = gm.match_strings([b(q) for q, _ in case["queries"]], mode)
        got = sets_of(res, live)
        for i, (q, exp) in enumerate(case["queries"]):
            want = sorted(b(x) for x in exp) if mode == L.EGM_MODE_TRIE else sorted(
                R.routes_semantics(b(q), live.values()))
            assert got[i] == want, (case["name"], q)


@pytest.mark.parametrize("seed", range(3))
def test_random_small_with_deltas(gm, seed):
    rng = random.Random(seed)
    filters = list(dict.fromkeys([rand_filter(rng) for _ in range(300)] + [b"$x", b"a/b", b"$", b""]))
    gm.build_strings(filters)
    live = dict(enumerate(filters))
    topics = [rand_topic(rng) for _ in range(2000)] + [b"", b"$", b"/", b"a/b", b"$x", b"+", b"#", b"a/+/#"]
    for rnd in range(3):
        for mode in MODES:
            res = gm.match_strings(topics, mode)
            got = sets_of(res, live)
            for i, t in enumerate(topics):
                want = R.trie_semantics(t, live.values()) if mode == 0 else R.routes_semantics(t, live.values())
                assert got[i] == sorted(want), (rnd, mode, t)
            wc = np.array([R.wildcard(t) for t in topics])
            assert np.array_equal((res.flags & L.EGM_TF_WILDCARD) != 0, wc)
        # mutate: delete a slice, insert new filters with fresh ids
        dels = [live[k] for k in list(live)[rnd::4]]
        news = list(dict.fromkeys(f for f in (rand_filter(rng) for _ in range(60)) if f not in live.values()))
        base = 10_000 * (rnd + 1)
        gm.apply(inserts=news, deletes=dels, insert_ids=list(range(base, base + len(news))))
        for k in [k for k, v in live.items() if v in set(dels)]:
            del live[k]
        for j, f in enumerate(news):
            if f not in set(dels):
                live[base + j] = f
        gm.commit()


def test_deep_and_long(gm):
    T = b"a/b/c/d/e/f/g/h/i/j/k/l/m/n/o/p/q/r/s/t/u/v/w/x/y/z"
    deep = b"/".join(b"l%d" % i for i in range(300))
    filters = [b"#", T + b"/#", T + b"/+", b"/".join([b"+"] * 26) + b"/#",
               b"a/+/c/+/e/+/g/+/i/+/k/+/m/+/o/+/q/+/s/+/u/+/w/+/y/+/#", deep, deep + b"/#",
               b"/".join([b"+"] * 299) + b"/+", b"x" * 5000 + b"/+"]
    gm.build_strings(filters)
    topics = [T, T + b"/1", deep, deep + b"/more", b"x" * 5000 + b"/y", b"/".join([b"q"] * 300)]
    for mode in MODES:
        res = gm.match_strings(topics, mode)
        got = sets_of(res, dict(enumerate(filters)))
        for i, t in enumerate(topics):
            want = R.trie_semantics(t, filters) if mode == 0 else R.routes_semantics(t, filters)
            assert got[i] == sorted(want), (mode, t[:40])


def test_tokenise_segments_and_long_topics(gm):
    """k_tokenise splits a block into segments that fit LDS: C3-sized topics
    (~100 B, 16 levels), a topic longer than the LDS byte stage, one with more
    words than the LDS word table, and short topics around them in one block."""
    rng = random.Random(11)
    huge = b"h" * 30_000 + b"/t"                   # > TOK_LDS bytes: lane path from global memory
    many = b"/".join([b"w"] * 4_000)               # > TOK_WORDS words
    deep = [b"/".join(b"d%d_%d" % (l, rng.randrange(4)) for l in range(16)) for _ in range(700)]
    short = [b"s/%d" % rng.randrange(50) for _ in range(300)]
    topics = short[:150] + [huge] + deep[:350] + [many] + short[150:] + deep[350:] + [b"", b"$SYS/x", b"a/+"]
    filters = [b"#", b"s/+", b"h" * 30_000 + b"/+", b"w/w/#", b"$SYS/#", b"a/+", b"/".join([b"+"] * 16),
               b"d0_1/#", b"d0_2/+/d2_3/#"] + deep[:5] + [b"/".join([b"w"] * 4_000)]
    gm.build_strings(filters)
    names = dict(enumerate(filters))
    for mode in MODES:
        got = sets_of(gm.match_strings(topics, mode), names)
        for i, t in enumerate(topics):
            want = R.trie_semantics(t, filters) if mode == 0 else R.routes_semantics(t, filters)
            assert got[i] == sorted(want), (mode, i, t[:40])


def test_heavy_path_wide_frontier(gm):
    # every filter of depth 11 over {'+', 'k<l>'} : a matching topic hits 2^11
    # filters, far above the per-wave LDS stage -> chunk deferred to k_heavy
    D = 11
    filters = []
    for m in range(1 << D):
        filters.append(b"/".join(b"+" if (m >> l) & 1 else b"k%d" % l for l in range(D)))
    filters += [b"#", b"k0/#"]
    gm.build_strings(filters)
    topics = [b"/".join(b"k%d" % l for l in range(D)), b"k0/zz", b"/".join(b"k%d" % l for l in range(D - 1)) +
              b"/no"] + [b"p/q/r"] * 300
    res = gm.match_strings(topics, L.EGM_MODE_TRIE)
    assert res.n_error == 0
    gm.set_debug(1)   # EGM_DEBUG_FORCE_HEAVY: the same batch through k_heavy
    try:
        hv = gm.match_strings(topics, L.EGM_MODE_TRIE)
    finally:
        gm.set_debug(0)
    assert hv.n_heavy == len(topics) and hv.n_error == 0
    assert sets_of(hv) == sets_of(res)
    got = sets_of(res)
    assert len(got[0]) == (1 << D) - 1 + 1 + 1   # all but the all-literal filter, + '#', 'k0/#'
    names = dict(enumerate(filters))
    for i, t in enumerate(topics[:3]):
        assert sorted(names[x] for x in got[i]) == sorted(R.trie_semantics(t, filters))
    rr = gm.match_strings(topics, L.EGM_MODE_ROUTES)
    assert sets_of(rr)[0] == sorted(got[0] + [0])   # + the exact filter k0/../k10


@pytest.mark.parametrize("mode", MODES)
def test_config_c0_vs_cpp_oracle(gm, mode):
    f, t = synth.config("c0")
    gm.build(f.blob, f.off)
    res = gm.match(t.blob, t.off, mode)
    o = OracleTrie(True, mode)
    o.add(f.blob, f.off)
    row, ids = o.match(t.blob, t.off, threads=8)
    assert np.array_equal(res.row_ptr, row)
    assert np.array_equal(canonical(res.row_ptr, res.ids), canonical(row, ids))
    # the roofline numerator's V_t: the kernels' count of states created equals
    # the oracle's independent count (string prefixes; tests/test_oracle_visited.py)
    vt, _ = o.visited_counts(t.blob, t.off, threads=8)
    assert res.visited == vt > 0


@pytest.mark.parametrize("mode", MODES)
def test_config_c0_heavy_path_vs_cpp_oracle(gm, mode):
    """The overflow kernel alone (every chunk deferred) is also bit-exact."""
    f, t = synth.config("c0", n_topics=30_000)
    gm.build(f.blob, f.off)
    gm.set_debug(1)
    try:
        res = gm.match(t.blob, t.off, mode)
    finally:
        gm.set_debug(0)
    assert res.n_heavy == t.n
    o = OracleTrie(True, mode)
    o.add(f.blob, f.off)
    row, ids = o.match(t.blob, t.off, threads=8)
    assert np.array_equal(res.row_ptr, row)
    assert np.array_equal(canonical(res.row_ptr, res.ids), canonical(row, ids))
    assert res.visited == o.visited_counts(t.blob, t.off, threads=8)[0]   # k_heavy counts V_t too


@pytest.mark.parametrize("mode", MODES)
def test_walk_orders_vs_cpp_oracle(gm, mode, monkeypatch):
    """The walk's locality order (the key k_tokenise computes, the radix sort,
    the walk reading sorted topic records and fixed-stride words) and the
    output path (flush records chained per chunk, k_rec_burst) never change a
    result: several key shapes, input order, a partial last chunk, sorted +
    every chunk through k_heavy, and records of 1..40 entries in segments of
    64-100 u32 (every chunk's chain jumps between segments many times), all
    bit-exact against the C++ oracle (egm_kernels.hip launch_match)."""
    f, t = synth.config("c0", n_topics=70_001)
    gm.build(f.blob, f.off)
    monkeypatch.setenv("EGM_WALK_SORT_MIN_BYTES", "0")   # sort whatever the table size
    o = OracleTrie(True, mode)
    o.add(f.blob, f.off)
    row, ids = o.match(t.blob, t.off, threads=8)
    want = canonical(row, ids)
    for bits, debug, flush_at, seg in (("a86", 0, 320, 16384), ("8888", 0, 320, 16384), ("444", 0, 320, 16384),
                                       ("68a6", 0, 320, 16384), ("0", 0, 320, 16384), ("a86", 4, 320, 16384),
                                       ("a86", 1, 320, 16384), ("a86", 0, 1, 64), ("a86", 0, 7, 100),
                                       ("0", 0, 40, 64), ("a86", 1, 1, 64), ("8a86", 0, 300, 400)):
        monkeypatch.setenv("EGM_WALK_KEY", bits)   # key bits per level (hex nibbles, level 0 lowest)
        monkeypatch.setenv("EGM_FLUSH_AT", str(flush_at))   # staged emits per flush record
        monkeypatch.setenv("EGM_REC_SEG", str(seg))         # u32 per record segment
        gm.set_debug(debug)   # 4: EGM_DEBUG_INPUT_ORDER, 1: EGM_DEBUG_FORCE_HEAVY
        try:
            res = gm.match(t.blob, t.off, mode)
        finally:
            gm.set_debug(0)
        assert res.n_error == 0
        assert np.array_equal(res.row_ptr, row), (bits, debug, flush_at, seg)
        assert np.array_equal(canonical(res.row_ptr, res.ids), want), (bits, debug, flush_at, seg)


def ordered_to_input(row_w, topic, ids_w):
    """Rows in walk order (egm_match_device_ordered) -> the input-order CSR;
    asserts topic is a permutation."""
    n = len(topic)
    assert np.array_equal(np.sort(topic), np.arange(n, dtype=topic.dtype))
    cnt_w = np.diff(row_w.astype(np.int64))
    cnt = np.zeros(n, np.int64)
    cnt[topic] = cnt_w
    row = np.zeros(n + 1, np.uint64)
    row[1:] = np.cumsum(cnt)
    out = np.empty(int(row[-1]), np.uint32)
    for k in range(n):   # (small batches only)
        a, b = int(row_w[k]), int(row_w[k + 1])
        s = int(row[topic[k]])
        out[s:s + b - a] = ids_w[a:b]
    return row, out


@pytest.mark.parametrize("mode", MODES)
def test_device_ordered_vs_cpp_oracle(gm, mode, monkeypatch):
    """egm_match_device_ordered (rows in walk order + the row -> topic map,
    the bench's form): every topic's set equals the oracle's, sorted and
    input-order walks, the heavy path, short records with jumps."""
    import torch
    f, t = synth.config("c0", n_topics=40_003)
    gm.build(f.blob, f.off)
    monkeypatch.setenv("EGM_WALK_SORT_MIN_BYTES", "0")
    o = OracleTrie(True, mode)
    o.add(f.blob, f.off)
    row, ids = o.match(t.blob, t.off, threads=8)
    want = canonical(row, ids)
    dev = torch.device("cuda:0")
    d_blob = torch.from_numpy(t.blob).to(dev)
    d_off = torch.from_numpy(t.off.view(np.int32)).to(dev)
    n, cap = t.n, len(ids) + 1024
    for debug, flush_at, seg in ((0, 320, 16384), (4, 320, 16384), (1, 320, 16384), (0, 3, 64)):
        monkeypatch.setenv("EGM_FLUSH_AT", str(flush_at))
        monkeypatch.setenv("EGM_REC_SEG", str(seg))
        d_row = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_top = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_ids = torch.zeros(cap, dtype=torch.int32, device=dev)
        gm.set_debug(debug)
        try:
            gm.match_device_ordered(d_blob.data_ptr(), int(t.off[-1]), d_off.data_ptr(), n, mode, 0,
                                    d_row.data_ptr(), d_top.data_ptr(), d_ids.data_ptr(), cap)
            st = gm.last_stats()
        finally:
            gm.set_debug(0)
        assert st["overflow"] == 0 and st["errors"] == 0 and st["n_ids"] == len(ids)
        row_w = d_row.cpu().numpy().view(np.uint64)
        topic = d_top.cpu().numpy().view(np.uint32)
        ids_w = d_ids.cpu().numpy().view(np.uint32)[:len(ids)]
        if debug == 4:
            assert np.array_equal(topic, np.arange(n, dtype=np.uint32))   # input order: the identity map
        r2, i2 = ordered_to_input(row_w, topic, ids_w)
        assert np.array_equal(r2, row), (debug, flush_at)
        assert np.array_equal(canonical(r2, i2), want), (debug, flush_at)
    # too small: overflow reported, nothing written past the buffer
    gm.match_device_ordered(d_blob.data_ptr(), int(t.off[-1]), d_off.data_ptr(), n, mode, 0, d_row.data_ptr(),
                            d_top.data_ptr(), d_ids.data_ptr(), 16)
    assert gm.last_stats()["overflow"] != 0


@pytest.mark.parametrize("mode", MODES)
def test_config_c3_vs_cpp_oracle(gm, mode):
    """C3 shape at reduced size (depth-16 topics and filters,
    '+' p=.35, last-level '#' p=.7): deep chunks are walked as sub-chunks of
    staged words, and wide frontiers exercise the stack-overflow hand-off to
    k_heavy.  Bit-exact against the C++ oracle in both match modes."""
    f, t = synth.config("c3", n_filters=20_000, n_topics=20_000)
    gm.build(f.blob, f.off)
    res = gm.match(t.blob, t.off, mode)
    assert res.n_error == 0
    o = OracleTrie(True, mode)
    o.add(f.blob, f.off)
    row, ids = o.match(t.blob, t.off, threads=8)
    assert np.array_equal(res.row_ptr, row)
    assert np.array_equal(canonical(res.row_ptr, res.ids), canonical(row, ids))
    assert res.visited == o.visited_counts(t.blob, t.off, threads=8)[0]


def test_golden_fixture(gm):
    import gzip
    import json
    import os
    p = os.path.join(os.path.dirname(__file__), "golden", "c0_small.json.gz")
    with gzip.open(p, "rt") as fh:
        g = json.load(fh)
    filters = [x.encode() for x in g["filters"]]
    topics = [x.encode() for x in g["topics"]]
    gm.build_strings(filters)
    for mode, key in ((L.EGM_MODE_TRIE, "trie"), (L.EGM_MODE_ROUTES, "routes")):
        res = gm.match_strings(topics, mode)
        got = sets_of(res)
        assert got == [sorted(x) for x in g[key]], key


def test_device_api_matches_host_api(gm):
    import torch
    f, t = synth.config("c0", n_topics=50_000)
    gm.build(f.blob, f.off)
    host = gm.match(t.blob, t.off, L.EGM_MODE_TRIE)
    dev = torch.device("cuda:0")
    d_blob = torch.from_numpy(t.blob).to(dev)
    d_off = torch.from_numpy(t.off.view(np.int32)).to(dev)
    n = t.n
    cap = len(host.ids) + 1024
    d_row = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_ids = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_fl = torch.zeros(n, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    gm.match_device(d_blob.data_ptr(), int(t.off[-1]), d_off.data_ptr(), n, L.EGM_MODE_TRIE, s, d_row.data_ptr(),
                    d_ids.data_ptr(), cap, d_fl.data_ptr())
    st = gm.last_stats()
    assert st["overflow"] == 0 and st["n_ids"] == len(host.ids)
    row = d_row.cpu().numpy().view(np.uint64)
    ids = d_ids.cpu().numpy().view(np.uint32)[: len(host.ids)]
    assert np.array_equal(row, host.row_ptr)
    assert np.array_equal(canonical(row, ids), canonical(host.row_ptr, host.ids))
    assert np.array_equal(d_fl.cpu().numpy(), host.flags)
    # too-small capacity reports overflow instead of writing past the buffer
    gm.match_device(d_blob.data_ptr(), int(t.off[-1]), d_off.data_ptr(), n, L.EGM_MODE_TRIE, s, d_row.data_ptr(),
                    d_ids.data_ptr(), 16, 0)
    assert gm.last_stats()["overflow"] != 0


def _pack(items):
    return pack_strings(items)


@pytest.mark.parametrize("mode", MODES)
def test_incremental_commits_vs_cpp_oracle(gm, mode):
    """Route churn (emqx_router add/delete -> emqx_trie
    insert/delete, emqx_trie.erl:82-96): rounds of deletes + inserts, each
    committed incrementally (records patched into the idle device copy), are
    bit-exact against the C++ oracle mutated the same way, and a small delta
    moves a small fraction of the table."""
    pool = synth.filters(40_000, seed=0xE3C0_1234)
    pl = list(dict.fromkeys(pool.to_list()))
    assert len(pl) > 30_000
    f0 = list(range(10_000))
    gm.build(*_pack([pl[i] for i in f0]), np.array(f0, dtype=np.uint32))
    o = OracleTrie(True, mode)
    o.add(*_pack([pl[i] for i in f0]), np.array(f0, dtype=np.uint32))
    live = set(f0)
    nxt = 10_000
    t = synth.topics(20_000, pool, seed=0xE3C0_4321)
    rng = random.Random(mode)
    full_bytes = gm.stats()["device_bytes"]
    small = 0
    for rnd in range(8):
        dels = rng.sample(sorted(live), 300)
        ins = list(range(nxt, nxt + (300 if rnd < 6 else 3000)))   # the last rounds grow the table
        nxt = ins[-1] + 1
        gm.apply(inserts=[pl[i] for i in ins], deletes=[pl[i] for i in dels], insert_ids=ins)
        gm.commit()
        cs = gm.commit_stats()
        assert cs["patched"] > 0 or cs["h2d_bytes"] > 0, cs
        # the first commit after a build copies the other slot on the device;
        # a delta that rehashes the dictionary or edge table copies that array
        small += rnd >= 1 and cs["h2d_bytes"] < full_bytes // 10
        o.add(*_pack([pl[i] for i in ins]), np.array(ins, dtype=np.uint32))
        o.remove(*_pack([pl[i] for i in dels]))
        live.update(ins)
        live.difference_update(dels)
        res = gm.match(t.blob, t.off, mode)
        row, ids = o.match(t.blob, t.off, threads=8)
        assert np.array_equal(res.row_ptr, row), rnd
        assert np.array_equal(canonical(res.row_ptr, res.ids), canonical(row, ids)), rnd
    assert small >= 4, "small deltas should patch, not re-upload"
    # a rebuild of the same live set gives the same answers
    m2 = GpuMatcher(0)
    try:
        lv = sorted(live)
        m2.build(*_pack([pl[i] for i in lv]), np.array(lv, dtype=np.uint32))
        r2 = m2.match(t.blob, t.off, mode)
        assert np.array_equal(canonical(r2.row_ptr, r2.ids), canonical(res.row_ptr, res.ids))
    finally:
        m2.close()


def test_commit_waits_for_batches_in_flight(gm):
    """A batch enqueued on a caller stream keeps the epoch it started with:
    two commits later its device copy is rewritten only after it finished."""
    import torch
    f, t = synth.config("c0", n_topics=100_000)
    fl = f.to_list()
    gm.build(f.blob, f.off)
    host = gm.match(t.blob, t.off, L.EGM_MODE_ROUTES)
    dev = torch.device("cuda:0")
    d_blob = torch.from_numpy(t.blob).to(dev)
    d_off = torch.from_numpy(t.off.view(np.int32)).to(dev)
    n = t.n
    cap = len(host.ids) + 1024
    d_row = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_ids = torch.zeros(cap, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):   # queue several batches so the walk is still running
        gm.match_device(d_blob.data_ptr(), int(t.off[-1]), d_off.data_ptr(), n, L.EGM_MODE_ROUTES,
                        stream.cuda_stream, d_row.data_ptr(), d_ids.data_ptr(), cap, 0)
    gm.apply(deletes=fl[:5000])
    gm.commit()
    gm.apply(deletes=fl[5000:])
    gm.commit()          # writes the copy the queued batches read
    stream.synchronize()
    row = d_row.cpu().numpy().view(np.uint64)
    ids = d_ids.cpu().numpy().view(np.uint32)[: len(host.ids)]
    assert np.array_equal(row, host.row_ptr)
    assert np.array_equal(canonical(row, ids), canonical(host.row_ptr, host.ids))
    assert gm.empty()
    gone = gm.match(t.blob, t.off, L.EGM_MODE_ROUTES)
    assert len(gone.ids) == 0


def test_logical_shards_union(gm):
    """Filter sharding: union over shards == whole table."""
    f, t = synth.config("c0", n_topics=30_000)
    fl = f.to_list()
    G = 3
    from emqx_amd.dist import shard_of
    sh = shard_of(f, G)
    parts = []
    for g in range(G):
        idx = np.nonzero(sh == g)[0]
        m = GpuMatcher(0)
        blob, off = pack_strings([fl[i] for i in idx])
        m.build(blob, off, idx.astype(np.uint32))
        parts.append(m.match(t.blob, t.off, L.EGM_MODE_TRIE))
        m.close()
    gm.build(f.blob, f.off)
    whole = gm.match(t.blob, t.off, L.EGM_MODE_TRIE)
    from tests.shard_ref import merge_shard_results
    row, ids = merge_shard_results([(p.row_ptr, p.ids) for p in parts])
    assert np.array_equal(row, whole.row_ptr)
    assert np.array_equal(canonical(row, ids), canonical(whole.row_ptr, whole.ids))


def test_fanout_vs_oracle(gm):
    f, t = synth.config("c0", n_topics=20_000)
    gm.build(f.blob, f.off)
    res = gm.match(t.blob, t.off, L.EGM_MODE_ROUTES)
    assert len(res.ids) > 0
    row, subs = synth.subscribers(f.n, p_big=0.002, n_big=2000, p_share=0.1)
    gm.subs_build(row, subs)
    drow, dfid, dsub = gm.fanout(res)
    # oracle: per topic, the multiset of (filter, sub) over matched filters
    for i in range(0, t.n, 97):
        want = []
        for fid in res.row(i).tolist():
            want += [(fid, int(s)) for s in subs[row[fid]:row[fid + 1]]]
        got = list(zip(dfid[drow[i]:drow[i + 1]].tolist(), dsub[drow[i]:drow[i + 1]].tolist()))
        assert sorted(got) == sorted(want)
    assert drow[-1] == sum(int(row[x + 1] - row[x]) for x in res.ids.tolist())


def _expected_deliveries(mids, srow, subs):
    """emqx_broker:dispatch/2 order: per match entry, its filter's subscriber row."""
    mids = mids.astype(np.int64)
    cnt = (srow[mids + 1] - srow[mids]).astype(np.int64)
    fid = np.repeat(mids, cnt)
    starts = np.repeat(srow[mids].astype(np.int64) - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt)
    sub = subs[starts + np.arange(int(cnt.sum()))]
    return fid.astype(np.uint32), sub.astype(np.uint32)


@pytest.mark.parametrize("walk_sorted", [False, True])
def test_fanout_device_exact_and_guarded(gm, monkeypatch, walk_sorted):
    """Device fan-out (the bench's C4 step) element-for-element against numpy,
    with 1% of filters at 2 000 subscribers (windows of one wave spanning
    thousands of deliveries); an overflowed match batch is refused, not read.
    walk_sorted: the match sorts its batch (forced on this small table) and
    the fan-out counts in the match's walk order (k_fan_count_ord, A/B)."""
    import torch
    if walk_sorted:
        monkeypatch.setenv("EGM_WALK_SORT_MIN_BYTES", "0")
        monkeypatch.setenv("EGM_FAN_ORDER", "walk")
    f, t = synth.config("c1", n_filters=50_000, n_topics=30_000)
    gm.build(f.blob, f.off)
    srow, subs = synth.subscribers(f.n, p_big=0.01, n_big=2000, p_share=0.1)
    gm.subs_build(srow, subs)
    host = gm.match(t.blob, t.off, L.EGM_MODE_ROUTES)
    assert len(host.ids) > 0, gm.stats()
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    d_blob = torch.from_numpy(t.blob).to(dev)
    d_off = torch.from_numpy(t.off.view(np.int32)).to(dev)
    n, cap = t.n, len(host.ids) + 64
    d_row = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_ids = torch.zeros(cap, dtype=torch.int32, device=dev)
    gm.match_device(d_blob.data_ptr(), int(t.off[-1]), d_off.data_ptr(), n, L.EGM_MODE_ROUTES, s,
                    d_row.data_ptr(), d_ids.data_ptr(), cap)
    torch.cuda.synchronize()
    mrow = d_row.cpu().numpy().view(np.uint64)
    mids = d_ids.cpu().numpy().view(np.uint32)[: int(mrow[-1])]
    assert np.array_equal(mrow, host.row_ptr), (int(mrow[-1]), len(host.ids), gm.last_stats())
    want_fid, want_sub = _expected_deliveries(mids, srow, subs)
    tot = len(want_fid)
    assert tot > 100_000
    d_drow = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_fid = torch.zeros(tot + 8, dtype=torch.int32, device=dev)
    d_sub = torch.zeros(tot + 8, dtype=torch.int32, device=dev)
    gm.fanout_device(d_row.data_ptr(), d_ids.data_ptr(), cap, n, s, d_drow.data_ptr(), d_fid.data_ptr(),
                     d_sub.data_ptr(), tot + 8)
    torch.cuda.synchronize()
    drow = d_drow.cpu().numpy().view(np.uint64)
    cnt = (srow[mids.astype(np.int64) + 1] - srow[mids.astype(np.int64)]).astype(np.uint64)
    want_row = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)[mrow.astype(np.int64)]
    assert np.array_equal(drow, want_row)
    assert np.array_equal(d_fid.cpu().numpy().view(np.uint32)[:tot], want_fid)
    assert np.array_equal(d_sub.cpu().numpy().view(np.uint32)[:tot], want_sub)
    # the compact form: subscriber ids only + each match entry's first delivery
    d_pos = torch.zeros(len(mids) + 1, dtype=torch.int64, device=dev)
    d_sub2 = torch.zeros(tot + 8, dtype=torch.int32, device=dev)
    d_drow2 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    gm.fanout_device_compact(d_row.data_ptr(), d_ids.data_ptr(), cap, n, s, d_drow2.data_ptr(), d_pos.data_ptr(),
                             d_sub2.data_ptr(), tot + 8)
    torch.cuda.synchronize()
    assert np.array_equal(d_drow2.cpu().numpy().view(np.uint64), want_row)
    assert np.array_equal(d_pos.cpu().numpy().view(np.uint64), np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64))
    assert np.array_equal(d_sub2.cpu().numpy().view(np.uint32)[:tot], want_sub)
    assert gm.last_fanout() == {"deliveries": tot, "overflow": 0}
    # the host-buffer API gives the same rows
    hrow, hfid, hsub = gm.fanout(host)
    assert int(hrow[-1]) == tot
    # delivery buffer too small: nothing written past it, the total and every row still reported
    d_sub[1000:] = -7
    d_fid[1000:] = -7
    d_drow.zero_()
    gm.fanout_device(d_row.data_ptr(), d_ids.data_ptr(), cap, n, s, d_drow.data_ptr(), d_fid.data_ptr(),
                     d_sub.data_ptr(), 1000)
    torch.cuda.synchronize()
    assert int(d_drow[n].item()) == tot
    assert np.array_equal(d_drow.cpu().numpy().view(np.uint64), want_row)
    assert bool((d_sub[1000:] == -7).all()) and bool((d_fid[1000:] == -7).all())
    # an overflowed match batch (row total > id buffer) is refused before any kernel reads ids
    gm.match_device(d_blob.data_ptr(), int(t.off[-1]), d_off.data_ptr(), n, L.EGM_MODE_ROUTES, s,
                    d_row.data_ptr(), d_ids.data_ptr(), 16)
    with pytest.raises(L.EgmError):
        gm.fanout_device(d_row.data_ptr(), d_ids.data_ptr(), 16, n, s, d_drow.data_ptr(), d_fid.data_ptr(),
                         d_sub.data_ptr(), tot + 8)


@pytest.mark.slow
def test_full_size_c1_properties(gm):
    """C1 at full size: 1M filters x 10M topics.  Every one of the 10M rows
    against the C++ oracle as a SET — its count and an order-independent
    checksum of its ids (rows were compared by count) —
    200K sampled rows id-exact, determinism across runs."""
    f, t = synth.config("c1")
    gm.build(f.blob, f.off)
    a = gm.match(t.blob, t.off, L.EGM_MODE_ROUTES)
    b2 = gm.match(t.blob, t.off, L.EGM_MODE_ROUTES)
    assert np.array_equal(a.row_ptr, b2.row_ptr)
    # every row the same set in both runs: a per-row order-independent checksum
    # (the whole-batch canonical sort of 180M ids took ~20 s of the suite's budget)
    from tests.rowsum import row_checksums
    gsum = row_checksums(a.row_ptr, a.ids)
    assert np.array_equal(gsum, row_checksums(b2.row_ptr, b2.ids))
    o = OracleTrie(True, 1)
    o.add(f.blob, f.off)
    want, wsum = o.match_sums(t.blob, t.off, threads=16)
    got = np.diff(a.row_ptr).astype(np.uint32)
    bad = np.nonzero((got != want) | (gsum != wsum))[0]
    assert len(bad) == 0, (len(bad), [(int(i), int(got[i]), int(want[i])) for i in bad[:5]])
    rng = np.random.default_rng(5)
    idx = np.sort(rng.choice(t.n, 200_000, replace=False))
    sub = t.subset(idx)
    row, ids = o.match(sub.blob, sub.off, threads=16)
    got_row = np.zeros(len(idx) + 1, np.uint64)
    got_row[1:] = np.cumsum(np.diff(a.row_ptr)[idx])
    assert np.array_equal(got_row, row)
    got_ids = np.concatenate([a.row(int(i)) for i in idx])
    assert np.array_equal(canonical(got_row, got_ids), canonical(row, ids))
