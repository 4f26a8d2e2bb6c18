"""Path matrix: the boundary corpus (tests/corpus.py) through every path of
the match kernels — chunk sizes 4..64, sorted and input-order walks, the first
pass, the deep pass and k_heavy, input-order and walk-order rows, default and
short flush records, and a table patched by deltas.

Batches are assembled from the corpus's distinct topics by repetition; the
expected CSR is a numpy gather of the per-topic brute-force expectation
(oracle.trie_ref, the reference of record; tests/test_corpus.py ties it to
the C++ oracle and the walk emulator on the CPU).  Every cell checks row_ptr,
the ids of every row as a set, no duplicate id in a row, the wildcard flag,
n_error == 0, the walk guards, and `visited` against the C++ oracle's V_t
summed over the batch — hence identical in all cells of a batch.

Each cell prints its deep / deferred chunk counts (egm_last_walk_chunks) and,
for input-order walks, the most flush records a chunk needs (its expected ids
over the stage), so a run with -s shows which paths ran.
"""
import numpy as np
import pytest

from emqx_amd import _lib as L
from emqx_amd.engine import GpuMatcher, pack_strings
from oracle import trie_ref as R
from oracle.cpp import OracleTrie
from tests import corpus as K

pytestmark = pytest.mark.gpu

MODES = [L.EGM_MODE_TRIE, L.EGM_MODE_ROUTES]
HEAVY, INPUT = L.EGM_DEBUG_FORCE_HEAVY, L.EGM_DEBUG_INPUT_ORDER
DEEP_MIN, LIGHT_DMAX = 12, 440          # egm_kernels.hip: EGM_WALK_DEEP_MIN, light_dmax(504, 448)
SORT_MIN_TOPICS = 16384
DEFAULT_FLUSH = (None, None)            # EGM_FLUSH_AT, EGM_REC_SEG unset: the default stage and segments


def chunk_topics(n):
    """walk_chunk_topics (egm_kernels.h): topics per chunk for a batch of n."""
    ct = 64
    while ct > 4 and n < ct * 2048:
        ct >>= 1
    return ct


class Env:
    def __init__(self, build=True):
        self.c = K.build()
        self.ref = K.reference()
        blob, off = pack_strings(self.c.topics)
        self.vt = {}
        for mode in MODES:
            o = OracleTrie(True, mode)
            o.add(*pack_strings(self.c.filters))
            self.vt[mode] = o.visited_counts(blob, off, threads=4)[1].astype(np.int64)
        self.wild = np.array([R.wildcard(t) for t in self.c.topics])
        self.gm = GpuMatcher(0)
        if build:
            self.gm.build_strings(self.c.filters)
        self.visited = {}    # (batch name, mode) -> visited of its first cell

    def pool(self, max_depth, *families):
        c = self.c
        idx = [i for i in range(len(c.topics)) if c.depth[i] <= max_depth
               and (not families or c.tags[i].split(":")[0] in families)]
        return np.array(idx, np.int64)


@pytest.fixture(scope="module")
def X():
    x = Env()
    yield x
    x.gm.close()


def sorted_keys(row, ids):
    """(row << 32 | id) of every entry, sorted: the ids of each row as a set, in row order."""
    import torch
    rid = np.repeat(np.arange(len(row) - 1, dtype=np.int64), np.diff(row.astype(np.int64)))
    key = (rid << 32) | ids.astype(np.int64)
    if len(key) < 100_000:
        return np.sort(key)
    return torch.sort(torch.from_numpy(key).to("cuda:0")).values.cpu().numpy()


def ordered_to_input(row_w, topic, ids_w):
    """Rows in walk order (egm_match_device_ordered) -> the input-order CSR
    (tests/test_gpu_parity.py ordered_to_input, vectorised)."""
    n = len(topic)
    assert np.array_equal(np.sort(topic), np.arange(n, dtype=topic.dtype))
    t = topic.astype(np.int64)
    cnt_w = np.diff(row_w.astype(np.int64))
    cnt = np.zeros(n, np.int64)
    cnt[t] = cnt_w
    row = np.zeros(n + 1, np.int64)
    row[1:] = np.cumsum(cnt)
    out = np.empty(int(row[-1]), np.uint32)
    dst = np.repeat(row[t] - row_w[:-1].astype(np.int64), cnt_w) + np.arange(len(ids_w), dtype=np.int64)
    out[dst] = ids_w
    return row.astype(np.uint64), out


def set_flush(monkeypatch, flush):
    for name, v in zip(("EGM_FLUSH_AT", "EGM_REC_SEG"), flush):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


class Batch:
    """One batch: the distinct topics idx[k], packed once, with its expectation per mode."""

    def __init__(self, X, name, idx, ref=None, vt=None):
        self.X, self.name, self.idx = X, name, np.asarray(idx, np.int64)
        self.n = len(self.idx)
        self.blob, self.off = K.pack(X.c, self.idx)
        self.ref = ref or X.ref
        self.vt = vt or X.vt
        self.want = {}
        self.dev = None

    def expect(self, mode):
        if mode not in self.want:
            row, ids = self.ref.gather(mode, self.idx)
            rid = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(row.astype(np.int64)))
            self.want[mode] = (row, (rid << 32) | ids.astype(np.int64), int(self.vt[mode][self.idx].sum()))
        return self.want[mode]

    def host_chunks(self):
        """Input-order walk: chunks for the deep pass / for k_heavy, and the
        most flush records one chunk needs (its ids / the stage)."""
        ct = chunk_topics(self.n)
        pad = (-self.n) % ct
        d = np.concatenate([self.X.c.depth[self.idx], np.zeros(pad, np.int64)]).reshape(-1, ct).max(axis=1)
        return int(np.count_nonzero((d > DEEP_MIN) & (d <= LIGHT_DMAX))), int(np.count_nonzero(d > LIGHT_DMAX))

    def max_records(self, mode, stage=K.STAGE):
        ct = chunk_topics(self.n)
        cnt = self.ref.count(mode)[self.idx]
        cnt = np.concatenate([cnt, np.zeros((-self.n) % ct, np.int64)]).reshape(-1, ct).sum(axis=1)
        return int(-(-cnt.max() // stage))

    def check(self, mode, row, ids, what, flags=None, visited=None, n_error=0, stats=None):
        """Everything a cell asserts; `stats`: walk_chunks() of the run."""
        X = self.X
        want_row, want_keys, want_vt = self.expect(mode)
        assert n_error == 0, what
        assert X.gm.last_guard() == 0, what
        assert np.array_equal(row, want_row), what
        got = sorted_keys(row, ids)
        assert np.all(np.diff(got) != 0), ("duplicate id in a row", what)
        bad = np.nonzero(got != want_keys)[0]
        assert len(bad) == 0, (what, len(bad), X.c.topics[self.idx[int(got[bad[0]] >> 32)]][:60])
        if flags is not None:
            assert np.array_equal((flags & L.EGM_TF_WILDCARD) != 0, X.wild[self.idx]), what
        if visited is not None:
            assert visited == want_vt, (what, visited, want_vt)
            assert X.visited.setdefault((self.name, mode), visited) == visited, what   # the same in every cell
        print("PATH-MATRIX %s mode=%d %s n=%d ids=%d deep=%s deferred=%s max_records_per_chunk(input order)=%d" % (
            self.name, mode, what, self.n, len(ids), stats and stats["deep"], stats and stats["deferred"],
            self.max_records(mode)))

    def run_host(self, mode, debug, what, monkeypatch, sort=True, key="a86", flush=DEFAULT_FLUSH):
        """egm_match_batch.  Returns walk_chunks()."""
        gm = self.X.gm
        if sort:
            monkeypatch.setenv("EGM_WALK_SORT_MIN_BYTES", "0")   # sort whatever the table size
        else:
            monkeypatch.delenv("EGM_WALK_SORT_MIN_BYTES", raising=False)
        monkeypatch.setenv("EGM_WALK_KEY", key)
        set_flush(monkeypatch, flush)
        gm.set_debug(debug)
        try:
            res = gm.match(self.blob, self.off, mode)
            st = gm.walk_chunks()
        finally:
            gm.set_debug(0)
        if debug & HEAVY:
            assert res.n_heavy == self.n and st["deferred"] == -(-self.n // chunk_topics(self.n)), what
        elif (debug & INPUT) or self.n < SORT_MIN_TOPICS:
            assert (st["deep"], st["deferred"]) == self.host_chunks(), what
        self.check(mode, res.row_ptr, res.ids, what, res.flags, res.visited, res.n_error, st)
        return st

    def run_device(self, mode, debug, what, monkeypatch, ordered, flush=DEFAULT_FLUSH):
        """egm_match_device / egm_match_device_ordered on device buffers."""
        import torch
        gm = self.X.gm
        dev = torch.device("cuda:0")
        if self.dev is None:
            self.dev = (torch.from_numpy(self.blob).to(dev), torch.from_numpy(self.off.view(np.int32)).to(dev))
        d_blob, d_off = self.dev
        n, nids = self.n, int(self.expect(mode)[0][-1])
        cap = nids + 1024
        monkeypatch.setenv("EGM_WALK_SORT_MIN_BYTES", "0")
        monkeypatch.setenv("EGM_WALK_KEY", "a86")
        set_flush(monkeypatch, flush)
        d_row = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_ids = torch.zeros(cap, dtype=torch.int32, device=dev)
        d_top = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_fl = torch.zeros(n, dtype=torch.uint8, device=dev)
        gm.set_debug(debug)
        try:
            if ordered:
                gm.match_device_ordered(d_blob.data_ptr(), int(self.off[-1]), d_off.data_ptr(), n, mode, 0,
                                        d_row.data_ptr(), d_top.data_ptr(), d_ids.data_ptr(), cap)
            else:
                gm.match_device(d_blob.data_ptr(), int(self.off[-1]), d_off.data_ptr(), n, mode, 0, d_row.data_ptr(),
                                d_ids.data_ptr(), cap, d_fl.data_ptr())
            st = gm.last_stats()
            wc = gm.walk_chunks()
        finally:
            gm.set_debug(0)
        assert st["overflow"] == 0 and st["n_ids"] == nids, (what, st)
        row = d_row.cpu().numpy().view(np.uint64)
        ids = d_ids.cpu().numpy().view(np.uint32)[:nids]
        flags = None
        if ordered:
            topic = d_top.cpu().numpy().view(np.uint32)
            if debug & INPUT:
                assert np.array_equal(topic, np.arange(n, dtype=np.uint32)), what
            row, ids = ordered_to_input(row, topic, ids)
        else:
            flags = d_fl.cpu().numpy()
        if (debug & INPUT) and not (debug & HEAVY):
            assert (wc["deep"], wc["deferred"]) == self.host_chunks(), what
        self.check(mode, row, ids, what, flags, st["visited"], st["errors"], wc)
        return wc


# ---------------------------------------------------------------- chunk-size ladder ----
def capped(X, idx, cap=256):
    """At most `cap` copies of the fan-out topic and of its 8-level prefix (the rest become 'a')."""
    idx = idx.copy()
    for t in (K.J(K.FAN_TOPIC), K.J(K.FAN_TOPIC[:-1])):
        at = np.nonzero(idx == X.c.t(t))[0]
        idx[at[cap:]] = X.c.t(b"a")
    return idx


@pytest.mark.parametrize("n", [3, 16_383, 16_384, 32_767, 32_768, 65_536, 131_071, 131_073])
def test_chunk_size_ladder(X, n, monkeypatch):
    """walk_chunk_topics(n) changes at 16 384, 32 768, 65 536 and 131 072 and
    the sort starts at 16 384: the corpus up to 57 levels tiled to each size
    just below, at or above, sorted and in input order."""
    assert [chunk_topics(k) for k in (3, 16_383, 16_384, 32_767, 32_768, 65_536, 131_071, 131_073)] == \
        [4, 4, 8, 8, 16, 32, 32, 64]
    pool = X.pool(57)
    b = Batch(X, "ladder-n%d" % n, capped(X, K.tile(pool, n)) if n > 3 else
              np.array([X.c.t(K.J(K.FAN_TOPIC)), X.c.t(b"a/+"), X.c.t(K.J(K.ladder_words(13, 0)))]))
    for mode in MODES:
        st = b.run_host(mode, 0, "sorted", monkeypatch)
        b.run_host(mode, INPUT, "input-order", monkeypatch)
        assert st["deferred"] == 0 and st["deep"] > 0


# ---------------------------------------------------------------- depth ladder ----
@pytest.mark.parametrize("mode", MODES)
def test_depth_ladder(X, mode, monkeypatch):
    """Every ladder depth up to 440 in one batch: the first pass (S = 64 up to
    7 levels, 32 from 8), the deep pass from 13 levels (S halving at 14/15,
    28/29, 56/57, 112/113, 224/225) and nothing deferred: 440 levels is the
    deepest chunk the deep pass takes (light_dmax(504, 448) = 440).  With the
    441- and 442-level topics added, their chunks go to k_heavy."""
    pool = X.pool(LIGHT_DMAX)
    assert set(K.LADDER) - {441} <= set(X.c.depth[pool].tolist()) and X.c.depth[pool].max() == 440
    # each depth class fills whole chunks: every topic 128 times in a row, chunks of 8
    by_depth = pool[np.argsort(X.c.depth[pool], kind="stable")]
    whole = Batch(X, "depth-whole", np.repeat(by_depth, 128))
    assert whole.n >= SORT_MIN_TOPICS and chunk_topics(whole.n) == 8
    deep, deferred = whole.host_chunks()
    assert deferred == 0 and deep == 16 * int(np.count_nonzero(X.c.depth[pool] > DEEP_MIN))
    st = whole.run_host(mode, INPUT, "input-order", monkeypatch)
    assert (st["deep"], st["deferred"]) == (deep, 0)
    mixed = Batch(X, "depth-shuffled", K.tile(pool, SORT_MIN_TOPICS))
    st = mixed.run_host(mode, 0, "sorted-a86", monkeypatch)
    assert st["deferred"] == 0 and st["deep"] > 0
    st = mixed.run_host(mode, INPUT, "input-order", monkeypatch)
    assert st["deferred"] == 0 and st["deep"] > 0
    # ... plus the topics of more than 440 levels: their chunks are deferred, every topic still exact
    over = X.pool(10 ** 6)
    assert X.c.depth[over].max() == 442 and 441 in X.c.depth[over]
    heavy = Batch(X, "depth-441", K.tile(over, SORT_MIN_TOPICS))
    st = heavy.run_host(mode, 0, "sorted-a86", monkeypatch)
    assert st["deferred"] > 0 and st["deep"] > 0
    st = heavy.run_host(mode, INPUT, "input-order", monkeypatch)
    assert st["deferred"] > 0 and st["deep"] > 0


# ---------------------------------------------------------------- mixed chunks ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deep", [False, True])
def test_mixed_chunks(X, deep, mode, monkeypatch):
    """Every chunk of 64 interleaves 1-, 8-, 9- and 12-level topics, wildcard,
    '$', empty-word and zero-match topics and the fan-out topic (> 1 500
    ids); every 128th chunk carries 24 copies of it, more ids than REC_DIR
    flush records of the default stage hold, so its records continue along
    the chain.  Without a 13-level topic the chunks stay in the first pass,
    with one they all go to the deep pass.  Through egm_match_device and
    egm_match_device_ordered, at the default stage and with records of 1 and 7
    entries in segments of 64 u32."""
    b = Batch(X, "mixed-deep%d" % deep, K.mixed_batch(X.c, deep))
    assert chunk_topics(b.n) == 64
    assert b.max_records(mode) > K.REC_DIR      # the condition of this cell: a chunk's ids / the stage > REC_DIR
    assert b.host_chunks() == (2048 if deep else 0, 0)
    for flush in (DEFAULT_FLUSH, (1, 64), (7, 64)):
        for ordered in (False, True):
            wc = b.run_device(mode, INPUT, "input-order ordered=%d flush=%s" % (ordered, flush[0]), monkeypatch,
                              ordered, flush)
            assert (wc["deep"], wc["deferred"]) == (2048 if deep else 0, 0)


# ---------------------------------------------------------------- neighbour bait ----
def bait_batch(X, n_chunks=2048):
    """Chunks of 64 in input order, each 32 x (bait topic, its neighbour) of
    one depth, so the chunk's dmax is the bait's depth and the neighbour's
    words lie directly behind the bait's in the LDS word stage."""
    c = X.c
    chunks = []
    for dmax in K.BAIT_DMAX:
        pairs = [p for p in c.bait_pairs if c.depth[p[0]] == dmax]
        assert pairs and all(c.depth[nb] <= dmax for _, nb in pairs)
        chunks.append(np.array([x for k in range(32) for x in pairs[k % len(pairs)]], np.int64))
    return np.concatenate([chunks[k % len(chunks)] for k in range(n_chunks)])


@pytest.mark.parametrize("mode", MODES)
def test_neighbour_bait(X, mode, monkeypatch):
    """The '+' skip reads the words at level + 1 and + 2 unclamped from the
    word stage: for a topic of D == dmax levels they are the next topic's
    first words.  Filters that would match if those were the topic's own
    levels D and D + 1 must stay out (and the topic's own matches in)."""
    b = Batch(X, "bait", bait_batch(X))
    assert b.n == 131_072 and chunk_topics(b.n) == 64
    st = b.run_host(mode, INPUT, "input-order", monkeypatch)
    assert (st["deep"], st["deferred"]) == (0, 0)
    b.run_host(mode, INPUT | HEAVY, "input-order forced-heavy", monkeypatch)
    b.run_host(mode, 0, "sorted-a86", monkeypatch)


# ---------------------------------------------------------------- wildcard and '$' topics ----
def special_pool(X, max_depth):
    c = X.c
    lad = [c.t(K.J(K.ladder_words(D, v))) for D in (1, 2, 7, 8, 9, 12, 13) for v in (0, 1)]
    fam = X.pool(max_depth, "wild", "dollar", "empty", "zero", "unknown", "fanout8")
    return np.unique(np.concatenate([fam, np.array(lad, np.int64)]))


@pytest.mark.parametrize("mode", MODES)
def test_wildcard_and_dollar_topics_on_every_path(X, mode, monkeypatch):
    """Wildcard publish topics (ROUTES: exact_walk, the reader of
    hash_child[]; TRIE: nothing), '$' topics (root_flags, the one-word '$'
    probe), empty words, zero-match topics and unknown words: sorted (fixed-
    stride words up to 8 levels, wid[] from 9), input order, the deep pass
    (the 13-level ones), k_heavy (the 441-level ones, and every chunk
    forced), input-order and walk-order rows."""
    b = Batch(X, "special", K.tile(special_pool(X, LIGHT_DMAX), SORT_MIN_TOPICS))
    fams = {X.c.tags[i].split(":")[0] for i in b.idx}
    assert fams >= {"wild", "dollar", "empty", "zero", "unknown"}
    assert {9, 13} <= set(X.c.depth[b.idx[X.wild[b.idx]]].tolist())
    st = b.run_host(mode, 0, "sorted-a86", monkeypatch)
    assert st["deep"] > 0 and st["deferred"] == 0
    st = b.run_host(mode, INPUT, "input-order", monkeypatch)
    assert st["deep"] > 0 and st["deferred"] == 0
    b.run_host(mode, HEAVY, "sorted forced-heavy", monkeypatch)
    b.run_host(mode, 0, "sorted short-records", monkeypatch, flush=(7, 64))
    b.run_device(mode, 0, "sorted ordered-rows", monkeypatch, True)
    b.run_device(mode, INPUT, "input-order ordered-rows", monkeypatch, True)
    b.run_device(mode, HEAVY, "sorted forced-heavy ordered-rows", monkeypatch, True)
    b.run_device(mode, 0, "sorted device-rows", monkeypatch, False)
    # with the 441-level wildcard topics: their chunks go to k_heavy on their own
    h = Batch(X, "special-441", K.tile(special_pool(X, 10 ** 6), SORT_MIN_TOPICS))
    assert 441 in X.c.depth[h.idx[X.wild[h.idx]]]
    for debug, what in ((0, "sorted-a86"), (INPUT, "input-order")):
        st = h.run_host(mode, debug, what, monkeypatch)
        assert st["deferred"] > 0 and st["deep"] > 0
    wc = h.run_device(mode, 0, "sorted ordered-rows", monkeypatch, True)
    assert wc["deferred"] > 0


# ---------------------------------------------------------------- after deltas ----
def test_after_deltas(monkeypatch):
    """The table built from half of the filters, the rest applied as one
    epoch; then the '#'- and '+'-ending filters of the wildcard family deleted
    (checked against a brute force over the remaining filters) and inserted
    again under their ids: that patches hash_child[], a '+' child outside the
    dense region and the edge slots' child_pflags.  The wildcard, '$' and bait
    cells rerun after each of the commits that follow, so on both device
    copies."""
    x = Env(build=False)   # its own matcher: the module's table stays as built
    full = x.c
    blob, off = pack_strings(full.topics)
    fl, ids = full.filters, np.arange(len(full.filters), dtype=np.uint32)
    try:
        x.gm.build_strings(fl[::2], ids[::2])
        x.gm.apply(inserts=fl[1::2], insert_ids=ids[1::2].tolist())
        x.gm.commit()
        special = K.tile(special_pool(x, 10 ** 6), SORT_MIN_TOPICS)
        bait = bait_batch(x)

        def cells(tag, ref=None, vt=None):
            for name, idx in (("special", special), ("bait", bait)):
                b = Batch(x, "delta-%s-%s" % (tag, name), idx, ref, vt)
                for mode in MODES:
                    b.run_host(mode, INPUT, "input-order", monkeypatch)
                    if name == "special":
                        b.run_host(mode, 0, "sorted-a86", monkeypatch)
                        b.run_device(mode, 0, "sorted ordered-rows", monkeypatch, True)

        cells("applied")
        # delete the wildcard family's '#'- and '+'-ending filters
        gone = [full.topics[i] for i in full.wild_present if full.topics[i][-1:] in (b"#", b"+")]
        assert len(gone) >= 8 and {b"+", b"#", b"a/+", b"a/#", b"a/+/#", b"+/+/+"} <= set(gone)
        gone_ids = [fl.index(f) for f in gone]
        x.gm.apply(deletes=gone)
        x.gm.commit()
        # the expectation without them: brute force over the remaining filters, for the topics of these cells
        keep = [f for f in fl if f not in set(gone)]
        fid = {f: i for i, f in enumerate(fl)}
        used = np.unique(np.concatenate([special, bait]))
        sets = {0: [[] for _ in full.topics], 1: [[] for _ in full.topics]}
        for i in used:
            sets[0][i] = sorted(fid[f] for f in R.trie_semantics(full.topics[i], keep))
            sets[1][i] = sorted(fid[f] for f in R.routes_semantics(full.topics[i], keep))
        vt = {}
        for mode in MODES:
            o = OracleTrie(True, mode)
            o.add(*pack_strings(keep))
            vt[mode] = o.visited_counts(blob, off, threads=4)[1].astype(np.int64)
        cells("deleted", K.Reference(sets, 0.0), vt)
        # insert them again under their ids: the full expectation holds again, on this device copy ...
        x.gm.apply(inserts=gone, insert_ids=gone_ids)
        x.gm.commit()
        cells("reinserted")
        # ... and, after one more delete + insert of the same filters in one epoch, on the other
        x.gm.apply(deletes=gone)
        x.gm.apply(inserts=gone, insert_ids=gone_ids)
        x.gm.commit()
        cells("second-copy")
    finally:
        x.gm.close()
