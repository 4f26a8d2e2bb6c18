"""k_tokenise's slash map and its LDS shapes (egm_kernels.hip: TOK_SHAPES).

Pass 1 keeps each topic's '/' positions in a 128-bit map that starts at the
topic's first staged word; pass 2 walks the map, and a topic that overruns it
is rescanned — a choice per lane.  The staged bytes and words per block are
run-time capacities picked from the batch's mean topic length;
EGM_TOK_SHAPE=<index> pins one.  No input may change a result under any shape.

Every batch here is matched against oracle.cpp.OracleTrie id-exact (rows as
sorted sets, both modes) under each pinned shape and under the automatic pick,
each with a matcher of its own.  The batches sit where the kernel changes
path: topic lengths around 64 and 128 B with '/' at the map's word
boundaries, blocks exactly at, and just over, a shape's byte and word
capacity (computed here as the kernel computes them, and asserted), single
topics that fit no segment, batch means either side of the picker's
threshold, the sorted and the unsorted walk, and a padded slot.
"""
import os

import numpy as np
import pytest

from emqx_amd import _lib as L
from emqx_amd import synth
from emqx_amd.engine import GpuMatcher, pack_strings, unpack_strings
from oracle.cpp import OracleTrie, canonical

pytestmark = pytest.mark.gpu

MODES = [L.EGM_MODE_TRIE, L.EGM_MODE_ROUTES]
SHAPES = [(12288, 2296), (16256, 2528)]     # egm_kernels.hip TOK_SHAPES: staged bytes, words
MEAN_MAX = [40]                             # ... and the picker's thresholds, bytes per topic
BLOCK = 256                                 # TOK_BLOCK
SORT_MIN_TOPICS = 16384
SETTINGS = [None] + [str(k) for k in range(len(SHAPES))]   # EGM_TOK_SHAPE: unset (the pick), then each index


def topic(length, slashes=()):
    b = bytearray(b"a" * length)
    for p in slashes:
        b[p] = 0x2F
    return bytes(b)


def boundary_topics():
    """Lengths around the map's 64- and 128-bit edges x where the '/' are."""
    out = []
    for n in (0, 1, 63, 64, 65, 127, 128, 129):
        pats = [(), tuple(range(n))]                                  # no '/', all '/'
        if n:
            pats += [(0,), (n - 1,), (0, n - 1)]
        pats += [tuple(p for p in (63, 64) if p < n), tuple(p for p in (62, 63, 64, 65, 126, 127, 128) if p < n)]
        out += [topic(n, p) for p in pats]
    return sorted(set(out))


_FILTER_SET = []


def filter_set():
    """A few thousand C2-like filters (generated once)."""
    if not _FILTER_SET:
        _FILTER_SET.append(synth.filters(3000, 4, 8, 1.0, 0.15, 0.5, seed=synth.SEED_BASE + 77))
    return _FILTER_SET[0]


def short_topics(n, seed):
    """C2-like topics (4-8 levels of w{l}_{k}) over the module's filters."""
    t = synth.topics(n, filter_set(), 4, 8, seed=seed)
    return unpack_strings(t.blob, t.off)


def filters():
    fl = unpack_strings(filter_set().blob, filter_set().off)
    # one filter per level count (a topic's levels must be exact to match), some ending in '#', a literal at a depth
    fl += [b"/".join([b"+"] * k) for k in range(1, 12)] + [b"#", b"+/#", b"+/+/+/#", b"/#", b"a/+", b"+/a", b"+/+/a/#"]
    fl += [b"/".join([b"+"] * 8 + [b"a"]), b"/".join([b"+"] * 130)]
    # the boundary topics themselves: words of up to 129 B compared byte for byte in the dictionary
    fl += [t for t in boundary_topics() if t]
    seen, out = set(), []
    for f in fl:
        if f not in seen:
            seen.add(f)
            out.append(f)
    return out


def block_stats(topics):
    """Per block of 256: the staged span (ea - sa) and the words, as k_tokenise counts them."""
    off = np.zeros(len(topics) + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t in topics])
    out = []
    for b0 in range(0, len(topics), BLOCK):
        b1 = min(b0 + BLOCK, len(topics))
        span = ((off[b1] + 3) & ~3) - (off[b0] & ~3)
        out.append((int(span), sum(t.count(b"/") for t in topics[b0:b1]) + b1 - b0))
    return out


def bytes_block(total):
    """256 '/'-poor topics of `total` bytes in all (a block's span is total rounded up to 4 when it starts at 0)."""
    q, r = divmod(total, BLOCK)
    return [topic(q + (1 if k < r else 0), (1, 3)) for k in range(BLOCK)]


def words_block(words):
    """256 topics with `words` words in all, all of them one byte or empty."""
    q, r = divmod(words - BLOCK, BLOCK)
    return [topic(2 * (q + (1 if k < r else 0)) + 1, range(1, 2 * (q + (1 if k < r else 0)), 2)) for k in range(BLOCK)]


def build_batches():
    rng = np.random.default_rng(20240611)
    B = {}
    # bitmap boundary: every boundary topic twice among short ones, shuffled, so map lanes and rescan lanes share waves
    # and the topics start at every alignment
    mix = boundary_topics() * 2 + short_topics(700, 1)
    B["bitmap-boundary"] = [mix[i] for i in rng.permutation(len(mix))]
    tail = short_topics(50, 2)
    for k, (cb, cw) in enumerate(SHAPES):
        for d in (0, 1, 4):
            B["shape%d-bytes+%d" % (k, d)] = bytes_block(cb + d) + tail
        for d in (0, 1):
            B["shape%d-words+%d" % (k, d)] = words_block(cw + d) + tail
        # one topic longer than the shape's bytes among short ones: segments halve to one topic, then the lane path
        B["shape%d-long-topic" % k] = short_topics(100, 3) + [topic(cb + 40, (5, 9, cb))] + short_topics(200, 4)
        # one topic with more words than the shape holds (and fewer bytes): the second fallback
        B["shape%d-wordy-topic" % k] = short_topics(100, 5) + [topic(cw + 3, range(cw + 3))] + short_topics(200, 6)
    for m in MEAN_MAX:   # the picker: mean bytes per topic at the threshold, one byte over, and just below
        for d in (-1, 0, 1):
            B["mean%d%+d" % (m, d)] = [topic(m, (2, 7, 20))] * 511 + [topic(m + d, (2, 7, 20))]
    nine = b"/".join([b"a"] * 9)   # 9 levels: past FIX_WORDS, its word ids go to wid[] in a sorted batch
    B["unsorted"] = short_topics(3000, 7) + [nine] + boundary_topics()
    big = short_topics(SORT_MIN_TOPICS, 8) + [nine, topic(130, (64, 128))] + boundary_topics()
    B["sorted"] = [big[i] for i in rng.permutation(len(big))]
    return B


class Env:
    def __init__(self):
        self.filters = filters()
        self.fblob, self.foff = pack_strings(self.filters)
        self.batches = {k: (v,) + pack_strings(v) for k, v in build_batches().items()}
        self._want = {}

    def want(self, name, mode):
        """The oracle's (row_ptr, ids sorted within rows) of a batch: computed once."""
        if (name, mode) not in self._want:
            o = OracleTrie(True, mode)
            o.add(self.fblob, self.foff)
            _, blob, off = self.batches[name]
            row, ids = o.match(blob, off, threads=4)
            self._want[(name, mode)] = (row, canonical(row, ids))
        return self._want[(name, mode)]


@pytest.fixture(scope="module")
def E():
    return Env()


@pytest.fixture(scope="module", params=SETTINGS, ids=lambda s: "shape-%s" % (s if s is not None else "auto"))
def M(request, E):
    """A fresh matcher under one EGM_TOK_SHAPE setting (sorting whatever the table's size)."""
    keep = {k: os.environ.get(k) for k in ("EGM_TOK_SHAPE", "EGM_WALK_SORT_MIN_BYTES")}
    os.environ["EGM_WALK_SORT_MIN_BYTES"] = "0"
    if request.param is None:
        os.environ.pop("EGM_TOK_SHAPE", None)
    else:
        os.environ["EGM_TOK_SHAPE"] = request.param
    gm = GpuMatcher(0)
    gm.build(E.fblob, E.foff)
    yield gm
    gm.close()
    for k, v in keep.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def check_host(E, gm, name):
    _, blob, off = E.batches[name]
    for mode in MODES:
        res = gm.match(blob, off, mode)
        row, ids = E.want(name, mode)
        assert res.n_error == 0 and gm.last_guard() == 0, (name, mode)
        assert np.array_equal(res.row_ptr, row), (name, mode)
        assert np.array_equal(canonical(res.row_ptr, res.ids), ids), (name, mode)


def test_batches_sit_on_the_boundaries(E):
    """The inputs are what the cases below say they are (host arithmetic only)."""
    for k, (cb, cw) in enumerate(SHAPES):
        first = lambda name: block_stats(E.batches[name][0])[0]
        assert first("shape%d-bytes+0" % k)[0] == cb and first("shape%d-bytes+0" % k)[1] <= SHAPES[0][1]
        assert first("shape%d-bytes+1" % k)[0] == cb + 4 and first("shape%d-bytes+4" % k)[0] == cb + 4
        assert first("shape%d-words+0" % k)[1] == cw and first("shape%d-words+0" % k)[0] <= SHAPES[0][0]
        assert first("shape%d-words+1" % k)[1] == cw + 1
        # ... and one halving is enough: each half fits
        for name in ("shape%d-bytes+4" % k, "shape%d-words+1" % k):
            t = E.batches[name][0]
            for half in (t[:128], t[128:256]):
                assert all(s <= cb and w <= cw for s, w in block_stats(half))
        assert max(len(t) for t in E.batches["shape%d-long-topic" % k][0]) > cb
        wordy = max(E.batches["shape%d-wordy-topic" % k][0], key=len)
        assert wordy.count(b"/") + 1 > cw and len(wordy) + 4 <= cb
    for m in MEAN_MAX:
        for d in (-1, 0, 1):
            t = E.batches["mean%d%+d" % (m, d)][0]
            assert sum(len(x) for x in t) == m * len(t) + d
    lens = {len(t) for t in E.batches["bitmap-boundary"][0]}
    assert {0, 1, 63, 64, 65, 127, 128, 129} <= lens
    assert len(E.batches["sorted"][0]) >= SORT_MIN_TOPICS > len(E.batches["unsorted"][0])


def test_bitmap_boundary(E, M):
    check_host(E, M, "bitmap-boundary")


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_shape_boundary(E, M, k):
    """A block's bytes / words exactly at shape k's capacity, then over it by 1 (and 4 bytes)."""
    for name in ["shape%d-bytes+%d" % (k, d) for d in (0, 1, 4)] + ["shape%d-words+%d" % (k, d) for d in (0, 1)]:
        check_host(E, M, name)


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_topics_that_fit_no_segment(E, M, k):
    """Halving down to one topic, then the lane path from global memory (too long) / from LDS (too many words)."""
    check_host(E, M, "shape%d-long-topic" % k)
    check_host(E, M, "shape%d-wordy-topic" % k)


def test_picker_thresholds(E, M):
    for m in MEAN_MAX:
        for d in (-1, 0, 1):
            check_host(E, M, "mean%d%+d" % (m, d))


def test_unsorted_path(E, M):
    check_host(E, M, "unsorted")


def run_ordered(E, gm, name, mode):
    """egm_match_device_ordered -> (rows of the walk, row -> topic map, ids)."""
    import torch
    dev = torch.device("cuda:0")
    _, blob, off = E.batches[name]
    n = len(off) - 1
    row, ids = E.want(name, mode)
    cap = len(ids) + 1024
    d_blob, d_off = torch.from_numpy(blob).to(dev), torch.from_numpy(off.view(np.int32)).to(dev)
    d_row = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_top = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_ids = torch.zeros(cap, dtype=torch.int32, device=dev)
    gm.match_device_ordered(d_blob.data_ptr(), int(off[-1]), d_off.data_ptr(), n, mode, 0, d_row.data_ptr(),
                            d_top.data_ptr(), d_ids.data_ptr(), cap)
    st = gm.last_stats()
    assert st["overflow"] == 0 and st["errors"] == 0 and st["n_ids"] == len(ids), (name, st)
    return (d_row.cpu().numpy().view(np.uint64), d_top.cpu().numpy().view(np.uint32),
            d_ids.cpu().numpy().view(np.uint32)[:len(ids)])


def to_input_order(row_w, top, ids_w):
    n = len(top)
    assert np.array_equal(np.sort(top), np.arange(n, dtype=top.dtype))
    t = top.astype(np.int64)
    cnt_w = np.diff(row_w.astype(np.int64))
    cnt = np.zeros(n, np.int64)
    cnt[t] = cnt_w
    row = np.zeros(n + 1, np.int64)
    row[1:] = np.cumsum(cnt)
    out = np.empty(int(row[-1]), np.uint32)
    out[np.repeat(row[t] - row_w[:-1].astype(np.int64), cnt_w) + np.arange(len(ids_w), dtype=np.int64)] = ids_w
    return row.astype(np.uint64), out


def test_sorted_path(E, M):
    """n >= SORT_MIN_TOPICS: the fixed-stride words, the key and the record come from the tokeniser."""
    check_host(E, M, "sorted")
    for mode in MODES:
        row_w, top, ids_w = run_ordered(E, M, "sorted", mode)
        assert not np.array_equal(top, np.arange(len(top), dtype=top.dtype)), "the batch was not sorted"
        row, ids = to_input_order(row_w, top, ids_w)
        want_row, want_ids = E.want("sorted", mode)
        assert np.array_equal(row, want_row) and np.array_equal(canonical(row, ids), want_ids), mode


def test_walk_order_is_the_same_under_every_shape(E):
    """The sort's key and value are computed in the tokeniser: the walk-order map must not depend on the shape."""
    keep = {k: os.environ.get(k) for k in ("EGM_TOK_SHAPE", "EGM_WALK_SORT_MIN_BYTES")}
    maps = []
    try:
        os.environ["EGM_WALK_SORT_MIN_BYTES"] = "0"
        for s in SETTINGS:
            if s is None:
                os.environ.pop("EGM_TOK_SHAPE", None)
            else:
                os.environ["EGM_TOK_SHAPE"] = s
            gm = GpuMatcher(0)
            try:
                gm.build(E.fblob, E.foff)
                maps.append(run_ordered(E, gm, "sorted", L.EGM_MODE_ROUTES)[1])
            finally:
                gm.close()
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for m in maps[1:]:
        assert np.array_equal(m, maps[0])


@pytest.mark.parametrize("name,live", [("unsorted", 2500), ("sorted", SORT_MIN_TOPICS - 100)])
def test_padded_slot(E, M, name, live):
    """A slot of n topics of which `live` count: the rest are padding (TF_SKIP) with empty rows."""
    import torch
    dev = torch.device("cuda:0")
    _, blob, off = E.batches[name]
    n = len(off) - 1
    assert live < n
    hdr = torch.tensor([live, int(off[live]), 0, 0], dtype=torch.int32, device=dev)
    d_blob, d_off = torch.from_numpy(blob).to(dev), torch.from_numpy(off.view(np.int32)).to(dev)
    for mode in MODES:
        want_row, want_ids = E.want(name, mode)
        nids = int(want_row[live])
        d_row = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
        d_ids = torch.zeros(nids + 1024, dtype=torch.int32, device=dev)
        M.match_device_counted(d_blob.data_ptr(), int(off[-1]), d_off.data_ptr(), n, hdr.data_ptr(), mode, 0,
                               d_row.data_ptr(), d_ids.data_ptr(), d_ids.numel())
        st = M.last_stats()
        assert st["overflow"] == 0 and st["errors"] == 0 and st["n_ids"] == nids, (name, mode, st)
        row = d_row.cpu().numpy().view(np.uint64)
        ids = d_ids.cpu().numpy().view(np.uint32)[:nids]
        assert np.array_equal(row[:live + 1], want_row[:live + 1]) and np.all(row[live:] == nids), (name, mode)
        assert np.array_equal(canonical(row, ids), want_ids[:nids]), (name, mode)
