"""GPU parity over the '+'-children-first node layout (egm_common.h
NODE_LAYOUT_VERSION), at the smallest shapes that reach every reader of
nodes[]: k_walk's '+' record read and root read, k_heavy's, the ROUTES exact
lookup of a wildcard topic (nodes[] and hash_child[] at any node), and
k_patch writing records of nodes appended outside the dense region.  Every
case is compared with the C++ oracle as sets, in both match modes, through
egm_match_device (input-order rows) and egm_match_device_ordered (walk-order
rows + the row -> topic map)."""
import os

import numpy as np
import pytest

from emqx_amd import _lib as L
from emqx_amd import synth
from emqx_amd.engine import GpuMatcher, TableImage, pack_strings
from oracle.cpp import OracleTrie, canonical
from tests.test_gpu_parity import ordered_to_input

pytestmark = pytest.mark.gpu

MODES = [L.EGM_MODE_ROUTES, L.EGM_MODE_TRIE]
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def gm():
    m = GpuMatcher(0)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def sorted_walk(monkeypatch):
    monkeypatch.setenv("EGM_WALK_SORT_MIN_BYTES", "0")   # sort the batch whatever the table size


def build_bulk(gm, f, ids=None):
    """gm.build through the parallel bulk builder whatever the filter count."""
    old = os.environ.get("EGM_BULK_MIN")
    os.environ["EGM_BULK_MIN"] = "0"
    try:
        gm.build(f.blob, f.off, ids)
    finally:
        if old is None:
            del os.environ["EGM_BULK_MIN"]
        else:
            os.environ["EGM_BULK_MIN"] = old


def check_both_paths(gm, blob, off, want_row, want_ids, mode, debug=0):
    """egm_match_device and egm_match_device_ordered against the oracle's CSR."""
    import torch
    dev = torch.device("cuda:0")
    n, cap = len(off) - 1, len(want_ids) + 1024
    want = canonical(want_row, want_ids)
    d_blob = torch.from_numpy(blob).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(off, np.uint32).view(np.int32)).to(dev)
    for ordered in (False, True):
        d_row = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_top = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_ids = torch.zeros(cap, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        gm.set_debug(debug)
        try:
            if ordered:
                gm.match_device_ordered(d_blob.data_ptr(), int(off[-1]), d_off.data_ptr(), n, mode, 0,
                                        d_row.data_ptr(), d_top.data_ptr(), d_ids.data_ptr(), cap)
            else:
                gm.match_device(d_blob.data_ptr(), int(off[-1]), d_off.data_ptr(), n, mode, 0, d_row.data_ptr(),
                                d_ids.data_ptr(), cap)
            st = gm.last_stats()
            guard = gm.last_guard()
        finally:
            gm.set_debug(0)
        assert st["overflow"] == 0 and st["errors"] == 0 and guard == 0, (st, guard)
        assert st["n_ids"] == len(want_ids)
        if debug == L.EGM_DEBUG_FORCE_HEAVY:
            assert st["deferred_chunks"] > 0
        row = d_row.cpu().numpy().view(np.uint64)
        ids = d_ids.cpu().numpy().view(np.uint32)[:len(want_ids)]
        if ordered:
            row, ids = ordered_to_input(row, d_top.cpu().numpy().view(np.uint32), ids)
        assert np.array_equal(row, want_row), (mode, ordered, debug)
        assert np.array_equal(canonical(row, ids), want), (mode, ordered, debug)


def oracle_of(f, mode, ids=None):
    o = OracleTrie(True, mode)
    o.add(f.blob, f.off, ids)
    return o


_c0 = {}


def c0_case(mode):
    """The first-pass shape and its oracle result, computed once per mode."""
    if "ft" not in _c0:
        _c0["ft"] = synth.config("c0", n_filters=10_000, n_topics=20_000)
    f, t = _c0["ft"]
    if mode not in _c0:
        _c0[mode] = oracle_of(f, mode).match(t.blob, t.off, threads=8)
    return f, t, _c0[mode]


@pytest.mark.parametrize("mode", MODES)
def test_first_pass_bulk_built(gm, mode):
    f, t, (row, ids) = c0_case(mode)
    build_bulk(gm, f)
    check_both_paths(gm, t.blob, t.off, row, ids, mode)


@pytest.mark.parametrize("mode", MODES)
def test_heavy_path(gm, mode):
    f, t, (row, ids) = c0_case(mode)
    build_bulk(gm, f)
    check_both_paths(gm, t.blob, t.off, row, ids, mode, debug=L.EGM_DEBUG_FORCE_HEAVY)


@pytest.mark.parametrize("mode", MODES)
def test_deep_pass(gm, mode):
    """The C3 shape (depth 16, '+' p=.35): chains of '+' children inside the
    dense region; built by the insert loop + relayout."""
    f, t = synth.config("c3", n_filters=2_000, n_topics=2_000)
    gm.build(f.blob, f.off)
    row, ids = oracle_of(f, mode).match(t.blob, t.off, threads=8)
    assert len(ids) > 0
    check_both_paths(gm, t.blob, t.off, row, ids, mode)


@pytest.mark.parametrize("mode", MODES)
def test_deltas_append_outside_the_dense_region(gm, mode):
    """50 '+' filters added and 50 removed after the build, committed as a
    patch: the new '+' children are appended past the dense region (checked on
    a host image taken through the same builder and the same changes) and the
    walk reads their records there."""
    f, t, _ = c0_case(mode)
    fl = f.to_list()
    adds = [b"delta%d/+/x%d/+" % (k, k) for k in range(50)]
    add_ids = np.arange(1_000_000, 1_000_050, dtype=np.uint32)
    dels = [x for x in fl if b"+" in x.split(b"/")][::7][:50]
    assert len(dels) == 50
    build_bulk(gm, f)
    gm.apply(inserts=adds, deletes=dels, insert_ids=add_ids.tolist())
    gm.commit()
    # the same table on the host
    im = TableImage()
    im.bulk_build(f.blob, f.off)
    a0 = im.arrays()
    n0 = len(a0["nodes"])
    pc0 = a0["nodes"][:, 0]
    P = int(np.count_nonzero(pc0 != NONE))
    assert set(pc0[pc0 != NONE].tolist()) == set(range(1, P + 1)) and 0 < P < n0
    for x, i in zip(adds, add_ids.tolist()):
        assert im.insert(x, i) == 0
    for x in dels:
        assert im.remove(x) == 0
    pc1 = im.arrays()["nodes"][:, 0]
    new_plus = sorted(set(pc1[pc1 != NONE].tolist()) - set(pc0.tolist()))
    assert len(new_plus) == 100 and min(new_plus) >= n0 > P
    # topics that walk the appended records, among the batch
    extra = [b"delta%d/u/x%d/v" % (k, k) for k in range(50)] + [b"delta%d/u/x%d" % (k, k) for k in range(50)]
    topics = t.to_list() + extra
    tb, to = pack_strings(topics)
    o = oracle_of(f, mode)
    ab, ao = pack_strings(adds)
    o.add(ab, ao, add_ids)
    db, do = pack_strings(dels)
    o.remove(db, do)
    row, ids = o.match(tb, to, threads=8)
    hit = np.diff(row.astype(np.int64))[t.n:t.n + 50]
    assert np.all(hit >= 1)
    check_both_paths(gm, tb, to, row, ids, mode)
