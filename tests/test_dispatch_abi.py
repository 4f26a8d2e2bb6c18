"""The dispatch entry points (liveness bitmap, $share member table,
egm_dispatch_*) at the native boundary, without a device: the library exports
them, the ctypes binding and the header agree on them, and a call without a
context is refused.  (The argument errors that need a context — a triple in
both delta lists, a subscriber id with bit 31 set — need a device to open
one: tests/test_gpu_dispatch.py.)"""
import ctypes as C
import os
import re

from emqx_amd import _lib as L
from emqx_amd.broker import STRATEGIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("egm_subs_set_dead", "egm_share_build", "egm_share_apply_delta", "egm_share_commit", "egm_dispatch_device",
         "egm_dispatch_batch", "egm_last_dispatch", "egm_get_dispatch_timing")


def _header():
    with open(os.path.join(ROOT, "include", "emqx_gpu_match.h")) as fh:
        return fh.read()


def test_library_exports_the_dispatch_symbols():
    lib = L.load()
    h = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name


def test_pick_constants_mirror_the_strategies():
    h = _header()
    codes = {k.lower(): int(v) for k, v in re.findall(r"#define\s+EGM_PICK_(\w+)\s+(\d+)", h)}
    assert set(codes) == set(STRATEGIES)
    assert codes == L.PICK
    assert len(set(codes.values())) == len(codes)
    assert re.search(r"#define\s+EGM_SUB_NONE\s+0xFFFFFFFFu", h) and L.EGM_SUB_NONE == 0xFFFFFFFF


def test_structs_match_the_header_layout():
    assert C.sizeof(L.egm_dispatch) == 64          # u32 (+pad), 2 x u64, 5 pointers
    assert L.egm_dispatch.entry_pos.offset == 32 and L.egm_dispatch.entry_shared.offset == 56


def test_null_context_is_refused():
    lib = L.load()
    ids = (C.c_uint32 * 2)(1, 2)
    rows = (C.c_uint32 * 3)(0, 0, 1)
    out = C.POINTER(L.egm_dispatch)()
    assert lib.egm_subs_set_dead(None, ids, 2, 1) == L.EGM_E_INVAL
    assert lib.egm_share_build(None, rows, 1) == L.EGM_E_INVAL
    assert lib.egm_share_apply_delta(None, rows, 1, rows, 1) == L.EGM_E_INVAL
    assert lib.egm_share_commit(None, None) == L.EGM_E_INVAL
    assert lib.egm_dispatch_device(None, None, None, 0, 0, None, 0, 0, None, None, None, None, 0, None, None) == \
        L.EGM_E_INVAL
    assert lib.egm_dispatch_batch(None, None, None, 0, 0, C.byref(out)) == L.EGM_E_INVAL
    assert lib.egm_last_dispatch(None, None, None, None, None) == L.EGM_E_INVAL
    assert lib.egm_get_dispatch_timing(None, None, None) == L.EGM_E_INVAL


def test_nif_binds_the_dispatch_calls_on_dirty_schedulers():
    with open(os.path.join(ROOT, "c_src", "emqx_gpu_match_nif.c")) as fh:
        c = fh.read()
    with open(os.path.join(ROOT, "erl", "emqx_gpu_match.erl")) as fh:
        erl = fh.read()
    table = {name: (int(arity), flags) for name, arity, flags in re.findall(r'\{"(\w+)", (\d), nif_\w+, (\w+)\}', c)}
    exports = set()
    for group in re.findall(r"-export\(\[(.*?)\]\)", erl, re.S):
        exports |= set(re.findall(r"(\w+)/(\d+)", group))
    for name, arity in {"subs_set_dead": 3, "share_build": 2, "share_delta": 3, "dispatch_batch": 5}.items():
        assert table[name] == (arity, "ERL_NIF_DIRTY_JOB_CPU_BOUND"), name
        assert (name, str(arity)) in exports, name
        assert re.search(r"^%s\(%s\) -> erlang:nif_error" % (name, ", ".join(["_\\w*"] * arity)), erl, re.M), name
