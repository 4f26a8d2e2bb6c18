"""The cluster-route entry points (egm_routes_*, egm_forward_*) at the native
boundary, without a device: the library exports them, the ctypes binding and
the header agree on them, and a call without a context is refused.  (The
argument errors that need a context — a node id past the limit, a pair in both
delta lists — need a device to open one: tests/test_gpu_forward.py.)"""
import ctypes as C
import os
import re

from emqx_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("egm_routes_build", "egm_routes_apply_delta", "egm_routes_commit", "egm_routes_last_commit",
         "egm_routes_drop_node", "egm_forward_device", "egm_forward_batch", "egm_last_forward",
         "egm_get_forward_timing")


def _header():
    with open(os.path.join(ROOT, "include", "emqx_gpu_match.h")) as fh:
        return fh.read()


def test_library_exports_the_forward_symbols():
    lib = L.load()
    h = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name


def test_node_limit_mirrors_the_header():
    m = re.search(r"#define\s+EGM_ROUTE_MAX_NODES\s+(\d+)", _header())
    assert m and int(m.group(1)) == L.EGM_ROUTE_MAX_NODES == 64


def test_structs_match_the_header_layout():
    assert C.sizeof(L.egm_route_pair) == 8 and L.egm_route_pair.node.offset == 4
    assert C.sizeof(L.egm_forward) == 64            # 2 x u32, 2 x u64, 5 pointers
    assert L.egm_forward.n_nodes.offset == 4 and L.egm_forward.n_forwards.offset == 16
    assert L.egm_forward.node_row.offset == 24 and L.egm_forward.topic_fwd.offset == 56
    h = _header()
    body = re.search(r"typedef struct egm_forward \{(.*?)\} egm_forward;", h, re.S).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f[0] for f in L.egm_forward._fields_]


def test_null_context_is_refused():
    lib = L.load()
    masks = (C.c_uint64 * 2)(1, 2)
    pairs = (C.c_uint32 * 2)(0, 1)
    out = C.POINTER(L.egm_forward)()
    ids, n = L._u32p(), C.c_uint64()
    assert lib.egm_routes_build(None, masks, 2, 0) == L.EGM_E_INVAL
    assert lib.egm_routes_apply_delta(None, pairs, 1, pairs, 1) == L.EGM_E_INVAL
    assert lib.egm_routes_commit(None, None) == L.EGM_E_INVAL
    assert lib.egm_routes_last_commit(None, None, None) == L.EGM_E_INVAL
    assert lib.egm_routes_drop_node(None, 1, C.byref(ids), C.byref(n)) == L.EGM_E_INVAL
    assert lib.egm_forward_device(None, None, None, 0, 0, None, None, None, None, 0, None, None) == L.EGM_E_INVAL
    assert lib.egm_forward_batch(None, None, C.byref(out)) == L.EGM_E_INVAL
    assert lib.egm_last_forward(None, None, None) == L.EGM_E_INVAL
    assert lib.egm_get_forward_timing(None, None, None) == L.EGM_E_INVAL


def test_nif_binds_the_route_calls_on_dirty_schedulers():
    with open(os.path.join(ROOT, "c_src", "emqx_gpu_match_nif.c")) as fh:
        c = fh.read()
    with open(os.path.join(ROOT, "erl", "emqx_gpu_match.erl")) as fh:
        erl = fh.read()
    table = {name: (int(arity), flags) for name, arity, flags in re.findall(r'\{"(\w+)", (\d), nif_\w+, (\w+)\}', c)}
    exports = set()
    for group in re.findall(r"-export\(\[(.*?)\]\)", erl, re.S):
        exports |= set(re.findall(r"(\w+)/(\d+)", group))
    for name, arity in {"routes_build": 3, "routes_delta": 3, "routes_drop_node": 2, "forward": 2}.items():
        assert table[name] == (arity, "ERL_NIF_DIRTY_JOB_CPU_BOUND"), name
        assert (name, str(arity)) in exports, name
        assert re.search(r"^%s\(%s\) -> erlang:nif_error" % (name, ", ".join(["_\\w*"] * arity)), erl, re.M), name
