"""The retained store's newer entry points at every boundary, without a GPU:
the header declares them, the built library exports them, the ctypes binding
knows them, and the NIF table lists every rs_* function with its stub's arity."""
import os
import re

from emqx_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS_NIFS = {"rs_open": 1, "rs_put": 4, "rs_delete": 2, "rs_delete_matching": 2,
           "rs_set_max_retained": 2, "rs_clean": 1, "rs_size": 1,
           "rs_commit": 1, "rs_clear_expired": 2, "rs_match": 4}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_header_declares_the_delete_and_the_limit():
    h = re.sub(r"/\*.*?\*/", "", _read("include", "emqx_gpu_match.h"), flags=re.S)
    assert re.search(r"int\s+egm_rstore_delete_matching\s*\(\s*egm_rstore\s*\*\s*\w+,\s*const\s+uint8_t\s*\*\s*\w+,"
                     r"\s*const\s+uint32_t\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*uint32_t\s*\*\*\s*\w+,"
                     r"\s*uint64_t\s*\*\s*\w+\)\s*;", h)
    assert re.search(r"int\s+egm_rstore_set_max_retained\s*\(\s*egm_rstore\s*\*\s*\w+,\s*uint64_t\s+\w+\)\s*;", h)
    codes = dict(re.findall(r"#define\s+(EGM_E_\w+)\s+\((-\d+)\)", h))
    assert "EGM_E_FULL" in codes
    assert len(set(codes.values())) == len(codes), codes          # beside the others: a code of its own
    assert int(codes["EGM_E_FULL"]) == L.EGM_E_FULL


def test_library_exports_the_delete_and_the_limit():
    lib = L.load()
    for name in ("egm_rstore_delete_matching", "egm_rstore_set_max_retained"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    # argument checks need no device: a null store is refused
    assert lib.egm_rstore_set_max_retained(None, 5) == L.EGM_E_INVAL
    assert lib.egm_rstore_delete_matching(None, None, None, 0, None, None) == L.EGM_E_INVAL


def test_nif_table_lists_every_rs_function_with_its_stub():
    c = _read("c_src", "emqx_gpu_match_nif.c")
    erl = _read("erl", "emqx_gpu_match.erl")
    table = {name: (int(arity), flags) for name, arity, flags in
             re.findall(r'\{"(rs_\w+)", (\d), nif_\w+, (\w+)\}', c)}
    assert {k: v[0] for k, v in table.items()} == RS_NIFS
    exports = set()
    for group in re.findall(r"-export\(\[(.*?)\]\)", erl, re.S):
        exports |= set(re.findall(r"(\w+)/(\d+)", group))
    for name, arity in RS_NIFS.items():
        assert (name, str(arity)) in exports, name
        assert re.search(r"^%s\(%s\) -> erlang:nif_error" % (name, ", ".join(["_\\w*"] * arity)), erl, re.M), name
    # whatever reaches the device runs on a dirty scheduler
    for name in ("rs_open", "rs_delete_matching", "rs_commit", "rs_clear_expired", "rs_match"):
        assert table[name][1] == "ERL_NIF_DIRTY_JOB_CPU_BOUND", name
    # every C-ABI call the shim makes is one the header declares
    h = _read("include", "emqx_gpu_match.h")
    for fn in set(re.findall(r"\b(egm_rstore_\w+)\s*\(", c)):
        assert re.search(r"\b%s\s*\(" % fn, h), fn
