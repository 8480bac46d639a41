"""The boundary of include/hgx_sets.h: every function the header declares is exported by libhgx.so, unmangled, and
bound in hypergraphdb_amd._lib; the other headers do not grow; the entry points refuse null arguments without
touching a device.  No GPU compute."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)                      # prose names other headers' functions
    return sorted(set(re.findall(r"\b(hgx_[a-z_]+)\s*\(", src)))


def test_sets_abi_exported_and_bound():
    import hypergraphdb_amd
    from hypergraphdb_amd import _lib
    assert hypergraphdb_amd.VisitedSets is hypergraphdb_amd.algorithms.VisitedSets
    assert hypergraphdb_amd.reachable_batch is hypergraphdb_amd.algorithms.reachable_batch
    declared = header_symbols("hgx_sets.h")
    assert declared == sorted(_lib.EXPORTED_SETS) and len(declared) == 6
    for other in ("hgx.h", "hgx_linkpred.h", "hgx_paths.h", "hgx_hops.h", "hgx_sibling.h", "hgx_atoms.h"):
        assert not set(declared) & set(header_symbols(other)), other      # an extension header: the others do not grow
    out = os.popen(f"nm -D --defined-only {os.path.join(ROOT, 'hypergraphdb_amd', 'libhgx.so')}").read()
    L = _lib.lib()
    for s in declared:
        assert re.search(rf"\sT {s}$", out, re.M), s
        assert getattr(L, s).argtypes is not None, s
    src = open(os.path.join(ROOT, "include", "hgx_sets.h")).read()
    assert (_lib.HGX_SETS_DEPTHS, _lib.HGX_SETS_COUNT_ONLY) == (1, 2)
    assert re.search(r"#define HGX_SETS_DEPTHS\s+1\b", src) and re.search(r"#define HGX_SETS_COUNT_ONLY\s+2\b", src)


def test_sets_null_arguments_without_gpu():
    from hypergraphdb_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.hgx_bfs_result_sets(None, None, 0, 0, -1, None, 0, -1, C.byref(h)) == _lib.HGX_E_INVALID
    assert b"null result" in L.hgx_last_error()
    assert L.hgx_visited_sets_info(None, None, None, None) == _lib.HGX_E_INVALID
    assert L.hgx_visited_sets_offsets(None, None) == _lib.HGX_E_INVALID
    assert L.hgx_visited_sets_read(None, 0, 0, None, None) == _lib.HGX_E_INVALID
    assert L.hgx_visited_sets_stats(None, None, None, None, None) == _lib.HGX_E_INVALID
    L.hgx_visited_sets_free(None)
