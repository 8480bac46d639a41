"""The boundary of include/hgx_sibling.h: every function the header declares is exported by libhgx.so and bound
in hypergraphdb_amd._lib, hgx.h and hgx_linkpred.h do not grow, and the entry points refuse null arguments
without touching a device.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)                      # prose names other headers' functions
    return sorted(set(re.findall(r"\b(hgx_[a-z_]+)\s*\(", src)))


def test_sibling_abi_exported_and_bound():
    import hypergraphdb_amd
    from hypergraphdb_amd import _lib
    assert hypergraphdb_amd.AtomPredicate is hypergraphdb_amd.algorithms.AtomPredicate
    declared = header_symbols("hgx_sibling.h")
    assert declared == sorted(_lib.EXPORTED_SIBLING) and len(declared) == 8
    for other in ("hgx.h", "hgx_linkpred.h", "hgx_paths.h", "hgx_hops.h"):
        assert not set(declared) & set(header_symbols(other)), other      # an extension header: the others do not grow
    out = os.popen(f"nm -D --defined-only {os.path.join(ROOT, 'hypergraphdb_amd', 'libhgx.so')}").read()
    L = _lib.lib()
    for s in declared:
        assert re.search(rf"\sT {s}$", out, re.M), s
        assert getattr(L, s).argtypes is not None, s


def test_sibling_null_arguments_without_gpu():
    from hypergraphdb_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.hgx_graph_set_atom_types(None, None) == _lib.HGX_E_INVALID
    assert L.hgx_atom_predicate_create(None, 0, None, None, None, 0, C.byref(h)) == _lib.HGX_E_INVALID
    assert L.hgx_atom_predicate_create_mask(None, None, C.byref(h)) == _lib.HGX_E_INVALID
    assert L.hgx_atom_predicate_info(None, None, None, None, None) == _lib.HGX_E_INVALID
    assert b"null predicate" in L.hgx_last_error()
    assert L.hgx_atom_predicate_flags(None, 0, 0, None) == _lib.HGX_E_INVALID
    L.hgx_atom_predicate_free(None)
    seeds = np.zeros(1, np.int32)
    assert L.hgx_bfs_batch_sib(None, seeds.ctypes.data, 1, 1, None, None, None, C.byref(h)) == _lib.HGX_E_INVALID
    assert L.hgx_shortest_paths_sib(None, seeds.ctypes.data, seeds.ctypes.data, 1, None, None, None, None,
                                    C.byref(h)) == _lib.HGX_E_INVALID
