"""The boundary of include/hgx_atoms.h: every function the header declares is exported by libhgx.so and bound in
hypergraphdb_amd._lib, the other headers do not grow, and the entry points refuse null arguments without touching
a device.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)                      # prose names other headers' functions
    return sorted(set(re.findall(r"\b(hgx_[a-z_]+)\s*\(", src)))


def test_atoms_abi_exported_and_bound():
    import hypergraphdb_amd
    from hypergraphdb_amd import _lib
    assert hypergraphdb_amd.pattern_batch_atoms is hypergraphdb_amd.query.pattern_batch_atoms
    declared = header_symbols("hgx_atoms.h")
    assert declared == sorted(_lib.EXPORTED_ATOMS) and len(declared) == 3
    for other, pinned in (("hgx.h", _lib.EXPORTED), ("hgx_join.h", _lib.EXPORTED_JOIN), ("hgx_scan.h", _lib.EXPORTED_SCAN),
                          ("hgx_sibling.h", _lib.EXPORTED_SIBLING), ("hgx_not.h", _lib.EXPORTED_NOT),
                          ("hgx_dnf.h", _lib.EXPORTED_DNF), ("hgx_linkpred.h", _lib.EXPORTED_LINKPRED),
                          ("hgx_paths.h", _lib.EXPORTED_PATHS), ("hgx_hops.h", _lib.EXPORTED_HOPS)):
        syms = header_symbols(other)
        assert not set(declared) & set(syms), other                       # an extension header: the others do not grow
        assert syms == sorted(pinned), other
    out = os.popen(f"nm -D --defined-only {os.path.join(ROOT, 'hypergraphdb_amd', 'libhgx.so')}").read()
    L = _lib.lib()
    for s in declared:
        assert re.search(rf"\sT {s}$", out, re.M), s
        assert getattr(L, s).argtypes is not None, s
    assert _lib.HGX_ATOMS_TYPE_SCAN == 1


def test_atoms_null_arguments_without_gpu():
    from hypergraphdb_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    one = np.zeros(1, np.int64)
    assert L.hgx_graph_type_atoms(None, None, 0, None) == _lib.HGX_E_INVALID
    assert b"hgx_graph_type_atoms" in L.hgx_last_error()
    args = [one.ctypes.data, None, None, one.ctypes.data] + [None] * 15
    assert L.hgx_pattern_batch_atoms(None, 0, *args, 0, 0, C.byref(h)) == _lib.HGX_E_INVALID
    assert b"hgx_pattern_batch_atoms" in L.hgx_last_error()
    assert L.hgx_query_result_atoms_stats(None, None, None, None, None, None) == _lib.HGX_E_INVALID
    assert b"null result" in L.hgx_last_error()
