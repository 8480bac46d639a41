"""CPU tests of the hop-path reference (tests/hop_ref.py) and of the hgx_hops.h boundary: with unit weights
the minimum-rank atom of the previous BFS level is the reference's final predecessorMatrix entry, and
libhgx.so exports and binds the new entry points.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np

import hop_ref as H
import kat_graphs as K
import sp_ref as R
from oracle_ctypes import OracleGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle(g):
    return OracleGraph(g["num_atoms"], np.asarray(g["link_atom"], np.int32), np.asarray(g["tgt_off"], np.int64),
                       np.asarray(g["tgt_idx"], np.int32),
                       None if g.get("link_type") is None else np.asarray(g["link_type"], np.int32))


def graphs():
    yield "linkage", K.linkage_graph(), None
    yield "queries", K.queries_graph(), None
    yield "pattern", K.pattern_graph(), None
    for seed in range(6):
        rng = np.random.default_rng(7000 + seed)
        yield f"random{seed}", K.random_graph(rng, 120, 260, max_arity=7, n_types=2), rng


def test_min_rank_of_previous_level_is_the_reference_predecessor():
    """hop_rule == sp_ref.dijkstra / dijkstra_heap with default weights and == sp_ref.rule_r: pred[n] for
    every reached atom, dm[n] == depth[n]; all five modes, typed and untyped."""
    entries, deepest = 0, 0
    for name, g, rng in graphs():
        orc = oracle(g)
        A = g["num_atoms"]
        starts = list(range(A)) if rng is None else rng.integers(0, A, 6).tolist()
        for mode in R.MODES.values():
            for lt in (-1, 1):
                opts = R.opts_of(mode, lt)
                gen = R.memo_generate(orc, opts)
                for s in starts:
                    depth, pred = H.hop_rule(gen, s)
                    if rng is None:
                        _, dm, rp, _ = R.dijkstra(orc, s, None, opts)
                    else:
                        _, dm, rp, _ = R.dijkstra_heap(gen, s, None)
                    assert set(dm) == set(depth), (name, mode, lt, s)
                    assert all(dm[n] == float(depth[n]) for n in dm), (name, mode, lt, s)
                    assert {n: k[0] for n, k in pred.items()} == rp, (name, mode, lt, s)
                    assert R.rule_r(gen, None, dm, s, list(dm)) == pred, (name, mode, lt, s)
                    for n in list(depth)[:: max(1, len(depth) // 5)]:
                        atoms, links = H.follow(pred, s, n)
                        R.check_path(gen, None, s, n, atoms, links, float(depth[n]))
                    entries += len(depth)
                    deepest = max(deepest, max(depth.values()))
    assert entries >= 10000 and deepest >= 8, (entries, deepest)


def test_max_depth_bounds_the_levels():
    g = K.queries_graph()
    gen = R.memo_generate(oracle(g), None)
    full, _ = H.hop_rule(gen, g["names"]["n4"])
    cut, pred = H.hop_rule(gen, g["names"]["n4"], 1)
    assert cut == {n: d for n, d in full.items() if d <= 1} and set(pred) == set(cut) - {g["names"]["n4"]}


def hops_header_symbols():
    src = open(os.path.join(ROOT, "include", "hgx_hops.h")).read()
    return sorted(set(re.findall(r"\b(hgx_[a-z_]+)\s*\(", src)))


def test_hops_abi_exported_and_bound():
    from hypergraphdb_amd import _lib
    declared = sorted(set(hops_header_symbols()) - set(_lib.EXPORTED))   # the header's comments may name hgx.h entries
    assert declared == sorted(_lib.EXPORTED_HOPS) and len(declared) >= 8
    out = os.popen(f"nm -D --defined-only {os.path.join(ROOT, 'hypergraphdb_amd', 'libhgx.so')}").read()
    L = _lib.lib()
    for s in declared:
        assert re.search(rf"\sT {s}$", out, re.M), s
        assert getattr(L, s).argtypes is not None, s


def test_hops_null_arguments_without_gpu():
    from hypergraphdb_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    one = np.zeros(1, np.int32)

    def invalid(rc, name):
        assert rc == _lib.HGX_E_INVALID
        assert name in L.hgx_last_error()

    invalid(L.hgx_bfs_result_paths(None, one.ctypes.data, one.ctypes.data, 1, C.byref(h)), b"hgx_bfs_result_paths")
    n, t = C.c_int32(), C.c_int64()
    invalid(L.hgx_hop_paths_info(None, C.byref(n), C.byref(t)), b"hgx_hop_paths_info")
    invalid(L.hgx_hop_paths_offsets(None, None, None), b"hgx_hop_paths_offsets")
    invalid(L.hgx_hop_paths_read(None, None, None), b"hgx_hop_paths_read")
    invalid(L.hgx_hop_paths_stats(None, None, None, None, None, None), b"hgx_hop_paths_stats")
    invalid(L.hgx_bfs_result_depth_row(None, 0, 0, 0, None), b"hgx_bfs_result_depth_row")
    invalid(L.hgx_bfs_result_predecessor_row(None, 0, 0, 0, None, None), b"hgx_bfs_result_predecessor_row")
    L.hgx_hop_paths_free(None)
