"""CPU tests of the shortest-path reference (tests/sp_ref.py) and of the hgx_paths.h boundary: the
restatement reproduces the reference's own known answers, the exactness and rule-R claims the GPU tests
rest on hold, and libhgx.so exports the new entry points.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np

import kat_graphs as K
import pyref
import sp_ref as R
from oracle_ctypes import OracleGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle(g):
    return OracleGraph(g["num_atoms"], np.asarray(g["link_atom"], np.int32), np.asarray(g["tgt_off"], np.int64),
                       np.asarray(g["tgt_idx"], np.int32),
                       None if g.get("link_type") is None else np.asarray(g["link_type"], np.int32))


def random_graphs(n, seed0=0):
    for seed in range(seed0, seed0 + n):
        rng = np.random.default_rng(seed)
        yield seed, rng, K.random_graph(rng, 40, 60)


def test_reference_kat():
    """TC/query/Queries.java:299-310: dijkstra(n5, n3) == dijkstra(n6, n3) and dijkstra(n0, n1) == 1.0."""
    g = K.queries_graph()
    n, orc = g["names"], oracle(g)
    assert R.dijkstra(orc, n["n0"], n["n1"])[0] == 1.0
    l5 = R.dijkstra(orc, n["n5"], n["n3"])[0]
    assert l5 is not None and l5 == R.dijkstra(orc, n["n6"], n["n3"])[0]
    assert R.dijkstra(orc, n["n10"], n["n0"])[0] is None     # the duplicated bean is in no link


def test_heap_variant_equals_restatement():
    for seed, rng, g in random_graphs(50):
        orc = oracle(g)
        w = rng.integers(1, 8, len(g["link_atom"])).astype(np.float64)
        wf = R.row_weights(g, w)
        mode = R.MODES[seed % 5]
        opts = R.opts_of(mode)
        start = int(rng.integers(0, g["num_atoms"]))
        for goal in (None, int(rng.integers(0, g["num_atoms"]))):
            a = R.dijkstra(orc, start, goal, opts, wf)
            b = R.dijkstra_heap(R.memo_generate(orc, opts), start, goal, wf)
            assert a[0] == b[0] and a[3] == b[3], (seed, goal)
            assert a[1] == b[1] and a[2] == b[2], (seed, goal)


def test_exactness_fixed_point_bitwise():
    """The reference's distances are the least fixed point of the min-plus relaxation, bit for bit,
    also with zero and absorbed weights: Bellman-Ford sweeps over pyref.reachable edges reach the same
    uint64 patterns as the restatement."""
    for seed, rng, g in random_graphs(20, 100):
        orc = oracle(g)
        M = len(g["link_atom"])
        w = rng.random(M)
        w[rng.random(M) < 0.2] = 0.0
        w[rng.random(M) < 0.2] = 2.0 ** -60
        wf = R.row_weights(g, w)
        for mode, tup in R.MODES.items():
            e = R.edges(g, mode)
            for start in rng.integers(0, g["num_atoms"], 2).tolist():
                _, dm, _, _ = R.dijkstra(orc, start, None, R.opts_of(tup), wf)
                ref = np.full(g["num_atoms"], np.inf)
                for a, d in dm.items():
                    ref[a] = d
                bf = R.bellman_ford(g["num_atoms"], e, w, start)
                assert np.array_equal(bf.view(np.uint64), ref.view(np.uint64)), (seed, mode, start)


def test_rule_r_is_the_reference_predecessor_for_integer_weights():
    """With weights 1..7 (every relaxation strictly inflationary) the reference's final predecessor is
    rule R -- for every reached atom of a full run, and for the settled atoms and the goal of a run that
    stopped at a goal."""
    for seed, rng, g in random_graphs(20, 200):
        orc = oracle(g)
        w = rng.integers(1, 8, len(g["link_atom"])).astype(np.float64)
        wf = R.row_weights(g, w)
        for mode, tup in R.MODES.items():
            opts = R.opts_of(tup)
            gen = R.memo_generate(orc, opts)
            start = int(rng.integers(0, g["num_atoms"]))
            _, dm, pred, order = R.dijkstra(orc, start, None, opts, wf)
            rr = R.rule_r(gen, wf, dm, start, list(dm))
            assert {n: a for n, (a, _) in rr.items()} == pred, (seed, mode)
            reached = [a for a in dm if a != start]
            if not reached:
                continue
            goal = reached[int(rng.integers(0, len(reached)))]
            d, dm2, pred2, order2 = R.dijkstra(orc, start, goal, opts, wf)
            assert d == dm[goal]
            rr2 = R.rule_r(gen, wf, dm2, start, order2)
            for n in order2[1:] + [goal]:
                assert rr2[n][0] == pred2[n] == pred[n], (seed, mode, n)


def paths_header_symbols():
    src = open(os.path.join(ROOT, "include", "hgx_paths.h")).read()
    return sorted(set(re.findall(r"\b(hgx_[a-z_]+)\s*\(", src)))


def test_paths_abi_exported_and_bound():
    from hypergraphdb_amd import _lib
    syms = [s for s in paths_header_symbols()]
    declared = sorted(set(syms) - set(_lib.EXPORTED))      # the header's comments may name hgx.h entries
    assert declared == sorted(_lib.EXPORTED_PATHS) and len(declared) >= 10
    out = os.popen(f"nm -D --defined-only {os.path.join(ROOT, 'hypergraphdb_amd', 'libhgx.so')}").read()
    L = _lib.lib()
    for s in declared:
        assert re.search(rf"\sT {s}$", out, re.M), s
        assert getattr(L, s).argtypes is not None, s


def test_paths_null_arguments_without_gpu():
    from hypergraphdb_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    one = np.zeros(1, np.int32)
    assert L.hgx_shortest_paths(None, one.ctypes.data, one.ctypes.data, 1, None, None, C.byref(h)) == _lib.HGX_E_INVALID
    assert b"hgx_shortest_paths" in L.hgx_last_error()
    assert L.hgx_link_weights_create(None, None, C.byref(h)) == _lib.HGX_E_INVALID
    n = C.c_int32()
    assert L.hgx_sp_result_info(None, C.byref(n)) == _lib.HGX_E_INVALID
    assert L.hgx_sp_result_distances(None, None, None) == _lib.HGX_E_INVALID
    k = C.c_int64()
    assert L.hgx_sp_result_path(None, 0, None, None, 0, C.byref(k)) == _lib.HGX_E_INVALID
    assert L.hgx_sp_result_distance_row(None, 0, 0, 0, None) == _lib.HGX_E_INVALID
    assert L.hgx_sp_result_predecessor_row(None, 0, 0, 0, None, None) == _lib.HGX_E_INVALID
    assert L.hgx_sp_result_stats(None, None, None, None, None, None, None) == _lib.HGX_E_INVALID
    L.hgx_sp_result_free(None)
    L.hgx_link_weights_free(None)
