"""hg.or on the GPU pattern path (hgx_pattern_batch_dnf, include/hgx_dnf.h): every And / Or tree over the
accelerated leaves as one device call -- the clauses through the single-pass pattern pipeline, then a sorted
union on the device.  Expected results: np.unique of the oracle's per-clause results (OrToQuery chaining
UnionResults, OrToQuery.java:14-43), compared as exact lists; trees also against the brute-force evaluator of
tests/dnf_ref.py."""
import threading

import numpy as np
import pytest

import dnf_ref as D
import kat_graphs as K
from oracle_ctypes import OracleGraph

pytestmark = pytest.mark.gpu


def snapshot(g):
    from hypergraphdb_amd import HyperGraphSnapshot
    return HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g.get("link_type"))


def oracle(g):
    return OracleGraph(g["num_atoms"], np.asarray(g["link_atom"], np.int32), np.asarray(g["tgt_off"], np.int64),
                       np.asarray(g["tgt_idx"], np.int32), np.asarray(g["link_type"], np.int32))


def clause(types=(), inc=(), pos=(), patterns=(), arity=-1):
    return {"types": list(types), "inc": list(inc), "pos": list(pos), "patterns": list(patterns), "arity": arity}


def expected(orc, query):
    """(np.unique of the per-clause oracle results, the per-clause results)"""
    parts = [orc.and_query_ext(c["types"], c["inc"], c["pos"], c["patterns"], c["arity"]) for c in query]
    assert all(p is not None for p in parts)
    allh = np.concatenate(parts) if parts else np.empty(0, np.int32)
    return np.unique(allh).tolist(), parts


def check_batch(r, orc, queries):
    assert len(r) == len(queries)
    dup = 0
    for q, query in enumerate(queries):
        exp, parts = expected(orc, query)
        assert r[q].tolist() == exp, (q, query)
        dup += sum(len(p) for p in parts) - len(exp)
    assert r.union["clause_hits"] - r.union["kept"] == dup
    assert r.union["kept"] == int(r.offsets[-1]) == len(r.ids)
    return dup


@pytest.mark.parametrize("case", range(4))
def test_random_dnf_batches_vs_oracle(case):
    from hypergraphdb_amd import pattern_batch_dnf
    rng = np.random.default_rng(1200 + case)
    g = K.random_graph(rng, 400, 4000, max_arity=8, n_types=3, link_targets=case % 2 == 0)
    snap, orc = snapshot(g), oracle(g)
    A, off, tg = g["num_atoms"], g["tgt_off"], g["tgt_idx"]
    queries = []
    for _ in range(1500):
        row = int(rng.integers(0, len(g["link_atom"])))
        row_t = tg[off[row]:off[row + 1]]
        query = []
        for _ in range(int(rng.integers(1, 7))):
            t = int(rng.integers(-1, 3))
            k = int(rng.integers(1, 3))
            if len(row_t) and rng.random() < 0.6:
                inc = [int(x) for x in rng.choice(row_t, k)]
            else:
                inc = [int(x) for x in rng.integers(0, A, k)]
            query.append(clause([t] if t >= 0 else [], inc))
        queries.append(query)
    # the input is not trivial (from the oracle's results alone)
    nonempty = multi = with_dup = 0
    for query in queries:
        exp, parts = expected(orc, query)
        nonempty += len(exp) > 0
        multi += sum(len(p) > 0 for p in parts) >= 2
        with_dup += sum(len(p) for p in parts) > len(exp)
    assert nonempty >= 0.6 * len(queries)
    assert multi >= 0.4 * len(queries)
    assert with_dup >= 0.2 * len(queries)
    if case == 0:
        snap.set_timing(True)
    r = pattern_batch_dnf(snap, queries)
    assert check_batch(r, orc, queries) > 0
    assert r.union["bytes_union"] > 0
    if case == 0:
        assert 0 < r.union["ms_union"] <= r.ms["ms_total"]
    snap.close()


def test_trees_end_to_end_and_find_all():
    from hypergraphdb_amd import find_all, hg, pattern_batch_dnf
    rng = np.random.default_rng(78)
    g = K.random_graph(rng, 150, 600, max_arity=6)
    snap, pg = snapshot(g), D.graph_of(g)
    trees = [D.random_tree(rng, g) for _ in range(300)]
    r = pattern_batch_dnf(snap, trees)
    for q, tree in enumerate(trees):
        assert r[q].tolist() == D.evaluate(pg, tree), tree
    for tree in trees[:5]:
        assert find_all(snap, tree) == D.evaluate(pg, tree), tree
    snap.close()
    # the reference's query test graph
    g = K.queries_graph()
    snap, pg, n = snapshot(g), D.graph_of(g), g["names"]
    cond = hg.or_(hg.incident(n["n0"]), hg.incident(n["n1"]))
    assert find_all(snap, cond) == D.evaluate(pg, cond) == sorted([n["valuelink"], n["linkH"]])
    cond = hg.and_(hg.type(K.T_TESTLINK), hg.or_(hg.incident(n["n0"]), hg.incident(n["n2"])))   # And holding an Or
    assert find_all(snap, cond) == D.evaluate(pg, cond) == sorted([n["linkH"], n["linkH1"], n["link5"]])
    cond = hg.or_(hg.and_(hg.incident(n["n0"]), hg.orderedLink()), hg.incident(n["n2"]))        # a NOP clause
    assert find_all(snap, cond) == D.evaluate(pg, cond)
    # an Or with a traversal part: the host union of the parts
    bfs = hg.bfs(n["n0"])
    got = find_all(snap, hg.or_(hg.incident(n["n2"]), bfs))
    assert got == sorted(set(find_all(snap, hg.incident(n["n2"]))) | set(find_all(snap, bfs)))
    got = find_all(snap, hg.and_(hg.or_(hg.incident(n["n2"]), bfs), hg.incident(n["n3"])))
    assert got == [n["valuelink"], n["linkH1"]]
    snap.close()


def test_flat_mapping_edges():
    """Queries with 0 clauses, 1 clause, only empty clauses, a clause three times, and 200 clauses (more
    than a wavefront has lanes), with empty queries before and after each."""
    from hypergraphdb_amd import pattern_batch_dnf
    rng = np.random.default_rng(5)
    g = K.random_graph(rng, 300, 2000, max_arity=6)
    snap, orc = snapshot(g), oracle(g)
    deg = np.bincount(g["tgt_idx"], minlength=g["num_atoms"])
    busy = [int(a) for a in np.argsort(-deg)[:200]]
    lonely = [int(a) for a in np.nonzero(deg == 0)[0][:3]]
    assert len(lonely) == 3 and deg[busy[-1]] > 0
    nop = clause(inc=[busy[0]], patterns=[()])
    cases = [[clause(inc=[busy[0]])],
             [clause(inc=[a]) for a in lonely] + [nop],
             [clause(types=[1], inc=[busy[1]])] * 3,
             [clause(inc=[a]) for a in busy]]
    queries = [[]]
    for c in cases:
        queries += [c, [], [nop]]
    r = pattern_batch_dnf(snap, queries)
    check_batch(r, orc, queries)
    assert len(r[1]) > 0 and len(r[4]) == 0 and len(r[7]) > 0 and len(r[10]) > len(r[1])
    assert pattern_batch_dnf(snap, [[], []]).offsets.tolist() == [0, 0, 0]      # no clause at all
    assert len(pattern_batch_dnf(snap, [])) == 0
    snap.close()


def hub_graph(n_links, n_types=3):
    b = K.Builder()
    h = b.node("h")
    xs = [b.node(f"x{i}") for i in range(7)]
    for i in range(n_links):
        b.link(None, i % n_types, h, xs[i % 7])
    return b.arrays()


def test_long_runs():
    """One atom with 1,500 incident links over 3 types: runs crossing the 64-hit and 256-thread
    boundaries, fully contained in a later / an earlier run, and two disjoint interleaving runs."""
    from hypergraphdb_amd import hg, pattern_batch_dnf
    g = hub_graph(1500)
    snap, orc = snapshot(g), oracle(g)
    h = g["names"]["h"]
    t0, t1, every = clause([0], [h]), clause([1], [h]), clause([], [h])
    queries = [[t0, t1, every], [every, t1, t0], [t0, t1], [t1, t0], [every, every]]
    r = pattern_batch_dnf(snap, queries)
    check_batch(r, orc, queries)
    full = orc.and_query_ext([], [h]).tolist()
    assert len(full) == 1500 and r[0].tolist() == full and r[1].tolist() == full and r[4].tolist() == full
    assert len(r[2]) == 1000 and r[2].tolist() == r[3].tolist()
    tree = hg.or_(hg.and_(hg.type(0), hg.incident(h)), hg.and_(hg.type(1), hg.incident(h)), hg.incident(h))
    assert pattern_batch_dnf(snap, [tree])[0].tolist() == full
    snap.close()


def test_workspace_growth():
    """On a fresh snapshot the first DNF batch needs more candidates than the initial workspace holds
    (16 n + 4096): the clause stage reports the overflow, the union does nothing, the host grows the workspace
    and runs once more; the next call reuses it."""
    from hypergraphdb_amd import pattern_batch_dnf
    g = hub_graph(6000)
    snap, orc = snapshot(g), oracle(g)
    h = g["names"]["h"]
    queries = [[clause([], [h]), clause([2], [h])]]
    assert 2 * 6000 > 16 * 2 + 4096
    for rep in range(2):
        r = pattern_batch_dnf(snap, queries)
        check_batch(r, orc, queries)
        assert len(r[0]) == 6000 and r.union["clause_hits"] == 8000
    snap.close()


def test_errors_contexts_and_plain_path_unchanged():
    from hypergraphdb_amd import HGXError, HGXUnsupported, _lib, hg, pattern_batch, pattern_batch_dnf
    g = K.queries_graph()
    snap, n = snapshot(g), g["names"]
    ok = clause(inc=[n["n0"]])
    with pytest.raises(HGXUnsupported) as e:          # clause 1 of query 2 has no incidence anchor
        pattern_batch_dnf(snap, [[ok], [], [ok, clause(types=[K.T_TESTLINK])]])
    assert "query 2 clause 1" in str(e.value)
    with pytest.raises(HGXUnsupported):
        pattern_batch_dnf(snap, [hg.or_(hg.incident(n["n0"]), hg.type(K.T_TESTLINK))])
    with pytest.raises(HGXError) as e:                # atom id out of range
        pattern_batch_dnf(snap, [[ok], [ok, ok, clause(inc=[g["num_atoms"] + 5])]])
    assert e.value.code == _lib.HGX_E_INVALID and "query 1 clause 2" in str(e.value)
    from hypergraphdb_amd.query import _ext_arrays, pattern_batch_dnf_arrays
    with pytest.raises(HGXError) as e:                # clause_off not monotone
        pattern_batch_dnf_arrays(snap, [0, 2, 1], *_ext_arrays([ok, ok]))
    assert e.value.code == _lib.HGX_E_INVALID
    snap.close()
    from test_gpu_partition import parts
    sh = parts(g, 2)
    with pytest.raises(HGXUnsupported):               # a shard is not a whole snapshot
        pattern_batch_dnf(sh[0], [[clause(inc=[0])]])
    for s in sh:
        s.close()
    # one batch from 4 threads, each on its own execution context; the plain path before and after
    rng = np.random.default_rng(9)
    g = K.random_graph(rng, 300, 3000, max_arity=6)
    snap = snapshot(g)
    orc = oracle(g)
    A = g["num_atoms"]
    queries = [[clause([int(t)] if t >= 0 else [], [int(a)]) for t, a in
                zip(rng.integers(-1, 3, int(rng.integers(0, 5))), rng.integers(0, A, 4))] for _ in range(400)]
    plain = [c for q in queries for c in q]
    before = pattern_batch(snap, plain)
    ref = pattern_batch_dnf(snap, queries)
    check_batch(ref, orc, queries)
    ctxs = [snap.context() for _ in range(4)]
    out, errs = [None] * 4, []

    def work(i):
        try:
            for _ in range(3):
                out[i] = pattern_batch_dnf(ctxs[i], queries)
        except Exception as ex:   # noqa: BLE001
            errs.append(ex)

    ths = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs
    for r in out:
        assert np.array_equal(r.offsets, ref.offsets) and np.array_equal(r.ids, ref.ids)
    after = pattern_batch(snap, plain)
    assert np.array_equal(before.offsets, after.offsets) and np.array_equal(before.ids, after.ids)
    for q, c in enumerate(plain[:200]):
        assert after[q].tolist() == orc.and_query_ext(c["types"], c["inc"]).tolist()
    for c in ctxs:
        c.close()
    snap.close()
