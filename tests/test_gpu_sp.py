"""GPU parity: batched weighted shortest paths (include/hgx_paths.h) against the restatement of
GraphClassics.dijkstra in tests/sp_ref.py.  Distances are compared bitwise (uint64 views); with integer
weights the predecessors and paths are compared exactly (rule R == the reference's predecessorMatrix,
tests/test_sp_ref.py), with zero / absorbed weights the paths are checked for validity."""
import numpy as np
import pytest

import kat_graphs as K
import sp_ref as R
from oracle_ctypes import OracleGraph

pytestmark = pytest.mark.gpu

INF = float("inf")


def snapshot(g):
    from hypergraphdb_amd import HyperGraphSnapshot
    return HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g.get("link_type"))


def oracle(g):
    return OracleGraph(g["num_atoms"], np.asarray(g["link_atom"], np.int32), np.asarray(g["tgt_off"], np.int64),
                       np.asarray(g["tgt_idx"], np.int32),
                       None if g.get("link_type") is None else np.asarray(g["link_type"], np.int32))


def gen(snap, mode, lt=-1):
    from hypergraphdb_amd import AtomTypeCondition, DefaultALGenerator
    P, S, Rv, RS = mode
    return DefaultALGenerator(snap, None if lt < 0 else AtomTypeCondition(lt), None, P, S, Rv, RS)


def u64(x):
    return np.asarray(x, np.float64).view(np.uint64)


def dm_row(A, dm):
    row = np.full(A, np.inf)
    for a, d in dm.items():
        row[a] = d
    return row


def builder_graph(n_nodes, links):
    """nodes 0..n_nodes-1, then one atom per link (targets)."""
    off = np.zeros(len(links) + 1, np.int64)
    tg = []
    for i, t in enumerate(links):
        tg += list(t)
        off[i + 1] = len(tg)
    return dict(num_atoms=n_nodes + len(links), link_atom=np.arange(n_nodes, n_nodes + len(links), dtype=np.int32),
                tgt_off=off, tgt_idx=np.array(tg, np.int32), link_type=np.zeros(len(links), np.int32))


def check_pred_rows_valid(genf, wf, start, drow, pa, pl):
    """Every reached atom but the start has a predecessor joined to it by the reported link over a tight
    edge, and the chain of predecessors ends at the start."""
    A = len(drow)
    for n in range(A):
        if n == start or not np.isfinite(drow[n]):
            assert pa[n] == -1 and pl[n] == -1, n
            continue
        a, l = int(pa[n]), int(pl[n])
        assert a >= 0 and a != n and (l, n) in genf(a), (n, a, l)
        assert R.bits(drow[a] + wf(l)) == R.bits(drow[n]), (n, a, l)
        x, steps = n, 0
        while x != start:
            x = int(pa[x])
            steps += 1
            assert x >= 0 and steps <= A, n


# ---------------------------------------------------------------------------------------------------
# 1. the reference's known-answer graphs, every pair, every mode + one link type, unit weights
# ---------------------------------------------------------------------------------------------------
KATS = {"linkage": (K.linkage_graph, K.T_PLAIN), "queries": (K.queries_graph, K.T_TESTLINK),
        "pattern": (K.pattern_graph, K.T_PLAIN), "compilation": (K.compilation_graph, K.T_PLAIN),
        "positioned": (K.positioned_graph, K.T_TESTLINK)}


@pytest.mark.parametrize("name", sorted(KATS))
def test_kat_graphs_every_pair(name):
    from hypergraphdb_amd import shortest_paths
    make, lt = KATS[name]
    g = make()
    A = g["num_atoms"]
    snap, orc = snapshot(g), oracle(g)
    starts = np.repeat(np.arange(A), A)
    goals = np.tile(np.arange(A), A)
    for mode, t in [(m, -1) for m in R.MODES.values()] + [(R.MODES[0], lt)]:
        opts = R.opts_of(mode, t)
        genf = R.memo_generate(orc, opts)
        with shortest_paths(snap, starts, goals, gen(snap, mode, t)) as res:
            for s in range(A):
                _, dm, _, _ = R.dijkstra(orc, s, None, opts)
                for q in range(A):
                    i = s * A + q
                    assert bool(res.reached[i]) == (q in dm), (name, mode, t, s, q)
                    assert u64(res.distance[i]) == u64(dm.get(q, INF)), (name, mode, t, s, q)
                    atoms, links = res.path(i)
                    if q in dm:
                        R.check_path(genf, None, s, q, atoms, links, dm[q])
                    else:
                        assert len(atoms) == 0 and len(links) == 0
    if name == "queries":   # TC/query/Queries.java:299-310
        n = g["names"]
        with shortest_paths(snap, [n["n0"], n["n5"], n["n6"]], [n["n1"], n["n3"], n["n3"]]) as res:
            assert res.distance[0] == 1.0 and res.distance[1] == res.distance[2] and res.reached.all()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 2. / 3. random hypergraphs (links targeting links, repeated targets, arity 0 / 1)
# ---------------------------------------------------------------------------------------------------
def random_case(seed):
    rng = np.random.default_rng(1000 + seed)
    g = K.random_graph(rng, 40, 60)
    A = g["num_atoms"]
    starts = rng.integers(0, A, 6).tolist()
    pairs = [(s, None) for s in starts]
    for s in starts:
        pairs += [(s, int(q)) for q in rng.integers(0, A, 8)]
    return rng, g, pairs


@pytest.mark.parametrize("seed", range(10))
def test_random_integer_weights_exact_predecessors(seed):
    from hypergraphdb_amd import shortest_paths
    rng, g, pairs = random_case(seed)
    A = g["num_atoms"]
    w = rng.integers(1, 8, len(g["link_atom"])).astype(np.float64)
    wf = R.row_weights(g, w)
    mode = R.MODES[seed % 5]
    lt = 1 if seed >= 5 and seed % 2 else -1
    opts = R.opts_of(mode, lt)
    snap, orc = snapshot(g), oracle(g)
    genf = R.memo_generate(orc, opts)
    with shortest_paths(snap, [p[0] for p in pairs], [p[1] for p in pairs], gen(snap, mode, lt), w) as res:
        for i, (s, q) in enumerate(pairs):
            d, dm, pred, order = R.dijkstra(orc, s, q, opts, wf)
            if q is None:
                assert res.reached[i] and res.distance[i] == 0.0
                assert np.array_equal(u64(res.distances(i)), u64(dm_row(A, dm))), (seed, i)
                rr = R.rule_r(genf, wf, dm, s, list(dm))
                pa, pl = res.predecessors(i)
                exp_a = np.full(A, -1, np.int32)
                exp_l = np.full(A, -1, np.int32)
                for n, a in pred.items():
                    exp_a[n], exp_l[n] = a, rr[n][1]
                    assert rr[n][0] == a
                assert np.array_equal(pa, exp_a) and np.array_equal(pl, exp_l), (seed, i)
                assert len(res.path(i)[0]) == 0
                continue
            assert bool(res.reached[i]) == (d is not None), (seed, i)
            assert u64(res.distance[i]) == u64(INF if d is None else d), (seed, i)
            atoms, links = res.path(i)
            if d is None:
                assert len(atoms) == 0
                continue
            chain = [q]
            while chain[-1] != s:
                chain.append(pred[chain[-1]])
            chain.reverse()
            assert atoms.tolist() == chain, (seed, i)       # the reference's predecessor chain, exactly
            rr = R.rule_r(genf, wf, dm, s, order)
            assert links.tolist() == [rr[n][1] for n in chain[1:]], (seed, i)
            R.check_path(genf, wf, s, q, atoms, links, d)
    snap.close()


@pytest.mark.parametrize("seed", range(10))
def test_random_absorbing_weights(seed):
    from hypergraphdb_amd import shortest_paths
    rng, g, pairs = random_case(seed)
    A, M = g["num_atoms"], len(g["link_atom"])
    w = rng.random(M)
    w[rng.random(M) < 0.3] = 0.0
    w[rng.random(M) < 0.2] = 2.0 ** -60
    wf = R.row_weights(g, w)
    mode = R.MODES[seed % 5]
    opts = R.opts_of(mode)
    snap, orc = snapshot(g), oracle(g)
    genf = R.memo_generate(orc, opts)
    with shortest_paths(snap, [p[0] for p in pairs], [p[1] for p in pairs], gen(snap, mode), w) as res:
        for i, (s, q) in enumerate(pairs):
            d, dm, _, _ = R.dijkstra(orc, s, q, opts, wf)
            if q is None:
                drow = res.distances(i)
                assert np.array_equal(u64(drow), u64(dm_row(A, dm))), (seed, i)
                pa, pl = res.predecessors(i)
                check_pred_rows_valid(genf, wf, s, drow, pa, pl)
                continue
            assert bool(res.reached[i]) == (d is not None), (seed, i)
            assert u64(res.distance[i]) == u64(INF if d is None else d), (seed, i)
            atoms, links = res.path(i)
            if d is None:
                assert len(atoms) == 0
            else:
                R.check_path(genf, wf, s, q, atoms, links, d)
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 4. a hub above kHeavyDegree (512) and kChunkEntries (4096)
# ---------------------------------------------------------------------------------------------------
def test_hub_chunks():
    from hypergraphdb_amd import shortest_paths
    n_leaf, n_tail = 5000, 10
    hub, leaf0, tail0 = 0, 1, 1 + 5000
    links = [(hub, leaf0 + i) for i in range(n_leaf)]
    chain = [leaf0] + [tail0 + i for i in range(n_tail)]
    links += [(chain[i], chain[i + 1]) for i in range(n_tail)]
    links.append((leaf0 + 7, tail0 + 4))            # a detour that avoids the hub, too heavy to win
    g = builder_graph(1 + n_leaf + n_tail, links)
    rng = np.random.default_rng(5)
    w = rng.integers(1, 4, len(links)).astype(np.float64)
    w[-1] = 1000.0
    wf = R.row_weights(g, w)
    snap, orc = snapshot(g), oracle(g)
    assert snap.degree([hub])[0] == n_leaf
    genf = R.memo_generate(orc)
    end = tail0 + n_tail - 1
    pairs = [(leaf0 + 7, end), (hub, None), (end, leaf0 + 4999), (leaf0 + 3, None)]
    with shortest_paths(snap, [p[0] for p in pairs], [p[1] for p in pairs], None, w) as res:
        for i, (s, q) in enumerate(pairs):
            d, dm, pred, _ = R.dijkstra_heap(genf, s, q, wf)
            if q is None:
                assert np.array_equal(u64(res.distances(i)), u64(dm_row(g["num_atoms"], dm)))
                pa, _ = res.predecessors(i)
                assert all(pa[n] == a for n, a in pred.items())
                continue
            assert u64(res.distance[i]) == u64(d)
            atoms, links_ = res.path(i)
            assert hub in atoms.tolist()
            R.check_path(genf, wf, s, q, atoms, links_, d)
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 5. many rounds: a 3000-atom chain, and a ladder whose atoms are lowered several times
# ---------------------------------------------------------------------------------------------------
def test_many_rounds_and_requeueing():
    from hypergraphdb_amd import shortest_paths
    n_chain, n_rung = 3000, 200
    s, mid, rung0 = 0, n_chain, n_chain + 1
    links, w = [], []
    for i in range(n_chain - 1):
        links.append((i, i + 1)); w.append(1.0)
    links.append((s, mid)); w.append(1.0)
    for i in range(n_rung):
        links.append((s, rung0 + i)); w.append(1000.0)      # round 1: every rung at 1000
        links.append((mid, rung0 + i)); w.append(500.0)     # round 2: every rung at 501
    links.append((s, rung0)); w.append(1.0)
    for i in range(n_rung - 1):
        links.append((rung0 + i, rung0 + i + 1)); w.append(1.0)   # then one rung a round: i + 1
    g = builder_graph(n_chain + 1 + n_rung, links)
    w = np.array(w)
    wf = R.row_weights(g, w)
    snap, orc = snapshot(g), oracle(g)
    genf = R.memo_generate(orc)
    pairs = [(s, None), (s, n_chain - 1), (s, rung0 + n_rung - 1)]
    with shortest_paths(snap, [p[0] for p in pairs], [p[1] for p in pairs], None, w) as res:
        _, dm, pred, _ = R.dijkstra_heap(genf, s, None, wf)
        assert np.array_equal(u64(res.distances(0)), u64(dm_row(g["num_atoms"], dm)))
        pa, _ = res.predecessors(0)
        assert all(pa[n] == a for n, a in pred.items())
        assert res.distance[1] == n_chain - 1 and res.distance[2] == float(n_rung)
        assert res.path(1)[0].tolist() == list(range(n_chain))
        assert res.path(2)[0].tolist() == [s] + [rung0 + i for i in range(n_rung)]
    with shortest_paths(snap, [s], [None], None, w) as res:
        st = res.stats()
        assert st["rounds"] >= n_chain - 1
        # the chain atoms and mid improve once, every rung past the second three times (1000, 501, i + 1)
        assert st["improved"] >= (n_chain - 1) + 1 + 3 * (n_rung - 2) and st["improved"] > len(dm), st
        assert st["relaxed"] >= st["improved"] and st["expanded"] >= len(dm) - 1
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 6. a batch of 300 pairs, one chunk / one pair per chunk / an execution context
# ---------------------------------------------------------------------------------------------------
def test_batch_chunks_and_context():
    from hypergraphdb_amd import LinkWeights, _lib, shortest_paths
    rng = np.random.default_rng(77)
    g = K.random_graph(rng, 80, 120)
    A = g["num_atoms"]
    w = rng.integers(1, 8, len(g["link_atom"])).astype(np.float64)
    wf = R.row_weights(g, w)
    snap, orc = snapshot(g), oracle(g)
    full = {}

    def ref(s):
        if s not in full:
            full[s] = R.dijkstra(orc, s, None, None, wf)[1]
        return full[s]
    starts = rng.integers(0, A, 300)
    goals = rng.integers(0, A, 300)
    goals[::7] = -1
    goals[3::11] = starts[3::11]
    starts[200:250], goals[200:250] = starts[:50], goals[:50]      # duplicated pairs
    unreachable = [i for i in range(300) if goals[i] >= 0 and goals[i] not in ref(int(starts[i]))]
    assert unreachable and (goals == starts).any() and (goals < 0).any()

    def run(target):
        out = []
        with LinkWeights(snap, w) as lw, shortest_paths(target, starts, goals, None, lw) as res:
            for i in range(300):
                a, l = res.path(i)
                rows = (res.distances(i).tobytes(), res.predecessors(i)[0].tobytes(),
                        res.predecessors(i)[1].tobytes()) if goals[i] < 0 else None
                out.append((u64(res.distance[i]).item(), bool(res.reached[i]), a.tolist(), l.tolist(), rows))
        return out
    base = run(snap)
    for i in range(300):
        dm = ref(int(starts[i]))
        if goals[i] < 0:
            assert base[i][4][0] == dm_row(A, dm).tobytes(), i
        else:
            assert base[i][0] == u64(dm.get(int(goals[i]), INF)).item(), i
            assert base[i][1] == (int(goals[i]) in dm), i
    snap.set_option(_lib.HGX_OPT_SP_BUDGET, 1)          # one pair per chunk
    assert run(snap) == base
    snap.set_option(_lib.HGX_OPT_SP_BUDGET, 48 << 30)
    ctx = snap.context()
    assert run(ctx) == base
    ctx.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 7. a medium power-law graph against the heap variant
# ---------------------------------------------------------------------------------------------------
def test_medium_power_law():
    from hypergraphdb_amd import shortest_paths, synth
    g = synth.hypergraph(20000, 60000, 2, 8, 2.1, 4, seed=7)
    rng = np.random.default_rng(7)
    w = rng.integers(1, 17, 60000).astype(np.float64)
    row = np.full(g["num_atoms"], -1, np.int64)
    row[g["link_atom"]] = np.arange(60000)
    wl, row = w.tolist(), row.tolist()

    def wf(l):
        return wl[row[l]]
    snap, orc = snapshot(g), oracle(g)
    genf = R.memo_generate(orc)
    src = synth.sources(g, 9, 11).tolist()
    starts = [src[0]] * 4 + [src[1]] * 4 + [src[2]]
    goals = src[3:7] + src[5:9] + [None]
    with shortest_paths(snap, starts, goals, None, w) as res:
        for i, (s, q) in enumerate(zip(starts, goals)):
            d, dm, _, _ = R.dijkstra_heap(genf, s, q, wf)
            if q is None:
                assert np.array_equal(u64(res.distances(i)), u64(dm_row(g["num_atoms"], dm)))
            else:
                assert u64(res.distance[i]) == u64(INF if d is None else d), i
                if d is not None:
                    a, l = res.path(i)
                    R.check_path(genf, wf, s, q, a, l, d)
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------------------------------
def test_errors():
    from hypergraphdb_amd import HGXError, HGXUnsupported, LinkWeights, _lib, shortest_paths
    from hypergraphdb_amd.partition import Shard, ShardSnapshot
    g = K.queries_graph()
    A, M = g["num_atoms"], len(g["link_atom"])
    snap = snapshot(g)
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        w = np.ones(M)
        w[2] = bad
        with pytest.raises(HGXError) as e:
            LinkWeights(snap, w)
        assert e.value.code == _lib.HGX_E_INVALID, bad
    for s, q in ((A, 0), (-1, 0), (0, A), (0, -2)):
        with pytest.raises(HGXError) as e:
            shortest_paths(snap, [s], [q])
        assert e.value.code == _lib.HGX_E_INVALID, (s, q)
    # -0.0 is 0.0
    n = g["names"]
    wz, wn = np.zeros(M), np.full(M, -0.0)
    with shortest_paths(snap, [n["n0"]], [None], None, wz) as a, shortest_paths(snap, [n["n0"]], [None], None, wn) as b:
        assert np.array_equal(u64(a.distances(0)), u64(b.distances(0)))
        assert u64(b.distances(0))[n["n1"]] == 0
    # a live result blocks the update; a weights object made for another link count is refused
    lw = LinkWeights(snap, np.ones(M))
    res = shortest_paths(snap, [n["n0"]], [n["n1"]], None, lw)
    with pytest.raises(HGXError):
        snap.update(add={A: (K.T_PLAIN, [n["n0"], n["n10"]])}, num_atoms=A + 1)
    res.close()
    snap.update(add={A: (K.T_PLAIN, [n["n0"], n["n10"]])}, num_atoms=A + 1)
    with pytest.raises(HGXError) as e:
        shortest_paths(snap, [n["n0"]], [n["n1"]], None, lw)
    assert e.value.code == _lib.HGX_E_INVALID
    lw.close()
    with shortest_paths(snap, [n["n0"]], [n["n10"]]) as r2:    # the new link connects the lone bean
        assert r2.distance[0] == 1.0
    snap.close()
    # partition shards
    plan = np.zeros(M, np.int32)
    sh = Shard.build(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"], 1, 0, plan)
    ss = ShardSnapshot(sh)
    with pytest.raises(HGXUnsupported):
        shortest_paths(ss, [0], [1])
    ss.close()
    sh.close()


# ---------------------------------------------------------------------------------------------------
# 9. the Python mirror of GraphClassics.dijkstra
# ---------------------------------------------------------------------------------------------------
def test_graph_classics_mirror():
    from hypergraphdb_amd import DefaultALGenerator, GraphClassics
    g = K.queries_graph()
    n = g["names"]
    snap, orc = snapshot(g), oracle(g)
    al = DefaultALGenerator(snap)
    assert GraphClassics.dijkstra(n["n0"], n["n1"], al) == 1.0
    assert GraphClassics.dijkstra(n["n10"], n["n0"], al) is None
    assert GraphClassics.dijkstra(n["n5"], n["n3"], al) == GraphClassics.dijkstra(n["n6"], n["n3"], al)
    w = np.arange(1, len(g["link_atom"]) + 1, dtype=np.float64)
    wf = R.row_weights(g, w)
    dmat, pmat = {}, {}
    d = GraphClassics.dijkstra(n["n5"], n["n1"], al, w, dmat, pmat)
    dr, dm, pred, _ = R.dijkstra(orc, n["n5"], n["n1"], None, wf)
    assert d == dr
    chain = [n["n1"]]
    while chain[-1] != n["n5"]:
        chain.append(pred[chain[-1]])
    assert set(dmat) == set(chain) and all(dmat[a] == dm[a] for a in chain)
    assert pmat == {a: pred[a] for a in chain if a != n["n5"]}
    # a callable weight, and goal=None: the complete maps
    dmat, pmat = {}, {}
    assert GraphClassics.dijkstra(n["n5"], None, al, wf, dmat, pmat) is None
    _, dm, pred, _ = R.dijkstra(orc, n["n5"], None, None, wf)
    assert dmat == dm and pmat == pred
    snap.close()
