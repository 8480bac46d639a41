"""GPU parity: shortest hop paths and predecessor rows read out of a batched BFS (include/hgx_hops.h)
against tests/hop_ref.py (the unit-weight rule R, checked on the CPU against the restatement of
GraphClassics.dijkstra in tests/test_hop_ref.py).  Everything is compared exactly: hops, every atom and
every link of every path, whole depth and predecessor rows."""
import threading

import numpy as np
import pytest

import hop_ref as H
import kat_graphs as K
import sp_ref as R
from oracle_ctypes import OracleGraph

pytestmark = pytest.mark.gpu


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


def builder_graph(n_nodes, links):
    """nodes 0..n_nodes-1, then one atom per link (targets)."""
    off = np.zeros(len(links) + 1, np.int64)
    tg = []
    for i, t in enumerate(links):
        tg += list(t)
        off[i + 1] = len(tg)
    return dict(num_atoms=n_nodes + len(links), link_atom=np.arange(n_nodes, n_nodes + len(links), dtype=np.int32),
                tgt_off=off, tgt_idx=np.array(tg, np.int32), link_type=np.zeros(len(links), np.int32))


class Ref:
    """hop_ref.hop_rule per start over one memoised generator."""

    def __init__(self, orc, mode, lt=-1, max_depth=None):
        self.gen = R.memo_generate(orc, R.opts_of(mode, lt))
        self.max_depth = max_depth
        self.rows = {}

    def of(self, start):
        start = int(start)
        if start not in self.rows:
            self.rows[start] = H.hop_rule(self.gen, start, self.max_depth)
        return self.rows[start]


def check_paths(hp, starts, goals, ref, tag=()):
    """Pair i of hp is hop_ref's path starts[i] .. goals[i]: hops, every atom (the predecessors) and every
    link (the lowest qualifying one), or -1 and an empty path."""
    assert hp.n_pairs == len(starts) == len(goals)
    for i, (s, q) in enumerate(zip(map(int, starts), map(int, goals))):
        depth, pred = ref.of(s)
        atoms, links = hp.path(i)
        if q not in depth:
            assert hp.hops[i] == -1 and not hp.reached[i] and len(atoms) == 0 and len(links) == 0, (tag, i, s, q)
            continue
        ea, el = H.follow(pred, s, q)
        assert hp.hops[i] == depth[q] and hp.reached[i], (tag, i, s, q, hp.hops[i], depth[q])
        assert atoms.tolist() == ea and links.tolist() == el, (tag, i, s, q, atoms, links, ea, el)


def check_rows(res, i, start, A, ref, tag=(), levels=None):
    """The whole depth and predecessor rows of seed i against hop_ref (and, with ``levels``, the depth row
    against the oracle's per-depth sets, OracleGraph.bfs_levels)."""
    depth, pred = ref.of(start)
    if levels is not None:
        assert {int(n): d for d, lv in enumerate(levels) for n in lv} == depth, (tag, i, start)
    ed = np.full(A, -1, np.int32)
    ea = np.full(A, -1, np.int32)
    el = np.full(A, -1, np.int32)
    for n, d in depth.items():
        ed[n] = d
    for n, (a, l) in pred.items():
        ea[n], el[n] = a, l
    assert np.array_equal(res.depths(i), ed), (tag, i, start)
    pa, pl = res.predecessors(i)
    assert np.array_equal(pa, ea), (tag, i, start, np.nonzero(pa != ea)[0][:8])
    assert np.array_equal(pl, el), (tag, i, start, np.nonzero(pl != el)[0][:8])
    assert np.array_equal(res.depths(i, 1, min(5, A - 1)), ed[1:1 + min(5, A - 1)])     # a sub-range of the cached row
    pa2, pl2 = res.predecessors(i, A // 2, A - A // 2)
    assert np.array_equal(pa2, ea[A // 2:]) and np.array_equal(pl2, el[A // 2:])


# ---------------------------------------------------------------------------------------------------
# 1. the reference's known-answer graphs, every ordered pair, every mode + one link type
# ---------------------------------------------------------------------------------------------------
KATS = {"linkage": (K.linkage_graph, K.T_PLAIN), "queries": (K.queries_graph, K.T_TESTLINK),
        "pattern": (K.pattern_graph, K.T_PLAIN)}


@pytest.mark.parametrize("name", sorted(KATS))
def test_kat_graphs_every_pair(name):
    from hypergraphdb_amd import bfs_batch
    make, lt = KATS[name]
    g = make()
    A = g["num_atoms"]
    snap, orc = snapshot(g), oracle(g)
    si = np.repeat(np.arange(A), A)
    goals = np.tile(np.arange(A), A)
    for mode, t in [(m, -1) for m in R.MODES.values()] + [(R.MODES[0], lt)]:
        opts = R.opts_of(mode, t)
        ref = Ref(orc, mode, t)
        res = bfs_batch(snap, np.arange(A), None, gen(snap, mode, t))
        with res.paths(si, goals) as hp:
            check_paths(hp, si, goals, ref, (name, mode, t))
            for s in range(A):
                _, dm, pred, _ = R.dijkstra(orc, s, None, opts)
                for q in range(A):
                    i = s * A + q
                    assert hp.hops[i] == (-1 if q not in dm else int(dm[q])), (name, mode, t, s, q)
                    if q in dm:
                        atoms, links = hp.path(i)
                        assert all(pred[int(atoms[k])] == atoms[k - 1] for k in range(1, len(atoms)))
                        R.check_path(ref.gen, None, s, q, atoms, links, float(hp.hops[i]))
        res.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 2. random hypergraphs: rows past 8 targets, repeated targets, links as targets; W = 1, 2, 8
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 64, 65, 300])
def test_random_graphs_rows_and_pairs(S):
    from hypergraphdb_amd import _lib, bfs_batch
    rng = np.random.default_rng(4200 + S)
    g = K.random_graph(rng, 600, 2500, max_arity=12, n_types=3)
    A = g["num_atoms"]
    snap, orc = snapshot(g), oracle(g)
    snap.set_option(_lib.HGX_OPT_BFS_BLOCK, 0)   # the level rows (W words a row); the other forms: test 4
    seeds = rng.choice(A, S, replace=False).astype(np.int32)
    picked = np.unique(np.linspace(0, S - 1, min(S, 8)).astype(np.int64))
    deepest = 0
    for mode in R.MODES.values():
        for lt in (-1, 1):
            ref = Ref(orc, mode, lt)
            res = bfs_batch(snap, seeds, None, gen(snap, mode, lt))
            for i in picked:
                check_rows(res, int(i), seeds[i], A, ref, (S, mode, lt),
                           orc.bfs_levels(int(seeds[i]), -1, R.opts_of(mode, lt)))
            si = rng.choice(picked, 200).astype(np.int32)
            goals = rng.integers(0, A, 200).astype(np.int32)
            with res.paths(si, goals) as hp:
                check_paths(hp, seeds[si], goals, ref, (S, mode, lt))
                deepest = max(deepest, int(hp.hops.max()))
                st = hp.stats()
                assert st["steps"] >= hp.hops.max() and (st["entries"] > 0) == (hp.hops.max() > 0)
                assert st["probes"] > 0 and st["bytes"] > 0
            res.close()
    assert deepest >= 3
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 3. hubs: a row of several chunks as the current node; a power-law graph with 1024 seeds
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [0, 1])
def test_star_hub_with_a_tail(block):
    from hypergraphdb_amd import _lib, bfs_batch
    L, T = 6000, 5
    hub, leaf0, tail0 = 0, 1, 1 + L
    links = [(hub, leaf0 + i) for i in range(L)]
    links += [(leaf0 + 2, tail0)] + [(tail0 + k, tail0 + k + 1) for k in range(T - 1)]
    g = builder_graph(1 + L + T, links)
    A = g["num_atoms"]
    snap, orc = snapshot(g), oracle(g)
    snap.set_option(_lib.HGX_OPT_BFS_BLOCK, block)
    tail_end = tail0 + T - 1
    seeds = np.array([leaf0 + 5, tail_end, hub, leaf0 + 4000], np.int32)
    for mode in (R.MODES[0], R.MODES[1]):   # symmetric; after-first: hub -> leaf, leaf 2 -> tail ... -> tail end
        ref = Ref(orc, mode)
        res = bfs_batch(snap, seeds, None, gen(snap, mode))
        si = np.array([0, 0, 1, 1, 2, 2, 3, 2], np.int32)
        goals = np.array([leaf0 + 4000, leaf0 + 5999, hub, leaf0 + 77, tail_end, leaf0 + 2, leaf0 + 5, hub], np.int32)
        with res.paths(si, goals) as hp:
            check_paths(hp, seeds[si], goals, ref, (block, mode))
            if mode == R.MODES[0]:
                assert hp.hops.tolist() == [2, 2, T + 1, T + 2, T + 1, 1, 2, 0]
                assert hp.path(2)[0].tolist() == [tail_end - k for k in range(T)] + [leaf0 + 2, hub]
            else:
                assert hp.hops.tolist() == [-1, -1, -1, -1, T + 1, 1, -1, 0]
        for i in (1, 2):
            check_rows(res, i, seeds[i], A, ref, (block, mode))
        res.close()
    snap.close()


_POWER = {}


def power_law():
    """The power-law case of tests 3, 4 and 7 (made once): graph, snapshot, oracle, 1024 seeds."""
    if not _POWER:
        from hypergraphdb_amd import synth
        g = synth.hypergraph(3000, 20000, 2, 8, 2.1, 3, seed=17)
        _POWER.update(g=g, snap=snapshot(g), orc=oracle(g), seeds=np.asarray(synth.sources(g, 1024, 5), np.int32))
    return _POWER["g"], _POWER["snap"], _POWER["orc"], _POWER["seeds"]


@pytest.mark.parametrize("mi", [1, 4, 7, 10])   # K.ALGEN_MODES[1::3]
def test_power_law_1024_seeds(mi):
    from hypergraphdb_amd import bfs_batch
    g, snap, orc, seeds = power_law()
    A = g["num_atoms"]
    mode = K.ALGEN_MODES[mi]
    rng = np.random.default_rng(500 + mi)
    ref = Ref(orc, mode)
    res = bfs_batch(snap, seeds, None, gen(snap, mode))
    picked = np.array([0, 63, 64, 500, 1000, 1023])
    si = np.repeat(picked, 50).astype(np.int32)
    goals = rng.integers(0, A, 300).astype(np.int32)
    goals[::5] = rng.integers(0, g["n_nodes"], 60)        # more goals among the nodes
    with res.paths(si, goals) as hp:
        check_paths(hp, seeds[si], goals, ref, (mi,))
    for i in picked[:4]:
        check_rows(res, int(i), seeds[i], A, ref, (mi,))
    res.close()


# ---------------------------------------------------------------------------------------------------
# 4. every storage form gives the same answer
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mi", [0, 1])
def test_storage_forms_agree(mi):
    from hypergraphdb_amd import _lib, bfs_batch
    g, snap0, orc, _ = power_law()
    A = g["num_atoms"]
    mode = K.ALGEN_MODES[mi]
    rng = np.random.default_rng(77 + mi)
    seeds = rng.integers(0, g["n_nodes"], 1100).astype(np.int32)   # two batches
    seeds[::10] = rng.integers(g["n_nodes"], A, 110)                # links: atoms without incidence (closure {seed})
    seeds[1050:1060] = np.asarray(_POWER["seeds"][:10])
    si = np.concatenate([rng.integers(0, 1100, 280), np.arange(1090, 1100), [3, 3, 3, 1055, 1055], [7, 7, 7, 7, 7]])
    goals = np.concatenate([rng.integers(0, A, 290), [11, 11, 11, 2, 2], rng.integers(0, g["n_nodes"], 5)])
    si, goals = si.astype(np.int32), goals.astype(np.int32)
    max_depth = 3 if mi == 0 else 2         # mi 1: closures of a few hundred atoms stay inside a workgroup, hubs outgrow it
    ref = Ref(orc, mode, -1, max_depth)
    got = {}
    snap = snapshot(g)
    for block in (0, 1):
        snap.set_option(_lib.HGX_OPT_BFS_BLOCK, block)
        res = bfs_batch(snap, seeds, max_depth, gen(snap, mode))
        if block == 1:
            st = res.stats(accounting=False)
            assert st["block_seeds"] > 0 and (mi != 0 or st["block_rerun"] > 0), st   # both forms in one result
        with res.paths(si, goals) as hp:
            got[block] = (hp.hops.copy(), [hp.path(i)[0].tolist() for i in range(len(si))],
                          [hp.path(i)[1].tolist() for i in range(len(si))])
            k = np.nonzero(np.isin(si, [3, 7, 1055, 1091, 1095]))[0]
            check_paths_subset(hp, k, seeds[si], goals, ref, (mi, block))
        for i in (3, 1055):
            check_rows(res, i, seeds[i], A, ref, (mi, block))
        res.close()
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1] and got[0][2] == got[1][2]
    # the grid stage: a batch of <= 64 seeds
    snap.set_option(_lib.HGX_OPT_BFS_BLOCK, 2)
    res = bfs_batch(snap, seeds[:64], max_depth, gen(snap, mode))
    k = np.nonzero(si < 64)[0]
    assert len(k) >= 10
    with res.paths(si[k], goals[k]) as hp:
        assert np.array_equal(hp.hops, got[0][0][k])
        for j, i in enumerate(k):
            assert hp.path(j)[0].tolist() == got[0][1][i] and hp.path(j)[1].tolist() == got[0][2][i]
    check_rows(res, 3, seeds[3], A, ref, (mi, 2))
    res.close()
    snap.close()


def check_paths_subset(hp, idx, starts, goals, ref, tag):
    for i in idx:
        s, q = int(starts[i]), int(goals[i])
        depth, pred = ref.of(s)
        atoms, links = hp.path(int(i))
        if q not in depth:
            assert hp.hops[i] == -1 and len(atoms) == 0, (tag, i)
        else:
            ea, el = H.follow(pred, s, q)
            assert hp.hops[i] == depth[q] and atoms.tolist() == ea and links.tolist() == el, (tag, i)


# ---------------------------------------------------------------------------------------------------
# 5. deep ordered traversals (20+ levels)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [(False, True, False, False), (False, True, True, False)])
def test_deep_subsumption(mode):
    from hypergraphdb_amd import bfs_batch, synth
    g = synth.config5(scale=0.002, n_sources=500)
    A = g["num_atoms"]
    lt = int(g["subsumes_type"])
    snap, orc = snapshot(g), oracle(g)
    seeds = np.asarray(g["seeds"], np.int32)
    rng = np.random.default_rng(9)
    ref = Ref(orc, mode, lt)
    res = bfs_batch(snap, seeds, None, gen(snap, mode, lt))
    # the 6 seeds with the most levels, 50 goals each: 40 out of the seed's own closure, 10 anywhere
    cnt = res.counts()
    picked = np.argsort(-(cnt > 0).sum(1), kind="stable")[:6]
    si, goals = [], []
    for i in picked:
        depth, _ = ref.of(seeds[i])
        reach = np.array(sorted(depth, key=lambda n: (-depth[n], n))[:200])
        si += [i] * 50
        goals += rng.choice(reach, 40).tolist() + rng.integers(0, A, 10).tolist()
    si, goals = np.array(si, np.int32), np.array(goals, np.int32)
    with res.paths(si, goals) as hp:
        check_paths(hp, seeds[si], goals, ref, (mode,))
        assert hp.hops.max() >= 8, hp.hops.max()
    for i in picked[:4]:
        check_rows(res, int(i), seeds[i], A, ref, (mode,))
    res.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------------------------------
def test_edges():
    from hypergraphdb_amd import bfs_batch
    # a path 0-1-2-3-4, the isolated node 5 and a separate pair 6-7
    g = builder_graph(8, [(0, 1), (1, 2), (2, 3), (3, 4), (6, 7)])
    A = g["num_atoms"]
    snap, orc = snapshot(g), oracle(g)
    ref = Ref(orc, R.MODES[0])
    seeds = np.array([0, 5, 6], np.int32)
    res = bfs_batch(snap, seeds)
    with res.paths([0, 0, 0, 1, 1, 2], [0, 4, 6, 5, 0, 7]) as hp:
        assert hp.hops.tolist() == [0, 4, -1, 0, -1, 1] and hp.total_atoms == 1 + 5 + 1 + 2
        assert hp.path(0)[0].tolist() == [0] and len(hp.path(0)[1]) == 0       # goal == seed
        assert hp.path(1)[0].tolist() == [0, 1, 2, 3, 4] and hp.path(1)[1].tolist() == [8, 9, 10, 11]
        assert len(hp.path(2)[0]) == 0 and len(hp.path(2)[1]) == 0             # unreachable
        assert hp.path(3)[0].tolist() == [5]                                   # a seed without incidence
        assert hp.path(5)[0].tolist() == [6, 7] and hp.path(5)[1].tolist() == [12]
        check_paths(hp, seeds[[0, 0, 0, 1, 1, 2]], [0, 4, 6, 5, 0, 7], ref)
    for i in range(3):
        check_rows(res, i, seeds[i], A, ref)
    with res.paths([], []) as hp:                                              # n_pairs = 0
        assert hp.n_pairs == 0 and hp.total_atoms == 0 and len(hp.hops) == 0
        assert hp.stats()["steps"] == 0
    res.close()
    res = bfs_batch(snap, seeds, 2)                                            # max_depth = 2
    with res.paths([0, 0, 0], [2, 3, 4]) as hp:
        assert hp.hops.tolist() == [2, -1, -1] and hp.path(0)[0].tolist() == [0, 1, 2]
    check_rows(res, 0, 0, A, Ref(orc, R.MODES[0], -1, 2))
    res.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 7. agreement with the relaxation engine (both are rule R with strictly inflationary weights)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mi", [0, 1])
def test_agrees_with_shortest_paths(mi):
    from hypergraphdb_amd import hop_paths, shortest_paths
    g, snap, _, seeds = power_law()
    A = g["num_atoms"]
    mode = K.ALGEN_MODES[mi]
    rng = np.random.default_rng(60 + mi)
    starts = seeds[rng.integers(0, 40, 200)]
    goals = rng.integers(0, A, 200).astype(np.int32)
    goals[::2] = rng.integers(0, g["n_nodes"], 100)
    with hop_paths(snap, starts, goals, gen(snap, mode)) as hp, \
            shortest_paths(snap, np.concatenate([starts, starts[:2]]), list(goals) + [None, None], gen(snap, mode)) as sp:
        exp = np.where(hp.reached, hp.hops.astype(np.float64), np.inf)
        assert np.array_equal(exp.view(np.uint64), sp.distance[:200].view(np.uint64))
        assert np.array_equal(hp.reached, sp.reached[:200]) and hp.reached.sum() >= 20
        for i in range(200):
            a, l = hp.path(i)
            b, m = sp.path(i)
            assert np.array_equal(a, b) and np.array_equal(l, m), (mi, i)
        for k in range(2):                                 # the rows of two NO_GOAL pairs
            i = int(np.nonzero(hp.owner.seeds == starts[k])[0][0])
            d = sp.distances(200 + k)
            assert np.array_equal(np.where(np.isfinite(d), d, -1).astype(np.int32), hp.owner.depths(i))
            pa, pl = sp.predecessors(200 + k)
            qa, ql = hp.owner.predecessors(i)
            assert np.array_equal(pa, qa) and np.array_equal(pl, ql)


# ---------------------------------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------------------------------
def test_errors():
    from hypergraphdb_amd import HGXError, HGXUnsupported, _lib, bfs_batch
    from hypergraphdb_amd.partition import Shard, ShardSnapshot, partition_plan, pbfs_batch_group
    g = K.queries_graph()
    A = g["num_atoms"]
    snap = snapshot(g)
    res = bfs_batch(snap, [0, 1])
    with pytest.raises(HGXError) as e:
        res.paths([0, 1, 0], [1, 2, A])
    assert e.value.code == _lib.HGX_E_INVALID and "pair 2" in str(e.value) and "hgx_bfs_result_paths" in str(e.value)
    with pytest.raises(HGXError) as e:
        res.paths([0], [-1])
    assert e.value.code == _lib.HGX_E_INVALID and "pair 0" in str(e.value)
    for bad in (2, -1):
        with pytest.raises(HGXError) as e:
            res.paths([0, bad], [1, 1])
        assert e.value.code == _lib.HGX_E_NOTFOUND
        with pytest.raises(HGXError) as e:
            res.depths(bad)
        assert e.value.code == _lib.HGX_E_NOTFOUND
        with pytest.raises(HGXError) as e:
            res.predecessors(bad)
        assert e.value.code == _lib.HGX_E_NOTFOUND
    with pytest.raises(HGXError) as e:
        res.depths(0, 1, A)                 # past the last atom
    assert e.value.code == _lib.HGX_E_INVALID
    hp = res.paths([0], [1])
    hp.close()
    with pytest.raises(ValueError):
        hp.stats()
    res.close()
    with pytest.raises(ValueError):         # a closed result
        res.paths([0], [1])
    with pytest.raises(ValueError):
        res.depths(0)
    # a partition shard's result holds owned atoms only
    plan = partition_plan(A, g["link_atom"], g["tgt_off"], g["tgt_idx"], g.get("link_type"), 2)
    sh = []
    for p in range(2):
        s = Shard.build(A, g["link_atom"], g["tgt_off"], g["tgt_idx"], g.get("link_type"), 2, p, plan)
        sh.append(ShardSnapshot(s, 0))
        s.close()
    pres = pbfs_batch_group(sh, [0, 1], None)
    for part in pres.parts:
        with pytest.raises(HGXUnsupported):
            part.paths([0], [1])
        with pytest.raises(HGXUnsupported):
            part.depths(0, 0, 1)
        with pytest.raises(HGXUnsupported):
            part.predecessors(0, 0, 1)
    pres.close()
    for s in sh:
        s.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 9. the mirror
# ---------------------------------------------------------------------------------------------------
def test_mirror():
    from hypergraphdb_amd import DefaultALGenerator, GraphClassics, HopPaths, hop_paths
    g = K.queries_graph()
    n = g["names"]
    snap, orc = snapshot(g), oracle(g)
    ref = Ref(orc, R.MODES[0])
    starts = [n["n5"], n["n0"], n["n5"], n["n10"], n["n0"], n["n6"]]          # duplicate starts
    goals = [n["n3"], n["n1"], n["n1"], n["n0"], n["n0"], n["n3"]]
    with hop_paths(snap, starts, goals) as hp:
        assert isinstance(hp, HopPaths) and hp.owner.n_seeds == 4
        check_paths(hp, starts, goals, ref)
        assert hp.hops[1] == 1 and hp.hops[3] == -1 and hp.hops[4] == 0 and hp.hops[0] == hp.hops[5]
    assert hp.owner._h is None              # the BFS result closed with it
    far = [q for q, d in ref.of(n["n5"])[0].items() if d == 2]
    with hop_paths(snap, [n["n5"], n["n5"]], [far[0], n["n1"]], max_depth=1) as hp:
        assert hp.hops.tolist() == [-1, 1]
    al = DefaultALGenerator(snap)
    assert GraphClassics.dijkstra(n["n0"], n["n1"], al) == 1.0
    assert GraphClassics.dijkstra(n["n10"], n["n0"], al) is None
    d = GraphClassics.dijkstra(n["n5"], n["n3"], al)
    assert isinstance(d, float) and d == GraphClassics.dijkstra(n["n6"], n["n3"], al) == float(ref.of(n["n5"])[0][n["n3"]])
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 10. execution contexts: paths on a context while the parent snapshot runs a BFS
# ---------------------------------------------------------------------------------------------------
def test_context_next_to_parent():
    from hypergraphdb_amd import bfs_batch
    g, snap, orc, seeds = power_law()
    A = g["num_atoms"]
    mode = K.ALGEN_MODES[0]
    ref = Ref(orc, mode)
    ctx = snap.context()
    res = bfs_batch(ctx, seeds[:128], None, gen(ctx, mode))
    rng = np.random.default_rng(3)
    si = np.repeat([0, 127], 30).astype(np.int32)
    goals = rng.integers(0, A, 60).astype(np.int32)
    out, err = {}, []

    def paths():
        try:
            out["hp"] = res.paths(si, goals)
        except Exception as e:   # noqa: BLE001
            err.append(e)

    def parent():
        try:
            r = bfs_batch(snap, seeds, None, gen(snap, mode))
            out["levels"] = r.n_levels
            r.close()
        except Exception as e:   # noqa: BLE001
            err.append(e)

    th = [threading.Thread(target=paths), threading.Thread(target=parent)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    assert out["levels"] >= 2
    check_paths(out["hp"], seeds[si], goals, ref)
    out["hp"].close()
    res.close()
    ctx.close()
