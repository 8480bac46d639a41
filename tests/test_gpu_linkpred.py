"""GPU parity: traversals over any accelerated link predicate (include/hgx_linkpred.h).

DefaultALGenerator.generate() calls linkPredicate.satisfies(graph, link) once per incident link and nowhere else
(C/algorithms/DefaultALGenerator.java:300-308), so the expected output of a predicate traversal on ``g`` is the
frozen oracle's output on ``linkpred_ref.flagged(g, tree)`` -- the graph with link_type = the predicate's flags,
evaluated by direct recursion over the tree -- with algen(link_type=1).  Everything is compared exactly: flags,
per-depth sets and counts, next() sequences pair by pair, distances bit for bit, hop paths and predecessor rows.

Shapes: random_graph(600, 2500, max_arity=12, 3 types) has rows past the 8 register targets of the evaluation
kernel, links targeting links, repeated targets and M no multiple of 64; synth.hypergraph(3000, 20000, ...) has hubs
(heavy incidence chunks); config5(scale=0.002) holds the closures; one deep chain of 300 levels."""
import ctypes as C

import numpy as np
import pytest

import deep_graphs as D
import kat_graphs as K
import linkpred_ref as LP
import sp_ref as R
from oracle_ctypes import algen
from test_gpu_bfs import gen, gpu_levels, levels_from_seq, oracle, snapshot
from test_gpu_hops import Ref, check_paths, check_rows

pytestmark = pytest.mark.gpu
_CACHE = {}


def opt(name):
    from hypergraphdb_amd import _lib
    return getattr(_lib, "HGX_OPT_" + name)


def pgen(snap, mode, pred):
    from hypergraphdb_amd import DefaultALGenerator
    return DefaultALGenerator(snap, pred, None, *mode)


def random_case():
    """The random graph, three predicate trees over it, their reference flags and the oracles of the flagged graphs."""
    if "random" not in _CACHE:
        from hypergraphdb_amd import hg
        from hypergraphdb_amd.query import ANY
        rng = np.random.default_rng(20261)
        g = K.random_graph(rng, 600, 2500, max_arity=12, n_types=3)
        deg = np.bincount(g["tgt_idx"], minlength=g["num_atoms"])
        x = int(np.argmax(deg))                                  # the atom most links touch
        a = int(g["tgt_idx"][g["tgt_off"][np.argmax(np.diff(g["tgt_off"]) >= 3)]])   # the first target of a link
        trees = {"typeplus": hg.typePlus([0, 2]),
                 "type_not_incident": hg.and_(hg.type(1), hg.not_(hg.incident(x))),
                 "arity_or_ordered": hg.or_(hg.arity(2), hg.orderedLink(a, ANY))}
        fl = {k: LP.flags(g, t) for k, t in trees.items()}
        for k, f in fl.items():
            assert 0 < f.sum() < len(f), k
        orcs = {k: oracle(LP.flagged(g, None, f)) for k, f in fl.items()}
        seeds = {n: rng.integers(0, g["num_atoms"], n).astype(np.int32) for n in (300, 1024)}
        _CACHE["random"] = (g, x, a, trees, fl, orcs, seeds)
    return _CACHE["random"]


def check_sets(res, seeds, maxd, mode, orc_flagged, sample, tag=()):
    """Counts of every seed and the sets of the sampled seeds against the oracle on the flagged graph."""
    counts = res.counts()
    nl = counts.shape[1]
    oc, _ = orc_flagged.bfs_many(seeds, -1 if maxd is None else maxd, nl + 2, algen(1, *mode))
    assert np.array_equal(oc[:, :nl], counts) and not oc[:, nl:].any(), (tag, mode, maxd)
    for i in sample:
        l, a, d, _ = orc_flagged.bfs(int(seeds[i]), -1 if maxd is None else maxd, algen(1, *mode))
        exp = levels_from_seq(int(seeds[i]), zip(l.tolist(), a.tolist(), d.tolist()))
        assert gpu_levels(res, i) == exp, (tag, i, int(seeds[i]), mode, maxd)


def check_seq(res, seeds, maxd, mode, orc_flagged, tag=()):
    trav = 0
    for i, s in enumerate(seeds):
        l, a, d, tr = orc_flagged.bfs(int(s), -1 if maxd is None else maxd, algen(1, *mode))
        gl, ga, gd = res.pairs(i)
        assert np.array_equal(ga, a), (tag, i, s, mode, maxd, "atoms")
        assert np.array_equal(gl, l), (tag, i, s, mode, maxd, "links")
        assert np.array_equal(gd, d), (tag, i, s, mode, maxd, "dists")
        trav += tr
    assert res.traversed_edges == float(trav), (tag, mode, maxd)


def seq_on(snap, seeds, maxd, g_, engine):
    from hypergraphdb_amd import bfs_sequence
    snap.set_option(opt("SEQ_ENGINE"), engine)
    try:
        return bfs_sequence(snap, seeds, maxd, g_)
    finally:
        snap.set_option(opt("SEQ_ENGINE"), 0)


# ---------------------------------------------------------------------------------------------------
# 1. the evaluation kernel on its own: flags and the device count
# ---------------------------------------------------------------------------------------------------
def leaf_trees(g, x, a):
    """Every leaf kind alone (to be used at both polarities), chosen so that each accepts some links only."""
    from hypergraphdb_amd import hg
    from hypergraphdb_amd.query import ANY
    off, tg = g["tgt_off"], g["tgt_idx"]
    long_row = int(np.argmax(np.diff(off) >= 10))               # a row past the 8 register targets
    lt = tg[off[long_row]:off[long_row + 1]].tolist()
    late = next(t for t in lt[8:] if t not in lt[:8]) if any(t not in lt[:8] for t in lt[8:]) else lt[-1]
    ar = np.diff(off)
    plain = next(r for r in range(len(ar)) if ar[r] >= 2 and len(set(tg[off[r]:off[r + 1]].tolist())) == ar[r])
    two = tg[off[plain]:off[plain] + 2].tolist()                # two targets of a link without a repeated target
    return {"type": hg.type(1), "typePlus": hg.typePlus([0, 2]), "incident": hg.incident(x),
            "incident_tail": hg.incident(late),                 # found only by the loop over the tail
            "incidentAt": hg.incidentAt(x, 0, 1), "incidentAt_end": hg.incidentAt(lt[-1], -1),
            "incidentNotAt": hg.incidentNotAt(x, 0), "orderedLink": hg.orderedLink(a, ANY),
            "orderedLink_tail": hg.orderedLink(lt[0], ANY, late), "orderedLink_empty": hg.orderedLink(),
            "link": hg.link(*two), "link_any": hg.link(x, ANY), "arity": hg.arity(2), "arity_long": hg.arity(len(lt))}


def test_flags_every_leaf_kind_both_polarities_and_paging():
    from hypergraphdb_amd import LinkPredicate, hg
    g, x, a, trees, fl, _, _ = random_case()
    M = len(g["link_atom"])
    assert M % 64 != 0 and (np.diff(g["tgt_off"]) > 8).any()
    snap = snapshot(g)
    snap.set_timing(True)
    cases = {}
    for k, leaf in leaf_trees(g, x, a).items():
        cases[k] = leaf
        cases["not_" + k] = hg.not_(leaf)
    cases.update(empty_or=hg.or_(), empty_and=hg.and_(), type_only=hg.or_(hg.type(0), hg.and_(hg.typePlus([1, 2]), hg.not_(hg.arity(3)))),
                 mixed=hg.or_(hg.and_(hg.type(1), hg.not_(hg.incident(x))), hg.and_(hg.arity(2), hg.orderedLink(ANY_())),
                              hg.not_(hg.or_(hg.typePlus([0, 1]), hg.link(x)))), **trees)
    seen_mixed = 0
    for k, tree in cases.items():
        exp = LP.flags(g, tree)
        with LinkPredicate(snap, tree) as p:
            assert p.num_links == M and p.num_satisfied == int(exp.sum()), (k, p.num_satisfied, int(exp.sum()))
            got = p.flags()
            assert got.dtype == np.uint8 and np.array_equal(got, exp), (k, np.nonzero(got != exp)[0][:8])
            st = p.stats()
            assert st["ms_eval"] > 0 and st["bytes_eval"] >= 12.0 * M, (k, st)
            if k == "mixed":                                   # paged readback at the wave boundaries
                for first, n in ((0, 0), (0, 1), (0, 64), (63, 2), (64, 64), (65, 127), (M - 1, 1), (M - 64, 64), (M, 0),
                                 (M // 2, M - M // 2)):
                    assert np.array_equal(p.flags(first, n), exp[first:first + n]), (first, n)
        seen_mixed += 0 < exp.sum() < M
    assert LP.flags(g, cases["empty_or"]).sum() == 0 and LP.flags(g, cases["empty_and"]).sum() == M
    assert seen_mixed >= len(cases) - 6                         # (the two empties, the empty pattern, link_any and their negations)
    snap.close()


def ANY_():
    from hypergraphdb_amd.query import ANY
    return ANY


def test_type_only_program_reads_no_targets():
    """The algorithmic bytes of a type / arity program hold no target read; a target-reading program adds 4 bytes
    per target."""
    from hypergraphdb_amd import LinkPredicate, hg
    g, x, _, _, _, _, _ = random_case()
    M, P = len(g["link_atom"]), len(g["tgt_idx"])
    snap = snapshot(g)
    I = int(sum(len(snap.incidence(int(t))) for t in np.unique(g["tgt_idx"])))
    with LinkPredicate(snap, hg.and_(hg.typePlus([0, 1]), hg.not_(hg.arity(2)))) as p:
        assert p.stats()["bytes_eval"] == 8.0 * (M + 1) + 4.0 * M + 4.0 * M + 12.0 * I
    with LinkPredicate(snap, hg.arity(2)) as p:                # no type read either
        assert p.stats()["bytes_eval"] == 8.0 * (M + 1) + 4.0 * M + 12.0 * I
    with LinkPredicate(snap, hg.incident(x)) as p:
        assert p.stats()["bytes_eval"] == 8.0 * (M + 1) + 4.0 * P + 4.0 * M + 12.0 * I
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 2. per-depth sets: every mode, default engines and the rows engine, 300 / 1024 seeds, bounded and not
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", (1, 0))
@pytest.mark.parametrize("name", ("typeplus", "type_not_incident", "arity_or_ordered"))
def test_set_bfs_every_mode(name, block):
    from hypergraphdb_amd import LinkPredicate, bfs_batch
    g, _, _, trees, _, orcs, seeds = random_case()
    snap = snapshot(g)
    snap.set_option(opt("BFS_BLOCK"), block)
    with LinkPredicate(snap, trees[name]) as p:
        for mode in K.ALGEN_MODES:
            for n, maxd in ((300, None), (300, 2), (1024, None), (1024, 3)):
                res = bfs_batch(snap, seeds[n], maxd, pgen(snap, mode, p))
                check_sets(res, seeds[n], maxd, mode, orcs[name], (0, 1, 63, 64, n // 2, n - 1), (name, block, n))
                res.close()
    snap.close()


def test_set_bfs_raw_tree_hubs_and_heavy_chunks():
    """A power-law graph (hub atoms, heavy incidence chunks), the tree given raw to the generator (compiled per
    call, released when the call returns: the result keeps it alive)."""
    from hypergraphdb_amd import bfs_batch, hg, synth
    g = synth.hypergraph(3000, 20000, 2, 8, 2.1, 3, seed=21)
    hub = int(np.argmax(np.bincount(g["tgt_idx"], minlength=g["num_atoms"])))
    tree = hg.or_(hg.and_(hg.type(0), hg.not_(hg.arity(2))), hg.and_(hg.typePlus([1, 2]), hg.incident(hub)))
    f = LP.flags(g, tree)
    assert 0 < f.sum() < len(f)
    orc = oracle(LP.flagged(g, None, f))
    rng = np.random.default_rng(8)
    seeds = np.concatenate([[hub], rng.integers(0, g["num_atoms"], 299)]).astype(np.int32)
    for block in (1, 0):
        snap = snapshot(g)
        snap.set_option(opt("BFS_BLOCK"), block)
        for mode in (K.ALGEN_MODES[0], K.ALGEN_MODES[1], K.ALGEN_MODES[5], K.ALGEN_MODES[6]):
            for maxd in (None, 2):
                res = bfs_batch(snap, seeds, maxd, pgen(snap, mode, tree))
                check_sets(res, seeds, maxd, mode, orc, (0, 1, 150, 299), ("hubs", block))
                res.close()
        snap.close()


def test_kat_graphs_sets_and_sequences_every_seed_every_mode():
    from hypergraphdb_amd import bfs_batch, bfs_sequence, hg
    for make in (K.linkage_graph, K.queries_graph, K.pattern_graph):
        g = make()
        ty = LP.link_types(g)
        first = int(g["tgt_idx"][0])
        tree = hg.or_(hg.and_(hg.type(int(ty[0])), hg.not_(hg.incident(first))), hg.arity(3))
        f = LP.flags(g, tree)
        orc = oracle(LP.flagged(g, None, f))
        snap = snapshot(g)
        seeds = np.arange(g["num_atoms"], dtype=np.int32)
        for mode in K.ALGEN_MODES:
            for maxd in (None, 1):
                res = bfs_batch(snap, seeds, maxd, pgen(snap, mode, tree))
                check_sets(res, seeds, maxd, mode, orc, range(len(seeds)), make.__name__)
                res.close()
                check_seq(bfs_sequence(snap, seeds, maxd, pgen(snap, mode, tree)), seeds, maxd, mode, orc, make.__name__)
        snap.close()


def config5_case():
    if "c5" not in _CACHE:
        from hypergraphdb_amd import TypePlusCondition, synth
        g = synth.config5(scale=0.002, n_sources=500)
        T = int(g["subsumes_type"])
        tree = TypePlusCondition([T])
        f = LP.flags(g, tree)
        assert np.array_equal(f, (g["link_type"] == T).astype(np.uint8))
        _CACHE["c5"] = (g, T, tree, oracle(LP.flagged(g, None, f)), oracle(g))
    return _CACHE["c5"]


def test_config5_closures_both_directions():
    """hg.subsumed / hg.subsumes closures with a TypePlusCondition over the subsumes type: sets on both engines,
    sequences with the root classes among the seeds (closures beyond one workgroup's pairs)."""
    from hypergraphdb_amd import bfs_batch, bfs_sequence
    g, T, tree, orc, _ = config5_case()
    seeds = np.asarray(g["seeds"], np.int32)
    for block in (1, 0):
        snap = snapshot(g)
        snap.set_option(opt("BFS_BLOCK"), block)
        for rev in (False, True):
            mode = (False, True, rev, False)
            res = bfs_batch(snap, seeds, None, pgen(snap, mode, tree))
            check_sets(res, seeds, None, mode, orc, (0, 1, 250, 499), ("c5", block, rev))
            res.close()
        snap.close()
    snap = snapshot(g)
    sseeds = np.concatenate([np.arange(6, dtype=np.int32), seeds[:58]])
    for rev in (False, True):
        mode = (False, True, rev, False)
        for eng in (0, 2):
            res = seq_on(snap, sseeds, None, pgen(snap, mode, tree), eng)
            check_seq(res, sseeds, None, mode, orc, ("c5", rev, eng))
            if eng == 2:
                assert res.n_block == 0 and res.n_level == len(sseeds)
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 3. the predicate type(T) is the AtomTypeCondition(T) path
# ---------------------------------------------------------------------------------------------------
def test_type_predicate_equals_typed_generator():
    from hypergraphdb_amd import LinkPredicate, bfs_batch, bfs_sequence, hg
    g, _, _, _, _, _, seeds = random_case()
    snap = snapshot(g)
    s = seeds[300]
    with LinkPredicate(snap, hg.type(1)) as p:
        for mode in K.ALGEN_MODES:
            for maxd in (None, 2):
                a, b = bfs_batch(snap, s, maxd, gen(snap, mode, 1)), bfs_batch(snap, s, maxd, pgen(snap, mode, p))
                assert a.n_levels == b.n_levels and np.array_equal(a.counts(), b.counts()), (mode, maxd)
                for i in (0, 1, 150, 299):
                    assert gpu_levels(a, i) == gpu_levels(b, i), (mode, maxd, i)
                a.close()
                b.close()
                qa, qb = bfs_sequence(snap, s, maxd, gen(snap, mode, 1)), bfs_sequence(snap, s, maxd, pgen(snap, mode, p))
                assert np.array_equal(qa.offsets, qb.offsets) and np.array_equal(qa.atoms, qb.atoms)
                assert np.array_equal(qa.links, qb.links) and np.array_equal(qa.dists, qb.dists)
                assert qa.traversed_edges == qb.traversed_edges and qa.n_levels == qb.n_levels
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 4. order-exact sequences: every mode on the workgroup (+ grid), key-array and level engines
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("typeplus", "type_not_incident", "arity_or_ordered"))
def test_sequences_every_mode_every_engine(name):
    from hypergraphdb_amd import LinkPredicate
    g, _, _, trees, _, orcs, seeds = random_case()
    snap = snapshot(g)
    s = np.concatenate([seeds[300][:99], seeds[300][:1]])
    with LinkPredicate(snap, trees[name]) as p:
        for mode in K.ALGEN_MODES:
            for maxd in (None, 2):
                for eng in (0, 1, 2):
                    check_seq(seq_on(snap, s, maxd, pgen(snap, mode, p), eng), s, maxd, mode, orcs[name], (name, eng))
    snap.close()


def test_sequence_grid_stage_closures():
    """The seeds whose closure outgrows a workgroup's 2046 pairs run on the order-exact grid stage, which needs
    the generator's yield adjacency -- here the predicate's own: the root classes of config 5 under typePlus."""
    from hypergraphdb_amd import LinkPredicate, bfs_batch, bfs_sequence
    g, T, tree, orc, _ = config5_case()
    snap = snapshot(g)
    mode = (False, True, False, False)
    with LinkPredicate(snap, tree) as p:
        cand = np.arange(2000, dtype=np.int32)
        r = bfs_batch(snap, cand, None, pgen(snap, mode, p))
        size = r.counts()[:, 1:].sum(1)
        r.close()
        # closures that outgrow the workgroup engine's 2046 pairs and stay below the stage's per-level key space,
        # picked as tests/test_gpu_seq.py picks them
        big = cand[(size > 2100) & (size < 30000)][:4]
        assert len(big) >= 1, size.max()                        # (class 0's closure is most of the 10000 classes)
        seeds = np.concatenate([big, np.asarray(g["seeds"][:20], np.int32)])
        for maxd in (None, 3):
            res = bfs_sequence(snap, seeds, maxd, pgen(snap, mode, p))
            check_seq(res, seeds, maxd, mode, orc, ("grid", maxd))
            if maxd is None:                                    # the grid stage finished every seed handed on
                assert res.n_coop >= 1 and res.n_coop == res.n_level, (res.n_coop, res.n_level)
                assert res.n_block + res.n_level == len(seeds) and res.n_level >= len(big), (res.n_block, res.n_level)
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 5. weighted shortest paths, hop paths, predecessor rows, GraphClassics.dijkstra
# ---------------------------------------------------------------------------------------------------
def u64(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", ("typeplus", "type_not_incident", "arity_or_ordered"))
def test_shortest_paths_random_weights(name):
    from hypergraphdb_amd import GraphClassics, LinkPredicate, shortest_paths
    g, _, _, trees, _, orcs, _ = random_case()
    A = g["num_atoms"]
    rng = np.random.default_rng(55)
    w = rng.integers(1, 9, len(g["link_atom"])).astype(np.float64) * 0.37
    wf = R.row_weights(g, w)
    snap = snapshot(g)
    starts = rng.integers(0, A, 3).tolist()
    pairs = [(s, None) for s in starts] + [(s, int(q)) for s in starts for q in rng.integers(0, A, 4)]
    with LinkPredicate(snap, trees[name]) as p:
        for mode in (K.ALGEN_MODES[0], K.ALGEN_MODES[5]):     # (the reference Dijkstra is Python: a few seconds)
            opts = R.opts_of(mode, 1)
            genf = R.memo_generate(orcs[name], opts)
            with shortest_paths(snap, [x[0] for x in pairs], [x[1] for x in pairs], pgen(snap, mode, p), w) as res:
                rows = {s: R.dijkstra(orcs[name], s, None, opts, wf)[1] for s in starts}   # every final distance of s
                for i, (s, q) in enumerate(pairs):
                    dm = rows[s]
                    d = None if q is None else dm.get(q)
                    if q is None:
                        row = np.full(A, np.inf)
                        for n, v in dm.items():
                            row[n] = v
                        assert np.array_equal(u64(res.distances(i)), u64(row)), (name, mode, i)
                        continue
                    assert bool(res.reached[i]) == (d is not None), (name, mode, i)
                    assert u64(res.distance[i]) == u64(np.inf if d is None else d), (name, mode, i)
                    atoms, links = res.path(i)
                    if d is None:
                        assert len(atoms) == 0
                    else:
                        R.check_path(genf, wf, s, q, atoms, links, d)     # valid under the predicate, of that length
            s, q = pairs[len(starts)]
            d = rows[s].get(q)
            assert GraphClassics.dijkstra(s, q, pgen(snap, mode, trees[name]), w) == d     # a raw tree, compiled per call
    snap.close()


@pytest.mark.parametrize("block", (1, 0))
def test_hop_paths_and_predecessor_rows(block):
    from hypergraphdb_amd import LinkPredicate, bfs_batch, hop_paths
    g, _, _, trees, _, orcs, _ = random_case()
    A = g["num_atoms"]
    rng = np.random.default_rng(66)
    snap = snapshot(g)
    snap.set_option(opt("BFS_BLOCK"), block)
    for name in ("type_not_incident", "arity_or_ordered"):
        for mode in (K.ALGEN_MODES[0], K.ALGEN_MODES[1], K.ALGEN_MODES[3]):
            ref = Ref(orcs[name], mode, 1)
            starts = rng.integers(0, A, 40).astype(np.int32)
            goals = rng.integers(0, A, 40).astype(np.int32)
            with hop_paths(snap, starts, goals, pgen(snap, mode, trees[name])) as hp:      # raw tree
                check_paths(hp, starts, goals, ref, (name, mode))
            with LinkPredicate(snap, trees[name]) as p:
                res = bfs_batch(snap, starts[:3], None, pgen(snap, mode, p))
            for i in range(3):                                  # (the predicate is closed: the result holds it)
                check_rows(res, i, int(starts[i]), A, ref, (name, mode))
            res.close()
    snap.close()


def test_find_all_bfs_condition_with_a_tree():
    from hypergraphdb_amd import find_all, hg
    g, _, _, trees, _, orcs, seeds = random_case()
    snap = snapshot(g)
    for name, tree in trees.items():
        s = int(seeds[300][7])
        _, a, _, _ = orcs[name].bfs(s, -1, algen(1, True, True, False, False))
        assert find_all(snap, hg.bfs(s, link_predicate=tree)) == a.tolist()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 6. the per-(mode, type) caches of the snapshot: a predicate is keyed apart from types and predicates
# ---------------------------------------------------------------------------------------------------
def test_cache_isolation_types_and_predicates():
    from hypergraphdb_amd import LinkPredicate, bfs_batch, bfs_sequence, hg
    g, x, _, trees, fl, orcs, seeds = random_case()
    A_tree = trees["type_not_incident"]
    B_tree = hg.not_(A_tree)
    C_tree = hg.or_(hg.type(0), hg.arity(3))
    fB, fC = LP.flags(g, B_tree), LP.flags(g, C_tree)
    assert np.array_equal(fB, 1 - fl["type_not_incident"])
    orc_T, orc_A = oracle(g), orcs["type_not_incident"]
    orc_B, orc_C = oracle(LP.flagged(g, None, fB)), oracle(LP.flagged(g, None, fC))
    s = seeds[300][:64]
    snap = snapshot(g)

    def typed(mode):
        gn = gen(snap, mode, 1)
        res = bfs_batch(snap, s, None, gn)
        counts = res.counts()
        oc, _ = orc_T.bfs_many(s, -1, counts.shape[1] + 2, algen(1, *mode))
        assert np.array_equal(oc[:, :counts.shape[1]], counts) and not oc[:, counts.shape[1]:].any(), mode
        for i in (0, 63):
            l, a, d, _ = orc_T.bfs(int(s[i]), -1, algen(1, *mode))
            assert gpu_levels(res, i) == levels_from_seq(int(s[i]), zip(l.tolist(), a.tolist(), d.tolist()))
        res.close()
        q = bfs_sequence(snap, s, None, gn)
        for i, sd in enumerate(s):
            l, a, d, _ = orc_T.bfs(int(sd), -1, algen(1, *mode))
            gl, ga, gd = q.pairs(i)
            assert np.array_equal(ga, a) and np.array_equal(gl, l) and np.array_equal(gd, d), ("typed", mode, i)

    def with_pred(p, orc, mode, tag):
        res = bfs_batch(snap, s, None, pgen(snap, mode, p))
        check_sets(res, s, None, mode, orc, (0, 63), tag)
        res.close()
        check_seq(bfs_sequence(snap, s, None, pgen(snap, mode, p)), s, None, mode, orc, tag)

    for block in (1, 0):
        snap.set_option(opt("BFS_BLOCK"), block)
        for mode in (K.ALGEN_MODES[1], K.ALGEN_MODES[2], K.ALGEN_MODES[4], K.ALGEN_MODES[7]):   # ordered modes
            pA, pB = LinkPredicate(snap, A_tree), LinkPredicate(snap, B_tree)
            typed(mode)
            with_pred(pA, orc_A, mode, "A")
            typed(mode)
            with_pred(pB, orc_B, mode, "B")
            with_pred(pA, orc_A, mode, "A again")
            pA.close()                                          # its lists go with it ...
            with LinkPredicate(snap, C_tree) as pC:             # ... and a third predicate may land on its memory
                with_pred(pC, orc_C, mode, "C")
                with_pred(pB, orc_B, mode, "B after C")
            with LinkPredicate(snap, A_tree) as pA2:
                with_pred(pA2, orc_A, mode, "A recreated")
            typed(mode)
            pB.close()
    # many short-lived predicates do not use up the snapshot's list slots: the typed lists still build
    for k in range(12):
        with LinkPredicate(snap, hg.or_(hg.arity(2 + k % 3), hg.type(k % 3))) as p:
            bfs_sequence(snap, s[:4], 2, pgen(snap, K.ALGEN_MODES[1], p))
    typed(K.ALGEN_MODES[5])
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 7. lifetime and errors
# ---------------------------------------------------------------------------------------------------
def test_result_outlives_its_predicate_and_update_is_blocked():
    from hypergraphdb_amd import HGXError, LinkPredicate, _lib, bfs_batch
    g, _, _, trees, _, orcs, _ = random_case()
    A = g["num_atoms"]
    mode = K.ALGEN_MODES[0]
    ref = Ref(orcs["arity_or_ordered"], mode, 1)
    snap = snapshot(g)
    snap.set_option(opt("BFS_BLOCK"), 0)
    p = LinkPredicate(snap, trees["arity_or_ordered"])
    starts = np.array([5, 17, 300], np.int32)
    res = bfs_batch(snap, starts, None, pgen(snap, mode, p))
    p.close()
    goals = np.array([17, 400, 5], np.int32)
    with res.paths(np.arange(3, dtype=np.int32), goals) as hp:   # reads the predicate's flags after its free
        check_paths(hp, starts, goals, ref)
    check_rows(res, 1, 17, A, ref)
    new_link = {A: (0, [1, 2])}
    with pytest.raises(HGXError) as e:                          # the result (and through it the predicate) lives
        snap.update(add=new_link, num_atoms=A + 1)
    assert e.value.code == _lib.HGX_E_INVALID
    res.close()
    p2 = LinkPredicate(snap, trees["typeplus"])
    with pytest.raises(HGXError) as e:                          # a live predicate alone blocks the update
        snap.update(add=new_link, num_atoms=A + 1)
    assert e.value.code == _lib.HGX_E_INVALID
    p2.close()
    snap.update(add=new_link, num_atoms=A + 1)                  # accepted once it is freed
    assert snap.M == len(g["link_atom"]) + 1
    snap.close()


def test_predicate_on_contexts_and_other_graphs():
    from hypergraphdb_amd import HGXError, LinkPredicate, _lib, bfs_batch, bfs_sequence, shortest_paths
    g, _, _, trees, _, orcs, seeds = random_case()
    snap, other = snapshot(g), snapshot(g)
    ctx = snap.context()
    mode = K.ALGEN_MODES[1]
    s = seeds[300][:32]
    with LinkPredicate(snap, trees["typeplus"]) as p, LinkPredicate(ctx, trees["arity_or_ordered"]) as pc:
        res = bfs_batch(ctx, s, None, pgen(ctx, mode, p))       # a predicate of the snapshot on its context
        check_sets(res, s, None, mode, orcs["typeplus"], (0, 31), "ctx")
        res.close()
        check_seq(bfs_sequence(ctx, s, None, pgen(ctx, mode, p)), s, None, mode, orcs["typeplus"], "ctx")
        check_seq(bfs_sequence(snap, s, 2, pgen(snap, mode, pc)), s, 2, mode, orcs["arity_or_ordered"], "made on ctx")
        for call in (lambda: bfs_batch(other, s, None, pgen(other, mode, p)),
                     lambda: bfs_sequence(other, s, None, pgen(other, mode, p)),
                     lambda: shortest_paths(other, [1], [2], pgen(other, mode, p))):
            with pytest.raises(HGXError) as e:
                call()
            assert e.value.code == _lib.HGX_E_INVALID and "another graph" in str(e.value)
        # a type next to a predicate: the type belongs inside the predicate
        L = _lib.lib()
        h = C.c_void_p()
        o = _lib.AlgenOpts(1, 1, 1, 0, 0)
        sp = np.ascontiguousarray(s)
        assert L.hgx_bfs_batch_pred(snap.handle, sp.ctypes.data, len(sp), -1, C.byref(o), p.handle, C.byref(h)) == \
            _lib.HGX_E_INVALID
        assert b"HGX_NO_TYPE" in L.hgx_last_error()
        assert L.hgx_bfs_sequence_pred(snap.handle, sp.ctypes.data, len(sp), -1, C.byref(o), p.handle, C.byref(h)) == \
            _lib.HGX_E_INVALID
        assert L.hgx_shortest_paths_pred(snap.handle, sp.ctypes.data, sp.ctypes.data, 1, C.byref(o), None, p.handle,
                                         C.byref(h)) == _lib.HGX_E_INVALID
        # a NULL predicate is the entry point without _pred
        assert L.hgx_bfs_batch_pred(snap.handle, sp.ctypes.data, len(sp), 2, C.byref(o), None, C.byref(h)) == _lib.HGX_OK
        a = bfs_batch(snap, s, 2, gen(snap, K.ALGEN_MODES[0], 1))
        from hypergraphdb_amd.algorithms import BfsResult
        b = BfsResult(snap, h, s)
        assert np.array_equal(a.counts(), b.counts())
        a.close()
        b.close()
    ctx.close()
    other.close()
    snap.close()


def test_contexts_created_and_closed_around_predicate_calls():
    """Execution contexts of the snapshot are created and closed from another thread while predicate traversals
    run on the snapshot (and on a context of their own): closing a context releases nothing the snapshot owns,
    whatever the snapshot's traversal sees as its type arrays at that moment.  Afterwards the typed traversal, a
    new predicate and the untyped traversal still equal the oracle."""
    import threading
    from hypergraphdb_amd import LinkPredicate, bfs_batch, bfs_sequence
    g, _, _, trees, fl, orcs, seeds = random_case()
    snap = snapshot(g)
    mode = K.ALGEN_MODES[1]
    s = seeds[1024]
    errors = []

    def traverse(target, name, rounds):
        try:
            for k in range(rounds):
                res = bfs_batch(target, s, None, pgen(target, mode, trees[name]))     # a raw tree: compiled per call
                check_sets(res, s, None, mode, orcs[name], (0, 1023), ("churn", name, k))
                res.close()
        except Exception as e:                                  # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    def churn(rounds):
        try:
            for _ in range(rounds):
                c = snap.context()
                c.close()
        except Exception as e:                                  # noqa: BLE001
            errors.append(e)

    own = snap.context()
    threads = [threading.Thread(target=traverse, args=(snap, "typeplus", 12)),
               threading.Thread(target=traverse, args=(own, "type_not_incident", 12)),
               threading.Thread(target=churn, args=(40,)), threading.Thread(target=churn, args=(40,))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    own.close()
    orc = oracle(g)
    for lt in (1, -1):                                          # the snapshot's own type arrays are intact
        res = bfs_batch(snap, s[:300], None, gen(snap, mode, lt))
        counts = res.counts()
        oc, _ = orc.bfs_many(s[:300], -1, counts.shape[1] + 2, algen(lt, *mode))
        assert np.array_equal(oc[:, :counts.shape[1]], counts) and not oc[:, counts.shape[1]:].any(), lt
        res.close()
    with LinkPredicate(snap, trees["arity_or_ordered"]) as p:   # reads link_type again
        assert np.array_equal(p.flags(), fl["arity_or_ordered"])
        check_seq(bfs_sequence(snap, s[:32], None, pgen(snap, mode, p)), s[:32], None, mode, orcs["arity_or_ordered"])
    snap.close()


def test_malformed_programs_and_shards_are_refused_before_any_launch():
    from hypergraphdb_amd import HGXUnsupported, LinkPredicate, _lib, hg
    from hypergraphdb_amd.partition import Shard, ShardSnapshot
    from hypergraphdb_amd.query import NOT_INCIDENT, NOT_ORDERED
    g = K.queries_graph()
    snap = snapshot(g)
    L = _lib.lib()

    def create(lit_off, lit, ops, graph=snap):
        h = C.c_void_p()
        lo, li, op = np.array(lit_off, np.int64), np.array(lit, np.int32), np.array(ops, np.int32)
        rc = L.hgx_link_predicate_create(graph.handle, len(lo) - 1, lo.ctypes.data, li.ctypes.data if len(li) else None,
                                         op.ctypes.data if len(op) else None, len(op), C.byref(h))
        assert (rc == _lib.HGX_OK) == bool(h.value)
        if h.value:
            L.hgx_link_predicate_free(h)
        return rc, L.hgx_last_error().decode()

    assert create([0, 1], [NOT_INCIDENT, 1, 0, 1], [3])[0] == _lib.HGX_OK
    rc, msg = create([0, 0, 1], [9, 1, 0, 1], [3])
    assert rc == _lib.HGX_E_INVALID and "term 1 literal 0" in msg and "unknown literal kind 9" in msg
    rc, msg = create([0, 1], [NOT_INCIDENT, 1, 0, 2], [3])
    assert rc == _lib.HGX_E_INVALID and "operand range outside ops" in msg
    rc, msg = create([0, 1], [NOT_INCIDENT, 1, 0, 1], [g["num_atoms"]])
    assert rc == _lib.HGX_E_INVALID and "atom id out of range" in msg
    rc, msg = create([0, 1], [NOT_ORDERED, 1, 0, 65], [1] * 65)
    assert rc == _lib.HGX_E_UNSUPPORTED and "term 0 literal 0" in msg
    assert create([0, 1], [NOT_ORDERED, 1, 0, 64], [1] * 64)[0] == _lib.HGX_OK
    rc, msg = create([0, 2, 1], [NOT_INCIDENT, 1, 0, 1, NOT_INCIDENT, 1, 0, 1], [3])
    assert rc == _lib.HGX_E_INVALID and "lit_off decreases" in msg
    M = len(g["link_atom"])
    sh = Shard.build(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"], 1, 0,
                     np.zeros(M, np.int32))
    ss = ShardSnapshot(sh)
    with pytest.raises(HGXUnsupported):
        LinkPredicate(ss, hg.arity(2))
    with LinkPredicate(snap, hg.arity(2)) as p:                 # and a shard takes no predicate of a snapshot
        h = C.c_void_p()
        seeds = np.zeros(1, np.int32)
        assert L.hgx_bfs_batch_pred(ss.handle, seeds.ctypes.data, 1, 1, None, p.handle, C.byref(h)) == \
            _lib.HGX_E_UNSUPPORTED
        assert L.hgx_bfs_sequence_pred(ss.handle, seeds.ctypes.data, 1, 1, None, p.handle, C.byref(h)) == \
            _lib.HGX_E_UNSUPPORTED
        assert L.hgx_shortest_paths_pred(ss.handle, seeds.ctypes.data, seeds.ctypes.data, 1, None, None, p.handle,
                                         C.byref(h)) == _lib.HGX_E_UNSUPPORTED
    ss.close()
    sh.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 8. a deep chain: every engine stops exactly at the link the predicate rejects
# ---------------------------------------------------------------------------------------------------
def test_deep_chain_stops_at_the_rejected_link():
    from hypergraphdb_amd import LinkPredicate, bfs_batch, hg
    n, cut = 400, 300
    g = D.path(n, rng=np.random.default_rng(3))
    pos = g["pos"]                                              # chain position -> atom; link i joins pos[i], pos[i + 1]
    tree = hg.not_(hg.link(int(pos[cut]), int(pos[cut + 1])))
    f = LP.flags(g, tree)
    assert f.sum() == len(f) - 1 and f[cut] == 0
    orc = oracle(LP.flagged(g, None, f))
    seeds = np.array([pos[0], pos[150], pos[cut + 1], pos[n - 1]], np.int32)
    for block in (1, 0):                                        # workgroup (+ grid stage) engines, rows engine
        snap = snapshot(g)
        snap.set_option(opt("BFS_BLOCK"), block)
        with LinkPredicate(snap, tree) as p:
            for mode in (D.SYM, D.FWD):
                res = bfs_batch(snap, seeds, None, pgen(snap, mode, p))
                check_sets(res, seeds, None, mode, orc, range(4), ("deep", block))
                c = res.counts()
                assert np.nonzero(c[0])[0].max() == cut and res.depth_of(0, int(pos[cut])) == cut   # 300 levels, then the cut
                assert res.depth_of(0, int(pos[cut + 1])) == -1
                res.close()
        snap.close()
    snap = snapshot(g)
    with LinkPredicate(snap, tree) as p:
        for eng in (0, 1, 2):
            for mode in (D.SYM, D.FWD):
                res = seq_on(snap, seeds, None, pgen(snap, mode, p), eng)
                check_seq(res, seeds, None, mode, orc, ("deep", eng))
                assert res.pairs(0)[1][-1] == pos[cut] and len(res.pairs(0)[1]) == cut
    snap.close()
