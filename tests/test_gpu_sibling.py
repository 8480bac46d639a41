"""GPU parity: batched traversals with a sibling predicate (include/hgx_sibling.h).

With a siblingPredicate the iterator of DefaultALGenerator yields the adjacency list of generate(src) without the
targets that fail it (DefaultALGenerator.java:120-150, 207-237), so the expected output of every traversal here is
the reference algorithm -- a plain level BFS, hop_ref.hop_rule, sp_ref.dijkstra_heap / rule_r -- run on
``sibling_ref.filtered(generate, keep)`` over the frozen oracle's generate.  Everything is compared exactly: flags,
per-depth sets and counts, hop paths and predecessor rows, distances bit for bit.

Shapes: random_graph(300, 400, 3 types) is 700 atoms, no multiple of 64, with links targeting links and repeated
targets; 1, 64, 65 and 1024 seeds give rows of 1, 1, 2 and 16 words, a partly filled last word and (1024 seeds on
700 atoms) many seeds on one atom; synth.hypergraph(3000, 20000, ...) has atoms above 512 incidences and above one
4096-entry chunk; deep_graphs.path(300) and ladder(40, 4) run hundreds / tens of levels.

Sets: counts() of every seed and depth always; visited(i, d) of every seed and depth for the batches of 1, 64 and 65
seeds and for the first symmetric and the first ordered mode of the unbounded 1024-seed batches under the mask that
keeps half, of seven sampled seeds (the first and the last, both sides of a word boundary, a failing seed, the
repeated atom) for the rest -- a reader call per seed and depth
over a thousand seeds, twelve modes, three masks and two option values would not stay within a few seconds."""
import ctypes as C

import numpy as np
import pytest

import deep_graphs as D
import kat_graphs as K
import linkpred_ref as LP
import sibling_ref as SR
import sp_ref as R
from test_gpu_bfs import gpu_levels, oracle, snapshot
from test_gpu_hops import Ref, check_paths, check_rows
from test_gpu_linkpred import leaf_trees, opt, u64

pytestmark = pytest.mark.gpu
_CACHE = {}


def sgen(snap, mode, sib, lp=None):
    from hypergraphdb_amd import DefaultALGenerator
    return DefaultALGenerator(snap, lp, sib, *mode)


def fgen_of(orc, mode, keep, lt=-1):
    return SR.filtered(R.memo_generate(orc, R.opts_of(mode, lt)), keep)


def trees():
    from hypergraphdb_amd import hg
    return {"type": hg.type(1), "typePlus": hg.typePlus([0, 2]), "not": hg.not_(hg.typePlus([1, 2])),
            "or_of_and": hg.or_(hg.and_(hg.typePlus([0, 1]), hg.not_(hg.type(0))), hg.and_(hg.type(2), hg.typePlus([2, 5]))),
            "empty_or": hg.or_(), "empty_and": hg.and_()}


def random_case():
    """The random graph, its atom types, three masks and the seed batches (built once, left unchanged)."""
    if "random" not in _CACHE:
        rng = np.random.default_rng(20262)
        g = K.random_graph(rng, 300, 400, n_types=3)
        A = g["num_atoms"]
        types = SR.atom_types(g, rng)
        masks = {"half": SR.flags(types, trees()["typePlus"]).astype(bool) & (rng.random(A) < 0.75),
                 "nothing": np.zeros(A, bool), "everything": np.ones(A, bool)}
        assert 0.3 * A < masks["half"].sum() < 0.7 * A
        seeds = {}
        for n in (1, 64, 65, 1024):
            s = rng.integers(0, A, n).astype(np.int32)
            if n > 1:
                s[-1] = s[0]                                             # two seeds on the same atom
                fail = np.nonzero(~masks["half"])[0]
                s[1], s[n // 2] = fail[0], fail[-1]                      # seeds that fail the predicate
            else:
                s[0] = np.nonzero(~masks["half"])[0][3]
            seeds[n] = s
        _CACHE["random"] = (g, types, masks, seeds, oracle(g))
    return _CACHE["random"]


def check_sets(res, seeds, many, every, tag):
    """counts() of every seed and depth; visited() of every seed (``every``) or of the sampled ones."""
    n = len(seeds)                                                       # (``many`` may hold more starts: the first n are these)
    counts = res.counts()
    exp = many.counts()[:n]
    nl = max(d + 1 for d in range(exp.shape[1]) if d == 0 or exp[:, d].any())
    exp = exp[:, :nl]
    assert counts.shape[1] >= nl and np.array_equal(counts[:, :nl], exp) and not counts[:, nl:].any(), tag
    sample = range(n) if every else sorted({0, 1, 63 % n, 64 % n, n // 2, n - 2, n - 1})
    for i in sample:
        lv = many.levels(i)
        while len(lv) > 1 and not lv[-1]:
            lv.pop()
        assert gpu_levels(res, i) == lv, (tag, i, int(seeds[i]))


# ---------------------------------------------------------------------------------------------------
# 1. the evaluation kernel on its own: flags, the device count, paging, the ballot tail, the mask constructor
# ---------------------------------------------------------------------------------------------------
def test_flags_every_tree_paging_and_mask_round_trip():
    from hypergraphdb_amd import AtomPredicate
    g, types, masks, _, _ = random_case()
    A = g["num_atoms"]
    assert A % 64 != 0
    snap = snapshot(g)
    snap.set_timing(True)
    snap.set_atom_types(types)
    for k, tree in trees().items():
        exp = SR.flags(types, tree)
        with AtomPredicate(snap, tree) as p:
            assert p.num_atoms == A and p.num_kept == int(exp.sum()), (k, p.num_kept, int(exp.sum()))
            got = p.flags()
            assert got.dtype == np.uint8 and np.array_equal(got, exp), (k, np.nonzero(got != exp)[0][:8])
            st = p.stats()
            assert st["ms_eval"] > 0 and st["bytes_eval"] == 4.0 * A + 8.0 * ((A + 63) // 64), (k, st)
            if k == "or_of_and":                                        # paged readback at the word boundaries
                for first, n in ((0, 0), (0, 1), (0, 64), (63, 2), (64, 64), (65, 127), (A - 1, 1), (A - 64, 64), (A, 0),
                                 (A // 2, A - A // 2)):
                    assert np.array_equal(p.flags(first, n), exp[first:first + n]), (first, n)
                for first, n in ((-1, 1), (0, A + 1), (A, 1), (A + 1, 0)):
                    with pytest.raises(Exception) as e:
                        p.flags(first, n)
                    assert "out of bounds" in str(e.value)
        if k not in ("empty_or", "empty_and"):
            assert 0 < exp.sum() < A, k
    assert SR.flags(types, trees()["empty_or"]).sum() == 0 and SR.flags(types, trees()["empty_and"]).sum() == A
    rng = np.random.default_rng(5)
    keep = rng.random(A) < 0.4
    with AtomPredicate.from_mask(snap, keep) as p:
        assert p.num_kept == int(keep.sum()) and np.array_equal(p.flags(), keep.astype(np.uint8))
        assert p.stats()["bytes_eval"] == 1.0 * A + 8.0 * ((A + 63) // 64)
    with AtomPredicate.from_mask(snap, lambda a: a % 3 == 0) as p:      # a callable, evaluated once per atom
        assert np.array_equal(p.flags(), (np.arange(A) % 3 == 0).astype(np.uint8))
    snap.close()


@pytest.mark.parametrize("A", (1, 63, 64, 65, 129))
def test_ballot_tail(A):
    """num_atoms on both sides of a word: the tail wave masks the lanes past the last atom."""
    from hypergraphdb_amd import AtomPredicate, HyperGraphSnapshot, hg
    la = np.array([A - 1], np.int32) if A > 1 else np.zeros(0, np.int32)
    tg = np.zeros(len(la), np.int32)
    snap = HyperGraphSnapshot(A, la, np.arange(len(la) + 1, dtype=np.int64), tg, np.full(len(la), 2, np.int32))
    types = (np.arange(A) % 3).astype(np.int32)
    if len(la):
        types[A - 1] = 2
    snap.set_atom_types(types)
    for tree in (hg.typePlus([0, 2]), hg.not_(hg.type(2)), hg.and_(), hg.or_()):
        exp = SR.flags(types, tree)
        with AtomPredicate(snap, tree) as p:
            assert p.num_kept == int(exp.sum()) and np.array_equal(p.flags(), exp), (A, tree)
            assert np.array_equal(p.flags(A - 1, 1), exp[A - 1:])
    keep = np.arange(A) % 2 == 0
    with AtomPredicate.from_mask(snap, keep) as p:
        assert p.num_kept == int(keep.sum()) and np.array_equal(p.flags(), keep.astype(np.uint8))
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 2. per-depth sets: every mode, both values of HGX_OPT_BFS_BLOCK, 1 / 64 / 65 / 1024 seeds, three masks
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", (1, 0))
@pytest.mark.parametrize("mask", ("half", "nothing", "everything"))
def test_set_bfs_every_mode(mask, block):
    from hypergraphdb_amd import AtomPredicate, bfs_batch
    from test_gpu_bfs import gen
    g, _, masks, seeds, orc = random_case()
    A = g["num_atoms"]
    keep = masks[mask]
    snap = snapshot(g)
    snap.set_option(opt("BFS_BLOCK"), block)
    with AtomPredicate.from_mask(snap, keep) as p:
        for mi, mode in enumerate(K.ALGEN_MODES):
            fgen = fgen_of(orc, mode, keep)
            for n, maxd in ((1, None), (64, None), (65, 2), (65, None), (1024, None), (1024, 3)):
                s = seeds[n]
                res = bfs_batch(snap, s, maxd, sgen(snap, mode, p))
                many = SR.ManyLevels(fgen, A, s, maxd)
                every = n <= 65 or (mask == "half" and mi in (0, 1) and maxd is None)
                check_sets(res, s, many, every, (mask, block, mi, n, maxd))
                if mask == "everything":                                 # bit for bit the plain bfs_batch
                    plain = bfs_batch(snap, s, maxd, gen(snap, mode))
                    assert plain.n_levels == res.n_levels and np.array_equal(plain.counts(), res.counts())
                    for i in sorted({0, 1 % n, n // 2, 63 % n, n - 1}):
                        for d in range(res.n_levels):
                            assert np.array_equal(plain.visited(i, d), res.visited(i, d)), (mi, n, i, d)
                    plain.close()
                if mask == "nothing":                                    # only the start's own neighbours fail: V_0 alone
                    assert res.counts()[:, 1:].sum() == 0
                res.close()
    snap.close()


def test_type_tree_given_raw_and_a_callable():
    """A raw type tree (compiled per call against the atom types, released on return) and a callable atom -> bool
    give what the AtomPredicate of the same truth values gives."""
    from hypergraphdb_amd import bfs_batch
    g, types, _, seeds, orc = random_case()
    A = g["num_atoms"]
    tree = trees()["or_of_and"]
    keep = SR.flags(types, tree).astype(bool)
    snap = snapshot(g)
    snap.set_atom_types(types)
    s = seeds[65]
    for mode in (K.ALGEN_MODES[0], K.ALGEN_MODES[4], K.ALGEN_MODES[6]):
        many = SR.ManyLevels(fgen_of(orc, mode, keep), A, s, None)
        for sib in (tree, lambda a: bool(keep[a])):
            res = bfs_batch(snap, s, None, sgen(snap, mode, sib))
            check_sets(res, s, many, True, ("raw", mode))
            res.close()
    snap.update()                                                        # nothing of a per-call predicate is left alive
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 3. every level kind of the rows engine on the hub graph, with a failing hub, a failing seed hub, failing leaves
# ---------------------------------------------------------------------------------------------------
SETTINGS = {   # what differs from flags 0x3BE, nf_pull 1, nf_hint 1, hub_mask 0, fused 1, the symmetric mode, 1024 seeds
    "default": {}, "unfused": dict(fused=0), "nf2_hint": dict(nf_pull=2), "nf2_nohint": dict(nf_pull=2, nf_hint=0),
    "nf0_mask2": dict(nf_pull=0, hub_mask=2), "nf0_mask0": dict(nf_pull=0, hub_mask=0), "fc": dict(flags=0x203BE),
    "fc_nf0": dict(flags=0x203BE, nf_pull=0), "flags0": dict(flags=0x0), "flags3fe": dict(flags=0x3FE),
    "flags39e": dict(flags=0x39E), "after_first": dict(mode=K.ALGEN_MODES[1]), "narrow_64": dict(S=64),
    "narrow_64_flags39e": dict(S=64, flags=0x39E), "narrow_64_after_first": dict(S=64, mode=K.ALGEN_MODES[1]),
}


def hub_case():
    if "hub" not in _CACHE:
        from hypergraphdb_amd import synth
        g = synth.hypergraph(3000, 20000, 2, 8, 2.1, 3, seed=21)
        A = g["num_atoms"]
        deg = np.bincount(g["tgt_idx"], minlength=A)
        assert deg.max() > 4096 and (deg > 512).sum() >= 2
        order = np.argsort(-deg)
        hub, hub2 = int(order[0]), int(order[1])
        rng = np.random.default_rng(9)
        has = np.nonzero(deg > 0)[0]
        seeds = rng.choice(has[(has != hub) & (has != hub2)], 1024, replace=False).astype(np.int32)
        leaves = np.ones(A, bool)
        leaves[rng.choice(np.nonzero(deg <= 8)[0], int(0.4 * (deg <= 8).sum()), replace=False)] = False
        one, two = np.ones(A, bool), np.ones(A, bool)
        one[hub] = False
        two[hub2] = False
        seeds_hub = seeds.copy()
        seeds_hub[5] = hub2                                              # a hub that is a seed and fails
        cases = {"failing_hub": (one, seeds), "failing_seed_hub": (two, seeds_hub), "failing_leaves": (leaves, seeds)}
        _CACHE["hub"] = (g, cases, oracle(g), {})
    return _CACHE["hub"]


@pytest.mark.parametrize("case", ("failing_hub", "failing_seed_hub", "failing_leaves"))
def test_every_level_kind_on_the_hub_graph(case):
    from hypergraphdb_amd import AtomPredicate, _lib, bfs_batch
    g, cases, orc, refs = hub_case()
    A = g["num_atoms"]
    keep, seeds = cases[case]
    snap = snapshot(g)
    snap.set_option(_lib.HGX_OPT_BFS_BLOCK, 0)
    kinds, launched, sts = set(), set(), {}
    with AtomPredicate.from_mask(snap, keep) as p:
        for name, c in SETTINGS.items():
            mode, S = c.get("mode", K.ALGEN_MODES[0]), c.get("S", 1024)
            s = seeds[:S]
            key = (case, mode)                                           # one reference per mode: the narrow batches are its first seeds
            if key not in refs:
                if mode not in refs:
                    refs[mode] = R.memo_generate(orc, R.opts_of(mode))
                refs[key] = SR.ManyLevels(SR.filtered(refs[mode], keep), A, seeds, None)
            snap.set_option(_lib.HGX_OPT_BFS_FLAGS, c.get("flags", 0x3BE))
            snap.set_option(_lib.HGX_OPT_NF_PULL, c.get("nf_pull", 1))
            snap.set_option(_lib.HGX_OPT_NF_HINT, c.get("nf_hint", 1))
            snap.set_option(_lib.HGX_OPT_HUB_MASK, c.get("hub_mask", 0))
            snap.set_option(_lib.HGX_OPT_COUNT_FUSED, c.get("fused", 1))
            res = bfs_batch(snap, s, None, sgen(snap, mode, p))
            check_sets(res, s, refs[key], False, (case, name))
            st = res.stats(accounting=False)
            n_exp = st["n_levels_expanded"]
            sts[name] = st
            kinds |= set(st["level_sparse"][:n_exp])
            launched |= {k for k, v in st["kernels"].items() if v["launches"] > 0}
            print(case, name, "kinds", st["level_sparse"][:n_exp], "hint", st["nf_hint_atoms"], "hub mask",
                  st["hub_mask_entries"], "count passes", st["count_pass_levels"])
            res.close()
    snap.close()
    print(case, "kernels launched:", sorted(launched))
    assert kinds >= {0, 1, 2, 3, 4}, kinds        # dense, both sparse pushes, the direct pull, the frontier-code pull
    assert sts["nf2_hint"]["nf_hint_atoms"] > 0 and sts["nf2_nohint"]["nf_hint_atoms"] == 0     # the direct pull's hint step
    assert 3 in sts["nf2_nohint"]["level_sparse"][:sts["nf2_nohint"]["n_levels_expanded"]]
    assert sts["default"]["count_pass_levels"] < sts["unfused"]["count_pass_levels"]            # the fused level counts
    assert {"hgx_atom_pull_heavy", "hgx_hub_finalize", "hgx_nf_pull"} <= launched, sorted(launched)
    assert sts["nf0_mask0"]["hub_mask_entries"] == 0
    if case != "failing_hub":                     # (the failing hub is the top atom: it is never on a frontier)
        assert sts["nf0_mask2"]["hub_mask_entries"] > 0                                          # the hub-mask step


# ---------------------------------------------------------------------------------------------------
# 4. deep graphs: hundreds of levels, one failing atom in the middle / one failing rail
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", (1, 0))
def test_deep_path_stops_before_the_failing_atom(block):
    from hypergraphdb_amd import AtomPredicate, bfs_batch
    n, cut = 300, 170
    g = D.path(n, rng=np.random.default_rng(3))
    A, pos = g["num_atoms"], g["pos"]
    keep = np.ones(A, bool)
    keep[pos[cut]] = False
    orc = oracle(g)
    seeds = np.array([pos[0], pos[100], pos[cut], pos[cut + 1], pos[n - 1]], np.int32)
    snap = snapshot(g)
    snap.set_option(opt("BFS_BLOCK"), block)
    with AtomPredicate.from_mask(snap, keep) as p:
        for mode in (D.SYM, D.FWD):
            many = SR.ManyLevels(fgen_of(orc, mode, keep), A, seeds, None)
            res = bfs_batch(snap, seeds, None, sgen(snap, mode, p))
            check_sets(res, seeds, many, True, ("path", block, mode))
            c = res.counts()
            # position 0 walks levels 0 .. cut - 1; in the symmetric mode the failing start walks back to position 0
            assert res.n_levels == len(many.rows) == (cut + 1 if mode == D.SYM else cut)
            assert np.nonzero(c[0])[0].max() == cut - 1 and res.depth_of(0, int(pos[cut - 1])) == cut - 1
            assert res.depth_of(0, int(pos[cut])) == -1 and res.depth_of(0, int(pos[cut + 1])) == -1
            assert res.depth_of(2, int(pos[cut + 1])) == 1               # the failing atom as a start is expanded
            assert res.depth_of(3, int(pos[cut])) == -1                  # and nothing else reaches it
            res.close()
    snap.close()


def test_deep_ladder_with_a_failing_rail():
    from hypergraphdb_amd import AtomPredicate, bfs_batch
    levels, width = 40, 4
    g = D.ladder(levels, width)
    A = g["num_atoms"]
    keep = np.ones(A, bool)
    keep[[l * width + 1 for l in range(levels + 1)]] = False            # column 1 fails in every layer
    orc = oracle(g)
    seeds = np.array([0, 1, 3, 2 * width + 2], np.int32)
    snap = snapshot(g)
    with AtomPredicate.from_mask(snap, keep) as p:
        for mode in (D.SYM, D.FWD):
            many = SR.ManyLevels(fgen_of(orc, mode, keep), A, seeds, None)
            res = bfs_batch(snap, seeds, None, sgen(snap, mode, p))
            check_sets(res, seeds, many, True, ("ladder", mode))
            assert res.n_levels == len(many.rows)
            if mode == D.FWD:                                            # from column 0 only column 0 is left
                assert res.counts()[0].tolist() == [1] * (levels + 1)
            res.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 5. a link predicate and a sibling predicate together
# ---------------------------------------------------------------------------------------------------
def test_link_and_sibling_predicate_together():
    """A tree of test_gpu_linkpred.leaf_trees on the links (its graph: rows past eight targets) and a type tree on the
    atoms, against the filtered generator over the flagged graph."""
    from hypergraphdb_amd import AtomPredicate, LinkPredicate, bfs_batch
    from test_gpu_linkpred import random_case as linkpred_case
    g, x, a, _, _, _, _ = linkpred_case()
    A = g["num_atoms"]
    rng = np.random.default_rng(31)
    types = SR.atom_types(g, rng)
    lt = leaf_trees(g, x, a)
    s = rng.integers(0, A, 65).astype(np.int32)
    snap = snapshot(g)
    snap.set_atom_types(types)
    for lname, sname in (("type", "not"), ("incident", "typePlus"), ("arity", "or_of_and"), ("orderedLink_tail", "type"),
                         ("link", "typePlus")):
        ltree, stree = lt[lname], trees()[sname]
        keep = SR.flags(types, stree).astype(bool)
        orc_f = oracle(LP.flagged(g, ltree))
        with LinkPredicate(snap, ltree) as lp, AtomPredicate(snap, stree) as ap:
            for mode in (K.ALGEN_MODES[0], K.ALGEN_MODES[1], K.ALGEN_MODES[9]):
                many = SR.ManyLevels(fgen_of(orc_f, mode, keep, 1), A, s, None)
                res = bfs_batch(snap, s, None, sgen(snap, mode, ap, lp))
                check_sets(res, s, many, True, (lname, sname, mode))
                res.close()
        res = bfs_batch(snap, s, 2, sgen(snap, K.ALGEN_MODES[0], stree, ltree))     # both raw, compiled per call
        check_sets(res, s, SR.ManyLevels(fgen_of(orc_f, K.ALGEN_MODES[0], keep, 1), A, s, 2), True, (lname, sname, "raw"))
        res.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 6. hop paths, depth and predecessor rows
# ---------------------------------------------------------------------------------------------------
class FRef(Ref):
    """test_gpu_hops.Ref over the filtered generator."""

    def __init__(self, orc, mode, keep, max_depth=None):
        super().__init__(orc, mode, -1, max_depth)
        self.gen = SR.filtered(self.gen, keep)


@pytest.mark.parametrize("block", (1, 0))
def test_hop_paths_and_predecessor_rows(block):
    from hypergraphdb_amd import AtomPredicate, bfs_batch, hop_paths
    g, _, masks, _, orc = random_case()
    A = g["num_atoms"]
    keep = masks["half"]
    ok, bad = np.nonzero(keep)[0], np.nonzero(~keep)[0]
    rng = np.random.default_rng(66)
    snap = snapshot(g)
    snap.set_option(opt("BFS_BLOCK"), block)
    for mode in (K.ALGEN_MODES[0], K.ALGEN_MODES[1], K.ALGEN_MODES[3]):
        ref = FRef(orc, mode, keep)
        starts = np.concatenate([rng.choice(ok, 30), rng.choice(bad, 10)]).astype(np.int32)      # starts that fail too
        goals = np.concatenate([rng.choice(ok, 25), rng.choice(bad, 15)]).astype(np.int32)       # goals that fail
        with hop_paths(snap, starts, goals, sgen(snap, mode, lambda a: bool(keep[a]))) as hp:     # a callable
            check_paths(hp, starts, goals, ref, ("hops", mode))
            for i in range(25, 40):                                       # a goal that fails is not reached ...
                assert not hp.reached[i] or goals[i] == starts[i], (mode, i)
            assert hp.reached[30:].sum() + hp.reached[:30].sum() > 0
        with AtomPredicate.from_mask(snap, keep) as p:
            res = bfs_batch(snap, starts[28:32], None, sgen(snap, mode, p))
        for i in range(4):                                                # (the predicate is closed: the result holds it)
            check_rows(res, i, int(starts[28 + i]), A, ref, ("rows", mode))
            d = res.depths(i)
            assert (d[bad] >= 0).sum() <= 1                               # no failing atom at any depth but the start itself
        assert (res.depths(2) > 0).any()                                  # ... and a start that fails still has paths
        with res.paths(np.arange(4, dtype=np.int32), goals[:4]) as hp:
            check_paths(hp, starts[28:32], goals[:4], ref, ("res.paths", mode))
        res.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 7. weighted shortest paths, GraphClassics.dijkstra
# ---------------------------------------------------------------------------------------------------
def test_shortest_paths_random_weights():
    from hypergraphdb_amd import AtomPredicate, GraphClassics, shortest_paths
    g, _, masks, _, orc = random_case()
    A = g["num_atoms"]
    keep = masks["half"]
    ok, bad = np.nonzero(keep)[0], np.nonzero(~keep)[0]
    rng = np.random.default_rng(55)
    w = rng.integers(1, 9, len(g["link_atom"])).astype(np.float64) * 0.37
    wf = R.row_weights(g, w)
    snap = snapshot(g)
    sym = fgen_of(orc, K.ALGEN_MODES[0], keep)
    with_nbrs = [int(a) for a in rng.permutation(ok) if sym(int(a))]
    starts = with_nbrs[:2] + [next(int(b) for b in bad if sym(int(b)))]                            # one start fails
    near = {s: sorted(n for n in SR.dijkstra(sym, s, None)[1] if n != s) for s in starts}          # reachable goals
    assert all(len(v) >= 2 for v in near.values())
    pairs = [(s, None) for s in starts] + [(s, int(q)) for s in starts for q in
                                           np.concatenate([rng.choice(near[s], 2), rng.choice(ok, 2), rng.choice(bad, 2)])]
    with AtomPredicate.from_mask(snap, keep) as p:
        for mode in (K.ALGEN_MODES[0], K.ALGEN_MODES[1]):
            fgen = fgen_of(orc, mode, keep)
            with shortest_paths(snap, [x[0] for x in pairs], [x[1] for x in pairs], sgen(snap, mode, p), w) as res:
                rows = {s: SR.dijkstra(fgen, s, None, wf)[1] for s in starts}                     # every final distance of s
                assert mode != K.ALGEN_MODES[0] or len(rows[starts[2]]) > 1                       # the failing start reaches atoms
                for i, (s, q) in enumerate(pairs):
                    dm = rows[s]
                    if q is None:
                        row = np.full(A, np.inf)
                        for n, v in dm.items():
                            row[n] = v
                        assert np.array_equal(u64(res.distances(i)), u64(row)), (mode, i)
                        assert not np.isfinite(row[bad][bad != s]).any()
                        rr = SR.rule_r(fgen, wf, dm, s, sorted(dm))
                        ea, el = np.full(A, -1, np.int32), np.full(A, -1, np.int32)
                        for n, (a, l) in rr.items():
                            ea[n], el[n] = a, l
                        pa, pl = res.predecessors(i)
                        assert np.array_equal(pa, ea) and np.array_equal(pl, el), (mode, i)
                        continue
                    d = dm.get(q)
                    assert bool(res.reached[i]) == (d is not None), (mode, i)
                    assert u64(res.distance[i]) == u64(np.inf if d is None else d), (mode, i)
                    atoms, links = res.path(i)
                    if d is None:
                        assert len(atoms) == 0
                    else:
                        R.check_path(fgen, wf, s, q, atoms, links, d)     # valid under the filter, of that length
            s, q = next(((s, q) for s, q in pairs[3:] if rows[s].get(q) is not None and q != s), (None, None))
            assert s is not None or mode != K.ALGEN_MODES[0]
            if s is None:
                s = starts[0]
            else:
                assert GraphClassics.dijkstra(s, q, sgen(snap, mode, lambda a: bool(keep[a])), w) == rows[s][q]
            fq = int(bad[bad != s][0])
            assert GraphClassics.dijkstra(s, fq, sgen(snap, mode, lambda a: bool(keep[a])), w) is None
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 8. lifetime and refusals
# ---------------------------------------------------------------------------------------------------
def test_result_outlives_its_predicate_and_update_drops_the_types():
    from hypergraphdb_amd import AtomPredicate, HGXError, HGXUnsupported, _lib, bfs_batch
    g, types, masks, seeds, orc = random_case()
    A = g["num_atoms"]
    mode = K.ALGEN_MODES[0]
    tree = trees()["typePlus"]
    keep = SR.flags(types, tree).astype(bool)
    ref = FRef(orc, mode, keep)
    snap = snapshot(g)
    snap.set_atom_types(types)
    p = AtomPredicate(snap, tree)
    starts = np.array([5, 17, 300], np.int32)
    res = bfs_batch(snap, starts, None, sgen(snap, mode, p))
    p.close()
    check_rows(res, 1, 17, A, ref)                                        # the result outlives its predicate
    new_link = {A: (0, [1, 2])}
    with pytest.raises(HGXError) as e:                                    # the result (and through it the predicate) lives
        snap.update(add=new_link, num_atoms=A + 1)
    assert e.value.code == _lib.HGX_E_INVALID
    res.close()
    p2 = AtomPredicate.from_mask(snap, keep)
    with pytest.raises(HGXError) as e:                                    # a live predicate alone blocks the update
        snap.update(add=new_link, num_atoms=A + 1)
    assert e.value.code == _lib.HGX_E_INVALID
    p2.close()
    snap.update(add=new_link, num_atoms=A + 1)                            # accepted once it is freed
    assert snap.A == A + 1
    with pytest.raises(HGXUnsupported) as e:                              # the update dropped the atom types
        AtomPredicate(snap, tree)
    assert "no atom types" in str(e.value)
    with pytest.raises(HGXUnsupported):
        bfs_batch(snap, starts, None, sgen(snap, mode, tree))
    snap.set_atom_types(np.concatenate([types, [0]]).astype(np.int32))   # set again: the new link atom has type 0
    with AtomPredicate(snap, tree) as p3:
        assert np.array_equal(p3.flags()[:A], keep.astype(np.uint8)) and p3.flags()[A] == 1
    with AtomPredicate.from_mask(snap, np.ones(A + 1, bool)) as p4:       # a mask needs no atom types
        snap.set_atom_types(None)
        assert p4.num_kept == A + 1
    snap.close()


def test_predicate_on_contexts_other_graphs_and_shards():
    from hypergraphdb_amd import AtomPredicate, HGXError, HGXUnsupported, _lib, bfs_batch, bfs_sequence, find_all, hg, \
        shortest_paths
    from hypergraphdb_amd.partition import Shard, ShardSnapshot
    g, types, masks, seeds, orc = random_case()
    A = g["num_atoms"]
    tree = trees()["not"]
    keep = SR.flags(types, tree).astype(bool)
    snap, other = snapshot(g), snapshot(g)
    snap.set_atom_types(types)
    ctx, ctx2 = snap.context(), snap.context()
    mode = K.ALGEN_MODES[1]
    s = seeds[64]
    many = SR.ManyLevels(fgen_of(orc, mode, keep), A, s, None)
    with AtomPredicate(ctx, tree) as pc, AtomPredicate.from_mask(ctx, keep) as pm:     # made through a context
        assert np.array_equal(pc.flags(), keep.astype(np.uint8))
        for target, p in ((snap, pc), (ctx2, pc), (ctx, pm), (snap, pm)):               # ... works on the snapshot and on another context
            res = bfs_batch(target, s, None, sgen(target, mode, p))
            check_sets(res, s, many, True, "ctx")
            res.close()
        for call in (lambda: bfs_batch(other, s, None, sgen(other, mode, pc)),
                     lambda: shortest_paths(other, [1], [2], sgen(other, mode, pm))):
            with pytest.raises(HGXError) as e:
                call()
            assert e.value.code == _lib.HGX_E_INVALID and "another graph" in str(e.value)
        with pytest.raises(HGXError) as e:                               # the types are read by a living predicate
            snap.set_atom_types(types)
        assert e.value.code == _lib.HGX_E_INVALID and "still alive" in str(e.value)
        # the order-exact sequence and find_all's traversal conditions keep refusing
        with pytest.raises(HGXUnsupported):
            bfs_sequence(snap, s, None, sgen(snap, mode, pc))
        with pytest.raises(HGXUnsupported):
            bfs_sequence(snap, s, None, sgen(snap, mode, pc, hg.arity(2)))
        with pytest.raises(HGXUnsupported):
            find_all(snap, hg.bfs(int(s[0]), sibling_predicate=tree))
        # a NULL atom predicate is the _pred entry point
        L = _lib.lib()
        h = C.c_void_p()
        o = _lib.AlgenOpts(-1, 1, 1, 0, 0)
        sp = np.ascontiguousarray(s)
        assert L.hgx_bfs_batch_sib(snap.handle, sp.ctypes.data, len(sp), 2, C.byref(o), None, None, C.byref(h)) == _lib.HGX_OK
        from hypergraphdb_amd.algorithms import BfsResult
        from test_gpu_bfs import gen
        a, b = bfs_batch(snap, s, 2, gen(snap, K.ALGEN_MODES[0])), BfsResult(snap, h, s)
        assert np.array_equal(a.counts(), b.counts())
        a.close()
        b.close()
    snap.set_atom_types(types)                                           # allowed again
    # set_atom_types refusals
    with pytest.raises(ValueError):
        snap.set_atom_types(types[:-1])
    bad = types.copy()
    bad[3] = -1
    with pytest.raises(HGXError) as e:
        snap.set_atom_types(bad)
    assert e.value.code == _lib.HGX_E_INVALID and "atom 3" in str(e.value)
    bad = types.copy()
    row = 7
    bad[g["link_atom"][row]] = (g["link_type"][row] + 1) % 3
    with pytest.raises(HGXError) as e:
        snap.set_atom_types(bad)
    assert e.value.code == _lib.HGX_E_INVALID and f"link row {row} " in str(e.value)
    with pytest.raises(HGXError) as e:
        ctx.set_atom_types(types)
    assert e.value.code == _lib.HGX_E_INVALID and "context" in str(e.value)
    with AtomPredicate(snap, tree) as p:                                 # the refused calls left the column as it was
        assert np.array_equal(p.flags(), keep.astype(np.uint8))
    # shards
    M = len(g["link_atom"])
    sh = Shard.build(A, g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"], 1, 0, np.zeros(M, np.int32))
    ss = ShardSnapshot(sh)
    L = _lib.lib()
    h = C.c_void_p()
    k8 = keep.astype(np.uint8)
    assert L.hgx_graph_set_atom_types(ss.handle, types.ctypes.data) == _lib.HGX_E_UNSUPPORTED
    assert L.hgx_atom_predicate_create_mask(ss.handle, k8.ctypes.data, C.byref(h)) == _lib.HGX_E_UNSUPPORTED
    assert L.hgx_atom_predicate_create(ss.handle, 0, None, None, None, 0, C.byref(h)) == _lib.HGX_E_UNSUPPORTED
    with AtomPredicate.from_mask(snap, keep) as p:                        # and a shard takes no predicate of a snapshot
        z = np.zeros(1, np.int32)
        assert L.hgx_bfs_batch_sib(ss.handle, z.ctypes.data, 1, 1, None, None, p.handle, C.byref(h)) == _lib.HGX_E_UNSUPPORTED
        assert L.hgx_shortest_paths_sib(ss.handle, z.ctypes.data, z.ctypes.data, 1, None, None, None, p.handle,
                                        C.byref(h)) == _lib.HGX_E_UNSUPPORTED
    ss.close()
    sh.close()
    for x in (ctx, ctx2, other, snap):
        x.close()


def test_malformed_programs_are_refused_before_any_launch():
    from hypergraphdb_amd import _lib
    from hypergraphdb_amd.query import NOT_ARITY, NOT_INCIDENT, NOT_TYPE
    g, types, _, _, _ = random_case()
    snap = snapshot(g)
    L = _lib.lib()

    def create(lit_off, lit, ops):
        h = C.c_void_p()
        lo, li, op = np.array(lit_off, np.int64), np.array(lit, np.int32), np.array(ops, np.int32)
        rc = L.hgx_atom_predicate_create(snap.handle, len(lo) - 1, lo.ctypes.data, li.ctypes.data if len(li) else None,
                                         op.ctypes.data if len(op) else None, len(op), C.byref(h))
        assert (rc == _lib.HGX_OK) == bool(h.value)
        if h.value:
            L.hgx_atom_predicate_free(h)
        return rc, L.hgx_last_error().decode()

    rc, msg = create([0, 1], [NOT_TYPE, 1, 0, 1], [2])                    # well formed, but no atom types yet
    assert rc == _lib.HGX_E_UNSUPPORTED and "no atom types" in msg
    snap.set_atom_types(types)
    assert create([0, 1], [NOT_TYPE, 1, 0, 1], [2])[0] == _lib.HGX_OK
    rc, msg = create([0, 0, 1], [9, 1, 0, 1], [3])
    assert rc == _lib.HGX_E_INVALID and "term 1 literal 0" in msg and "unknown literal kind 9" in msg
    rc, msg = create([0, 1], [NOT_TYPE, 1, 0, 2], [3])
    assert rc == _lib.HGX_E_INVALID and "operand range outside ops" in msg
    rc, msg = create([0, 1], [NOT_TYPE, 1, 0, 1], [-4])
    assert rc == _lib.HGX_E_INVALID and "bad type" in msg
    rc, msg = create([0, 2, 1], [NOT_TYPE, 1, 0, 1, NOT_TYPE, 1, 0, 1], [3])
    assert rc == _lib.HGX_E_INVALID and "lit_off decreases" in msg
    for kind in (NOT_ARITY, NOT_INCIDENT):
        rc, msg = create([0, 2], [NOT_TYPE, 1, 0, 1, kind, 1, 0, 1], [2])
        assert rc == _lib.HGX_E_UNSUPPORTED and "term 0 literal 1" in msg and "only type literals" in msg
    rc, msg = create([0, 1], [NOT_TYPE, 1, 0, 65537], list(range(65537)))
    assert rc == _lib.HGX_E_UNSUPPORTED and "term 0 literal 0" in msg
    snap.close()
