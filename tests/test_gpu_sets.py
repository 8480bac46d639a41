"""GPU parity: the visited sets of many seeds in one device pass (include/hgx_sets.h), all exact against
tests/sets_ref.py over the frozen oracle's per-depth sets.

Shapes: random_graph(300, 400, 3 types) is 700 atoms, no multiple of 64, with links targeting links; 1, 64, 65 and
1024 seeds give rows of 1, 1, 2 and 16 words and a partly filled last word, 1100 seeds two batches; the batches of
64 and 65 seeds hold two seeds on one atom.  deep_graphs.path(300) and ladder(40, 4) run 299 and 40 levels over a
handful of tiles (the bitmap skip); synth.hypergraph(3000, 20000, ...) is 23000 atoms = 360 tiles = 90 wavefronts
of four tiles, so the per-wavefront starts of the scan are exercised.  Every case runs with HGX_OPT_BFS_BLOCK 1
(the default: the workgroup stages finish these small traversals, so the host lists serve the seeds, or a mix)
and 0 (rows only: the kernels serve every seed).

The reference is pure Python over lists, so the calls over a thousand seeds are kept to a few per case."""
import numpy as np
import pytest

import deep_graphs as D
import kat_graphs as K
import sets_ref as S
import sibling_ref as SR
from oracle_ctypes import algen
from test_gpu_bfs import gen, gpu_levels, levels_from_seq, oracle, snapshot

pytestmark = pytest.mark.gpu
_CACHE = {}
SYM, ORD = (True, True, False, False), (False, True, False, False)
GENS = [(SYM, -1, None), (SYM, -1, 2), (ORD, -1, None), (ORD, -1, 2), (SYM, 1, None), (SYM, 1, 2)]


def opt(name):
    from hypergraphdb_amd import _lib
    return getattr(_lib, "HGX_OPT_" + name)


def tree():
    from hypergraphdb_amd import hg
    return hg.typePlus([0, 2])


def random_case():
    """The random graph, its atom types, the masks and the seed batches (built once, left unchanged)."""
    if "random" not in _CACHE:
        rng = np.random.default_rng(20271)
        g = K.random_graph(rng, 300, 400, n_types=3)
        A = g["num_atoms"]
        assert A == 700 and A % 64 != 0
        types = SR.atom_types(g, rng)
        masks = {"half": rng.random(A) < 0.5, "nothing": np.zeros(A, bool), "everything": np.ones(A, bool),
                 "tree": SR.flags(types, tree()).astype(bool)}
        assert 0.3 * A < masks["half"].sum() < 0.7 * A and 0 < masks["tree"].sum() < A
        seeds = {}
        for n in (1, 64, 65, 1024, 1100):
            s = rng.integers(0, A, n).astype(np.int32)
            if n > 1:
                s[-1] = s[0]                                             # two seeds on the same atom
            seeds[n] = s
        _CACHE["random"] = (g, types, masks, seeds, oracle(g))
    return _CACHE["random"]


def ref_levels(key, orc, seeds, mode, lt, maxd):
    """The oracle's per-depth sets of every seed (computed once per batch and generator, left unchanged)."""
    k = (key, len(seeds), mode, lt, maxd)
    if k not in _CACHE:
        out = []
        for s in seeds:
            l, a, d, _ = orc.bfs(int(s), -1 if maxd is None else maxd, algen(lt, *mode))
            out.append(levels_from_seq(int(s), zip(l.tolist(), a.tolist(), d.tolist())))
        _CACHE[k] = out
    return _CACHE[k]


def check(res, lv, sel=None, dmin=0, dmax=None, where=None, keep=None, depths=False, tag=None):
    """res.sets(...) against sets_ref.sets over the selected seeds' oracle levels; returns the VisitedSets."""
    idx = list(range(len(lv))) if sel is None else [int(i) for i in sel]
    off, atoms, deps = S.sets([lv[i] for i in idx], dmin, dmax, keep, depths)
    vs = res.sets(sel, dmin, dmax, where, depths=depths)
    assert len(vs) == len(idx) and vs.total == off[-1], (tag, vs.total, int(off[-1]))
    assert vs.offsets.dtype == np.int64 and np.array_equal(vs.offsets, off), tag
    assert np.array_equal(vs.counts, np.diff(off)), tag
    got = vs.flat()
    if depths:
        assert np.array_equal(got[0], atoms), tag
        assert np.array_equal(got[1], deps), tag                          # every entry's depth is the oracle's distance
    else:
        assert got.dtype == np.int32 and np.array_equal(got, atoms), tag
    return vs


def selections(n):
    edge = list(dict.fromkeys(i for i in (0, 63, 64, n - 1) if i < n))   # both sides of a word boundary
    return [None, [n // 2], edge, list(range(n - 1, -1, -1)), []]


# ---------------------------------------------------------------------------------------------------
# 1. the random graph: batches of 1, 64 and 65 seeds under every selection, depth range and predicate
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", (1, 0))
@pytest.mark.parametrize("n", (1, 64, 65))
def test_random_graph_small_batches(n, block):
    from hypergraphdb_amd import AtomPredicate, bfs_batch
    g, types, masks, seeds, orc = random_case()
    snap = snapshot(g)
    snap.set_option(opt("BFS_BLOCK"), block)
    snap.set_atom_types(types)
    s = seeds[n]
    with AtomPredicate.from_mask(snap, masks["half"]) as half:
        for mode, lt, maxd in GENS:
            tag = (n, block, mode, lt, maxd)
            lv = ref_levels("random", orc, s, mode, lt, maxd)
            res = bfs_batch(snap, s, maxd, gen(snap, mode, lt))
            before = res.counts().copy()
            for sel in selections(n):
                check(res, lv, sel, tag=(tag, "sel", sel)).close()
            for dmin, dmax in ((0, None), (1, None), (2, 2), (60, None), (60, 61)):   # the last two: beyond the last level
                vs = check(res, lv, None, dmin, dmax, half, masks["half"], tag=(tag, "range", dmin, dmax))
                assert dmin < 60 or vs.total == 0
                vs.close()
            for name in ("half", "nothing", "everything"):
                check(res, lv, None, 0, None, masks[name], masks[name], depths=True, tag=(tag, "mask", name)).close()
            check(res, lv, selections(n)[2], 1, None, tree(), masks["tree"], tag=(tag, "tree")).close()
            check(res, lv, None, 0, 2, None, None, depths=True, tag=(tag, "depths")).close()
            # the traversal is unchanged: `where` filters what is reported, not what was expanded
            res._counts = None
            assert np.array_equal(res.counts(), before), tag
            assert gpu_levels(res, n // 2) == lv[n // 2], tag
            res.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 2. 1024 seeds (16 words) and 1100 seeds (two batches, a selection from both in non-monotone order)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", (1, 0))
@pytest.mark.parametrize("n,case", [(1024, 0), (1024, 5), (1100, 2), (1100, 3)])
def test_random_graph_wide_batches(n, case, block):
    from hypergraphdb_amd import bfs_batch
    g, types, masks, seeds, orc = random_case()
    snap = snapshot(g)
    snap.set_option(opt("BFS_BLOCK"), block)
    mode, lt, maxd = GENS[case]
    s = seeds[n]
    tag = (n, block, mode, lt, maxd)
    lv = ref_levels("random", orc, s, mode, lt, maxd)
    res = bfs_batch(snap, s, maxd, gen(snap, mode, lt))
    before = res.counts().copy()
    full = check(res, lv, None, 0, None, masks["half"], masks["half"], tag=(tag, "all"))
    with res.sets(None, where=masks["half"], count_only=True) as co:
        assert np.array_equal(co.offsets, full.offsets), tag
    full.close()
    # both batches of the 1100, back and forth
    sel = list(dict.fromkeys([n - 50, 3, n - 1, 1023, 1024 % n, 0, 700, 64, 63, n - 2]))
    check(res, lv, sel, 0, None, None, None, depths=True, tag=(tag, "sel")).close()
    check(res, lv, sel[::-1], 1, 2, masks["half"], masks["half"], depths=True, tag=(tag, "sel range")).close()
    check(res, lv, list(range(n - 1, -1, -1)), 2, 2, tag=(tag, "reversed")).close()
    res._counts = None
    assert np.array_equal(res.counts(), before), tag
    res.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 3. count-only, the entry cap, paged reads, closing order, reading twice
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", (1, 0))
def test_count_only_cap_and_paged_reads(block):
    from hypergraphdb_amd import HGXError, _lib, bfs_batch
    g, types, masks, seeds, orc = random_case()
    snap = snapshot(g)
    snap.set_option(opt("BFS_BLOCK"), block)
    s = seeds[65]
    lv = ref_levels("random", orc, s, SYM, -1, None)
    res = bfs_batch(snap, s, None, gen(snap, SYM))
    off, atoms, deps = S.sets(lv, 0, None, masks["half"], True)
    total = int(off[-1])
    assert total > 1000
    # count-only: the offsets of the full call, and nothing to read
    co = res.sets(where=masks["half"], count_only=True)
    assert co.count_only and co.total == total and np.array_equal(co.offsets, off)
    with pytest.raises(HGXError) as e:
        co.flat()
    assert e.value.code == _lib.HGX_E_INVALID and "count-only" in str(e.value)
    with pytest.raises(HGXError):
        co.read(0, 1)
    co.close()
    # the cap: the total passes, one less is refused with the total in the message, and the result stays usable
    res.sets(where=masks["half"], max_entries=total).close()
    for kw in ({}, {"count_only": True}, {"depths": True}):
        with pytest.raises(HGXError) as e:
            res.sets(where=masks["half"], max_entries=total - 1, **kw)
        assert e.value.code == _lib.HGX_E_NOMEM and str(total) in str(e.value), kw
    res.sets(max_entries=0, min_depth=60).close()                       # an empty result fits any cap
    vs = check(res, lv, None, 0, None, masks["half"], masks["half"], depths=True, tag="after the cap")
    # depths of an object made without them
    plain = res.sets(where=masks["half"])
    out = np.empty(4, np.int32)
    assert _lib.lib().hgx_visited_sets_read(plain.handle, 0, 4, None, out.ctypes.data) == _lib.HGX_E_INVALID
    assert np.array_equal(plain.read(0, 4), atoms[:4])
    plain.close()
    # paged reads: inside a set, across a boundary, up to and past the end
    b = int(off[3])
    for first, n in ((0, 0), (0, 1), (b - 2, 5), (b, int(off[5] - off[3])), (total - 3, 3), (total - 3, 10), (total, 4),
                     (0, total), (1, total)):
        a, d = vs.read(first, n)
        assert np.array_equal(a, atoms[first:first + n]) and np.array_equal(d, deps[first:first + n]), (first, n)
    for first, n in ((-1, 1), (total + 1, 0), (0, -1)):
        with pytest.raises(HGXError) as e:
            vs.read(first, n)
        assert e.value.code == _lib.HGX_E_INVALID
    # read twice: the same bytes; the result used after its sets are closed
    a1, d1 = vs.read()
    a2, d2 = vs.read()
    assert a1.tobytes() == a2.tobytes() == atoms.tobytes() and d1.tobytes() == d2.tobytes() == deps.tobytes()
    st = vs.stats()
    assert st["bytes"] >= 8.0 * (65 + 1) + 8.0 * total
    if block == 0:                                                       # rows only: the kernels served the seeds
        assert st["rows_read"] > 0
    vs.close()
    with pytest.raises(ValueError):
        vs.read()
    assert gpu_levels(res, 7) == lv[7]
    check(res, lv, [7, 64, 0], tag="after close").close()
    res.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 4. deep graphs: the bitmap skip over hundreds of levels
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,block", [("path", 1), ("path", 0), ("ladder", 0)])
def test_deep_graphs_skip_tiles(name, block):
    """path(300): 299 levels, each holding one or two atoms of ten tiles; ladder(40, 4): 40 levels.  With
    HGX_OPT_BFS_BLOCK 0 the kernels serve the seeds and skip almost every (tile, level) pair.  With the default the
    workgroup stage finishes these traversals, the host lists serve them and no kernel runs: the counters then stay
    zero, which the design asks for (no launch when every selected seed is of that kind)."""
    from hypergraphdb_amd import bfs_batch
    g = D.path(300) if name == "path" else D.ladder(40, 4)
    snap, orc = snapshot(g), oracle(g)
    snap.set_option(opt("BFS_BLOCK"), block)
    seeds = np.array([0, 299, 150, 7] if name == "path" else [0, 3, 82, 163], np.int32)
    rng = np.random.default_rng(5)
    keep = rng.random(g["num_atoms"]) < 0.5
    for mode in (SYM, ORD):
        lv = ref_levels(name, orc, seeds, mode, -1, None)
        assert max(len(x) for x in lv) >= (299 if name == "path" else 40)
        res = bfs_batch(snap, seeds, None, gen(snap, mode))
        for kw in (dict(), dict(dmin=1, dmax=None, where=keep, keep=keep), dict(dmin=17, dmax=33),
                   dict(sel=[3, 0], dmin=2, dmax=250, where=keep, keep=keep)):
            vs = check(res, lv, depths=True, tag=(name, block, mode, sorted(kw)), **kw)
            st = vs.stats()
            if block == 0:
                assert st["tiles_skipped"] > 0 and st["rows_read"] > 0, (name, mode, st)
            else:
                assert st["tiles_skipped"] > 0 or st["rows_read"] == 0, (name, mode, st)
            vs.close()
        res.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 5. heavy atoms: sets of many tiles per wavefront, many wavefronts
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", (0, 1))
def test_heavy_atoms_many_wavefronts(block):
    """A = 23000: 360 tiles, four to a wavefront, 90 wavefronts -- every set spans many of them, so the
    per-wavefront starts of the scan place the entries.  HGX_OPT_BFS_BLOCK 0: the rows engine and the kernels;
    1: whatever mix of the two engines the batch comes to."""
    from hypergraphdb_amd import bfs_batch, synth
    if "heavy" not in _CACHE:
        g = synth.hypergraph(3000, 20000, 2, 8, 2.1, 4, seed=23)
        _CACHE["heavy"] = (g, oracle(g), np.random.default_rng(9).integers(0, g["num_atoms"], 64).astype(np.int32))
    g, orc, seeds = _CACHE["heavy"]
    A = g["num_atoms"]
    assert A == 23000 and (A + 63) // 64 // 4 >= 3
    snap = snapshot(g)
    snap.set_option(opt("BFS_BLOCK"), block)
    keep = np.random.default_rng(10).random(A) < 0.5
    lv = ref_levels("heavy", orc, seeds, SYM, -1, 3)
    res = bfs_batch(snap, seeds, 3, gen(snap, SYM))
    vs = check(res, lv, tag=("heavy", block))
    assert vs.counts.max() > 4 * 64 * 3                                   # a set over more than three wavefronts
    if block == 0:
        assert vs.stats()["rows_read"] > 0
    vs.close()
    check(res, lv, None, 1, 3, keep, keep, depths=True, tag=("heavy masked", block)).close()
    check(res, lv, [63, 5, 0, 17], 2, 3, depths=True, tag=("heavy sel", block)).close()
    res.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# 6. every refusal that needs a live result
# ---------------------------------------------------------------------------------------------------
def test_refusals():
    from hypergraphdb_amd import AtomPredicate, HGXError, HGXUnsupported, _lib, bfs_batch
    from hypergraphdb_amd.partition import Shard, ShardSnapshot, partition_plan, pbfs_batch_group
    g, types, masks, seeds, orc = random_case()
    A = g["num_atoms"]
    snap, other = snapshot(g), snapshot(g)
    s = seeds[65]
    res = bfs_batch(snap, s, None, gen(snap, SYM))
    lv = ref_levels("random", orc, s, SYM, -1, None)

    def refused(code, names, *a, **kw):
        with pytest.raises(HGXError) as e:
            res.sets(*a, **kw)
        assert e.value.code == code and names in str(e.value), (a, kw, str(e.value))

    refused(_lib.HGX_E_INVALID, "min_depth", None, -1)
    refused(_lib.HGX_E_INVALID, "max_depth 1 is below min_depth 2", None, 2, 1)
    refused(_lib.HGX_E_INVALID, "max_depth", None, 0, -2)
    refused(_lib.HGX_E_NOTFOUND, "set 1: no such seed index 65", [0, 65])
    refused(_lib.HGX_E_NOTFOUND, "no such seed index -1", [-1])
    refused(_lib.HGX_E_INVALID, "set 2: seed index 3 repeats set 0", [3, 4, 3])
    with AtomPredicate.from_mask(other, masks["half"]) as foreign:        # a predicate of another snapshot
        refused(_lib.HGX_E_INVALID, "another graph", None, 0, None, foreign)
    L, h = _lib.lib(), _lib.C.c_void_p()
    idx = np.array([0, 1], np.int32)
    assert L.hgx_bfs_result_sets(res.handle, idx.ctypes.data, 2, 0, -1, None, 4, -1, _lib.C.byref(h)) == _lib.HGX_E_INVALID
    assert b"unknown flag bits" in L.hgx_last_error()
    assert L.hgx_bfs_result_sets(res.handle, idx.ctypes.data, -1, 0, -1, None, 0, -1, _lib.C.byref(h)) == _lib.HGX_E_INVALID
    assert L.hgx_bfs_result_sets(res.handle, None, 2, 0, -1, None, 0, -1, _lib.C.byref(h)) == _lib.HGX_E_INVALID
    assert L.hgx_bfs_result_sets(res.handle, idx.ctypes.data, 2, 0, -1, None, 0, -1, None) == _lib.HGX_E_INVALID
    with pytest.raises(ValueError):                                       # a mask of the wrong length
        res.sets(where=np.ones(A + 1, bool))
    # the result is as usable as before
    check(res, lv, [64, 0], tag="after the refusals").close()
    res.close()
    # a partition shard's result holds owned atoms only
    plan = partition_plan(A, g["link_atom"], g["tgt_off"], g["tgt_idx"], g.get("link_type"), 2)
    sh = []
    for p in range(2):
        sd = Shard.build(A, g["link_atom"], g["tgt_off"], g["tgt_idx"], g.get("link_type"), 2, p, plan)
        sh.append(ShardSnapshot(sd, 0))
        sd.close()
    pres = pbfs_batch_group(sh, [0, 1], None)
    for part in pres.parts:
        with pytest.raises(HGXUnsupported) as e:
            part.sets([0])
        assert "partition shard" in str(e.value)
    pres.close()
    snap.close()
    other.close()


# ---------------------------------------------------------------------------------------------------
# 7. reachable_batch: find_all(hg.and_(where, hg.bfs(start))) as a sorted set, for many starts
# ---------------------------------------------------------------------------------------------------
def test_reachable_batch_equals_find_all():
    from hypergraphdb_amd import (And, HGQueryConfiguration, HGXUnsupported, find_all, hg, pattern_batch_atoms,
                                  reachable_batch)
    g, types, masks, seeds, orc = random_case()
    snap = snapshot(g)
    snap.set_atom_types(types)
    starts = seeds[65][3:11]

    class TypedAnd:
        """ConditionToQuery for the And of type trees find_all is left with beside the traversal: over the atom
        index, nodes and links alike (include/hgx_atoms.h)."""

        def getQuery(self, snapshot, cond):
            class _Q:
                def execute(_self):
                    return list(pattern_batch_atoms(snapshot, [cond])[0].tolist())
            return _Q()

    def find_and(start):
        cond = hg.and_(tree(), hg.bfs(int(start)))
        try:
            return find_all(snap, cond)
        except HGXUnsupported:                                            # a typed clause without an incidence anchor
            cfg = HGQueryConfiguration()
            cfg.addCompiler(And, TypedAnd())
            return find_all(snap, cond, cfg)

    with reachable_batch(snap, starts, where=tree()) as vs:
        assert len(vs) == 8
        for i, s in enumerate(starts):
            assert vs[i].tolist() == sorted(set(find_and(s))), (i, int(s))
    with reachable_batch(snap, starts) as vs, reachable_batch(snap, starts, count_only=True) as co:
        flat = vs.flat()
        assert np.array_equal(co.counts, vs.counts)
        for i, s in enumerate(starts):
            o = int(vs.offsets[i])
            assert flat[o:o + int(vs.counts[i])].tolist() == sorted(set(find_all(snap, hg.bfs(int(s))))), (i, int(s))
    # the generator, the depth limit, the start itself and the depths go through
    lv = ref_levels("random", orc, seeds[65], ORD, 1, 2)
    with reachable_batch(snap, seeds[65], gen(snap, ORD, 1), 2, masks["half"], include_start=True, depths=True) as vs:
        off, atoms, deps = S.sets(lv, 0, None, masks["half"], True)
        assert np.array_equal(vs.offsets, off) and np.array_equal(vs.flat()[0], atoms) and np.array_equal(vs.flat()[1], deps)
        res = vs.owner
    assert res._h is None                                                 # the traversal's result closed with the sets
    snap.close()
