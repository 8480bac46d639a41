"""GPU parity on deep graphs: hundreds to thousands of BFS levels on every traversal engine, bit-exact against the
oracle.  The graphs come from tests/deep_graphs.py; tests/test_deep_graphs.py proves their depths on the CPU.

Shapes (final):
  rows engine (a, b, e)   band(400, hubs=2), node ids permuted: 3602 atoms, 204 levels from a pendant of one hub to
                          the pendants of the other, two atoms of 701 incident links that enter the frontier at
                          late levels.  40 / 200 / 300 / 1024 / 1100 seeds (row widths 1, 4, 8, 16 and 16 + 2), 70 % of
                          them on the band, drawn with repetition.
  set grid stage (c)      path(D + 1) for deepest distances D = 1000, 1022, 1023, 1024, 1025, 1100; seeds: position 0
                          and three interior positions.
  order-exact (d)         path(2047 / 2048), ladder(750, 3), ladder(1100, 2), path(2100), ladder(1023 / 1024 / 1025, 3);
                          band(400, hubs=2) for the level and key-array engines.
  no level limit          path(4200): 4199 levels on the rows engine, whose counter blocks are a ring of 4096.
  hops (e)                the 300-seed band result; path(1600).
  partitions (f)          band(200, hubs=2) (104 levels), path(70); 3 parts, 300 seeds.

The level cap of the two grid stages (kCoMaxLevels = 1024, hgx_seq.hip) -- see CO_MAX_LEVELS below."""
import ctypes as C

import numpy as np
import pytest

import deep_graphs as D
from oracle_ctypes import algen
from test_gpu_bfs import gen, oracle, snapshot
from test_gpu_bfs_hub_mask import opt_value
from test_gpu_hops import Ref, check_paths, check_rows
from test_gpu_partition import compare
from test_gpu_seq import check_seq

pytestmark = pytest.mark.gpu

# hgx_seq.hip: `constexpr int kCoMaxLevels = 1024;`.  Both grid stages run iteration d of their level loop on the
# atoms at distance d and decide, in this order:
#   hgx_bfs_coop:  `if (st != 0 || nf == 0 || d >= a.maxd) break;` then `if (d >= kCoMaxLevels) { atomicOr(a.ctl + kCoSt,
#                  4ull); break; }` -- and the store `a.lvl_end[(int64_t)s * kCoMaxLevels + d - 1]` at the head of
#                  iteration d is the per-seed atom count after distance d, so its last slot (d - 1 = 1023) belongs to
#                  distance 1024;
#   hgx_seq_coop:  `if (nf == 0 || d >= a.maxd) { done = true; break; }` then `if (T > kScKeyCap || d >= kCoMaxLevels)
#                  { atomicOr(st_sticky, 8ull); break; }` -- its per-level counts `kScLcnt + d * 64` end at d = 1023.
# nf counts the level's work items, and an atom without anything to expand (no incident link in the symmetric mode,
# an empty yield list in an ordered one: co_step's `nch == 0`, sc_put_items' zero degree) appends none.  So a stage
# finishes a traversal exactly when no atom at distance >= kCoMaxLevels has something to expand:
CO_MAX_LEVELS = 1024
CO_LAST_EXPANDED = CO_MAX_LEVELS - 1      # the largest distance whose atoms a stage expands
# the deepest distance D a stage finishes itself:
CO_DEEPEST_SYM = CO_LAST_EXPANDED         # symmetric mode: the deepest atom has its own link to expand (finds nothing)
CO_DEEPEST_FWD = CO_LAST_EXPANDED + 1     # FWD on a path / ladder: the deepest atoms yield nothing, found from 1023
CO_DEEPEST_FWD_LOOP = CO_LAST_EXPANDED    # ... with deep_graphs' loop links they yield the seed again: as symmetric

SYM, FWD, BACK = D.SYM, D.FWD, D.BACK
STAT_LISTS = ("union_frontier", "level_ms", "level_new", "level_bytes", "level_sparse", "level_rows", "level_xbytes",
              "level_xpair_max", "level_xms", "level_xtrips")
_CACHE = {}


def opt(name):
    from hypergraphdb_amd import _lib
    return getattr(_lib, "HGX_OPT_" + name)


def band_case():
    """band(400, hubs=2) with permuted node ids, its oracle and a shared rows-engine snapshot (default options)."""
    if "band" not in _CACHE:
        g = D.band(400, hubs=2, rng=np.random.default_rng(2024))
        snap = snapshot(g)
        snap.set_option(opt("BFS_BLOCK"), 0)
        _CACHE["band"] = (g, oracle(g), snap)
    return _CACHE["band"]


def rows_snapshot(g, **options):
    snap = snapshot(g)
    snap.set_option(opt("BFS_BLOCK"), 0)
    for k, v in options.items():
        snap.set_option(opt(k), v)
    return snap


def band_seeds(g, n, connected=False):
    """n seeds with repetition, 70 % on the band; a pendant of either hub, both hubs, a link atom (no incidence),
    both band ends and a duplicate among the first ones and (for a second batch) among the last ones.
    connected: no link atom among them, so every traversal reaches every node and atoms become visited by all."""
    rng = np.random.default_rng(1000 + n)
    anywhere = rng.integers(0, g["n_nodes"] if connected else g["num_atoms"], n)
    s = np.where(rng.random(n) < 0.7, rng.choice(g["pos"], n), anywhere).astype(np.int32)
    special = [g["pendants"][1][0], g["hub"][0], g["link_atom"][5], g["pos"][0], g["pos"][-1], g["pos"][0],
               g["pendants"][0][3], g["hub"][1]]
    s[:len(special)] = special
    s[-3:] = [g["pendants"][0][7], g["pos"][1], g["link_atom"][0]]
    if connected:
        s[[2, n - 1]] = g["pos"][[7, 8]]
    return s


def oracle_counts(orc, seeds, maxd, mode, lt, n_levels):
    """bfs_many counts over n_levels + 1 columns (the last one must stay empty) and the traversed items."""
    return orc.bfs_many(seeds, -1 if maxd is None else maxd, n_levels + 1, algen(lt, *mode))


def sample_seeds(oc, n_seeds, k=8):
    """k seed indices at least: the three with the most levels, the special first ones, the last (second batch)."""
    deep = np.argsort(-(oc > 0).sum(1), kind="stable")[:3].tolist()
    return sorted(set(deep + [0, 1, 2, 7, n_seeds // 2, n_seeds - 3, n_seeds - 1]))


def check_counts_and_sets(res, orc, seeds, maxd, mode, lt, tag):
    """counts() and n_levels against bfs_many for every seed and level; whole sets for the sampled seeds."""
    L = res.n_levels
    oc, trav = oracle_counts(orc, seeds, maxd, mode, lt, L)
    counts = res.counts()
    assert counts.shape == (len(seeds), L), tag
    assert oc[:, L].sum() == 0 and oc[:, L - 1].sum() > 0, (tag, "n_levels", L)
    assert np.array_equal(counts, oc[:, :L]), (tag, np.argwhere(counts != oc[:, :L])[:5])
    sample = sample_seeds(oc, len(seeds))
    assert len(sample) >= 8 or len(seeds) < 8
    empty = np.empty(0, np.int32)
    for i in sample:
        lv = orc.bfs_levels(int(seeds[i]), -1 if maxd is None else maxd, algen(lt, *mode))
        for d in range(L):
            assert np.array_equal(res.visited(i, d), lv[d] if d < len(lv) else empty), (tag, i, d)
    return oc, trav, sample


def check_stats(st, n_levels, trav, tag):
    print(tag, "n_levels", n_levels, "expanded", st["n_levels_expanded"], "batches", st["n_batches"])
    assert st["traversed_edges"] == float(trav.sum()), tag
    assert n_levels - 1 <= st["n_levels_expanded"] <= n_levels, (tag, st["n_levels_expanded"], n_levels)
    if n_levels > 66:
        assert st["n_levels_expanded"] > 64, tag
    for key in STAT_LISTS:      # the per-level statistics hold the first 64 levels, no more
        assert len(st[key]) == min(st["n_levels_expanded"], 64), (tag, key, len(st[key]))
    # the fields behind the per-level arrays of hgx_bfs_stats: nothing was written past a 64th entry
    assert (st["block_seeds"], st["block_rerun"], st["block_coop"], st["coop_fallbacks"]) == (0, 0, 0, 0), tag
    assert st["ms_exchange"] == 0 and st["bytes_exchanged"] == 0 and st["xwords_total"] == 0, tag


# ---------------------------------------------------------------------------------------------------
# a. the rows engine past 64 levels, every row width
# ---------------------------------------------------------------------------------------------------
ROWS_RUNS = {"sym": (None, SYM, -1), "d63": (63, SYM, -1), "d64": (64, SYM, -1), "d65": (65, SYM, -1),
             "d130": (130, SYM, -1), "fwd": (None, FWD, -1), "back": (None, BACK, -1), "typed": (None, SYM, 0)}


@pytest.mark.parametrize("run", sorted(ROWS_RUNS))
@pytest.mark.parametrize("n_seeds", [40, 200, 300, 1024, 1100])
def test_rows_engine_deep(n_seeds, run):
    """W = 1, 4, 8, 16 and a second batch of 76 seeds: counts of every seed and level, n_levels, the TEPS numerator
    and sampled sets equal the oracle's over ~200 levels, unbounded and with depth limits around the 64-entry
    statistics arrays, in two ordered modes and with a link type."""
    from hypergraphdb_amd import bfs_batch
    g, orc, snap = band_case()
    maxd, mode, lt = ROWS_RUNS[run]
    seeds = band_seeds(g, n_seeds)
    res = bfs_batch(snap, seeds, maxd, gen(snap, mode, lt))
    tag = (n_seeds, run)
    oc, trav, _ = check_counts_and_sets(res, orc, seeds, maxd, mode, lt, tag)
    if maxd is not None:
        assert res.n_levels == maxd + 1, tag
    else:
        assert res.n_levels > 200, (tag, res.n_levels)
    check_stats(res.stats(), res.n_levels, trav, tag)
    res.close()


def test_rows_engine_deep_timed_statistics():
    """With device timing on, level_ms is one more 64-entry array filled per level (by the kernel's level tag)."""
    from hypergraphdb_amd import bfs_batch
    g, orc, _ = band_case()
    snap = rows_snapshot(g)
    snap.set_timing(True)
    seeds = band_seeds(g, 300)
    res = bfs_batch(snap, seeds, None, gen(snap, SYM))
    oc, trav, _ = check_counts_and_sets(res, orc, seeds, None, SYM, -1, "timed")
    st = res.stats()
    check_stats(st, res.n_levels, trav, "timed")
    assert len(st["level_ms"]) == 64 and min(st["level_ms"]) > 0 and st["ms_total"] > 0
    res.close()
    snap.close()


def test_depth_of_and_paged_sets_beyond_level_64():
    """depth_of on atoms at distance 0, 64, 65 and the deepest (and a never reached one); hgx_bfs_result_visited_range
    pages through the 700 pendants found at level 202 and through a two-atom level."""
    from hypergraphdb_amd import bfs_batch
    from hypergraphdb_amd._lib import check, lib, ptr
    g, orc, snap = band_case()
    seeds = band_seeds(g, 300)
    res = bfs_batch(snap, seeds, None, gen(snap, SYM))
    for i in (0, 3, 4):          # a pendant of the near hub (204 levels), position 0, position n - 1
        lv = orc.bfs_levels(int(seeds[i]), -1)
        assert len(lv) > 200
        for d in (0, 1, 64, 65, len(lv) - 2, len(lv) - 1):
            for a in lv[d][[0, -1]]:
                assert res.depth_of(i, int(a)) == d, (i, d, a)
        assert res.depth_of(i, int(g["link_atom"][0])) == -1
        for d in (70, len(lv) - 1):
            want = lv[d]
            for cap in (1, 256, 1000):
                got, first = [], 0
                while True:
                    out = np.full(cap, -7, np.int32)
                    n = C.c_int64()
                    check(lib().hgx_bfs_result_visited_range(res.handle, C.c_int32(i), C.c_int32(d), C.c_int64(first),
                                                             C.c_void_p(ptr(out)), C.c_int64(cap), C.byref(n)))
                    assert n.value == len(want), (i, d, cap, first)
                    k = min(cap, len(want) - first)
                    assert (out[k:] == -7).all()
                    got += out[:k].tolist()
                    first += cap
                    if first >= len(want):
                        break
                assert got == want.tolist(), (i, d, cap)
        assert len(lv[-1]) == D.PENDANTS      # the last level read above in pages: a hub's pendants
    res.close()


@pytest.mark.parametrize("block", [0, 1])
@pytest.mark.parametrize("mode_name,flags", [("sym", 0x3BE), ("fwd", 0x3BE), ("fwd", 0x1BE)])
def test_rows_engine_beyond_4096_levels(mode_name, flags, block):
    """path(4200): 4199 levels.  The rows engine's per-level counter blocks are a ring of 4096 (run_levels); it used to
    stop after 4095 expanded levels without an error (path(4097) from position 0 came back as 4096 atoms).  With
    HGX_OPT_BFS_BLOCK 1 the end seeds reach it through the workgroup and grid stages' hand-overs."""
    g = D.path(4200)
    snap, orc = snapshot(g), oracle(g)
    snap.set_option(opt("BFS_BLOCK"), block)
    snap.set_option(opt("BFS_FLAGS"), flags)
    seeds = np.array([0, 4199, 2100, 104, 0], np.int32)      # 104: 4095 levels to the far end
    st = check_set_batch(snap, orc, seeds, None, SYM if mode_name == "sym" else FWD, (mode_name, hex(flags), block))
    assert st["n_levels_expanded"] >= 4199 and st["coop_fallbacks"] == 0
    st = check_set_batch(snap, orc, seeds, 4097, SYM if mode_name == "sym" else FWD, (mode_name, hex(flags), block, 4097))
    snap.close()


# ---------------------------------------------------------------------------------------------------
# b. the deep levels really run the dense kernels; the engine options on the same run
# ---------------------------------------------------------------------------------------------------
def dense_base(connected=False):
    """The 1024-seed symmetric run with default options: counts, the sampled seeds' sets as bytes, statistics.
    connected: the seed set without link atoms (every traversal reaches every node)."""
    key = ("dense", connected)
    if key not in _CACHE:
        from hypergraphdb_amd import bfs_batch
        g, orc, snap = band_case()
        seeds = band_seeds(g, 1024, connected)
        res = bfs_batch(snap, seeds, None, gen(snap, SYM))
        oc, trav, sample = check_counts_and_sets(res, orc, seeds, None, SYM, -1, key)
        sets = [res.visited(i, d).tobytes() for i in sample for d in range(res.n_levels)]
        _CACHE[key] = dict(seeds=seeds, oc=oc, counts=res.counts().copy(), sample=sample, sets=sets,
                           st=res.stats(accounting=False), n_levels=res.n_levels)
        res.close()
    return _CACHE[key]


def test_dense_kernels_run_past_level_64():
    """level_sparse shows only 64 levels: the launch counts prove that the dense gather and the heavy-chunk pull ran on
    more than 64 levels of the 1024-seed run."""
    b = dense_base()
    k = b["st"]["kernels"]
    print("launches", {n: v["launches"] for n, v in k.items()}, "level_sparse", b["st"]["level_sparse"],
          "count_pass_levels", b["st"]["count_pass_levels"])
    assert b["n_levels"] > 200
    assert k["hgx_link_gather"]["launches"] > 64
    assert k["hgx_atom_pull_heavy"]["launches"] > 64
    assert b["st"]["count_pass_levels"] == 0          # fused counts on: no level left to the readout's pass


OPTION_RUNS = {
    "flags_0x0": dict(BFS_FLAGS=0x0), "flags_0x1BE": dict(BFS_FLAGS=0x1BE), "flags_0x3FE": dict(BFS_FLAGS=0x3FE),
    "flags_0xBBE": dict(BFS_FLAGS=0xBBE), "flags_0x83BE": dict(BFS_FLAGS=0x83BE), "flags_0x203BE": dict(BFS_FLAGS=0x203BE),
    "nf_pull_0": dict(NF_PULL=0), "nf_pull_2": dict(NF_PULL=2), "nf_pull_2_hint_0": dict(NF_PULL=2, NF_HINT=0),
    "count_fused_0": dict(COUNT_FUSED=0), "hub_mask_0": dict(HUB_MASK=0),
    "hub_mask_2": dict(HUB_MASK=opt_value(2, 1, 0x1)),
}


# The hint step of the direct pull decides an atom only when its row becomes full (visited by all 1024 traversals),
# which no atom does while a seed is a link atom that reaches nothing: the direct-pull options run once more on
# the connected seed set, where the late levels also skip the atoms and links every traversal has visited.
SWEEP = [(False, n) for n in sorted(OPTION_RUNS)] + \
        [(True, n) for n in ("flags_0x0", "flags_0x203BE", "nf_pull_0", "nf_pull_2", "nf_pull_2_hint_0", "hub_mask_2")]


@pytest.mark.parametrize("connected,name", SWEEP)
def test_dense_deep_option_sweep(connected, name):
    """Every engine option on the 1024-seed run: counts equal to the default run's and the oracle's, the sampled
    seeds' sets byte-identical; and the statistics that tell the option's path ran."""
    from hypergraphdb_amd import bfs_batch
    g, _, _ = band_case()
    b = dense_base(connected)
    snap = rows_snapshot(g, **OPTION_RUNS[name])
    res = bfs_batch(snap, b["seeds"], None, gen(snap, SYM))
    assert res.n_levels == b["n_levels"], name
    counts = res.counts()
    assert np.array_equal(counts, b["counts"]) and np.array_equal(counts, b["oc"][:, :res.n_levels]), name
    sets = [res.visited(i, d).tobytes() for i in b["sample"] for d in range(res.n_levels)]
    assert sets == b["sets"], name
    st = res.stats(accounting=False)
    print(connected, name, {n: v["launches"] for n, v in st["kernels"].items()}, "nf_hint_atoms", st["nf_hint_atoms"],
          "hub_mask_entries", st["hub_mask_entries"], "count_pass_levels", st["count_pass_levels"])
    if name == "nf_pull_2":
        assert st["kernels"]["hgx_nf_pull"]["launches"] > 64
        assert (st["nf_hint_atoms"] > 0) == connected
    if name == "nf_pull_2_hint_0":
        assert st["nf_hint_atoms"] == 0 and st["kernels"]["hgx_nf_pull"]["launches"] > 64
    if name == "hub_mask_2":
        assert st["hub_mask_entries"] > 0
    if name == "hub_mask_0":
        assert st["hub_mask_entries"] == 0
    if name == "count_fused_0":
        assert st["count_pass_levels"] > 64
    if name == "flags_0x203BE":
        assert st["kernels"]["hgx_fc_pull"]["launches"] > 0
    res.close()
    snap.close()


@pytest.mark.parametrize("n_seeds", [300, 1024])
def test_ordered_push_pipelined_and_not(n_seeds):
    """The ordered mode over ~200 push levels with the levels issued one ahead of the host (0x3BE, bit 9) and
    without (0x1BE): identical counts and sets, both the oracle's."""
    from hypergraphdb_amd import bfs_batch
    g, orc, _ = band_case()
    seeds = band_seeds(g, n_seeds)
    out = {}
    for flags in (0x3BE, 0x1BE):
        snap = rows_snapshot(g, BFS_FLAGS=flags)
        res = bfs_batch(snap, seeds, None, gen(snap, FWD))
        _, trav, sample = check_counts_and_sets(res, orc, seeds, None, FWD, -1, (n_seeds, hex(flags)))
        assert res.stats()["traversed_edges"] == float(trav.sum())
        out[flags] = (res.counts().copy(), [res.visited(i, d).tobytes() for i in sample for d in range(res.n_levels)])
        res.close()
        snap.close()
    assert np.array_equal(out[0x3BE][0], out[0x1BE][0]) and out[0x3BE][1] == out[0x1BE][1]


# ---------------------------------------------------------------------------------------------------
# c. the multi-workgroup set stage at its level cap
# ---------------------------------------------------------------------------------------------------
def stage_seeds(g, deepest):
    """Position 0 (the deep seed) and three interior positions."""
    return g["pos"][[0, deepest // 4, deepest // 2, deepest - 7]].astype(np.int32)


def check_set_batch(snap, orc, seeds, maxd, mode, tag):
    """One batch against the oracle: counts of every seed and level, the whole sets of seed 0.  Returns the stats."""
    from hypergraphdb_amd import bfs_batch
    res = bfs_batch(snap, seeds, maxd, gen(snap, mode))
    L = res.n_levels
    oc, trav = oracle_counts(orc, seeds, maxd, mode, -1, L)
    assert oc[:, L].sum() == 0 and oc[:, L - 1].sum() > 0, (tag, "n_levels", L)
    assert np.array_equal(res.counts(), oc[:, :L]), tag
    lv = orc.bfs_levels(int(seeds[0]), -1 if maxd is None else maxd, algen(-1, *mode))
    assert len(lv) == (oc[0] > 0).sum()
    for d in range(L):
        assert np.array_equal(res.visited(0, d), lv[d] if d < len(lv) else np.empty(0, np.int32)), (tag, d)
    st = res.stats()
    assert st["traversed_edges"] == float(trav.sum()), tag
    res.close()
    return st


def check_stage_clean(snap, g, orc, mode, deepest, tag, maxd=None):
    """After a handed-over batch: a shallow batch on the same snapshot, straight to the stage, is exact and the
    stage finishes it -- its per-seed bitmaps were left clean."""
    snap.set_option(opt("BFS_BLOCK"), 2)
    mid = deepest // 2
    seeds = g["pos"][[mid, mid + 7, mid - 9, mid]].astype(np.int32)
    st = check_set_batch(snap, orc, seeds, maxd, mode, (tag, "after"))
    assert st["block_coop"] == len(seeds) and st["block_rerun"] == 0 and st["coop_fallbacks"] == 0, (tag, st)


@pytest.mark.parametrize("mode_name,loop", [("sym", False), ("fwd", False), ("fwd", True)])
@pytest.mark.parametrize("deepest", [1000, 1022, 1023, 1024, 1025, 1100])
def test_set_grid_stage_level_cap(deepest, mode_name, loop):
    """HGX_OPT_BFS_BLOCK 2 on path(deepest + 1): up to the cap the stage finishes every seed of the batch itself;
    beyond it the whole batch goes to the rows engine -- exact either way, the level cap is no barrier timeout, and the
    stage is clean afterwards."""
    mode = SYM if mode_name == "sym" else FWD
    last = CO_DEEPEST_SYM if mode_name == "sym" else CO_DEEPEST_FWD_LOOP if loop else CO_DEEPEST_FWD
    g = D.path(deepest + 1, loop=loop)
    snap, orc = snapshot(g), oracle(g)
    snap.set_option(opt("BFS_BLOCK"), 2)
    seeds = stage_seeds(g, deepest)
    tag = (deepest, mode_name, loop)
    st = check_set_batch(snap, orc, seeds, None, mode, tag)
    print(tag, {k: st[k] for k in ("block_coop", "block_seeds", "block_rerun", "coop_fallbacks", "n_levels_expanded")})
    assert st["coop_fallbacks"] == 0, (tag, st)
    if deepest <= last:
        assert st["block_coop"] == len(seeds) and st["block_rerun"] == 0, (tag, st)
    else:
        assert st["block_coop"] == 0 and st["block_rerun"] == len(seeds) and st["block_seeds"] == 0, (tag, st)
        assert st["n_levels_expanded"] >= deepest          # the rows engine ran the levels
        # (with the loop link FWD walks the whole cycle from any seed: the shallow batch takes a depth limit)
        check_stage_clean(snap, g, orc, mode, deepest, tag, 600 if loop else None)
    # a depth limit at the cap ends the traversal before the cap does
    st = check_set_batch(snap, orc, seeds, CO_MAX_LEVELS, mode, (tag, "maxd"))
    assert st["block_coop"] == len(seeds), (tag, st)
    snap.close()


@pytest.mark.parametrize("mode_name", ["sym", "fwd"])
def test_chained_hand_over_behind_the_workgroup_stage(mode_name):
    """HGX_OPT_BFS_BLOCK 1: a seed on a 1640-atom path outgrows the workgroup, goes to the chained grid stage and
    from its level cap to the rows engine.  The workgroup holds kBbDisc = 1535 examined atoms with the seed
    (hgx_seq.hip), so the end of a 1534-atom and of a 1535-atom path stay in the workgroup stage (1533 and 1534
    levels in one launch) and the end of a 1536-atom path leaves it."""
    mode = SYM if mode_name == "sym" else FWD
    g = D.disjoint(D.path(1640), D.path(1534), D.path(1535), D.path(1536))
    snap, orc = snapshot(g), oracle(g)
    snap.set_option(opt("BFS_BLOCK"), 1)
    p0, p1, p2, p3 = g["pos"]
    # symmetric: position 1100 of the long path (1100 levels to the left, 539 to the right, 1639 atoms).  FWD reaches
    # only the atoms behind the seed, so a seed that outgrows the workgroup's atoms is deeper: position 0, 1639 levels
    deep = p0[1100] if mode_name == "sym" else p0[0]
    sym = mode_name == "sym"
    batches = [([deep, p1[0], p2[0], p3[0]], dict(block_seeds=2, block_rerun=2, block_coop=0)),
               ([deep, p2[0]], dict(block_seeds=1, block_rerun=1, block_coop=0)),
               ([p1[0], p2[0], p2[1], p1[0]], dict(block_seeds=4, block_rerun=0, block_coop=0)),
               ([p3[0]], dict(block_seeds=0, block_rerun=1, block_coop=0)),
               # 1535 atoms past the seed, 835 levels: symmetric, the chained stage finishes it (counted in
               # block_seeds too); FWD reaches 835 atoms and stays in the workgroup
               ([p3[700], p1[5]], dict(block_seeds=2, block_rerun=0, block_coop=1 if sym else 0))]
    for seeds, want in batches:
        seeds = np.asarray(seeds, np.int32)
        st = check_set_batch(snap, orc, seeds, None, mode, (mode_name, seeds.tolist()))
        print(mode_name, seeds.tolist(), {k: st[k] for k in ("block_coop", "block_seeds", "block_rerun", "coop_fallbacks")})
        assert {k: st[k] for k in want} == want and st["coop_fallbacks"] == 0, (seeds, want, st)
    # the stage the chained launches left at their level cap is clean: a shallow batch straight to it
    snap.set_option(opt("BFS_BLOCK"), 2)
    seeds = p0[[800, 830, 790]].astype(np.int32)
    st = check_set_batch(snap, orc, seeds, None, mode, (mode_name, "after"))
    assert st["block_coop"] == 3 and st["coop_fallbacks"] == 0, st
    snap.close()


# ---------------------------------------------------------------------------------------------------
# d. the order-exact engines
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_name", ["sym", "fwd"])
@pytest.mark.parametrize("n", [2047, 2048])
def test_order_exact_workgroup_engine_2046_pairs(n, mode_name):
    """path(2047) from position 0 is 2046 pairs over 2046 levels: the most the workgroup engine holds, in one launch.
    path(2048) has one pair more and goes to the level engine (in FWD through the grid stage, whose level cap
    it exceeds)."""
    mode = SYM if mode_name == "sym" else FWD
    g = D.path(n)
    res = check_seq(g, np.array([0], np.int32), None, mode)
    print(n, mode_name, "n_block", res.n_block, "n_level", res.n_level, "n_coop", res.n_coop)
    assert len(res.atoms) == n - 1 and res.dists.max() == n - 1
    if n == 2047:
        assert (res.n_block, res.n_level, res.n_coop) == (1, 0, 0)
    else:
        assert (res.n_block, res.n_level, res.n_coop) == (0, 1, 0)


def test_order_exact_grid_stage_750_levels():
    """ladder(750, 3): more than 2046 pairs over 750 levels, below the cap: the grid stage finishes the seed."""
    g = D.ladder(750, 3)
    snap, orc = snapshot(g), oracle(g)
    seeds = np.array([0, 1, 3 * 700, 0], np.int32)
    res = check_seq(g, seeds, None, FWD, -1, snap, orc)
    print("ladder(750, 3)", res.n_block, res.n_level, res.n_coop)
    assert len(res.pairs(0)[0]) == D.ladder_pairs(750, 3) > 2046
    assert res.n_coop == 3 and res.n_level == 3 and res.n_block == 1
    snap.close()


@pytest.mark.parametrize("shape", ["ladder", "path"])
def test_order_exact_grid_stage_above_the_cap(shape):
    """ladder(1100, 2) and path(2100): more than 2046 pairs and more than 1024 levels -- the grid stage hands the seed
    to the level engine; exact, and a following shallow call on the same snapshot is exact too."""
    g = D.ladder(1100, 2) if shape == "ladder" else D.path(2100)
    snap, orc = snapshot(g), oracle(g)
    res = check_seq(g, np.array([0], np.int32), None, FWD, -1, snap, orc)
    print(shape, res.n_block, res.n_level, res.n_coop)
    assert len(res.atoms) > 2046 and (res.n_block, res.n_level, res.n_coop) == (0, 1, 0)
    res = check_seq(g, np.array([g["n_nodes"] - 40, 0, 2 * 600], np.int32), 30, FWD, -1, snap, orc)
    assert res.n_block == 3
    snap.close()


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("levels", [1023, 1024, 1025])
def test_order_exact_grid_stage_level_cap(levels, loop):
    """Ladders of width 3 (more than 2046 pairs) whose deepest distance is 1023, 1024 and 1025: exact, finished by the
    grid stage up to the cap and by the level engine beyond; then a 825-level traversal on the same snapshot, which
    the stage must finish exactly (its bitmaps, hash and counts were left clean by the level-cap exit)."""
    g = D.ladder(levels, 3, loop=loop)
    snap, orc = snapshot(g), oracle(g)
    res = check_seq(g, np.array([0], np.int32), None, FWD, -1, snap, orc)
    print(levels, loop, res.n_block, res.n_level, res.n_coop)
    assert len(res.atoms) == D.ladder_pairs(levels, 3)
    last = CO_DEEPEST_FWD_LOOP if loop else CO_DEEPEST_FWD
    assert (res.n_block, res.n_level, res.n_coop) == (0, 1, 1 if levels <= last else 0)
    # (with the loop links FWD walks on from the last layer through atom 0: there the traversal takes a depth limit)
    res = check_seq(g, np.array([3 * 200, 3 * 201 + 1], np.int32), 700 if loop else None, FWD, -1, snap, orc)
    assert len(res.pairs(0)[0]) > 2046 and (res.n_block, res.n_level, res.n_coop) == (0, 2, 2)
    snap.close()


SEQ_DEFAULTS = {"SEQ_ENGINE": 0, "SEQ_PULL": 1, "SEQ_SMALL": 0, "SEQ_PACK_MIN": 0}
LEVEL_ENGINE_RUNS = {"pull_0": dict(SEQ_PULL=0), "pull_1": dict(SEQ_PULL=1), "pull_2": dict(SEQ_PULL=2),
                     "small": dict(SEQ_SMALL=1), "pack_every_level": dict(SEQ_PACK_MIN=1)}


def seq_with_options(g, snap, orc, seeds, mode, options):
    for k, v in options.items():
        snap.set_option(opt(k), v)
    try:
        return check_seq(g, seeds, None, mode, -1, snap, orc)
    finally:
        for k in options:
            snap.set_option(opt(k), SEQ_DEFAULTS[k])


@pytest.mark.parametrize("mode_name", ["sym", "fwd"])
@pytest.mark.parametrize("run", sorted(LEVEL_ENGINE_RUNS))
def test_order_exact_level_engine_200_levels(run, mode_name):
    """HGX_OPT_SEQ_ENGINE 2 over ~200 levels with 70 seeds: the 4-slot counter ring and the host polling one level
    behind, every level pushed / pulled / chosen by width, tiny starting capacities, packed transfers on every level."""
    g, orc, _ = band_case()
    if "seq_snap" not in _CACHE:
        _CACHE["seq_snap"] = snapshot(g)
    snap = _CACHE["seq_snap"]
    seeds = band_seeds(g, 70)
    res = seq_with_options(g, snap, orc, seeds, SYM if mode_name == "sym" else FWD,
                           dict(LEVEL_ENGINE_RUNS[run], SEQ_ENGINE=2))
    print(run, mode_name, "levels", res.n_levels, "pull_levels", res.pull_levels, "n_level", res.n_level)
    assert res.n_levels > 200 and res.n_level == 70 and res.n_block == 0 and res.n_coop == 0
    if run == "pull_0":
        assert res.pull_levels == 0
    if run == "pull_2":
        assert res.pull_levels > 64


@pytest.mark.parametrize("mode_name", ["sym", "fwd"])
def test_order_exact_key_array_engine_200_levels(mode_name):
    """HGX_OPT_SEQ_ENGINE 1 (two host round trips a level) over ~200 levels, 8 seeds."""
    g, orc, _ = band_case()
    snap = snapshot(g)
    seeds = band_seeds(g, 8)
    res = seq_with_options(g, snap, orc, seeds, SYM if mode_name == "sym" else FWD, dict(SEQ_ENGINE=1))
    assert res.n_levels > 200
    snap.close()


# ---------------------------------------------------------------------------------------------------
# e. hop paths: one step back per level
# ---------------------------------------------------------------------------------------------------
def goals_at(depth, distances, unreachable):
    """One goal per wanted distance (the lowest atom id there) and the unreachable ones."""
    by = {}
    for n, d in depth.items():
        by.setdefault(d, []).append(n)
    return [min(by[d]) for d in distances] + [max(by[d]) for d in distances] + list(unreachable)


def test_hop_paths_band_300_seeds():
    """Paths out of the 300-seed rows result (W = 8): goals at distances 0, 1, 64, 65 and the deepest, unreachable
    goals, whole distance and predecessor rows of the deepest seed."""
    from hypergraphdb_amd import bfs_batch
    g, orc, snap = band_case()
    seeds = band_seeds(g, 300)
    ref = Ref(orc, SYM)
    res = bfs_batch(snap, seeds, None, gen(snap, SYM))
    counts = res.counts()
    picked = [0, 3, 4, int(np.argsort(-(counts > 0).sum(1), kind="stable")[0]), 299 - 2]
    si, goals = [], []
    for i in picked:
        depth, _ = ref.of(seeds[i])
        deepest = max(depth.values())
        assert deepest == (counts[i] > 0).sum() - 1
        q = goals_at(depth, (0, 1, 64, 65, deepest - 1, deepest), [g["link_atom"][3], g["link_atom"][-1]])
        si += [i] * len(q)
        goals += q
    si += [2, 2]                       # the link-atom seed: itself, and an atom it does not reach
    goals += [int(seeds[2]), int(g["pos"][0])]
    si, goals = np.array(si, np.int32), np.array(goals, np.int32)
    with res.paths(si, goals) as hp:
        check_paths(hp, seeds[si], goals, ref, ("band",))
        deepest = (counts[0] > 0).sum() - 1          # seed 0: a pendant of the near hub, 204 levels
        assert hp.hops.max() == deepest == 204 and (hp.hops == -1).sum() == 2 * len(picked) + 1
        assert hp.stats()["steps"] >= 204
    check_rows(res, 0, seeds[0], g["num_atoms"], ref, ("band",), orc.bfs_levels(int(seeds[0]), -1))
    res.close()


@pytest.mark.parametrize("block", [0, 1, 2])
def test_hop_paths_path_1600(block):
    """path(1600) under the three HGX_OPT_BFS_BLOCK values.  Symmetric seeds at both ends: 1599 hops, distance and
    predecessor rows whose largest value exceeds 1024 (for 1 and 2 the result of a level-cap hand-over).  FWD seeds
    800 and 900 deep: the rows, the workgroup table and the grid stage's pair list as storage forms."""
    from hypergraphdb_amd import bfs_batch
    g = D.path(1600)
    A = g["num_atoms"]
    snap, orc = snapshot(g), oracle(g)
    snap.set_option(opt("BFS_BLOCK"), block)
    # symmetric, 1599 levels
    ref = Ref(orc, SYM)
    seeds = np.array([0, 1599, 400], np.int32)
    res = bfs_batch(snap, seeds, None, gen(snap, SYM))
    depth, _ = ref.of(0)
    q = goals_at(depth, (0, 1, 64, 65, 1024, 1025, 1599), [1600, A - 1])
    si = np.array([0] * len(q) + [1, 1, 2, 2], np.int32)
    goals = np.array(q + [0, 1598, 1599, 0], np.int32)
    with res.paths(si, goals) as hp:
        check_paths(hp, seeds[si], goals, ref, (block, "sym"))
        assert hp.hops.max() == 1599 and (hp.hops == -1).sum() == 2
    check_rows(res, 0, 0, A, ref, (block, "sym"), orc.bfs_levels(0, -1))
    assert res.depths(0).max() == 1599 and res.depths(1)[0] == 1599
    st = res.stats(accounting=False)
    assert st["block_coop"] == 0 and st["block_seeds"] == 0 and st["block_rerun"] == (3 if block else 0), st
    res.close()
    # FWD, 799 and 899 levels
    ref = Ref(orc, FWD)
    seeds = np.array([800, 700], np.int32)
    res = bfs_batch(snap, seeds, None, gen(snap, FWD))
    st = res.stats(accounting=False)
    print(block, {k: st[k] for k in ("block_coop", "block_seeds", "block_rerun")})
    assert (st["block_seeds"], st["block_coop"], st["block_rerun"]) == [(0, 0, 0), (2, 0, 0), (2, 2, 0)][block], st
    depth, _ = ref.of(700)
    q = goals_at(depth, (0, 1, 64, 65, 899), [699, 1600])
    si = np.array([1] * len(q) + [0, 0], np.int32)
    goals = np.array(q + [1599, 799], np.int32)
    with res.paths(si, goals) as hp:
        check_paths(hp, seeds[si], goals, ref, (block, "fwd"))
        assert hp.hops.max() == 899
    check_rows(res, 1, 700, A, ref, (block, "fwd"), orc.bfs_levels(700, -1, algen(-1, *FWD)))
    res.close()
    snap.close()


# ---------------------------------------------------------------------------------------------------
# f. partitioned BFS: one exchange per level
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_name,xb", [("sym", None), ("fwd", None), ("sym", (2, 2))])
def test_partitioned_band_100_levels(mode_name, xb):
    """Three parts over band(200, hubs=2) (104 levels) with 300 seeds: union of the parts' results against the whole
    snapshot and the oracle; every part expanded more than 64 levels."""
    g = D.band(200, hubs=2, rng=np.random.default_rng(77))
    seeds = band_seeds(g, 300)
    st = compare(g, 3, seeds, None, SYM if mode_name == "sym" else FWD, xb=xb)
    print(mode_name, xb, [s["n_levels_expanded"] for s in st])
    assert len(st) == 3
    for s in st:
        assert s["n_levels_expanded"] > 64 and len(s["level_xbytes"]) == 64 and len(s["level_xtrips"]) == 64


@pytest.mark.parametrize("mode_name", ["sym", "fwd"])
def test_partitioned_path_70(mode_name):
    """path(70): 69 levels against the parts' 64-entry per-level arrays."""
    g = D.path(70, rng=np.random.default_rng(78))
    rng = np.random.default_rng(79)
    seeds = rng.integers(0, g["num_atoms"], 300).astype(np.int32)
    seeds[:3] = g["pos"][[0, 69, 35]]
    st = compare(g, 3, seeds, None, SYM if mode_name == "sym" else FWD)
    assert max(s["n_levels_expanded"] for s in st) >= 69
