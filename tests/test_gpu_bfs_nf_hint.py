"""GPU parity of the hint step of the direct-pull BFS levels (HGX_OPT_NF_HINT): every listed atom first tries
the frontier row of its highest-degree neighbour (hgx_nf_hint), and only the atoms that row does not cover walk
their incidence.  Expected per-depth sets come from the oracle (check_batch) with the hint on; counts(), sampled
visited() sets and count_pass_levels are compared between hint 0 and 1, with HGX_OPT_NF_PULL = 2 (every dense
level on the direct pull) and 1 (the level rule).  stats()["nf_hint_atoms"] tells that the step ran."""
import numpy as np
import pytest

import kat_graphs as K
from oracle_ctypes import algen
from test_gpu_bfs import check_batch, gen, gpu_levels, levels_from_seq, oracle, snapshot
from test_gpu_bfs_direct_pull import exit_edges_graph, power_law, star

pytestmark = pytest.mark.gpu

SYM = K.ALGEN_MODES[0]


def run(snap, seeds, maxd, lt, pull, hint, sample, expected=None):
    """One batch; with `expected` (the oracle's levels per seed) every seed's sets and counts are checked as
    check_batch checks them.  Returns counts, the sampled seeds' sets and the stats."""
    from hypergraphdb_amd import _lib, bfs_batch
    snap.set_option(_lib.HGX_OPT_NF_PULL, pull)
    snap.set_option(_lib.HGX_OPT_NF_HINT, hint)
    res = bfs_batch(snap, seeds, maxd, gen(snap, SYM, lt))
    st = res.stats(accounting=False)
    counts = res.counts().copy()
    if expected is not None:
        for i, exp in enumerate(expected):
            assert gpu_levels(res, i) == exp, (i, int(seeds[i]), maxd, lt, pull)
            assert counts[i, :len(exp)].tolist() == [len(x) for x in exp]
            assert counts[i, len(exp):].sum() == 0
    sets = [[res.visited(int(i), d).tolist() for d in range(res.n_levels)] for i in sample]
    res.close()
    return counts, sets, st


def oracle_levels(orc, seeds, maxd, lt):
    """The oracle's per-depth sets of every seed, computed once per case."""
    out = []
    for s in seeds:
        l, a, d, _ = orc.bfs(int(s), -1 if maxd is None else maxd, algen(lt, *SYM))
        out.append(levels_from_seq(int(s), zip(l.tolist(), a.tolist(), d.tolist())))
    return out


def compare_hint(g, seeds, maxd=None, lt=-1, snap=None, orc=None):
    """Oracle sets with the hint on; counts, sampled sets and count_pass_levels equal with it off.  Under
    HGX_OPT_NF_PULL = 2 and 1.  Returns {pull: (stats without, stats with the hint)}."""
    from hypergraphdb_amd import _lib
    own = snap is None
    snap, orc = snap or snapshot(g), orc or oracle(g)
    snap.set_option(_lib.HGX_OPT_BFS_BLOCK, 0)   # the rows engine takes every seed
    sample = sorted({0, 1, len(seeds) // 2, len(seeds) - 1})
    expected = oracle_levels(orc, seeds, maxd, lt)
    out = {}
    for pull in (2, 1):
        on = run(snap, seeds, maxd, lt, pull, 1, sample, expected)
        off = run(snap, seeds, maxd, lt, pull, 0, sample)
        assert np.array_equal(on[0], off[0]), pull
        assert on[1] == off[1], pull
        assert on[2]["count_pass_levels"] == off[2]["count_pass_levels"], pull
        assert on[2]["level_sparse"] == off[2]["level_sparse"], pull   # the hint leaves the level rule alone
        assert on[2]["level_new"] == off[2]["level_new"], pull
        assert off[2]["nf_hint_atoms"] == 0, pull
        out[pull] = (off[2], on[2])
    if own:
        snap.close()
    return out


@pytest.mark.parametrize("n_seeds,lt,maxd", [
    (1024, -1, 4), (1024, -1, None), (1024, 1, 4), (1024, 1, None),      # W = 16, G = 8
    (300, -1, 4), (300, -1, None), (300, 1, 4), (300, 1, None),          # W = 8, G = 4
    (1500, -1, None),                                                    # two batches: 1024 + 476
])
def test_power_law_graphs(n_seeds, lt, maxd):
    g, has = power_law(21)
    seeds = np.random.default_rng(5).choice(has[lt], n_seeds, replace=False).astype(np.int32)
    out = compare_hint(g, seeds, maxd, lt)
    if lt >= 0:   # with a link-type condition a co-target need not be a neighbour: the hint is inert
        for pull in out:
            assert out[pull][1]["nf_hint_atoms"] == 0, pull


@pytest.mark.parametrize("n_seeds", [300, 1024])   # G = 4 and G = 8
@pytest.mark.parametrize("deg", [1, 2, 8, 9])
def test_exit_edges(deg, n_seeds):
    """Group A is decided by the hub's row, group B's hint is the hub behind its last entry, group C's hint (a
    private leaf) never covers: those atoms go through the residual list."""
    g, seeds = exit_edges_graph(deg, n_seeds)
    out = compare_hint(g, seeds)
    st = out[2][1]
    assert 3 in st["level_sparse"], st["level_sparse"]
    assert st["nf_hint_atoms"] > 0
    assert st["kernels"]["hgx_nf_pull"]["launches"] >= 1


@pytest.mark.parametrize("n_centre", [512, 513, 4096, 4097])   # the light bound; one and two hub chunks
def test_hub_that_never_covers(n_centre):
    """A listed hub whose hint is a leaf: the residual bitmap and the hub finalise behind the hint step."""
    g, seeds = star(n_centre)
    compare_hint(g, seeds)


def degenerate_graph():
    """A random graph with links longer than a lane group, plus: atom t1 whose only link is (t1, t1) (no hint),
    atom t2 with links (t2, t2, u) and (t2, t2) (its hint is u, never t2)."""
    base = K.random_graph(np.random.default_rng(8), 900, 2500, max_arity=12, n_types=2)
    A = base["num_atoms"]
    t1, l1, t2, l2, l3 = A, A + 1, A + 2, A + 3, A + 4
    u = int(base["tgt_idx"][0])
    rows = [(t1, t1), (t2, t2, u), (t2, t2)]
    off = base["tgt_off"].tolist()
    tg = base["tgt_idx"].tolist()
    for r in rows:
        tg += list(r)
        off.append(len(tg))
    g = dict(num_atoms=A + 5, link_atom=np.concatenate([base["link_atom"], np.array([l1, l2, l3], np.int32)]),
             tgt_off=np.array(off, np.int64), tgt_idx=np.array(tg, np.int32),
             link_type=np.concatenate([base["link_type"], np.zeros(3, np.int32)]))
    return g, t1, t2, u


@pytest.mark.parametrize("n_seeds", [1024, 300])
def test_degenerate_hints(n_seeds):
    g, t1, t2, u = degenerate_graph()
    rng = np.random.default_rng(3)
    seeds = rng.choice(g["num_atoms"] - 5, n_seeds - 3, replace=False).astype(np.int32)
    seeds = np.concatenate([seeds, np.array([t1, t2, u], np.int32)])   # t1 reaches nothing, t2 reaches u
    compare_hint(g, seeds)
    compare_hint(g, seeds[:-3], 3)   # t1 and t2 as listed atoms only (most hints are off the frontier at a level)


def test_update_rebuilds_the_table():
    """Atoms of group A lose every link to the hub (their old hint) and hang off a private leaf instead; atoms of
    group C gain a link to the hub (a new highest-degree neighbour).  A table kept across the update would let
    the hub's row decide atoms that no longer share a link with it."""
    deg, n_seeds, n_x = 2, 300, 90
    g, seeds = exit_edges_graph(deg, n_seeds)
    snap, orc = snapshot(g), oracle(g)
    before = compare_hint(g, seeds, snap=snap, orc=orc)
    assert before[2][1]["nf_hint_atoms"] > 0
    A = g["num_atoms"]
    hub, x0 = 0, 1 + n_seeds
    leaf0 = x0 + 3 * n_x
    moved = range(8)                                   # x_A,j: both hub links removed, one link to a leaf added
    remove = [int(g["link_atom"][n_seeds + deg * j + e]) for j in moved for e in range(deg)]
    add = {A + j: (0, [x0 + j, leaf0 + j]) for j in moved}
    add.update({A + 8 + j: (0, [hub, x0 + 2 * n_x + j]) for j in range(8)})   # x_C,j now sees the hub
    snap.update(add=add, remove=remove, num_atoms=A + 16)
    g2 = dict(num_atoms=snap.A, link_atom=snap.link_atom, tgt_off=snap.tgt_off, tgt_idx=snap.tgt_idx,
              link_type=snap.link_type)
    tg, off = np.asarray(g2["tgt_idx"]), np.asarray(g2["tgt_off"])
    for j in moved:   # no link holds both the hub and a moved atom any more
        assert not any(hub in tg[off[r]:off[r + 1]] and x0 + j in tg[off[r]:off[r + 1]] for r in range(len(off) - 1))
    from hypergraphdb_amd import _lib
    orc2 = oracle(g2)
    snap.set_option(_lib.HGX_OPT_NF_PULL, 2)
    snap.set_option(_lib.HGX_OPT_NF_HINT, 1)
    check_batch(g2, seeds, None, SYM, -1, snap, orc2)   # the first batch after the update rebuilds the table
    after = compare_hint(g2, seeds, snap=snap, orc=orc2)
    assert after[2][1]["nf_hint_atoms"] > 0
    snap.close()


def test_context_borrows_the_table():
    g, seeds = exit_edges_graph(8, 1024)
    snap = snapshot(g)
    from hypergraphdb_amd import _lib
    snap.set_option(_lib.HGX_OPT_BFS_BLOCK, 0)
    base = run(snap, seeds, None, -1, 2, 1, [0, 5, 1023])     # builds the table on the snapshot
    ctx = snap.context()
    ctx.set_option(_lib.HGX_OPT_BFS_BLOCK, 0)
    got = run(ctx, seeds, None, -1, 2, 1, [0, 5, 1023])
    again = run(snap, seeds, None, -1, 2, 1, [0, 5, 1023])
    ctx.close()
    snap.close()
    for other in (got, again):
        assert np.array_equal(other[0], base[0])
        assert other[1] == base[1]
        assert other[2]["nf_hint_atoms"] == base[2]["nf_hint_atoms"] > 0


def test_option_values():
    from hypergraphdb_amd import HGXError, _lib
    g, _ = exit_edges_graph(1, 300)
    snap = snapshot(g)
    for bad in (-1, 2):
        with pytest.raises(HGXError, match="HGX_OPT_NF_HINT"):
            snap.set_option(_lib.HGX_OPT_NF_HINT, bad)
    for ok in (0, 1):
        snap.set_option(_lib.HGX_OPT_NF_HINT, ok)
    snap.close()
