"""GPU parity of the direct pull of dense symmetric-mode levels (HGX_OPT_NF_PULL): hgx_nf_pull with the
cover test after every entry, chosen by the level rule (1) or forced onto every eligible dense level (2),
against the 8-entry step under the old rule (0).  Expected per-depth sets come from the oracle
(check_batch); counts() and sampled visited() sets are also compared between the three option values."""
import functools

import numpy as np
import pytest

import kat_graphs as K
from test_gpu_bfs import check_batch, gen, oracle, snapshot

pytestmark = pytest.mark.gpu

SYM = K.ALGEN_MODES[0]


def run(snap, seeds, maxd, lt, opt, sample):
    from hypergraphdb_amd import _lib, bfs_batch
    snap.set_option(_lib.HGX_OPT_NF_PULL, opt)
    res = bfs_batch(snap, seeds, maxd, gen(snap, SYM, lt))
    st = res.stats(accounting=False)
    counts = res.counts().copy()
    sets = [[res.visited(int(i), d).tolist() for d in range(res.n_levels)] for i in sample]
    res.close()
    return counts, sets, st


def compare_options(g, seeds, maxd=None, lt=-1, need_kind3=True):
    """Oracle sets under option 2; counts and sampled sets equal under 0, 1 and 2.  Returns the stats per option."""
    from hypergraphdb_amd import _lib
    snap, orc = snapshot(g), oracle(g)
    snap.set_option(_lib.HGX_OPT_BFS_BLOCK, 0)   # the rows engine takes every seed
    snap.set_option(_lib.HGX_OPT_NF_PULL, 2)
    check_batch(g, seeds, maxd, SYM, lt, snap, orc)
    sample = sorted({0, 1, len(seeds) // 2, len(seeds) - 1})
    out = {opt: run(snap, seeds, maxd, lt, opt, sample) for opt in (0, 1, 2)}
    snap.close()
    for opt in (1, 2):
        assert np.array_equal(out[opt][0], out[0][0]), opt
        assert out[opt][1] == out[0][1], opt
        assert out[opt][2]["count_pass_levels"] == out[0][2]["count_pass_levels"], opt
    st2 = out[2][2]
    if need_kind3:
        assert 3 in st2["level_sparse"], st2["level_sparse"]
        assert st2["kernels"]["hgx_nf_pull"]["launches"] >= 1
    assert 0 not in st2["level_sparse"], st2["level_sparse"]   # option 2: no gather + pull level is left
    return {opt: out[opt][2] for opt in out}


@functools.lru_cache(maxsize=None)
def power_law(seed):
    """(graph, atoms with incidence per link type or -1), built once and left unchanged."""
    from hypergraphdb_amd import synth
    g = synth.hypergraph(3000, 20000, 2, 8, 2.1, 3, seed=seed)
    off, tg, lt_of = np.asarray(g["tgt_off"]), np.asarray(g["tgt_idx"]), np.asarray(g["link_type"])
    has = {}
    for lt in (-1, 1):
        m = np.zeros(g["num_atoms"], bool)
        for r in (np.arange(len(off) - 1) if lt < 0 else np.nonzero(lt_of == lt)[0]):
            m[tg[off[r]:off[r + 1]]] = True
        has[lt] = np.nonzero(m)[0]
    return g, has


@pytest.mark.parametrize("n_seeds,lt,maxd", [
    (1024, -1, 4), (1024, -1, None), (1024, 1, 4), (1024, 1, None),      # W = 16, G = 8
    (300, -1, 4), (300, -1, None), (300, 1, 4), (300, 1, None),          # W = 8, G = 4
    (1500, -1, None),                                                    # two batches: 1024 + 476
])
def test_power_law_graphs(n_seeds, lt, maxd):
    g, has = power_law(21)
    seeds = np.random.default_rng(5).choice(has[lt], n_seeds, replace=False).astype(np.int32)
    compare_options(g, seeds, maxd, lt)


def star(n_centre, n_seeds=290, n_far=10):
    """A centre with n_centre incident links (centre, leaf i, leaf i + 1); the leaves also sit on two rings
    of pair links, so the seed level is dense.  A far component (a path) holds n_far seeds that never reach
    the centre: its row never covers every traversal, at any level."""
    n = n_centre
    centre, leaf0, far0 = 0, 1, 1 + n
    rows = [(centre, leaf0 + i, leaf0 + (i + 1) % n) for i in range(n)]
    rows += [(leaf0 + i, leaf0 + (i + 7) % n) for i in range(n)]
    rows += [(leaf0 + i, leaf0 + (i + 31) % n) for i in range(n)]
    n_path = 2 * n_far
    rows += [(far0 + i, far0 + i + 1) for i in range(n_path - 1)]
    n_nodes = 1 + n + n_path
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    g = dict(num_atoms=n_nodes + len(rows), link_atom=np.arange(n_nodes, n_nodes + len(rows), dtype=np.int32),
             tgt_off=off, tgt_idx=np.array([x for r in rows for x in r], np.int32),
             link_type=np.zeros(len(rows), np.int32))
    rng = np.random.default_rng(n)
    seeds = np.concatenate([leaf0 + rng.choice(n, n_seeds, replace=False), far0 + 2 * np.arange(n_far)])
    return g, seeds.astype(np.int32)


@pytest.mark.parametrize("n_centre", [512, 513, 4096, 4097])   # the light bound; one and two hub chunks
def test_hub_that_never_covers(n_centre):
    g, seeds = star(n_centre)
    compare_options(g, seeds)


def exit_edges_graph(deg, n_seeds):
    """Atom x_j has `deg` links.  In group A every link of x_j leads to a hub that all seeds reach
    early, so x_j covers at its first entry; in group B only the last link does (the others lead to private
    leaves), so it covers exactly at its last entry; in group C none does (never).  The hub also holds 1000
    pad links, so the level that expands it is dense."""
    rows, n_x = [], 90
    hub = 0
    seeds0 = 1                      # the seed nodes, all linked to the hub
    x0 = seeds0 + n_seeds
    leaf0 = x0 + 3 * n_x
    rows += [(hub, seeds0 + i) for i in range(n_seeds)]
    nleaf = 0
    for grp in range(3):
        for j in range(n_x):
            x = x0 + grp * n_x + j
            for e in range(deg):
                to_hub = grp == 0 or (grp == 1 and e == deg - 1)
                if to_hub:
                    rows.append((hub, x))
                else:
                    rows.append((leaf0 + nleaf, x))
                    nleaf += 1
    # the private leaves hang off one seed each, so they are on a frontier (with one bit) when x pulls
    for i in range(nleaf):
        rows.append((seeds0 + i % n_seeds, leaf0 + i))
    pad0 = leaf0 + nleaf
    rows += [(hub, pad0 + i) for i in range(1000)]
    n_nodes = pad0 + 1000
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    g = dict(num_atoms=n_nodes + len(rows), link_atom=np.arange(n_nodes, n_nodes + len(rows), dtype=np.int32),
             tgt_off=off, tgt_idx=np.array([x for r in rows for x in r], np.int32),
             link_type=np.zeros(len(rows), np.int32))
    return g, np.arange(seeds0, seeds0 + n_seeds, dtype=np.int32)


@pytest.mark.parametrize("n_seeds", [300, 1024])   # G = 4 and G = 8
@pytest.mark.parametrize("deg", [1, 2, 8, 9])
def test_exit_edges(deg, n_seeds):
    g, seeds = exit_edges_graph(deg, n_seeds)
    compare_options(g, seeds)


def test_duplicate_targets():
    """Links that hold the pulling atom twice, and a frontier co-target twice (the own-row skip)."""
    base = K.random_graph(np.random.default_rng(41), 700, 2600, max_arity=6, repeat_p=0.0, link_targets=False)
    off, tg = base["tgt_off"].tolist(), base["tgt_idx"].tolist()
    rows = [tg[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    for i, r in enumerate(rows):
        if len(r) >= 2 and i % 3 == 0:
            r.append(r[0])            # the first target twice: as t and as a co-target of the others
        if len(r) >= 2 and i % 5 == 0:
            r.insert(1, r[-1])
    g = dict(base, tgt_off=np.cumsum([0] + [len(r) for r in rows]).astype(np.int64),
             tgt_idx=np.array([x for r in rows for x in r], np.int32))
    seeds = np.random.default_rng(2).integers(0, g["num_atoms"], 1024).astype(np.int32)
    compare_options(g, seeds)
    compare_options(g, seeds[:300], 3, need_kind3=False)


@pytest.mark.parametrize("n_seeds", [1024, 300])
def test_long_links(n_seeds):
    """Arity above the group width: the rest-of-the-link path."""
    g = K.random_graph(np.random.default_rng(8), 900, 2500, max_arity=12, n_types=2)
    seeds = np.random.default_rng(3).integers(0, g["num_atoms"], n_seeds).astype(np.int32)
    compare_options(g, seeds)
    compare_options(g, seeds, None, 1, need_kind3=False)


def test_option_values_and_parent_level_kinds():
    from hypergraphdb_amd import HGXError, _lib
    from test_gpu_bfs_fused_counts import graph
    g, _, has = graph("hubs")
    snap = snapshot(g)
    for bad in (3, -1):
        with pytest.raises(HGXError, match="HGX_OPT_NF_PULL"):
            snap.set_option(_lib.HGX_OPT_NF_PULL, bad)
    snap.set_option(_lib.HGX_OPT_BFS_BLOCK, 0)
    seeds = np.random.default_rng(15).choice(has[-1], 1024, replace=False).astype(np.int32)   # the w16 inputs
    _, _, st0 = run(snap, seeds, None, -1, 0, [0])
    _, _, st1 = run(snap, seeds, None, -1, 1, [0])
    snap.close()
    kinds = st0["level_sparse"]
    # the parent's choice on these inputs: dense gather + pull levels first, then the non-full pull
    assert 0 in kinds and 3 in kinds, kinds
    first3 = kinds.index(3)
    assert all(k == 3 for k in kinds[first3:] if k in (0, 3)), kinds
    assert 0 in st1["level_sparse"] and 3 in st1["level_sparse"], st1["level_sparse"]
    assert st1["level_sparse"][kinds.index(0)] == 0, st1["level_sparse"]   # the first dense level stays on gather + pull
