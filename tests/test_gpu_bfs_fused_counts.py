"""GPU parity of the fused level counts (HGX_OPT_COUNT_FUSED): the dense-level kernels that store a
level's new rows (hgx_atom_pull2 + hgx_hub_finalize, hgx_nf_pull) also count them per source, and the
readout skips its counting pass for those levels.  counts() with the option on equals counts() with it
off, the size of every per-depth set, and the oracle's per-depth counts; stats()["count_pass_levels"]
tells whether a level was left to the pass."""
import functools

import numpy as np
import pytest

import kat_graphs as K
from oracle_ctypes import algen
from test_gpu_bfs import gen, oracle, snapshot

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def graph(name):
    """(graph, oracle, atoms with incidence per link type or -1), built once and left unchanged."""
    from hypergraphdb_amd import synth
    if name == "hubs":      # power-law hubs above 512 incidences (heavy chunks + hub finalise), dense from level 1
        g = synth.hypergraph(3000, 20000, 2, 8, 2.1, 3, seed=12)
    elif name == "tiny":    # one tile, A not a multiple of 64
        g = K.random_graph(np.random.default_rng(3), 50, 80)
    else:                   # "small": fewer tiles than waves, A not a multiple of 64
        g = K.random_graph(np.random.default_rng(77), 800, 2500, max_arity=7, n_types=3)
    off, tg = np.asarray(g["tgt_off"]), np.asarray(g["tgt_idx"])
    lt_of = g.get("link_type")
    has = {}
    for lt in (-1, 1):
        rows = np.arange(len(off) - 1) if lt < 0 or lt_of is None else np.nonzero(np.asarray(lt_of) == lt)[0]
        m = np.zeros(g["num_atoms"], bool)
        for r in rows:
            m[tg[off[r]:off[r + 1]]] = True
        has[lt] = np.nonzero(m)[0]
    return g, oracle(g), has


def run(snap, seeds, mode, lt, fused):
    from hypergraphdb_amd import _lib, bfs_batch
    snap.set_option(_lib.HGX_OPT_COUNT_FUSED, fused)
    res = bfs_batch(snap, seeds, None, gen(snap, mode, lt))
    st = res.stats(accounting=False)
    counts = res.counts().copy()
    sizes = np.array([[len(res.visited(i, d)) for d in range(res.n_levels)] for i in range(len(seeds))], np.int64)
    res.close()
    return counts, sizes, st


# (graph, seeds, link type, generator mode, every dense level fused?)
CASES = {
    "w16": ("hubs", 1024, -1, 0, True),          # W = 16, G = 8
    "w8": ("hubs", 300, -1, 0, True),            # W = 8, G = 4
    "w2_legacy": ("hubs", 100, -1, 0, False),    # W = 2: the one-row kernels, counted by the pass
    "two_batches": ("hubs", 1500, -1, 0, True),  # 1024 + 476
    "typed": ("hubs", 1024, 1, 0, True),
    "ordered": ("hubs", 1024, -1, 1, False),     # ordered mode: hgx_atom_pull, counted by the pass
    "tiny_40": ("tiny", 40, -1, 0, None),        # blocks without atoms
    "small_1024": ("small", 1024, -1, 0, True),  # duplicate seeds, fewer tiles than waves
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_counts_equal_pass_sets_and_oracle(case):
    from hypergraphdb_amd import _lib
    name, n_seeds, lt, mi, all_fused = CASES[case]
    g, orc, has = graph(name)
    mode = K.ALGEN_MODES[mi]
    rng = np.random.default_rng(15)
    if name == "hubs":   # seeds with (typed) incidence: atoms become full, late levels run the non-full pull
        seeds = rng.choice(has[lt], n_seeds, replace=False).astype(np.int32)
    elif name == "tiny":
        seeds = np.arange(n_seeds, dtype=np.int32)
    else:
        seeds = rng.integers(0, g["num_atoms"], n_seeds).astype(np.int32)
    snap = snapshot(g)
    snap.set_option(_lib.HGX_OPT_BFS_BLOCK, 0)   # the rows engine takes every seed
    c1, sizes1, st1 = run(snap, seeds, mode, lt, 1)
    c0, sizes0, st0 = run(snap, seeds, mode, lt, 0)
    snap.close()
    assert np.array_equal(c1, c0)
    assert np.array_equal(c1, sizes1) and np.array_equal(c0, sizes0)
    nl = c1.shape[1]
    oc, _ = orc.bfs_many(seeds, -1, nl + 1, algen(lt, *mode))
    assert np.array_equal(c1, oc[:, :nl]) and oc[:, nl:].sum() == 0
    kinds = st1["level_sparse"]
    assert kinds == st0["level_sparse"]
    if all_fused is True:
        assert st1["count_pass_levels"] == 0, (st1["count_pass_levels"], kinds)
    elif all_fused is False:
        assert st1["count_pass_levels"] > 0, kinds
    assert st0["count_pass_levels"] >= st1["count_pass_levels"]
    if name == "hubs":   # dense from level 1 on: with the option off those levels are left to the pass
        assert st0["count_pass_levels"] >= 1, kinds
    assert st0["n_batches"] == (n_seeds + 1023) // 1024
    if case == "w16":   # the fused kernels were the ones that ran: dense pull levels and a non-full pull level
        assert 0 in kinds and 3 in kinds, kinds
