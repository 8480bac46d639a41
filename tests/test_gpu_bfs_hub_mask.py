"""GPU parity of the hub mask of the dense BFS levels (HGX_OPT_HUB_MASK): C = the OR of the level rows of the
snapshot's top-degree atoms on the frontier; a hub chunk that covers C goes on reading only the rows of the links
marked in lr (hgx_hub_mask, hgx_link_gather2_fr, hgx_atom_pull_hub).  Expected per-depth sets come from the oracle
(check_batch) with the option at 2; counts(), sampled visited() sets, level_sparse, level_new and
count_pass_levels are compared between the option at 0, 1 and 2.  stats()["hub_mask_entries"] tells that hub
entries were walked in filtered mode.

hub_graph builds the smallest graphs on which the step runs: level 1 is a dense level whose frontier holds at
least two atoms of every link (so every link row is written), with a hub H that is first seen at depth 2, a top
atom T0 that every common seed reaches at depth 1 (its row is C), and rare seeds that reach H only through
one carrier atom at a chosen entry of H's incidence."""
import numpy as np
import pytest

import kat_graphs as K
from test_gpu_bfs import check_batch, gen, oracle, snapshot
from test_gpu_bfs_direct_pull import power_law, star

pytestmark = pytest.mark.gpu

SYM = K.ALGEN_MODES[0]


def opt_value(mode, T=0, sched=0):
    return mode + (T << 8) + (sched << 16)


def hub_graph(D, S, t0_top=True, t0_at=0, y_span=None, heavy_rare=False, long_links=False, hub_seed=False):
    """H = atom 0 with D incident links, in this order of its incidence: entry e holds T0 when e % 4096 == t0_at
    (every chunk meets T0 at that entry; t0_at None = never), a rare seed's light carrier at entry 256 (right
    after the first cover test) and at entry D - 1 (the last entry of the last chunk), with heavy_rare a carrier
    of degree > 512 at entry D - 2; every other entry holds two y atoms (all y, or the first y_span of them, so
    that H's links alone never cover C).  long_links: the entry-256 link has arity 12 with the carrier at
    position 10, the last link lists its carrier twice.  t0_top: T0 gets more links than H (the top atom, a hub)."""
    n = D + 8
    Sc = S - 3
    H, T0, y0 = 0, 1, 2
    c0 = y0 + n
    q0 = c0 + Sc                       # rare seeds q0, q1, q2
    r0 = q0 + 3                        # carriers r0, r1 (light), r2 (heavy); each with two companions
    w0 = r0 + 9                        # the heavy carrier's far atoms
    n_nodes = w0 + 522

    def y(j):
        return y0 + j % (y_span or n)

    rows = []
    for e in range(D):
        if t0_at is not None and e % 4096 == t0_at:
            rows.append((H, T0, y(e)))
        elif e == 256:
            rows.append((H,) + tuple(y(e + k) for k in range(9)) + (r0, y(e)) if long_links else (H, r0, y(e)))
        elif e == D - 1:
            rows.append((H, r0 + 1, r0 + 1, y(e)) if long_links else (H, r0 + 1, y(e)))
        elif heavy_rare and e == D - 2:
            rows.append((H, r0 + 2, y(e)))
        else:
            rows.append((H, y(e), y(e + 1)))
    rows += [(c0 + j % Sc, y0 + j, y0 + (j + 1) % n, y0 + (j + 2) % n, y0 + (j + 3) % n) for j in range(n)]
    rows += [(c0 + i, T0, y0 + i % n) for i in range(Sc)]
    if t0_top:
        rows += [(T0, y0 + j % n, y0 + (j + 1) % n, y0 + (j + 2) % n) for j in range(D + 16)]
    for k in range(3 if heavy_rare else 2):
        rows.append((q0 + k, r0 + k, r0 + 3 + 2 * k, r0 + 4 + 2 * k))
    if heavy_rare:
        rows += [(r0 + 2, w0 + j, w0 + j + 1) for j in range(520)]
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    g = dict(num_atoms=n_nodes + len(rows), link_atom=np.arange(n_nodes, n_nodes + len(rows), dtype=np.int32),
             tgt_off=off, tgt_idx=np.array([x for r in rows for x in r], np.int32),
             link_type=(np.arange(len(rows)) % 2).astype(np.int32))
    seeds = list(range(c0, c0 + Sc)) + [q0, q0 + 1, q0 + 2]
    if hub_seed:
        seeds[0] = H                   # (c0 leaves the batch: S stays the same)
    return g, np.array(seeds, np.int32)


def run(snap, seeds, maxd, mode, lt, opt, sample):
    from hypergraphdb_amd import _lib, bfs_batch
    snap.set_option(_lib.HGX_OPT_HUB_MASK, opt)
    res = bfs_batch(snap, seeds, maxd, gen(snap, mode, lt))
    st = res.stats(accounting=False)
    counts = res.counts().copy()
    sets = [[res.visited(int(i), d).tolist() for d in range(res.n_levels)] for i in sample]
    res.close()
    return counts, sets, st


def compare(g, seeds, maxd=None, lt=-1, T=0, sched=0, mode=SYM, nf_pull=0, snap=None, orc=None):
    """Oracle sets with the option at 2; counts, sampled sets, level kinds, level sizes and count_pass_levels
    equal at 0, 1 and 2.  Returns {option: stats}."""
    from hypergraphdb_amd import _lib
    own = snap is None
    snap, orc = snap or snapshot(g), orc or oracle(g)
    snap.set_option(_lib.HGX_OPT_BFS_BLOCK, 0)        # the rows engine takes every seed
    snap.set_option(_lib.HGX_OPT_NF_PULL, nf_pull)    # 0: the early dense levels stay gather + pull
    snap.set_option(_lib.HGX_OPT_HUB_MASK, opt_value(2, T, sched))
    check_batch(g, seeds, maxd, mode, lt, snap, orc)
    sample = sorted({0, 1, len(seeds) // 2, len(seeds) - 3, len(seeds) - 2, len(seeds) - 1})
    out = {m: run(snap, seeds, maxd, mode, lt, opt_value(m, T, sched), sample) for m in (0, 1, 2)}
    if own:
        snap.close()
    for m in (1, 2):
        assert np.array_equal(out[m][0], out[0][0]), m
        assert out[m][1] == out[0][1], m
        for key in ("level_sparse", "level_new", "count_pass_levels"):
            assert out[m][2][key] == out[0][2][key], (m, key)
    assert out[0][2]["hub_mask_entries"] == 0 and out[0][2]["hub_mask_skipped"] == 0
    return {m: out[m][2] for m in out}


def assert_filtered(st):
    assert st["level_sparse"][1] == 0, st["level_sparse"]     # level 1 ran gather + pull
    assert st["hub_mask_entries"] > 0
    assert 0 < st["hub_mask_skipped"] < st["hub_mask_entries"]   # the carriers' rows were read


def assert_inert(out):
    for m in out:
        assert out[m]["hub_mask_entries"] == 0 and out[m]["hub_mask_skipped"] == 0, m


@pytest.mark.parametrize("S", [300, 1024])                    # W = 8, G = 4 and W = 16, G = 8
@pytest.mark.parametrize("D", [513, 4096, 4097, 9000])        # light bound; one chunk; two; three with a short last
def test_hub_sizes_late_rare_sources(D, S):
    """A rare source behind a light carrier right after the switch and in the last entry of the last chunk, and
    one behind a heavy carrier: a missed lr bit is a missing source at depth 2.  With the default T the heavy
    carrier is listed, its source is in C and H's chunks cover C only behind the carrier's entry."""
    g, seeds = hub_graph(D, S, heavy_rare=True)
    out = compare(g, seeds, T=1)                              # T0 alone: a listed heavy carrier would put its source into C
    assert_filtered(out[2])
    # the rule: |C| = S - 3 passes at level 1, where the heavy carrier's degree against a quarter of the hub
    # incidence decides; it runs the step on a subset of the levels that option 2 runs it on
    assert out[1]["hub_mask_entries"] <= out[2]["hub_mask_entries"]
    if D >= 4096:
        assert_filtered(out[1])
    compare(g, seeds)


@pytest.mark.parametrize("S", [300, 1024])
def test_long_links(S):
    """The only fr atom of an arity-12 link at position 10, and a link that lists its carrier twice."""
    g, seeds = hub_graph(4096, S, long_links=True)
    out = compare(g, seeds)
    assert_filtered(out[2])
    assert_filtered(out[1])                                   # few carriers, |C| = S - 3: the rule runs the step
    assert compare(g, seeds, lt=0)[2]["hub_mask_entries"] > 0   # a link-type condition (H's even entries only)


def test_switch_after_the_final_test():
    """T0 at entry 3900 of H's chunk, behind the last scheduled test (entry 2048): nothing is filtered."""
    g, seeds = hub_graph(4096, 300, t0_top=False, t0_at=3900, y_span=40)
    assert_inert(compare(g, seeds, maxd=2))                   # depth 2: level 1 is the last (at level 2 vis[H] covers C)
    assert_inert(compare(g, seeds, maxd=2, sched=0xFFFF))     # T0 in round 15, the last: no test follows it
    compare(g, seeds)
    g, seeds = hub_graph(4096, 300, t0_top=False, t0_at=3500, y_span=40)
    out = compare(g, seeds, maxd=2, sched=0xFFFF)
    assert out[2]["hub_mask_entries"] == 4096 - 3584          # T0 in round 13, rounds 14 and 15 filtered


def test_chunk_that_never_covers():
    g, seeds = hub_graph(4096, 300, t0_top=False, t0_at=None, y_span=40)
    assert_inert(compare(g, seeds, maxd=2))
    compare(g, seeds)
    g, seeds = hub_graph(9000, 1024, t0_at=None, y_span=40)   # T0 is a hub itself: its own chunks switch
    compare(g, seeds)


@pytest.mark.parametrize("T", [1, 64])
def test_top_list_sizes(T):
    g, seeds = hub_graph(4096, 300)
    assert_filtered(compare(g, seeds, T=T)[2])                # T0 is the atom of largest degree


def test_no_listed_atom_on_the_frontier():
    g, seeds = hub_graph(4096, 300, t0_top=False)             # the top atom is H, first seen at depth 2
    assert_inert(compare(g, seeds, maxd=2, T=1))
    compare(g, seeds, T=1)
    assert_filtered(compare(g, seeds, T=2)[2])                # H and T0


@pytest.mark.parametrize("S", [300, 1024])
def test_hub_that_is_a_seed(S):
    g, seeds = hub_graph(4097, S, hub_seed=True)              # H is listed too (the second largest degree)
    compare(g, seeds)
    compare(g, seeds, maxd=2)


def test_fewer_atoms_than_the_list():
    """A graph of 40 atoms has no hub: the step is inert whatever T says."""
    g = K.random_graph(np.random.default_rng(4), 25, 15, max_arity=5, n_types=2)
    assert g["num_atoms"] < 64
    seeds = np.resize(np.arange(25, dtype=np.int32), 300)
    assert_inert(compare(g, seeds, T=64))


@pytest.mark.parametrize("n_seeds,maxd,nf_pull,sched", [
    (300, 4, 1, 0), (300, None, 0, 0xFFFF), (1024, 4, 0, 0xFFFF), (1024, None, 1, 0),
    (1500, 4, 1, 0), (1500, None, 0, 0),                      # two batches: 1024 + 476
])
def test_power_law_graphs(n_seeds, maxd, nf_pull, sched):
    g, has = power_law(21)
    seeds = np.random.default_rng(5).choice(has[-1], n_seeds, replace=False).astype(np.int32)
    compare(g, seeds, maxd, nf_pull=nf_pull, sched=sched)


@pytest.mark.parametrize("n_centre", [513, 4097])
def test_star(n_centre):
    g, seeds = star(n_centre)
    compare(g, seeds)


@pytest.mark.parametrize("mode", K.ALGEN_MODES[1:3])          # after-first and before-first: ordered generators
def test_inert_in_ordered_modes(mode):
    g, seeds = hub_graph(513, 300)
    assert_inert(compare(g, seeds, mode=mode))


def test_inert_on_narrow_batches():
    g, seeds = hub_graph(4096, 300)
    assert_inert(compare(g, seeds[-200:]))                    # W = 4


def test_update_rebuilds_the_list():
    """With T = 1 the list is T0.  The update moves the common seeds' links from T0 to a new atom T1 of larger
    degree: a list kept across the update names T0, which is no longer on the frontier of level 1."""
    D, S = 4096, 300
    g, seeds = hub_graph(D, S)
    snap, orc = snapshot(g), oracle(g)
    assert_filtered(compare(g, seeds, T=1, snap=snap, orc=orc)[2])
    A, n, Sc = g["num_atoms"], D + 8, S - 3
    y0, c0 = 2, 2 + n
    T1 = A
    first_t0 = D + n                                          # row of (c0, T0, y0): behind H's and the y links
    remove = [int(g["link_atom"][first_t0 + i]) for i in range(Sc)]
    add = {A + 1 + i: (0, [c0 + i, T1, y0 + i % n]) for i in range(Sc)}
    add.update({A + 1 + Sc + j: (0, [T1, y0 + j % n, y0 + (j + 1) % n, y0 + (j + 2) % n]) for j in range(2 * D)})
    add[A + 1 + Sc + 2 * D] = (0, [0, T1, y0])                # H meets T1 in a last entry
    snap.update(add=add, remove=remove, num_atoms=A + 2 + Sc + 2 * D)
    g2 = dict(num_atoms=snap.A, link_atom=snap.link_atom, tgt_off=snap.tgt_off, tgt_idx=snap.tgt_idx,
              link_type=snap.link_type)
    out = compare(g2, seeds, T=1, snap=snap, orc=oracle(g2))
    assert out[2]["level_sparse"][1] == 0 and out[2]["hub_mask_entries"] > 0
    snap.close()


def test_context_borrows_the_list():
    from hypergraphdb_amd import _lib
    g, seeds = hub_graph(4097, 1024)
    snap = snapshot(g)
    snap.set_option(_lib.HGX_OPT_BFS_BLOCK, 0)
    snap.set_option(_lib.HGX_OPT_NF_PULL, 0)
    early = snap.context()                                    # created before the list is built
    base = run(snap, seeds, None, SYM, -1, 2, [0, 5, 1023])   # builds the list on the snapshot
    late = snap.context()
    got = [run(c, seeds, None, SYM, -1, 2, [0, 5, 1023]) for c in (early, late, snap)]
    early.close()
    late.close()
    snap.close()
    for other in got:
        assert np.array_equal(other[0], base[0])
        assert other[1] == base[1]
        assert other[2]["hub_mask_entries"] == base[2]["hub_mask_entries"] > 0


def test_option_values():
    from hypergraphdb_amd import HGXError, _lib
    g, _ = star(513)
    snap = snapshot(g)
    for bad in (-1, 3, opt_value(1, T=65), 1 << 32):
        with pytest.raises(HGXError, match="HGX_OPT_HUB_MASK"):
            snap.set_option(_lib.HGX_OPT_HUB_MASK, bad)
    for ok in (0, 1, 2, opt_value(1, T=64), opt_value(2, T=8, sched=0xFFFF)):
        snap.set_option(_lib.HGX_OPT_HUB_MASK, ok)
    snap.close()
