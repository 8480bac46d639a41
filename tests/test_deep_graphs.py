"""The deep test graphs of tests/deep_graphs.py against the oracle, without a GPU: the closed-form depths the
GPU tests of tests/test_gpu_deep.py rest on (in particular the deepest distances around the grid stages'
1024-level cap), and OracleGraph.bfs_many against per-seed OracleGraph.bfs on a band with hubs."""
import numpy as np
import pytest

import deep_graphs as D
from oracle_ctypes import OracleGraph, algen


def oracle(g):
    return OracleGraph(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"])


def depth(orc, seed, mode=D.SYM, lt=-1):
    """(deepest distance, atoms reached) of one traversal."""
    _, a, d, _ = orc.bfs(int(seed), -1, algen(lt, *mode))
    return (int(d.max()) if len(d) else 0), len(a)


def check_form(g):
    A, M = g["num_atoms"], len(g["link_atom"])
    assert g["link_atom"].tolist() == list(range(g["n_nodes"], A)) and len(g["tgt_off"]) == M + 1
    assert g["tgt_off"][0] == 0 and g["tgt_off"][-1] == len(g["tgt_idx"]) and len(g["link_type"]) == M
    assert g["tgt_idx"].min() >= 0 and g["tgt_idx"].max() < g["n_nodes"]
    assert g["tgt_idx"].dtype == np.int32 and g["tgt_off"].dtype == np.int64


@pytest.mark.parametrize("n", [2, 70, 1024, 1025, 1026, 1534, 1535, 1536, 2047, 2048, 2100, 4097, 4200])
def test_path_depths(n):
    g = D.path(n)
    check_form(g)
    orc = oracle(g)
    assert depth(orc, 0) == (n - 1, n - 1)
    assert depth(orc, 0, D.FWD) == (n - 1, n - 1)
    assert depth(orc, n - 1, D.FWD) == (0, 0)
    assert depth(orc, n // 2) == (max(n // 2, n - 1 - n // 2), n - 1)
    l, a, d, _ = orc.bfs(0, -1, algen(-1, *D.FWD))
    assert a.tolist() == list(range(1, n)) and d.tolist() == list(range(1, n)) and l.tolist() == list(range(n, 2 * n - 1))


@pytest.mark.parametrize("n", [1024, 1025, 1026])
def test_path_loop_keeps_the_forward_depths(n):
    g = D.path(n, loop=True)
    check_form(g)
    orc = oracle(g)
    assert depth(orc, 0, D.FWD) == (n - 1, n - 1)
    assert orc.generate(n - 1, algen(-1, *D.FWD)) == [(g["num_atoms"] - 1, 0)]      # the deepest atom yields the seed
    assert oracle(D.path(n)).generate(n - 1, algen(-1, *D.FWD)) == []               # without the loop: nothing


def test_disjoint_union():
    parts = [D.path(1640), D.path(1534), D.path(1535), D.path(1536)]
    g = D.disjoint(*parts)
    check_form(g)
    orc = oracle(g)
    assert [len(p) for p in g["pos"]] == [1640, 1534, 1535, 1536]
    assert depth(orc, g["pos"][0][1100]) == (1100, 1639)
    assert depth(orc, g["pos"][1][0]) == (1533, 1533)        # 1534 atoms with the seed
    assert depth(orc, g["pos"][2][0]) == (1534, 1534)        # 1535 atoms with the seed
    assert depth(orc, g["pos"][2][0], D.FWD) == (1534, 1534)
    assert depth(orc, g["pos"][3][0]) == (1535, 1535) and depth(orc, g["pos"][3][700]) == (835, 1535)


@pytest.mark.parametrize("arity,n", [(3, 400), (3, 401), (4, 100), (5, 42)])
def test_path_arity(arity, n):
    g = D.path(n, arity)
    check_form(g)
    orc = oracle(g)
    deepest = -(-(n - 1) // (arity - 1))
    assert depth(orc, 0) == (deepest, n - 1)
    assert depth(orc, 0, D.FWD) == (deepest, n - 1)


@pytest.mark.parametrize("n", [200, 400, 401])
def test_band_depths(n):
    g = D.band(n)
    check_form(g)
    orc = oracle(g)
    half = -(-(n - 1) // 2)
    assert depth(orc, 0) == (half, n - 1)
    assert depth(orc, n // 2)[0] == -(-max(n // 2, n - 1 - n // 2) // 2)
    assert depth(orc, 0, D.FWD) == (half, n - 1)
    assert depth(orc, n - 1, D.FWD) == (0, 0)
    assert depth(orc, 0, D.BACK) == (half, n - 1)        # reversed iteration: "preceding" = later targets, last first
    assert depth(orc, n - 1, D.BACK) == (0, 0)
    if n == 400:
        assert [half, depth(orc, 200)[0]] == [200, 100]


@pytest.mark.parametrize("permuted", [False, True])
def test_band_with_hubs(permuted):
    n = 400
    g = D.band(n, hubs=2, rng=np.random.default_rng(5) if permuted else None)
    check_form(g)
    assert g["num_atoms"] < 6000
    pos, orc = g["pos"], oracle(g)
    if permuted:
        assert not np.array_equal(pos, np.arange(n)) and sorted(np.concatenate([pos, g["hub"], *g["pendants"]])) == \
            list(range(g["n_nodes"]))
    deg = np.bincount(g["tgt_idx"], minlength=g["num_atoms"])
    assert deg[g["hub"]].tolist() == [D.PENDANTS + 1] * 2 and deg[g["hub"]].min() > 512      # heavy atoms
    reach = n - 1 + 2 * (1 + D.PENDANTS)
    # the far hub is one level behind the band's end, its pendants two
    assert depth(orc, pos[0]) == (202, reach)
    assert depth(orc, pos[0], D.FWD) == (202, reach)     # (end, hub) links: both hubs lie behind their band end
    assert depth(orc, pos[n - 1], D.FWD) == (2, 1 + D.PENDANTS)
    assert depth(orc, pos[200]) == (102, reach)
    l, a, d, _ = orc.bfs(int(pos[100]), -1)
    assert int(d[a == g["hub"][0]][0]) == -(-(n - 1 - 100) // 2) + 1      # the end hub near level (n - 1 - p) / 2
    assert int(d[a == g["hub"][1]][0]) == 51
    # a typed traversal of key 0 keeps the deep chain and the hubs (a third of their pendants); keys 1, 2 are shallow
    assert depth(orc, pos[0], D.SYM, 0) == (202, n - 1 + 2 * (1 + len(range(0, D.PENDANTS, 3))))
    assert depth(orc, pos[0], D.SYM, 1) == (0, 0)
    assert depth(orc, g["hub"][0], D.SYM, 1) == (1, len(range(1, D.PENDANTS, 3)))
    assert depth(orc, g["hub"][0], D.SYM, 2) == (1, len(range(2, D.PENDANTS, 3)))
    assert depth(orc, g["pendants"][0][0])[0] == 204          # pendant -> hub -> band -> hub -> pendants
    assert depth(orc, g["link_atom"][0]) == (0, 0)            # a link atom has no incidence here


@pytest.mark.parametrize("levels,width", [(750, 3), (1100, 2), (1023, 3), (1024, 3), (1025, 3), (5, 1)])
def test_ladder_depths(levels, width):
    g = D.ladder(levels, width)
    check_form(g)
    orc = oracle(g)
    l, a, d, _ = orc.bfs(0, -1, algen(-1, *D.FWD))
    assert int(d.max()) == levels and len(a) == D.ladder_pairs(levels, width)
    assert np.bincount(d)[1:].tolist() == [min(width, k + 1) for k in range(1, levels + 1)]
    if width == 3:
        assert len(a) > 2046                   # more pairs than the order-exact workgroup engine holds
    assert depth(orc, levels * width, D.FWD) == (0, 0)       # the last layer yields nothing
    assert depth(orc, 0) == (levels, g["n_nodes"] - 1)     # symmetric: every atom, the other columns of layer 0 at distance 2
    if levels in (1023, 1024):     # the loop leaves the forward traversal as it is and gives the last layer a yield
        gl = D.ladder(levels, width, loop=True)
        check_form(gl)
        ol = oracle(gl)
        l2, a2, d2, _ = ol.bfs(0, -1, algen(-1, *D.FWD))
        assert np.array_equal(a2, a) and np.array_equal(d2, d) and np.array_equal(l2, l)
        assert [x[1] for x in ol.generate(levels * width + 1, algen(-1, *D.FWD))] == [0]


def test_bfs_many_agrees_with_bfs_on_a_band_with_hubs():
    g = D.band(400, hubs=2, rng=np.random.default_rng(6))
    orc = oracle(g)
    rng = np.random.default_rng(7)
    seeds = np.concatenate([rng.integers(0, g["num_atoms"], 60), g["hub"], g["pendants"][1][:2], g["pos"][[0, 399]],
                            g["link_atom"][:2]]).astype(np.int32)
    for mode, lt, maxd in ((D.SYM, -1, -1), (D.SYM, -1, 64), (D.FWD, -1, -1), (D.BACK, -1, -1), (D.SYM, 0, -1)):
        counts, trav = orc.bfs_many(seeds, maxd, 210, algen(lt, *mode))
        for i, s in enumerate(seeds):
            _, a, d, tr = orc.bfs(int(s), maxd, algen(lt, *mode))
            exp = np.zeros(210, np.int64)
            exp[0] = 1
            if len(d):
                exp[:int(d.max()) + 1] += np.bincount(d, minlength=int(d.max()) + 1)
            assert counts[i].tolist() == exp.tolist(), (mode, lt, maxd, i, s)
            assert trav[i] == tr, (mode, lt, maxd, i, s)
        if maxd == 64:
            assert counts[:, 65:].sum() == 0 and counts[:, 64].sum() > 0
