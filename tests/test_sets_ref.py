"""CPU tests of the visited-sets reference (tests/sets_ref.py, include/hgx_sets.h): the selection, the depth range,
the filter and the order, on the reference's own Queries.java graph, against lists written out by hand.  The
per-depth sets come from the frozen oracle.  No GPU compute."""
import numpy as np

import kat_graphs as K
import sets_ref as S
from oracle_ctypes import OracleGraph


def kat():
    """kat_graphs.queries_graph(): n0..n9 = 0..9, valuelink = 10 over all of them, n10 = 11 (no link),
    linkH = 12 = (n0, n1), linkH1 = 13 = (n2, n3, linkH), empty = 14, link5 = 15 = (n4, n5, n6, n2, linkH1)."""
    g = K.queries_graph()
    n = g["names"]
    assert [n[k] for k in ("n0", "n9", "valuelink", "n10", "linkH", "linkH1", "empty", "link5")] == \
        [0, 9, 10, 11, 12, 13, 14, 15] and g["num_atoms"] == 16
    orc = OracleGraph(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"])
    return g, orc


def test_oracle_levels_of_the_kat_graph_by_hand():
    _, orc = kat()
    lv = S.oracle_levels(orc, [0, 11, 12])
    # n0: the value link reaches n1..n9; linkH1 (from n2, n3) reaches linkH, link5 (from n2, n4..n6) reaches linkH1
    assert lv[0] == [[0], [1, 2, 3, 4, 5, 6, 7, 8, 9], [12, 13]]
    assert lv[1] == [[11]]                                       # n10 has no link
    # linkH is a target of linkH1 only: n2, n3; then everything the value link and link5 hold
    assert lv[2] == [[12], [2, 3], [0, 1, 4, 5, 6, 7, 8, 9, 13]]
    assert S.oracle_levels(orc, [0], 1) == [[[0], [1, 2, 3, 4, 5, 6, 7, 8, 9]]]


def test_sets_by_hand():
    _, orc = kat()
    lv = S.oracle_levels(orc, [0, 11, 12])
    off, atoms, deps = S.sets(lv, 0, None, None, True)
    assert off.tolist() == [0, 12, 13, 25] and off.dtype == np.int64 and atoms.dtype == np.int32
    assert atoms.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13] + [11] + [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13]
    assert deps.tolist() == [0] + [1] * 9 + [2, 2] + [0] + [2, 2, 1, 1] + [2] * 6 + [0, 2]
    # the order of the selection is the order of the sets
    off, atoms, deps = S.sets([lv[2], lv[0]], 1, 1)
    assert deps is None and off.tolist() == [0, 2, 11] and atoms.tolist() == [2, 3, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    # [1, inf): without the seeds
    off, atoms, _ = S.sets(lv, 1)
    assert off.tolist() == [0, 11, 11, 22] and atoms[:11].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13]
    assert S.sets(lv, 1, -1)[0].tolist() == [0, 11, 11, 22]      # a negative max_depth is unbounded too


def test_min_depth_zero_where_the_predicate_rejects_the_seed():
    _, orc = kat()
    lv = S.oracle_levels(orc, [0, 11, 12])
    keep = np.ones(16, bool)
    keep[[0, 11, 3]] = False                                     # two of the seeds and one other atom
    off, atoms, deps = S.sets(lv, 0, None, keep, True)
    assert off.tolist() == [0, 10, 10, 20]                       # the set of n10 is empty: its only atom is rejected
    assert atoms.tolist() == [1, 2, 4, 5, 6, 7, 8, 9, 12, 13] + [1, 2, 4, 5, 6, 7, 8, 9, 12, 13]
    # the seed 12 passes and is reported at depth 0; n0 is rejected as a seed and as a reached atom alike
    assert deps.tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 2, 2] + [2, 1, 2, 2, 2, 2, 2, 2, 0, 2]
    assert 0 not in atoms.tolist() and 3 not in atoms.tolist() and 11 not in atoms.tolist()


def test_a_depth_range_that_selects_nothing():
    _, orc = kat()
    lv = S.oracle_levels(orc, [0, 11, 12])
    for rng in ((3, None), (3, 7), (5, 5)):
        off, atoms, deps = S.sets(lv, rng[0], rng[1], None, True)
        assert off.tolist() == [0, 0, 0, 0] and len(atoms) == 0 and len(deps) == 0
    off, atoms, _ = S.sets(lv, 2, 2)
    assert off.tolist() == [0, 2, 2, 11] and atoms.tolist() == [12, 13, 0, 1, 4, 5, 6, 7, 8, 9, 13]
    assert S.sets([], 0)[0].tolist() == [0]                      # an empty selection
    assert S.sets(lv, 0, None, np.zeros(16, bool))[0].tolist() == [0, 0, 0, 0]
