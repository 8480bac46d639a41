"""CPU tests of the sibling predicate layer (include/hgx_sibling.h): the reference of tests/sibling_ref.py against
the frozen oracle and against hand-worked cases of DefaultALGenerator's filter(), the host lowering of a sibling
tree against the direct recursion of sibling_ref.holds, and what stays refused.  No GPU compute."""
import os

import numpy as np
import pytest

import kat_graphs as K
import pyref
import sibling_ref as SR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def pygraph(g):
    links = {}
    for r, la in enumerate(np.asarray(g["link_atom"]).tolist()):
        links[la] = (int(g["link_type"][r]), np.asarray(g["tgt_idx"])[g["tgt_off"][r]:g["tgt_off"][r + 1]].tolist())
    return pyref.Graph(list(range(int(g["num_atoms"]))), links)


def pygen(pg, mode, lt=None):
    P, S, R, RS = mode
    return lambda a: pyref.generate(pg, a, link_type=lt, preceding=P, succeeding=S, reverse=R, source=RS)


def levels_from_seq(seed, seq):
    d = {0: [seed]}
    for _, a, k in seq:
        d.setdefault(k, []).append(a)
    return [sorted(d.get(k, [])) for k in range(max(d) + 1)]


def test_all_true_mask_reproduces_the_frozen_oracle_in_every_mode():
    d = np.load(os.path.join(GOLD, "random_small.npz"))
    gi, modes = 0, set()
    while f"g{gi}_A" in d:
        g = dict(num_atoms=int(d[f"g{gi}_A"][0]), link_atom=d[f"g{gi}_link_atom"], tgt_off=d[f"g{gi}_tgt_off"],
                 tgt_idx=d[f"g{gi}_tgt_idx"], link_type=d[f"g{gi}_link_type"])
        pg = pygraph(g)
        keep = np.ones(g["num_atoms"], bool)
        pos, seq_all = 0, d[f"g{gi}_bfs_seq"].tolist()
        for seed, mi, lt, maxd, n in d[f"g{gi}_bfs_keys"].tolist():
            fgen = SR.filtered(pygen(pg, K.ALGEN_MODES[mi], None if lt < 0 else lt), keep)
            assert SR.levels(fgen, seed, maxd) == levels_from_seq(seed, seq_all[pos:pos + n]), (gi, seed, mi, lt, maxd)
            pos += n
            modes.add(mi)
        gi += 1
    assert gi >= 1 and modes == set(range(len(K.ALGEN_MODES)))


def linkage_plus():
    """kat_graphs.linkage_graph() -- x1 -l1- x2 -l2- x3 -- and one more link in which x1 occurs twice."""
    b = K.Builder()
    x1, x2, x3 = b.node("x1"), b.node("x2"), b.node("x3")
    b.link("l1", K.T_PLAIN, x1, x2)
    b.link("l2", K.T_PLAIN, x2, x3)
    g0 = K.linkage_graph()
    assert b.arrays()["tgt_idx"].tolist() == g0["tgt_idx"].tolist() and b.names == g0["names"]
    b.link("l3", K.T_PLAIN, x3, x1, x1)
    return b.arrays()


def test_hand_worked_linkage_graph():
    g = K.linkage_graph()
    n = g["names"]
    x1, x2, x3, l1, l2 = n["x1"], n["x2"], n["x3"], n["l1"], n["l2"]
    pg = pygraph(g)
    sym = pygen(pg, (True, True, False, False))
    everything = [[x1], [x2], [x3]]
    assert SR.levels(SR.filtered(sym, lambda a: True), x1) == everything
    # a failing seed is expanded: the start atom is never tested
    assert SR.levels(SR.filtered(sym, lambda a: a != x1), x1) == everything
    # ... but no other traversal reaches it
    assert SR.levels(SR.filtered(sym, lambda a: a != x1), x3) == [[x3], [x2]]
    # a failing middle atom cuts what lies behind it: never reached, so never expanded
    assert SR.levels(SR.filtered(sym, lambda a: a != x2), x1) == [[x1]]
    assert SR.levels(SR.filtered(sym, lambda a: a != x2), x3) == [[x3]]
    depth, pred = SR.hop_rule(SR.filtered(sym, lambda a: a != x3), x1)
    assert depth == {x1: 0, x2: 1} and pred == {x2: (x1, l1)}
    dist, dm, _, _ = SR.dijkstra(SR.filtered(sym, lambda a: a != x2), x1, x3)
    assert dist is None and dm == {x1: 0.0}
    dist, dm, _, _ = SR.dijkstra(SR.filtered(sym, lambda a: a != x1), x1, x3, lambda l: 2.5)
    assert dist == 5.0 and SR.rule_r(SR.filtered(sym, lambda a: a != x1), lambda l: 2.5, dm, x1, [x1, x2]) == \
        {x2: (x1, l1), x3: (x2, l2)}
    # returnSource: the focus atom itself goes through the filter
    src = pygen(pg, (True, True, False, True))
    assert src(x1) == [(l1, x1), (l1, x2)]
    assert SR.filtered(src, lambda a: a != x1)(x1) == [(l1, x2)]          # a failing focus
    assert SR.filtered(src, lambda a: a != x2)(x1) == [(l1, x1)]          # a passing focus, its sibling fails
    assert SR.filtered(src, lambda a: a != x3)(x1) == [(l1, x1), (l1, x2)]


def test_hand_worked_repeated_target():
    g = linkage_plus()
    n = g["names"]
    x1, x2, x3, l1, l2, l3 = (n[k] for k in ("x1", "x2", "x3", "l1", "l2", "l3"))
    sym = pygen(pygraph(g), (True, True, False, False))
    assert sym(x3) == [(l2, x2), (l3, x1), (l3, x1)]                     # x1 occurs twice in l3: yielded twice
    assert SR.filtered(sym, lambda a: a != x1)(x3) == [(l2, x2)]         # both occurrences go
    assert SR.filtered(sym, lambda a: a != x2)(x3) == [(l3, x1), (l3, x1)]   # the order of the rest is kept
    assert SR.levels(SR.filtered(sym, lambda a: a != x2), x3) == [[x3], [x1]]
    assert SR.filtered(sym, [True, False, True, True, True, True])(x3) == [(l3, x1), (l3, x1)]   # a mask array


def test_many_levels_equals_levels_start_by_start():
    rng = np.random.default_rng(77)
    g = K.random_graph(rng, 60, 90, n_types=3)
    A = g["num_atoms"]
    pg = pygraph(g)
    keep = rng.random(A) < 0.6
    seeds = np.concatenate([rng.integers(0, A, 69), [3, 3]]).astype(np.int32)       # two words, a repeated start
    assert not keep[seeds].all() and keep[seeds].any()
    for mode in K.ALGEN_MODES:
        for k in (keep, np.ones(A, bool), np.zeros(A, bool)):
            fgen = SR.filtered(pygen(pg, mode), k)
            for maxd in (None, 2):
                many = SR.ManyLevels(fgen, A, seeds, maxd)
                c = many.counts()
                for i, s in enumerate(seeds.tolist()):
                    lv = SR.levels(fgen, s, maxd)
                    got = many.levels(i)
                    assert got[:len(lv)] == lv and not any(got[len(lv):]), (mode, maxd, i)
                    assert c[i, :len(lv)].tolist() == [len(x) for x in lv] and not c[i, len(lv):].any()


def lowered_flags(types, tree):
    from hypergraphdb_amd.algorithms import lower_sibling_predicate
    from hypergraphdb_amd.query import terms_hold
    terms = lower_sibling_predicate(tree)
    return np.array([terms_hold(terms, [], int(t)) for t in types], np.uint8)


def test_lowering_round_trips():
    from hypergraphdb_amd import hg
    from hypergraphdb_amd.algorithms import decode_link_predicate, encode_link_predicate, lower_sibling_predicate
    from hypergraphdb_amd.query import NOT_TYPE
    types = np.arange(6)
    cases = {"not_typeplus": hg.not_(hg.typePlus([1, 3])),
             "or_of_ands": hg.or_(hg.and_(hg.typePlus([0, 1, 2]), hg.not_(hg.type(1))), hg.and_(hg.type(4), hg.typePlus([4, 5]))),
             "empty_or": hg.or_(), "empty_and": hg.and_(),
             "nested": hg.not_(hg.or_(hg.type(0), hg.and_(hg.typePlus([2, 3]), hg.not_(hg.type(3)))))}
    for k, tree in cases.items():
        exp = SR.flags(types, tree)
        assert np.array_equal(lowered_flags(types, tree), exp), k
        lit_off, lit, ops = encode_link_predicate(lower_sibling_predicate(tree))
        dec = decode_link_predicate(lit_off, lit, ops)
        assert all(kind == NOT_TYPE for term in dec for kind, _, _ in term), k
        got = [int(any(all((t in o) == bool(p) for _, p, o in term) for term in dec)) for t in types.tolist()]
        assert got == exp.tolist(), k                                     # the decoded program, evaluated on its own
    assert SR.flags(types, cases["not_typeplus"]).tolist() == [1, 0, 1, 0, 1, 1]
    assert SR.flags(types, cases["or_of_ands"]).tolist() == [1, 0, 1, 0, 1, 0]
    assert lower_sibling_predicate(hg.or_()) == [] and SR.flags(types, hg.or_()).sum() == 0      # keeps nothing
    assert lower_sibling_predicate(hg.and_()) == [()] and SR.flags(types, hg.and_()).sum() == 6   # keeps everything


def test_non_type_leaves_are_refused():
    from hypergraphdb_amd import AtomPredicate, DefaultALGenerator, HGXUnsupported, hg
    from hypergraphdb_amd.algorithms import lower_sibling_predicate
    from hypergraphdb_amd.query import ANY
    for bad in (hg.arity(2), hg.incident(3), hg.incidentAt(3, 0), hg.orderedLink(1, ANY), hg.link(1, 2),
                hg.and_(hg.type(1), hg.not_(hg.arity(2))), hg.or_(hg.typePlus([1, 2]), hg.incident(0)), hg.bfs(3)):
        with pytest.raises(HGXUnsupported):
            lower_sibling_predicate(bad)
        with pytest.raises(HGXUnsupported):
            AtomPredicate(None, bad)                                      # refused before the snapshot is touched
        with pytest.raises(HGXUnsupported):
            DefaultALGenerator(None, None, sibling_predicate=bad).compiled_sibling(None)


def test_generators_keep_refusing_outside_the_new_route():
    from hypergraphdb_amd import DefaultALGenerator, HGXUnsupported, _lib, hg
    for sp in (hg.type(0), lambda a: True):
        gen = DefaultALGenerator(None, None, sibling_predicate=sp)
        with pytest.raises(HGXUnsupported):
            gen.options()
        with pytest.raises(HGXUnsupported):
            gen.compiled(None)
    for mode in K.ALGEN_MODES:                                            # without a sibling predicate: compiled()
        gen = DefaultALGenerator(None, None, None, *mode)
        o, lp, ap, owned = gen.compiled_sibling(None)
        assert lp is None and ap is None and owned == [] and bytes(o) == bytes(gen.options())
        assert o.link_type == _lib.HGX_NO_TYPE
