"""CPU tests of the hg.not layer: to_dnf keeps a Not as a leaf (ExpressionBasedQuery.java:94-167, Not.java:46-57),
the host lowering (negation normal form + terms, include/hgx_not.h) evaluated in Python equals the brute-force
evaluator of tests/not_ref.py, the raw-satisfies truth tables, the encoding, and libhgx.so exports the
hgx_not.h boundary.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dnf_ref as D
import kat_graphs as K
import not_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lowered_result(pg, tree):
    """The result through to_dnf + normalize_clause + lower_not, evaluated in Python: the union over the
    clauses of the oracle-style positive result filtered by "no negated tree holds"."""
    from hypergraphdb_amd import to_dnf
    from hypergraphdb_amd.query import normalize_clause, terms_hold
    out = set()
    for cl in to_dnf(tree):
        norm, negs = normalize_clause(cl)
        for l in D.clause_result(pg, norm):
            t, tg = pg.links[l]
            if not any(terms_hold(terms, tg, t) for terms in negs):
                out.add(l)
    return sorted(out)


def test_to_dnf_with_not_leaves():
    from hypergraphdb_amd import And, Not, Or, hg, to_dnf
    a, b, c, d = (hg.incident(i) for i in range(4))
    na, nb = hg.not_(a), hg.not_(hg.or_(b, c))
    assert isinstance(na, Not) and na.negated is a
    # a Not is an opaque leaf: no De Morgan step, the Or inside it is not distributed
    got = to_dnf(hg.and_(a, nb))
    assert len(got) == 1 and list(got[0]) == [a, nb]
    # distribution over an Or next to it; the Not goes into every clause
    got = to_dnf(hg.and_(hg.or_(a, b), na, hg.or_(c, d)))
    assert [frozenset(cl) for cl in got] == [frozenset([x, na, y]) for x in (a, b) for y in (c, d)]
    # dedupe inside a clause and of clauses; equality is structural and order-sensitive
    got = to_dnf(hg.and_(a, hg.not_(hg.or_(b, c)), nb, hg.not_(hg.or_(c, b))))
    assert list(got[0]) == [a, nb, hg.not_(hg.or_(c, b))]
    got = to_dnf(hg.or_(hg.and_(a, na), hg.and_(hg.not_(hg.incident(0)), a), hg.and_(a, nb)))
    assert [frozenset(cl) for cl in got] == [frozenset([a, na]), frozenset([a, nb])]
    assert hg.not_(hg.and_(a, b)) == hg.not_(hg.and_(a, b)) and hg.not_(hg.and_(a, b)) != hg.not_(hg.and_(b, a))
    assert hg.not_(hg.and_(a, b)) != hg.not_(hg.or_(a, b)) and hg.not_(hg.not_(a)) != a and na != a
    assert hg.not_(hg.not_(a)) == hg.not_(hg.not_(hg.incident(0)))
    assert len({na, hg.not_(hg.incident(0)), nb, hg.not_(hg.or_(b, c)), hg.not_(hg.or_(c, b))}) == 3
    # "empty" is decided by the positive leaves alone
    got = to_dnf(hg.or_(hg.and_(hg.type(1), hg.type(2), a, na), hg.and_(b, hg.not_(hg.type(1)), hg.type(1))))
    assert [frozenset(cl) for cl in got] == [frozenset([b, hg.not_(hg.type(1)), hg.type(1)])]
    # a Not-free tree: exactly the earlier result
    tree = hg.or_(a, hg.and_(b, hg.or_(c, hg.and_(d, hg.or_(a, b)))))
    assert isinstance(to_dnf(tree), Or) and all(isinstance(cl, And) for cl in to_dnf(tree))
    assert [list(cl) for cl in to_dnf(tree)] == [[a], [b, c], [b, d, a], [b, d]]


def test_clause_cap_and_unsupported_inside_not():
    from hypergraphdb_amd import HGXUnsupported, hg, to_dnf
    from hypergraphdb_amd.query import MAX_DNF_CLAUSES, lower_not, normalize, normalize_clause
    a = hg.incident(1)
    twelve = [hg.or_(hg.incident(2 * i), hg.incident(2 * i + 1)) for i in range(12)]
    assert len(to_dnf(hg.and_(*twelve, hg.not_(a)))) == MAX_DNF_CLAUSES == 4096
    with pytest.raises(HGXUnsupported):
        to_dnf(hg.and_(*twelve, hg.or_(hg.incident(100), hg.incident(101)), hg.not_(a)))
    # normalize is what it was: a Not is refused, and so is anything else that is no leaf
    with pytest.raises(HGXUnsupported):
        normalize(hg.and_(a, hg.not_(a)))
    with pytest.raises(HGXUnsupported):
        normalize(hg.not_(a))
    assert normalize(hg.and_(a, hg.type(2))) == {"types": [2], "inc": [1], "pos": [], "patterns": [], "arity": -1}
    # bfs / apply / anything that is not an accelerated leaf inside a Not
    for bad in (hg.bfs(0), hg.apply(lambda x: x, a), "value"):
        with pytest.raises(HGXUnsupported):
            to_dnf(hg.and_(a, hg.not_(hg.or_(a, bad))))
        with pytest.raises(HGXUnsupported):
            lower_not(hg.not_(bad))
    # the term cap: the DNF of the negated tree is exponential like the clauses'
    assert len(lower_not(hg.not_(hg.and_(*twelve)))) == 4096
    with pytest.raises(HGXUnsupported):
        lower_not(hg.not_(hg.and_(*twelve, hg.or_(hg.incident(100), hg.incident(101)))))
    norm, negs = normalize_clause(hg.and_(a, hg.not_(hg.and_(*twelve))))
    assert norm["inc"] == [1] and len(negs) == 1 and len(negs[0]) == 4096
    with pytest.raises(HGXUnsupported):      # the terms of one clause are capped together
        normalize_clause(hg.and_(a, hg.not_(hg.and_(*twelve)), hg.not_(hg.incident(200))))
    # Not(Or) of twelve Ors is one conjunction of 24 negative literals
    terms = lower_not(hg.not_(hg.not_(hg.or_(*twelve))))
    assert len(terms) == 1 and len(terms[0]) == 24 and all(pol is False for _, pol in terms[0])


def test_lowering_shapes():
    from hypergraphdb_amd import hg
    from hypergraphdb_amd.query import lower_not
    a, b, c = hg.incident(1), hg.type(2), hg.arity(3)
    assert lower_not(hg.not_(a)) == [((a, True),)]
    assert lower_not(hg.not_(hg.not_(a))) == [((a, False),)]
    assert lower_not(hg.not_(hg.or_(a, b))) == [((a, True),), ((b, True),)]
    assert lower_not(hg.not_(hg.and_(a, b))) == [((a, True), (b, True))]
    assert lower_not(hg.not_(hg.not_(hg.and_(a, b)))) == [((a, False),), ((b, False),)]
    assert lower_not(hg.not_(hg.and_(a, hg.not_(hg.or_(b, c))))) == [((a, True), (b, False), (c, False))]
    assert lower_not(hg.not_(hg.or_())) == [] and lower_not(hg.not_(hg.and_())) == [()]
    assert lower_not(hg.not_(hg.or_(a, a, hg.and_(a)))) == [((a, True),)]


def test_truth_tables_of_raw_satisfies():
    """Where the raw satisfies differs from the positive path (Queries.java:178-206, LinkCondition.java:101-140)."""
    from hypergraphdb_amd import hg
    from hypergraphdb_amd.query import ANY, raw_satisfies
    g = K.queries_graph()
    pg, n = D.graph_of(g), g["names"]
    t, tg = pg.links[n["linkH"]]
    for pattern, exp in K.ordered_link_truth_table(g):
        assert raw_satisfies(hg.orderedLink(*pattern), tg, t) is exp
        assert N.raw(hg.orderedLink(*pattern), tg, t) is exp
    # an empty orderedLink inside a Not satisfies every link: Not(orderedLink()) rejects everything
    cond = hg.and_(hg.incident(n["n0"]), hg.not_(hg.orderedLink()))
    assert N.evaluate(pg, hg.incident(n["n0"])) and N.evaluate(pg, cond) == lowered_result(pg, cond) == []
    b0, b1 = n["n0"], n["n1"]
    cond = hg.and_(hg.incident(b0), hg.not_(hg.orderedLink(b1, b0)))
    assert N.evaluate(pg, cond) == lowered_result(pg, cond) == sorted([n["valuelink"], n["linkH"]])
    cond = hg.and_(hg.incident(b0), hg.not_(hg.orderedLink(b0, b1)))
    assert N.evaluate(pg, cond) == lowered_result(pg, cond) == []
    # arity(0): no link with a target has it; the queries graph's valuelink has arity 10
    for leaf, exp in ((hg.arity(0), False), (hg.arity(2), True), (hg.arity(10), False)):
        assert raw_satisfies(leaf, tg, t) is exp and N.raw(leaf, tg, t) is exp
    cond = hg.and_(hg.incident(b0), hg.not_(hg.arity(0)))
    assert N.evaluate(pg, cond) == lowered_result(pg, cond) == sorted([n["valuelink"], n["linkH"]])
    # link: positions are counted, so a link repeating a member of the set fails; ANY equals no target
    for targets, leaf, exp in (([5, 6, 7], hg.link(5, 7), True), ([5, 5, 7], hg.link(5, 7), False),
                               ([5, 6, 7], hg.link(5, 5, 7), True), ([5, 6], hg.link(5, 7), False),
                               ([5, 6], hg.link(5, ANY), False), ([5, 6], hg.link(), True),
                               ([5, 5], hg.link(5), False)):
        assert raw_satisfies(leaf, targets, 0) is exp and N.raw(leaf, targets, 0) is exp, (targets, leaf)
    # positioned: as the positive path (the same satisfies)
    for lb, ub, comp, exp in ((0, 0, False, True), (1, 1, False, False), (-2, -2, False, True), (0, 5, False, False),
                              (1, 1, True, True), (0, 0, True, False)):
        leaf = hg.incidentNotAt(b0, lb, ub) if comp else hg.incidentAt(b0, lb, ub)
        assert raw_satisfies(leaf, tg, t) is exp and N.raw(leaf, tg, t) is exp, (lb, ub, comp)


def check_trees(g, trees):
    pg = D.graph_of(g)
    both = 0
    for tree in trees:
        exp = N.evaluate(pg, tree)
        assert lowered_result(pg, tree) == exp, tree
        both += N.has_rejected_and_kept(pg, tree)
    return both


def test_lowering_equals_brute_force_on_the_queries_graph():
    from hypergraphdb_amd import hg
    g = K.queries_graph()
    n = g["names"]
    inc = [hg.incident(n[f"n{i}"]) for i in range(7)]
    T = hg.type(K.T_TESTLINK)
    trees = [hg.and_(inc[2], hg.not_(inc[3])), hg.and_(inc[2], hg.not_(inc[3]), hg.not_(T)),
             hg.and_(inc[2], hg.not_(hg.or_(inc[3], inc[4]))), hg.and_(inc[2], hg.not_(hg.and_(inc[3], T))),
             hg.and_(inc[2], hg.not_(hg.not_(inc[3]))), hg.and_(inc[2], hg.not_(inc[2])),
             hg.and_(hg.incident(n["n10"]), hg.not_(inc[0])),
             hg.or_(hg.and_(inc[2], hg.not_(inc[3])), hg.and_(inc[3], T)),
             hg.or_(hg.and_(inc[2], hg.not_(inc[4])), hg.and_(inc[3], hg.not_(inc[4]))),
             hg.and_(inc[2], hg.not_(hg.link(n["n2"], n["n3"]))), hg.and_(inc[2], hg.not_(hg.arity(3))),
             hg.and_(inc[2], hg.not_(hg.typePlus([K.T_VALUELINK, 77]))),
             hg.and_(inc[2], hg.not_(hg.incidentAt(n["n2"], 0)))]
    assert check_trees(g, trees) >= 4
    rng = np.random.default_rng(31)
    check_trees(g, [N.random_tree(rng, g, n_types=3) for _ in range(200)])


def test_lowering_equals_brute_force_on_a_random_graph():
    from hypergraphdb_amd.query import _has_not
    rng = np.random.default_rng(77)
    g = K.random_graph(rng, 150, 600, max_arity=10)
    trees = [N.random_tree(rng, g) for _ in range(300)]
    assert sum(_has_not(t) for t in trees) >= 250
    assert check_trees(g, trees) >= 75       # the Nots reject some hits and keep others


def test_encoding_round_trip():
    from hypergraphdb_amd import hg
    from hypergraphdb_amd.query import (ANY, NOT_ARITY, NOT_INCIDENT, NOT_LINK, NOT_ORDERED, NOT_POSITIONED, NOT_TYPE,
                                        decode_negations, encode_negations, lower_not)
    negs = [[lower_not(hg.not_(hg.or_(hg.incident(4), hg.not_(hg.and_(hg.type(1), hg.typePlus([3, 2])))))),
             lower_not(hg.not_(hg.and_(hg.orderedLink(7, ANY, 8), hg.link(9, 9, 10), hg.arity(2))))],
            [],
            [lower_not(hg.not_(hg.incidentNotAt(5, -2, 3))), lower_not(hg.not_(hg.or_())), lower_not(hg.not_(hg.and_())),
             lower_not(hg.not_(hg.orderedLink()))]]
    enc = encode_negations(negs)
    neg_off, term_off, lit_off, lit, ops = enc
    assert [a.dtype for a in enc] == [np.int64] * 3 + [np.int32] * 2
    assert neg_off.tolist() == [0, 2, 2, 6] and term_off.tolist() == [0, 3, 4, 5, 5, 6, 7]
    assert lit_off.tolist() == [0, 1, 2, 3, 6, 7, 7, 8] and len(lit) == 4 * 8
    assert decode_negations(*enc) == [
        [[((NOT_INCIDENT, 1, (4,)),), ((NOT_TYPE, 0, (1,)),), ((NOT_TYPE, 0, (2, 3)),)],
         [((NOT_ORDERED, 1, (7, ANY, 8)), (NOT_LINK, 1, (9, 10)), (NOT_ARITY, 1, (2,)))]],
        [],
        [[((NOT_POSITIONED, 1, (5, -2, 3, 1)),)], [], [()], [((NOT_ORDERED, 1, ()),)]]]
    empty = encode_negations([[], []])
    assert empty[0].tolist() == [0, 0, 0] and empty[1].tolist() == [0] and len(empty[3]) == 0


def not_header_symbols():
    src = open(os.path.join(ROOT, "include", "hgx_not.h")).read()
    return sorted(set(re.findall(r"\b(hgx_[a-z_]+)\s*\(", src)))


def test_not_abi_exported_and_bound():
    import hypergraphdb_amd
    from hypergraphdb_amd import _lib
    assert hypergraphdb_amd.Not is hypergraphdb_amd.query.Not
    # the header's comments may name hgx.h / hgx_dnf.h entries
    declared = sorted(set(not_header_symbols()) - set(_lib.EXPORTED) - set(_lib.EXPORTED_DNF))
    assert declared == sorted(_lib.EXPORTED_NOT) and len(declared) == 2
    hgx_h = open(os.path.join(ROOT, "include", "hgx.h")).read()
    assert not any(s in hgx_h for s in declared)          # an extension header: hgx.h does not grow
    out = os.popen(f"nm -D --defined-only {os.path.join(ROOT, 'hypergraphdb_amd', 'libhgx.so')}").read()
    L = _lib.lib()
    for s in declared:
        assert re.search(rf"\sT {s}$", out, re.M), s
        assert getattr(L, s).argtypes is not None, s
    # the kinds of the header are the ones the host lowering writes
    from hypergraphdb_amd import query as Q
    src = open(os.path.join(ROOT, "include", "hgx_not.h")).read()
    kinds = dict(re.findall(r"#define HGX_(NOT_[A-Z]+)\s+(\d+)", src))
    assert {k: int(v) for k, v in kinds.items()} == {k: getattr(Q, k) for k in
                                                      ("NOT_TYPE", "NOT_INCIDENT", "NOT_POSITIONED", "NOT_ORDERED",
                                                       "NOT_LINK", "NOT_ARITY")}


def test_not_null_arguments_without_gpu():
    from hypergraphdb_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    one = np.zeros(2, np.int64)
    nul = (None,) * 10
    prog = (None,) * 5
    assert L.hgx_pattern_batch_dnf_not(None, 0, one.ctypes.data, *nul, *prog, 0, C.byref(h)) == _lib.HGX_E_INVALID
    assert L.hgx_pattern_batch_dnf_not(None, 1, None, *nul, *prog, 0, None) == _lib.HGX_E_INVALID
    assert L.hgx_query_result_not_stats(None, None, None, None, None) == _lib.HGX_E_INVALID
    assert b"null result" in L.hgx_last_error()
