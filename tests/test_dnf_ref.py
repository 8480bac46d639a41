"""CPU tests of the DNF layer: to_dnf restates ExpressionBasedQuery.toDNF (ExpressionBasedQuery.java:94-167),
the union of its clauses equals a brute-force evaluation of the tree, and libhgx.so exports the
hgx_dnf.h boundary.  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dnf_ref as D
import kat_graphs as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clause_sets(dnf):
    return [frozenset(c) for c in dnf]


def test_to_dnf_nested_or_inside_and_inside_or():
    from hypergraphdb_amd import And, Or, hg, to_dnf
    a, b, c, d, e = (hg.incident(i) for i in range(5))
    got = to_dnf(hg.or_(a, hg.and_(b, hg.or_(c, hg.and_(d, hg.or_(e, a))))))
    assert isinstance(got, Or) and all(isinstance(cl, And) for cl in got)
    assert clause_sets(got) == [frozenset([a]), frozenset([b, c]), frozenset([b, d, e]), frozenset([b, d, a])]
    # a leaf and a plain And are one clause
    assert clause_sets(to_dnf(a)) == [frozenset([a])]
    assert clause_sets(to_dnf(hg.and_(a, hg.and_(b, hg.type(1))))) == [frozenset([a, b, hg.type(1)])]
    # And over two Ors: the full distribution, first operand slowest
    got = to_dnf(hg.and_(hg.or_(a, b), hg.or_(c, d), hg.arity(2)))
    assert clause_sets(got) == [frozenset([x, y, hg.arity(2)]) for x in (a, b) for y in (c, d)]
    assert clause_sets(to_dnf(hg.or_())) == [] and clause_sets(to_dnf(hg.and_(a, hg.or_()))) == []


def test_to_dnf_drops_duplicates_and_empty_clauses():
    from hypergraphdb_amd import hg, to_dnf
    a, b = hg.incident(3), hg.incident(4)
    got = to_dnf(hg.and_(a, hg.incident(3), b, hg.link(7, 8), hg.link(7, 8)))      # duplicate sub-conditions
    assert len(got) == 1 and list(got[0]) == [a, b, hg.link(7, 8)]
    got = to_dnf(hg.or_(hg.and_(a, b), hg.and_(b, a), a, hg.or_(hg.incident(3))))   # duplicate clauses
    assert clause_sets(got) == [frozenset([a, b]), frozenset([a])]
    got = to_dnf(hg.or_(hg.and_(hg.type(1), hg.type(2), a), b))                     # type(1) ^ type(2): Nothing
    assert clause_sets(got) == [frozenset([b])]
    got = to_dnf(hg.and_(hg.or_(hg.type(1), hg.arity(2)), hg.type(2), hg.arity(3), a))
    assert clause_sets(got) == []
    # equality of the leaves to_dnf relies on
    assert hg.orderedLink(1, -1, 2) == hg.orderedLink(1, -1, 2) and hg.orderedLink(1, 2) != hg.link(1, 2)
    assert hg.incidentAt(1, 0, 2) == hg.incidentAt(1, 0, 2) and hg.incidentAt(1, 0, 2) != hg.incidentNotAt(1, 0, 2)
    assert hg.typePlus({1, 2}) == hg.typePlus([2, 1]) and hg.arity(2) != hg.arity(3)
    assert len({hg.arity(2), hg.arity(2), hg.link(1), hg.link(1), hg.typePlus([1]), hg.typePlus([1])}) == 3


def test_to_dnf_unsupported_and_clause_cap():
    from hypergraphdb_amd import HGXUnsupported, hg, to_dnf
    from hypergraphdb_amd.query import MAX_DNF_CLAUSES, normalize
    with pytest.raises(HGXUnsupported):
        to_dnf(hg.or_(hg.incident(1), hg.and_(hg.incident(2), hg.bfs(0))))
    with pytest.raises(HGXUnsupported):
        to_dnf(hg.or_(hg.incident(1), hg.apply(lambda x: x, hg.incident(2))))
    assert MAX_DNF_CLAUSES == 4096
    twelve = [hg.or_(hg.incident(2 * i), hg.incident(2 * i + 1)) for i in range(12)]
    assert len(to_dnf(hg.and_(*twelve))) == 4096                                   # 2^12: at the cap
    with pytest.raises(HGXUnsupported):
        to_dnf(hg.and_(*twelve, hg.or_(hg.incident(100), hg.incident(101))))       # 2^13
    with pytest.raises(HGXUnsupported):
        to_dnf(hg.or_(*[hg.incident(i) for i in range(4097)]))
    # normalize and pattern_batch keep refusing anything that is not an And
    with pytest.raises(HGXUnsupported):
        normalize(hg.or_(hg.incident(1)))
    with pytest.raises(HGXUnsupported):
        normalize(hg.and_(hg.incident(1), hg.or_(hg.incident(2))))


def test_empty_ordered_link_is_nop_inside_an_and():
    """An empty orderedLink makes its And a NOP (QueryMetaData.EMPTY); the other clauses are unaffected."""
    from hypergraphdb_amd import hg, to_dnf
    from hypergraphdb_amd.query import normalize
    g = K.queries_graph()
    pg, n = D.graph_of(g), g["names"]
    cond = hg.or_(hg.and_(hg.incident(n["n0"]), hg.orderedLink()), hg.incident(n["n2"]))
    exp = D.evaluate(pg, cond)
    assert exp == D.evaluate(pg, hg.incident(n["n2"])) and len(exp) > 0
    assert D.union_of_clauses(pg, [normalize(c) for c in to_dnf(cond)]) == exp


def test_random_trees_dnf_union_equals_brute_force():
    from hypergraphdb_amd import to_dnf
    from hypergraphdb_amd.query import normalize
    rng = np.random.default_rng(77)
    g = K.random_graph(rng, 150, 600, max_arity=6)
    pg = D.graph_of(g)
    nonempty = multi = 0
    for i in range(300):
        tree = D.random_tree(rng, g)
        norms = [normalize(c) for c in to_dnf(tree)]
        exp = D.evaluate(pg, tree)
        assert D.union_of_clauses(pg, norms) == exp, tree
        nonempty += len(exp) > 0
        multi += len(norms) > 1
    assert nonempty >= 100 and multi >= 100      # the trees are not trivial


def dnf_header_symbols():
    src = open(os.path.join(ROOT, "include", "hgx_dnf.h")).read()
    return sorted(set(re.findall(r"\b(hgx_[a-z_]+)\s*\(", src)))


def test_dnf_abi_exported_and_bound():
    from hypergraphdb_amd import _lib
    declared = sorted(set(dnf_header_symbols()) - set(_lib.EXPORTED))   # the header's comments may name hgx.h entries
    assert declared == sorted(_lib.EXPORTED_DNF) and len(declared) == 2
    out = os.popen(f"nm -D --defined-only {os.path.join(ROOT, 'hypergraphdb_amd', 'libhgx.so')}").read()
    L = _lib.lib()
    for s in declared:
        assert re.search(rf"\sT {s}$", out, re.M), s
        assert getattr(L, s).argtypes is not None, s


def test_dnf_null_arguments_without_gpu():
    from hypergraphdb_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    one = np.zeros(2, np.int64)
    nul = (None,) * 10
    assert L.hgx_pattern_batch_dnf(None, 1, one.ctypes.data, *nul, C.byref(h)) == _lib.HGX_E_INVALID
    assert b"hgx_pattern_batch_dnf" in L.hgx_last_error()
    assert L.hgx_query_result_union_stats(None, None, None, None, None) == _lib.HGX_E_INVALID
    assert b"hgx_query_result_union_stats" in L.hgx_last_error()
