"""CPU tests of the link predicate layer (include/hgx_linkpred.h): the host lowering of a predicate tree (its
disjunctive normal form over the literals of hgx_not.h, without an outer Not) evaluated in Python equals the
direct recursion of tests/linkpred_ref.py on every link, the encoding round-trips, the generators that carry no
tree keep their old options, what is not accelerated is still refused, and libhgx.so exports the boundary.  No GPU
compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kat_graphs as K
import linkpred_ref as LP
import not_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lowered_flags(g, tree):
    from hypergraphdb_amd.algorithms import lower_link_predicate
    from hypergraphdb_amd.query import terms_hold
    terms = lower_link_predicate(tree)
    off, tg, ty = g["tgt_off"], g["tgt_idx"], LP.link_types(g)
    return np.array([terms_hold(terms, tg[off[r]:off[r + 1]].tolist(), int(ty[r])) for r in range(len(ty))], np.uint8)


def kinds_and_polarities(trees):
    from hypergraphdb_amd.algorithms import lower_link_predicate
    from hypergraphdb_amd.query import _literal
    return {(_literal(leaf)[0], bool(pol)) for t in trees for term in lower_link_predicate(t) for leaf, pol in term}


def test_lowering_equals_direct_recursion_on_random_trees():
    rng = np.random.default_rng(4242)
    g = K.random_graph(rng, 120, 400, max_arity=10, n_types=3)
    M = len(g["link_atom"])
    trees = [N._inner_tree(rng, g, int(rng.integers(0, M)), int(rng.integers(0, 4)), 3) for _ in range(300)]
    mixed = 0
    for tree in trees:
        exp = LP.flags(g, tree)
        assert np.array_equal(lowered_flags(g, tree), exp), tree
        mixed += 0 < exp.sum() < M
    assert mixed >= 100                                         # predicates that accept some links and reject others
    assert kinds_and_polarities(trees) == {(k, p) for k in range(1, 7) for p in (False, True)}


def test_lowering_shapes_and_encoding_round_trip():
    from hypergraphdb_amd import hg
    from hypergraphdb_amd.algorithms import decode_link_predicate, encode_link_predicate, lower_link_predicate
    from hypergraphdb_amd.query import ANY, NOT_ARITY, NOT_INCIDENT, NOT_LINK, NOT_ORDERED, NOT_POSITIONED, NOT_TYPE
    assert lower_link_predicate(hg.or_()) == [] and lower_link_predicate(hg.and_()) == [()]
    assert lower_link_predicate(hg.not_(hg.and_())) == [] and lower_link_predicate(hg.not_(hg.or_())) == [()]
    tree = hg.or_(hg.and_(hg.type(2), hg.not_(hg.incident(4))), hg.not_(hg.or_(hg.typePlus([3, 1]), hg.arity(2))),
                  hg.and_(hg.orderedLink(7, ANY, 8), hg.link(9, 9, 10), hg.incidentNotAt(5, -2, 3)))
    enc = encode_link_predicate(lower_link_predicate(tree))
    lit_off, lit, ops = enc
    assert [a.dtype for a in enc] == [np.int64, np.int32, np.int32]
    assert lit_off.tolist() == [0, 2, 4, 7] and len(lit) == 4 * 7
    assert decode_link_predicate(*enc) == [
        [(NOT_TYPE, 1, (2,)), (NOT_INCIDENT, 0, (4,))],
        [(NOT_TYPE, 0, (1, 3)), (NOT_ARITY, 0, (2,))],
        [(NOT_ORDERED, 1, (7, ANY, 8)), (NOT_LINK, 1, (9, 10)), (NOT_POSITIONED, 1, (5, -2, 3, 1))]]
    for t, exp in ((hg.or_(), [0]), (hg.and_(), [0, 0])):
        lo, li, op = encode_link_predicate(lower_link_predicate(t))
        assert lo.tolist() == exp and len(li) == 0 and len(op) == 0


def test_generators_without_a_tree_keep_their_options():
    from hypergraphdb_amd import AtomTypeCondition, DefaultALGenerator, _lib
    for mode in K.ALGEN_MODES:
        for lp, lt in ((None, _lib.HGX_NO_TYPE), (AtomTypeCondition(5), 5)):
            gen = DefaultALGenerator(None, lp, None, *mode)
            o = gen.options()
            assert (o.link_type, o.return_preceding, o.return_succeeding, o.reverse_order, o.return_source) == \
                   (lt, *map(int, mode))
            o2, pred, owned = gen.compiled(None)               # no predicate object, nothing to compile
            assert pred is None and owned is False
            assert bytes(o2) == bytes(o)


def test_unaccelerated_predicates_are_still_refused():
    from hypergraphdb_amd import DefaultALGenerator, HGXUnsupported, LinkPredicate, hg
    from hypergraphdb_amd.algorithms import lower_link_predicate
    tree = hg.or_(hg.type(1), hg.arity(2))
    with pytest.raises(HGXUnsupported):
        DefaultALGenerator(None, tree).options()               # options() carries a type key only
    with pytest.raises(HGXUnsupported):
        DefaultALGenerator(None, tree, sibling_predicate=hg.type(0)).compiled(None)
    with pytest.raises(HGXUnsupported):
        DefaultALGenerator(None, None, sibling_predicate=hg.type(0)).compiled(None)
    for bad in (hg.bfs(3), hg.and_(hg.type(1), hg.bfs(3)), hg.not_(hg.or_(hg.arity(2), hg.bfs(3))),
                hg.apply(lambda x: x, hg.type(1))):
        with pytest.raises(HGXUnsupported):
            lower_link_predicate(bad)
        with pytest.raises(HGXUnsupported):
            LinkPredicate(None, bad)                           # refused before the snapshot is touched


def linkpred_header_symbols():
    src = open(os.path.join(ROOT, "include", "hgx_linkpred.h")).read()
    return sorted(set(re.findall(r"\b(hgx_[a-z_]+)\s*\(", src)))


def test_linkpred_abi_exported_and_bound():
    import hypergraphdb_amd
    from hypergraphdb_amd import _lib
    assert hypergraphdb_amd.LinkPredicate is hypergraphdb_amd.algorithms.LinkPredicate
    assert hypergraphdb_amd.classics.LinkPredicate is hypergraphdb_amd.LinkPredicate      # next to LinkWeights
    declared = linkpred_header_symbols()
    assert declared == sorted(_lib.EXPORTED_LINKPRED) and len(declared) == 7
    hgx_h = open(os.path.join(ROOT, "include", "hgx.h")).read()
    assert not any(re.search(rf"\b{s}\b", hgx_h) for s in declared)    # an extension header: hgx.h does not grow
    out = os.popen(f"nm -D --defined-only {os.path.join(ROOT, 'hypergraphdb_amd', 'libhgx.so')}").read()
    L = _lib.lib()
    for s in declared:
        assert re.search(rf"\sT {s}$", out, re.M), s
        assert getattr(L, s).argtypes is not None, s


def test_linkpred_null_arguments_without_gpu():
    from hypergraphdb_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.hgx_link_predicate_create(None, 0, None, None, None, 0, C.byref(h)) == _lib.HGX_E_INVALID
    assert L.hgx_link_predicate_info(None, None, None, None, None) == _lib.HGX_E_INVALID
    assert b"null predicate" in L.hgx_last_error()
    assert L.hgx_link_predicate_flags(None, 0, 0, None) == _lib.HGX_E_INVALID
    L.hgx_link_predicate_free(None)
    seeds = np.zeros(1, np.int32)
    assert L.hgx_bfs_batch_pred(None, seeds.ctypes.data, 1, 1, None, None, C.byref(h)) == _lib.HGX_E_INVALID
    assert L.hgx_bfs_sequence_pred(None, seeds.ctypes.data, 1, 1, None, None, C.byref(h)) == _lib.HGX_E_INVALID
    assert L.hgx_shortest_paths_pred(None, seeds.ctypes.data, seeds.ctypes.data, 1, None, None, None,
                                     C.byref(h)) == _lib.HGX_E_INVALID
