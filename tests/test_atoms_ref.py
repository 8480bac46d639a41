"""The reference model of the atom tests (tests/atoms_ref.py) and the Python lowering for hgx_pattern_batch_atoms
(include/hgx_atoms.h), without a GPU: a hand-written known-answer graph pins every node rule, the model agrees
with not_ref on graphs without nodes of interest, and atom_parts / node_satisfies restate the same rules."""
import numpy as np
import pytest

import atoms_ref as AR
import kat_graphs as K
import not_ref as N
import dnf_ref as D
from hypergraphdb_amd import hg
from hypergraphdb_amd.query import ANY, And, atom_parts, is_type_tree, node_satisfies

P, Q = 5, 6   # type keys of the KAT graph


def kat():
    """n0 n1 n2: nodes of type P, P, Q; e = () and l = (n0, n1) of type P; m = (l, n2) of type Q."""
    b = K.Builder()
    n0, n1, n2 = b.node("n0"), b.node("n1"), b.node("n2")
    e = b.link("e", P)
    l = b.link("l", P, n0, n1)
    m = b.link("m", Q, l, n2)
    g = b.arrays()
    at = np.array([P, P, Q, P, P, Q], np.int32)
    return g, AR.AtomGraph(g, at), g["names"]


def test_kat_every_node_rule():
    g, ag, n = kat()
    ev = lambda c: AR.evaluate(ag, c)   # noqa: E731
    tp = hg.type(P)
    assert ev(tp) == [n["n0"], n["n1"], n["e"], n["l"]]                       # nodes and links of the type
    assert ev(hg.type(Q)) == [n["n2"], n["m"]]
    assert ev(hg.type(7)) == []
    # arity(k) holds on a node iff k == 0 (ArityCondition.java:54-55)
    assert ev(hg.and_(tp, hg.arity(0))) == [n["n0"], n["n1"], n["e"]]
    assert ev(hg.and_(tp, hg.arity(2))) == [n["l"]]
    assert ev(hg.and_(tp, hg.not_(hg.arity(0)))) == [n["l"]]
    assert ev(hg.and_(tp, hg.not_(hg.arity(2)))) == [n["n0"], n["n1"], n["e"]]
    # the leaves that read targets are false on a node: their negations keep it
    assert ev(hg.and_(tp, hg.not_(hg.incident(n["n0"])))) == [n["n0"], n["n1"], n["e"]]
    assert ev(hg.and_(tp, hg.not_(hg.incidentAt(n["n0"], 0)))) == [n["n0"], n["n1"], n["e"]]
    assert ev(hg.and_(tp, hg.not_(hg.incidentNotAt(n["n0"], 1)))) == [n["n0"], n["n1"], n["e"]]
    assert ev(hg.and_(tp, hg.not_(hg.link(n["n1"])))) == [n["n0"], n["n1"], n["e"]]
    assert ev(hg.and_(tp, hg.not_(hg.orderedLink(n["n0"], ANY)))) == [n["n0"], n["n1"], n["e"]]
    # the empty-pattern corner: orderedLink() / link() hold on every LINK (e too), never on a node
    assert ev(hg.and_(tp, hg.not_(hg.orderedLink()))) == [n["n0"], n["n1"]]
    assert ev(hg.and_(tp, hg.not_(hg.link()))) == [n["n0"], n["n1"]]
    assert ev(hg.and_(tp, hg.not_(hg.not_(hg.orderedLink())))) == [n["e"], n["l"]]
    # positive patterns: all-ANY of length m needs arity >= m; an empty one is a NOP
    assert ev(hg.and_(tp, hg.orderedLink(ANY))) == [n["l"]]
    assert ev(hg.and_(tp, hg.orderedLink())) == []
    # an Or of a scanned node type and an anchored clause
    assert ev(hg.or_(hg.type(Q), hg.incident(n["n0"]))) == [n["n2"], n["l"], n["m"]]
    assert ev(hg.typePlus({P, Q, 7})) == list(range(6))


def test_kat_projection_and_predicate():
    g, ag, n = kat()
    inc = hg.incident(n["n2"])                                               # m = (l, n2)
    assert AR.join(ag, [(0, inc)]) == [n["l"]] and AR.join(ag, [(1, inc)]) == [n["n2"]]
    assert AR.join(ag, [(0, hg.type(Q))]) == [n["l"]]                        # the node n2 projects to nothing
    assert AR.join(ag, [(1, inc)], hg.type(Q)) == [n["n2"]] and AR.join(ag, [(1, inc)], hg.type(P)) == []
    assert AR.join(ag, [(1, inc)], [0, 0, 1, 0, 0, 0]) == [n["n2"]]          # a mask predicate
    assert AR.join(ag, [], hg.type(P)) == []                                 # a predicate but no parts
    # the filter equals the type written as a scanned self part
    both = hg.typePlus({P, Q})
    for tree in (hg.type(P), hg.type(Q), hg.not_(hg.type(P))):
        self_part = hg.and_(both, tree) if not isinstance(tree, type(hg.type(P))) else tree
        assert AR.join(ag, [(1, hg.incident(n["n0"]))], tree) == AR.join(ag, [(1, hg.incident(n["n0"])), (None, self_part)])
    st = AR.stats(ag, [[(1, inc)], [(0, hg.type(P)), (1, inc)], []], [hg.type(P), None, hg.type(Q)])
    assert st["atoms"] == {"queries_filtered": 2, "values_tested": 1, "values_rejected": 1}
    assert st["join"] == {"parts": 3, "hits_projected": 1 + 4 + 1, "values_distinct": 1 + 1 + 1, "kept": 0}


def test_model_equals_not_ref_on_links():
    """On the link atoms, with one type per atom equal to the link types, the model is not_ref's evaluator."""
    import sibling_ref as SR
    rng = np.random.default_rng(77)
    g = K.random_graph(rng, 40, 120, max_arity=5, n_types=3)
    pg = D.graph_of(g)
    ag = AR.AtomGraph(g, SR.atom_types(g, rng))
    for _ in range(40):
        t = N.random_tree(rng, g, n_types=3, pg=pg)                          # every clause anchored: no node passes
        assert AR.evaluate(ag, t) == N.evaluate(pg, t)


def test_node_satisfies_and_lowering():
    leaves = [hg.type(P), hg.typePlus({P, Q}), hg.arity(0), hg.arity(1), hg.incident(1), hg.incidentAt(1, 0),
              hg.incidentNotAt(1, 0), hg.orderedLink(), hg.orderedLink(ANY), hg.link(), hg.link(1)]
    for leaf in leaves:
        for t in (P, Q):
            assert node_satisfies(leaf, t) == AR.node_raw(leaf, t), leaf
    assert is_type_tree(hg.and_(hg.type(1), hg.not_(hg.typePlus({2, 3})))) and not is_type_tree(hg.arity(0))
    assert not is_type_tree(hg.and_(hg.type(1), hg.incident(0))) and not is_type_tree(And([]))
    ta = hg.targetAt(None, 1)
    knows = hg.and_(hg.type(Q), hg.orderedLink(3, ANY))
    parts, tree = atom_parts(hg.and_(hg.type(P), hg.apply(ta, knows)))
    assert parts == [(1, knows)] and tree == hg.type(P)
    parts, tree = atom_parts(hg.and_(hg.type(P), hg.not_(hg.type(Q)), hg.incident(2), hg.apply(ta, knows)))
    assert [p for p, _ in parts] == [1, None] and parts[1][1] == hg.incident(2)
    assert tree == And([hg.type(P), hg.not_(hg.type(Q))])
    parts, tree = atom_parts(hg.type(P))                                      # no projection: one plain part
    assert parts == [(None, hg.type(P))] and tree is None
    from hypergraphdb_amd import HGXUnsupported
    with pytest.raises(HGXUnsupported):
        atom_parts(hg.and_(hg.type(P), hg.apply(lambda x: x, knows)))


def test_hand_graph_shape():
    g, at, T = AR.hand_graph()
    ag = AR.AtomGraph(g, at)
    n = g["names"]
    assert AR.type_count(ag) == {10: 1, 11: 63, 12: 64, 13: 65, 14: 129, 16: 78}
    assert all(a not in ag.links for a in range(ag.A) if at[a] in (T["NODE"], T["ONE"], T["PAD"]))
    assert all(a in ag.links for a in range(ag.A) if at[a] == T["LINK"])
    assert ag.links[n["empty"]] == [] and n["inner"] in ag.links[n["outer"]]
    assert g["link_type"][list(g["link_atom"]).index(n["untyped"])] == -1
    lt = g["link_type"]
    assert all(lt[i] in (-1, at[a]) for i, a in enumerate(g["link_atom"]))
