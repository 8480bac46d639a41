"""Reference for the hg.not tests (no GPU): a brute-force evaluator of an And / Or / Not condition tree, one
link at a time, and a generator of random trees with Not children.

Semantics (C = core/src/java/org/hypergraphdb): toDNF keeps a Not as an opaque leaf
(C/query/cond2qry/ExpressionBasedQuery.java:94-167), AndToQuery.getQuery puts it into the predicate list
(C/query/cond2qry/AndToQuery.java:126-135) and filters the intersection with it (:279-294);
Not.satisfies = !negated.satisfies(graph, candidate) (C/query/Not.java:33-36).  So outside a Not a leaf means
its query translation (dnf_ref.satisfies), inside a Not its raw satisfies() (``raw`` below).  The evaluator
knows nothing of negation normal form, terms or the encoding -- it recurses over the original tree -- so it
checks the lowering and the engine independently."""
from __future__ import annotations

import numpy as np

import dnf_ref as D
import pyref
from hypergraphdb_amd.algorithms import AtomTypeCondition
from hypergraphdb_amd.query import (ANY, And, ArityCondition, IncidentCondition, LinkCondition, Not, Or,
                                    OrderedLinkCondition, PositionedIncidentCondition, TypePlusCondition, hg)


def raw(cond, targets, type_) -> bool:
    """satisfies(graph, link) of the condition classes themselves, on a link with these targets and type."""
    if isinstance(cond, And):                         # C/query/And.java:66-76
        return all(raw(c, targets, type_) for c in cond)
    if isinstance(cond, Or):                          # C/query/Or.java:67-78
        return any(raw(c, targets, type_) for c in cond)
    if isinstance(cond, Not):                         # C/query/Not.java:33-36
        return not raw(cond.negated, targets, type_)
    if isinstance(cond, AtomTypeCondition):           # C/query/AtomTypeCondition.java:121-135
        return type_ == cond.type
    if isinstance(cond, TypePlusCondition):           # C/query/TypePlusCondition.java:63-71
        return any(type_ == t for t in cond.types)
    if isinstance(cond, IncidentCondition):           # C/query/IncidentCondition.java:63-76
        return any(t == cond.target for t in targets)
    if isinstance(cond, LinkCondition):               # C/query/LinkCondition.java:101-140
        # count++ for every POSITION whose target is in the (duplicate-free) target set, then
        # count == targetSet.size(): a link repeating a member fails, ANY equals no target
        target_set = set(cond.targets)
        count = 0
        for t in targets:
            if t in target_set:
                count += 1
        return count == len(target_set)
    if isinstance(cond, PositionedIncidentCondition):   # C/query/PositionedIncidentCondition.java:123-177
        return pyref.positioned(targets, cond.target, cond.lower, cond.upper, cond.complement)
    if isinstance(cond, OrderedLinkCondition):        # C/query/OrderedLinkCondition.java:92-124; [] => true
        return pyref.ordered_link(targets, cond.targets)   # (TC/query/Queries.java:178-206)
    if isinstance(cond, ArityCondition):              # C/query/ArityCondition.java:49-67
        return len(targets) == cond.arity
    raise TypeError(cond)


def satisfies(cond, targets, type_) -> bool:
    """Does the link belong to the result of the query the tree compiles to?"""
    if isinstance(cond, And):
        return all(satisfies(c, targets, type_) for c in cond)
    if isinstance(cond, Or):
        return any(satisfies(c, targets, type_) for c in cond)
    if isinstance(cond, Not):
        return not raw(cond.negated, targets, type_)
    return D.satisfies(cond, targets, type_)


def evaluate(pg: pyref.Graph, cond) -> list:
    """The sorted link atoms of the result."""
    return sorted(l for l, (t, tg) in pg.links.items() if satisfies(cond, tg, t))


def strip_nots(cond):
    """The tree without its Not children (the positive part of every clause)."""
    if isinstance(cond, (And, Or)):
        return type(cond)(strip_nots(c) for c in cond if not isinstance(c, Not))
    return cond


def filter_counts(pg: pyref.Graph, clauses) -> tuple:
    """(hits tested, hits rejected) of the clauses of a DNF (And lists of leaves and Nots): the hits of the
    positive part of every clause holding a Not, and those of them one of its Nots rejects."""
    tested = rejected = 0
    for cl in clauses:
        nots = [c for c in cl if isinstance(c, Not)]
        if not nots:
            continue
        for l, (t, tg) in pg.links.items():
            if satisfies(strip_nots(And(cl)), tg, t):
                tested += 1
                rejected += any(raw(n.negated, tg, t) for n in nots)
    return tested, rejected


def _inner_tree(rng, g, row, depth, n_types):
    """What a Not negates: a tree of depth <= ``depth`` over all seven leaves, nested Nots included."""
    if depth == 0 or rng.random() < 0.35:
        k = rng.random()
        if k < 0.08:
            return hg.orderedLink()
        return D._anchor_leaf(rng, g, row) if k < 0.7 else D._extra_leaf(rng, n_types)
    k = rng.random()
    if k < 0.2:
        return Not(_inner_tree(rng, g, row, depth - 1, n_types))
    kids = [_inner_tree(rng, g, row, depth - 1, n_types) for _ in range(int(rng.integers(1, 4)))]
    return Or(kids) if k < 0.6 else And(kids)


def _add_nots(rng, g, tree, row, n_types, top=True):
    if isinstance(tree, Or):
        return Or(_add_nots(rng, g, c, row, n_types, False) for c in tree)
    if isinstance(tree, And):
        kids = [_add_nots(rng, g, c, row, n_types, False) if isinstance(c, (And, Or)) else c for c in tree]
        kids += [Not(_inner_tree(rng, g, row, int(rng.integers(0, 3)), n_types))
                 for _ in range(int(rng.integers(1 if top else 0, 3)))]
        return And([kids[i] for i in rng.permutation(len(kids))])
    if top or rng.random() < 0.5:   # a leaf with an anchor: And(leaf, Not(...)) keeps it
        return And([tree, Not(_inner_tree(rng, g, row, int(rng.integers(0, 3)), n_types))])
    return tree


def random_tree(rng, g, depth=3, n_types=3, pg=None):
    """dnf_ref.random_tree (of a random depth <= ``depth``) with Not(subtree) children put into And nodes (a
    leaf may become And(leaf, Not)), so every clause of the DNF keeps an incidence anchor.  Most of
    dnf_ref's trees match no link or one, which no filter can split: a positive part is drawn again (8 times
    at most) until it has two hits, and the negated subtrees draw their atoms from the row of one of those
    hits, so that they reject some hits and keep others.  (The hits that steer the generator come from
    dnf_ref.union_of_clauses; what the tests expect comes from ``evaluate`` alone.)"""
    from hypergraphdb_amd.query import normalize, to_dnf
    pg = pg or D.graph_of(g)
    for _ in range(8):
        row = int(rng.integers(0, len(g["link_atom"])))
        pos = D.random_tree(rng, g, int(rng.integers(0, depth + 1)), n_types, row)
        hits = D.union_of_clauses(pg, [normalize(c) for c in to_dnf(pos)])
        if len(hits) >= 2 or rng.random() < 0.1:
            break
    if hits:
        row = int(np.searchsorted(g["link_atom"], hits[int(rng.integers(0, len(hits)))]))
    return _add_nots(rng, g, pos, row, n_types)


def has_rejected_and_kept(pg: pyref.Graph, tree) -> bool:
    """The tree's Nots reject a link its positive part matches, and its result is not empty."""
    res = set(evaluate(pg, tree))
    return bool(res) and bool(set(evaluate(pg, strip_nots(tree))) - res)
