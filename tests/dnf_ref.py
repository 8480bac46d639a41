"""Reference for the DNF tests (no GPU): a brute-force evaluator of an And / Or condition tree, one link
at a time, and a generator of random trees.  The evaluator knows nothing about DNF -- it recurses over
the tree with pyref's predicates -- so it checks to_dnf and the engine independently."""
from __future__ import annotations

import numpy as np

import pyref
from hypergraphdb_amd.algorithms import AtomTypeCondition
from hypergraphdb_amd.query import (ANY, And, ArityCondition, IncidentCondition, LinkCondition, Or,
                                    OrderedLinkCondition, PositionedIncidentCondition, TypePlusCondition, hg)


def graph_of(g) -> pyref.Graph:
    off, tg = g["tgt_off"], g["tgt_idx"]
    links = {int(a): (int(g["link_type"][i]), [int(x) for x in tg[off[i]:off[i + 1]]])
             for i, a in enumerate(g["link_atom"])}
    return pyref.Graph(list(range(int(g["num_atoms"]))), links)


def satisfies(cond, targets, type_) -> bool:
    """Does the link with these targets and this type satisfy the condition tree?"""
    if isinstance(cond, And):
        return all(satisfies(c, targets, type_) for c in cond)
    if isinstance(cond, Or):
        return any(satisfies(c, targets, type_) for c in cond)
    if isinstance(cond, AtomTypeCondition):
        return type_ == cond.type
    if isinstance(cond, TypePlusCondition):
        return type_ in cond.types
    if isinstance(cond, IncidentCondition):
        return cond.target in targets
    if isinstance(cond, LinkCondition):
        return all(t in targets for t in cond.targets if t != ANY)
    if isinstance(cond, PositionedIncidentCondition):
        return pyref.positioned(targets, cond.target, cond.lower, cond.upper, cond.complement)
    if isinstance(cond, OrderedLinkCondition):
        # an empty orderedLink compiles to HGQuery.NOP (QueryMetaData.EMPTY): nothing matches
        return len(cond.targets) > 0 and pyref.ordered_link(targets, cond.targets)
    if isinstance(cond, ArityCondition):
        return len(targets) == cond.arity
    raise TypeError(cond)


def evaluate(pg: pyref.Graph, cond) -> list:
    """The sorted link atoms that satisfy the tree."""
    return sorted(l for l, (t, tg) in pg.links.items() if satisfies(cond, tg, t))


def _anchor_leaf(rng, g, row):
    """A leaf that carries an incidence anchor; half the time drawn from the targets of link row
    ``row`` so that the conditions of one tree overlap."""
    A = g["num_atoms"]
    tg = g["tgt_idx"][g["tgt_off"][row]:g["tgt_off"][row + 1]]

    def atom():
        if len(tg) and rng.random() < 0.6:
            return int(tg[int(rng.integers(0, len(tg)))])
        return int(rng.integers(0, A))

    k = int(rng.integers(0, 5))
    if k == 0:
        return hg.incident(atom())
    if k == 1:
        return hg.link(*[atom() for _ in range(int(rng.integers(1, 3)))])
    if k == 2:
        return hg.incidentAt(atom(), int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
    if k == 3:
        return hg.incidentNotAt(atom(), int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
    pat = [atom() if rng.random() < 0.6 else ANY for _ in range(int(rng.integers(1, 4)))]
    if all(p == ANY for p in pat):
        pat[0] = atom()
    return hg.orderedLink(*pat)


def _extra_leaf(rng, n_types):
    k = int(rng.integers(0, 3))
    if k == 0:
        return hg.type(int(rng.integers(0, n_types)))
    if k == 1:
        return hg.typePlus({int(t) for t in rng.integers(0, n_types, 2)})
    return hg.arity(int(rng.integers(0, 5)))


def random_tree(rng, g, depth=3, n_types=3, row=None):
    """An And / Or tree of depth <= ``depth`` over anchor-bearing leaves; type, typePlus and arity leaves
    appear only as extra children of And nodes, so every DNF clause has an anchor.  No empty orderedLink."""
    if row is None:
        row = int(rng.integers(0, len(g["link_atom"])))
    if depth == 0 or rng.random() < 0.25:
        return _anchor_leaf(rng, g, row)
    kids = [random_tree(rng, g, depth - 1, n_types, row) for _ in range(int(rng.integers(1, 4)))]
    if rng.random() < 0.5:
        return Or(kids)
    kids += [_extra_leaf(rng, n_types) for _ in range(int(rng.integers(0, 3)))]
    return And([kids[i] for i in rng.permutation(len(kids))])


def clause_result(pg: pyref.Graph, norm) -> list:
    """pyref.and_query_ext on one normalised clause dict (normalize())."""
    return pyref.and_query_ext(pg, norm["types"], norm["inc"], norm["pos"], norm["patterns"], norm["arity"])


def union_of_clauses(pg: pyref.Graph, norms) -> list:
    parts = [clause_result(pg, n) for n in norms]
    assert all(p is not None for p in parts), "a clause without an anchor"
    return np.unique(np.array([x for p in parts for x in p], np.int64)).tolist()
