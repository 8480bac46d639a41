"""Reference for the link predicate tests (no GPU): a condition tree evaluated on one link by direct recursion
over And / Or / Not (C/query/And.java:66-76, Or.java:67-78, Not.java:33-36) down to the leaves' raw satisfies
(query.raw_satisfies).  It knows nothing of negation normal form, terms or the encoding, so it checks the
lowering and the engine independently.

DefaultALGenerator.generate() calls linkPredicate.satisfies(graph, link) once per incident link and nowhere else
(C/algorithms/DefaultALGenerator.java:300-308).  So a traversal of ``g`` under the predicate ``tree`` is, by
construction, the traversal of ``flagged(g, tree)`` -- the same graph with link_type = the predicate's flags --
under AtomTypeCondition(1): the frozen oracle run on the flagged graph with algen(link_type=1) is the expected
output of every predicate traversal."""
from __future__ import annotations

import numpy as np

from hypergraphdb_amd.query import And, Not, Or, raw_satisfies


def holds(tree, targets, type_) -> bool:
    if isinstance(tree, And):
        return all(holds(c, targets, type_) for c in tree)
    if isinstance(tree, Or):
        return any(holds(c, targets, type_) for c in tree)
    if isinstance(tree, Not):
        return not holds(tree.negated, targets, type_)
    return bool(raw_satisfies(tree, targets, type_))


def link_types(g) -> np.ndarray:
    lt = g.get("link_type")
    return np.zeros(len(g["link_atom"]), np.int32) if lt is None else np.asarray(lt, np.int32)


def flags(g, tree) -> np.ndarray:
    """uint8[M]: 1 where link row r satisfies the tree."""
    off, tg, ty = np.asarray(g["tgt_off"]), np.asarray(g["tgt_idx"]), link_types(g)
    return np.array([holds(tree, tg[off[r]:off[r + 1]].tolist(), int(ty[r])) for r in range(len(ty))], np.uint8)


def flagged(g, tree, f=None) -> dict:
    """A copy of the graph dict with link_type = the tree's flags (``f``: flags already computed)."""
    out = dict(g)
    out["link_type"] = (flags(g, tree) if f is None else f).astype(np.int32)
    return out
