"""Reference side of the type-scan tests (no GPU): random trees whose DNF has clauses without an incidence
anchor, and the counts the scan statistics must equal.

What the tests expect comes from not_ref.evaluate -- a brute-force pass over every link that knows nothing of
anchors, DNF or scans, so it answers a tree without an anchor like any other (the reference: AndToQuery.getQuery,
C/query/cond2qry/AndToQuery.java:120-294, scans indexByType.find(T) and filters it with the other conditions;
the snapshots of the tests hold link types only, so the link atoms of a type are all its instances).  The
helpers below only classify clauses (anchored or scanned) and count with that evaluator."""
from __future__ import annotations

import numpy as np

import not_ref as N
from hypergraphdb_amd.algorithms import AtomTypeCondition
from hypergraphdb_amd.query import (ANY, And, ArityCondition, IncidentCondition, LinkCondition, Not, Or,
                                    OrderedLinkCondition, PositionedIncidentCondition, TypePlusCondition, hg, to_dnf)


def is_anchor(leaf) -> bool:
    """The leaf gives its clause an incidence anchor (ExpressionBasedQuery.expand adds incident(x) for every
    non-ANY target of an orderedLink / link, ExpressionBasedQuery.java:730-746)."""
    if isinstance(leaf, (IncidentCondition, PositionedIncidentCondition)):
        return True
    if isinstance(leaf, (OrderedLinkCondition, LinkCondition)):
        return any(t != ANY for t in leaf.targets)
    return False


def clause_types(clause):
    """The type keys every positive type leaf of the clause allows (None: no type leaf)."""
    ts = None
    for c in clause:
        if isinstance(c, AtomTypeCondition):
            ts = {c.type} if ts is None else ts & {c.type}
        elif isinstance(c, TypePlusCondition):
            ts = set(c.types) if ts is None else ts & set(c.types)
    return ts


def is_scanned(clause) -> bool:
    return not any(is_anchor(c) for c in clause if not isinstance(c, Not))


def is_nop(clause) -> bool:
    return any(isinstance(c, OrderedLinkCondition) and not c.targets for c in clause)


def _scan_leaf(rng, n_types):
    """A bare leaf that anchors nothing: arity, an all-ANY orderedLink, a type, a typePlus."""
    k = int(rng.integers(0, 5))
    if k == 0:
        return hg.arity(int(rng.integers(0, 13)))
    if k == 1:
        return hg.orderedLink(*[ANY] * int(rng.integers(1, 11)))
    if k == 2:
        return hg.type(int(rng.integers(0, n_types)))
    if k == 3:
        return hg.typePlus({int(t) for t in rng.integers(0, n_types + 1, 2)})   # (n_types: an absent key)
    return hg.orderedLink(*[ANY] * int(rng.integers(1, 4)))


def random_tree(rng, g, n_types=3, pg=None, p_scan=0.45):
    """not_ref.random_tree with the anchors dropped from some clauses: the tree's DNF (to_dnf: an Or of Ands
    over leaves and Nots, the Nots kept as they are), where a clause is rewritten with probability ``p_scan``
    -- its anchor leaves go, a type or typePlus leaf comes in when it has none, and bare arity / all-ANY
    orderedLink leaves are added to some.  Every clause keeps an anchor or a type, as the engine asks; a clause
    whose types contradict each other is dropped by to_dnf like any "empty" one."""
    tree = N.random_tree(rng, g, n_types=n_types, pg=pg)
    out = []
    for cl in to_dnf(tree):
        cl = list(cl)
        if rng.random() < p_scan:
            cl = [c for c in cl if isinstance(c, Not) or not is_anchor(c)]
            if clause_types(cl) is None:
                cl.append(hg.type(int(rng.integers(0, n_types))) if rng.random() < 0.7 else
                          hg.typePlus({int(t) for t in rng.integers(0, n_types + 1, 2)}))
            cl += [_scan_leaf(rng, n_types) for _ in range(int(rng.integers(0, 2)))]
            if rng.random() < 0.05:
                cl.append(hg.orderedLink())   # a NOP clause
            cl = [cl[i] for i in rng.permutation(len(cl))]
        out.append(And(cl))
    return Or(out)


def clause_results(pg, tree):
    """[(clause, scanned?, its own result by the brute-force evaluator)] of the tree's DNF"""
    return [(cl, is_scanned(cl), N.evaluate(pg, And(cl))) for cl in to_dnf(tree)]


def properties(pg, tree):
    """(a scanned clause has a non-empty result, a scanned clause's Nots reject some rows of its positive part
    and keep others, an id is shared by a scanned and an anchored clause) -- by the evaluator alone"""
    cr = clause_results(pg, tree)
    nonempty = any(s and r for _, s, r in cr)
    split = any(s and r and set(N.evaluate(pg, N.strip_nots(And(cl)))) - set(r) for cl, s, r in cr)
    sc = set(x for _, s, r in cr if s for x in r)
    an = set(x for _, s, r in cr if not s for x in r)
    return nonempty, bool(split), bool(sc & an)


def scan_counts(pg, type_count, trees):
    """(clauses_scanned, rows_scanned, rows_kept) of a batch of trees: an anchor-free clause counts once per
    type key it allows (it is split into one clause per type); a clause that is no NOP covers every link of
    its type; the rows kept are its result.  ``type_count``: {type key: links of it}."""
    clauses = rows = kept = 0
    for t in trees:
        for cl, scanned, res in clause_results(pg, t):
            if not scanned:
                continue
            ts = clause_types(cl)
            clauses += len(ts)
            if not is_nop(cl):
                rows += sum(type_count.get(k, 0) for k in ts)
                kept += len(res)
    return clauses, rows, kept


def anchored_filter_counts(pg, trees):
    """(hits tested, hits rejected) of the filter stage: anchored clauses only"""
    tested = rejected = 0
    for t in trees:
        a, b = N.filter_counts(pg, [cl for cl in to_dnf(t) if not is_scanned(cl)])
        tested, rejected = tested + a, rejected + b
    return tested, rejected


def type_count(g):
    keys, cnt = np.unique(g["link_type"], return_counts=True)
    return {int(k): int(c) for k, c in zip(keys, cnt)}
