"""GPU-backed And-condition evaluation behind the reference's query API.

Reference (C = core/src/java/org/hypergraphdb):
  * HGQuery.hg DSL: hg.and / hg.type / hg.incident / hg.orderedLink / hg.anyHandle /
    hg.bfs / hg.subsumed / hg.subsumes / hg.apply(hg.targetAt)   (C/HGQuery.java:364-1823)
  * ConditionToQuery (C/query/cond2qry/ConditionToQuery.java:14-18) registered per graph with
    HGQueryConfiguration.addCompiler (C/query/HGQueryConfiguration.java:48) -- consulted before
    ToQueryMap by QueryCompile.translator (C/query/QueryCompile.java:80-87).
  * ExpressionBasedQuery.expand (C/query/cond2qry/ExpressionBasedQuery.java:689-737) flattening
    nested And and adding incident(x) for every non-ANY orderedLink target.
  * SubsumedCondition / SubsumesCondition -> BFS over HGSubsumes links
    (C/query/cond2qry/ToQueryMap.java:282-370).
  * hg.or: ExpressionBasedQuery.toDNF (ExpressionBasedQuery.java:94-167) turns any And / Or tree into an Or
    of Ands; OrToQuery (C/query/cond2qry/OrToQuery.java:14-43) chains UnionResults
    (C/query/impl/UnionResult.java).  Here: to_dnf + pattern_batch_dnf (one device call, include/hgx_dnf.h).
  * hg.not: toDNF keeps a Not as an opaque leaf, AndToQuery.getQuery (C/query/cond2qry/AndToQuery.java:126-135,
    :279-294) filters the clause's intersection with Not.satisfies (C/query/Not.java:33-36).  Here:
    normalize_clause + lower_not + encode_negations, run by hgx_pattern_batch_dnf_not (include/hgx_not.h).
  * A clause without an incidence anchor: AndToQuery.getQuery (AndToQuery.java:120-294) scans indexByType.find(T)
    and filters the scan with the remaining conditions.  Here, opt-in only: pattern_batch_dnf(..., type_scan=True)
    / GpuScanToQuery split such a clause into one clause per type (split_type_scan) and run the batch through
    hgx_pattern_batch_dnf_scan (include/hgx_scan.h), which scans the device type index.  THE SNAPSHOT KNOWS THE
    TYPES OF LINK ATOMS ONLY: a scanned clause delivers the LINK atoms of the type that pass its predicates;
    indexByType.find(T) also returns node atoms of type T.  The two agree whenever T has no node instances --
    the caller opts in knowing that, and nothing routes a clause to the scan by default.
  * hg.apply(hg.targetAt(graph, i), cond): ToQueryMap compiles a MapCondition to a ResultMapQuery over cond's
    query (C/query/cond2qry/ToQueryMap.java:409-427) whose mapping ends in LinkProjectionMapping.eval =
    link.getTargetAt(i) (C/query/impl/LinkProjectionMapping.java:33-36); the And of two such conditions is the
    reference's pattern test (testcore PatternTests.java:20-61).  Here: join_parts + pattern_batch_join, one
    device call through hgx_pattern_batch_join (include/hgx_join.h) -- the sorted SET of the projected atoms (the
    reference delivers duplicates in the inner order), a link too short for i contributing nothing (the
    reference's getTargetAt throws ArrayIndexOutOfBoundsException there).
  * Over every atom (include/hgx_atoms.h): with the atom types set (snapshot.set_atom_types) a clause without an
    anchor scans the ATOM index -- nodes and links of the type, the reference's indexByType.find(T) -- and a
    type tree next to projections, and(type(Person), apply(targetAt(g, 1), ...)), restricts the projected atoms
    through an AtomPredicate.  Here: atom_parts + pattern_batch_atoms; find_all routes the two shapes it
    otherwise refuses there when, and only when, the snapshot has atom types.  A node atom takes the
    reference's satisfies rules (node_satisfies).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import HGXUnsupported, check, lib, ptr
from .algorithms import AtomPredicate, AtomTypeCondition, DefaultALGenerator, HGException, bfs_sequence

ANY = _lib.HGX_ANY_HANDLE


class IncidentCondition:
    def __init__(self, target):
        self.target = int(target)

    def __eq__(self, o):
        return isinstance(o, IncidentCondition) and o.target == self.target

    def __hash__(self):
        return hash(("incident", self.target))

    def __repr__(self):
        return f"incident({self.target})"


class OrderedLinkCondition:
    def __init__(self, *targets):
        if len(targets) == 1 and isinstance(targets[0], (list, tuple)):
            targets = tuple(targets[0])
        self.targets = tuple(int(t) for t in targets)

    def satisfies(self, snapshot, link) -> bool:
        """C/query/OrderedLinkCondition.java:92-124 (host form, used by the API, not the batch path)."""
        if snapshot.row_of(link) < 0:
            return False
        tg = snapshot.targets(link)
        i = j = 0
        while i < len(tg) and j < len(self.targets):
            if self.targets[j] == ANY or self.targets[j] == tg[i]:
                j += 1
            i += 1
        return j == len(self.targets)

    def __eq__(self, o):
        return isinstance(o, OrderedLinkCondition) and o.targets == self.targets

    def __hash__(self):
        return hash(("orderedLink", self.targets))

    def __repr__(self):
        return f"orderedLink{self.targets}"


class LinkCondition:
    """hg.link(targets...): the link's targets include every given target
    (C/query/LinkCondition.java:101-139); expand turns it into incident(target) for every non-ANY
    target and drops it (C/query/cond2qry/ExpressionBasedQuery.java:739-746)."""

    def __init__(self, *targets):
        if len(targets) == 1 and isinstance(targets[0], (list, tuple, set)):
            targets = tuple(targets[0])
        self.targets = tuple(int(t) for t in targets)

    def __eq__(self, o):
        return isinstance(o, LinkCondition) and o.targets == self.targets

    def __hash__(self):
        return hash(("link", self.targets))

    def __repr__(self):
        return f"links{self.targets}"


class PositionedIncidentCondition:
    """hg.incidentAt / hg.incidentNotAt (C/query/PositionedIncidentCondition.java:123-177): the
    target sits at a position in [lower, upper] (negative = from the end), or outside it with
    ``complement``."""

    def __init__(self, target, lower, upper=None, complement=False):
        self.target, self.lower = int(target), int(lower)
        self.upper = self.lower if upper is None else int(upper)
        self.complement = bool(complement)

    def record(self):
        return (self.target, self.lower, self.upper, int(self.complement))

    def __eq__(self, o):
        return isinstance(o, PositionedIncidentCondition) and o.record() == self.record()

    def __hash__(self):
        return hash(("incidentAt",) + self.record())

    def __repr__(self):
        return f"incidentAt({self.target},{self.lower},{self.upper},{self.complement})"


class ArityCondition:
    """hg.arity(k) (C/query/ArityCondition.java:49-67): the link has exactly k targets."""

    def __init__(self, arity):
        self.arity = int(arity)

    def __eq__(self, o):
        return isinstance(o, ArityCondition) and o.arity == self.arity

    def __hash__(self):
        return hash(("arity", self.arity))

    def __repr__(self):
        return f"arity({self.arity})"


class TypePlusCondition:
    """hg.typePlus(base): the atom's type is the base or one of its subtypes
    (C/query/TypePlusCondition.java:26-71); expand turns it into an Or of AtomTypeConditions
    (ExpressionBasedQuery.java:606-627).  Here it carries the resulting set of type keys."""

    def __init__(self, types):
        self.types = frozenset(int(t) for t in types)

    @classmethod
    def from_subsumption(cls, snapshot, base_type_atom, subsumes_type, key_of_atom):
        """The subtypes the way TypePlusCondition.fetchSubTypes finds them: a DefaultALGenerator
        over HGSubsumes links (preceding=False, succeeding=True) from the base -- run as one GPU
        traversal.  ``key_of_atom`` maps a type atom to the type key used in link_type."""
        from .algorithms import bfs_batch
        gen = DefaultALGenerator(snapshot, AtomTypeCondition(subsumes_type), None, False, True, False)
        r = bfs_batch(snapshot, [int(base_type_atom)], None, gen)
        atoms = [int(base_type_atom)] + [int(a) for d in range(1, r.n_levels) for a in r.visited(0, d)]
        r.close()
        return cls(key_of_atom[a] for a in atoms if a in key_of_atom)

    def __eq__(self, o):
        return isinstance(o, TypePlusCondition) and o.types == self.types

    def __hash__(self):
        return hash(("typePlus", self.types))

    def __repr__(self):
        return f"typePlus{sorted(self.types)}"


class And(list):
    def __repr__(self):
        return "and(" + ", ".join(map(repr, self)) + ")"


class Or(list):
    """hg.or(...) (C/query/Or.java): a link atom matching at least one operand."""

    def __repr__(self):
        return "or(" + ", ".join(map(repr, self)) + ")"


def _tree_key(c):
    """A hashable, order-sensitive key of a condition tree: the reference's And / Or are lists and compare
    element by element (And.java / Or.java extend ArrayList); And and Or never compare equal."""
    if isinstance(c, And):
        return ("and",) + tuple(_tree_key(x) for x in c)
    if isinstance(c, Or):
        return ("or",) + tuple(_tree_key(x) for x in c)
    return c


class Not:
    """hg.not(pred) (C/query/Not.java): satisfies = !negated.satisfies (:33-36); Not(P) == Not(Q) iff P == Q
    (:46-57), structurally and order-sensitively, so toDNF's HashSets dedupe it like any leaf."""

    def __init__(self, negated):
        self.negated = negated

    def __eq__(self, o):
        return isinstance(o, Not) and _tree_key(o.negated) == _tree_key(self.negated)

    def __hash__(self):
        return hash(("not", _tree_key(self.negated)))

    def __repr__(self):
        return f"not({self.negated!r})"


class MapCondition:
    """hg.apply(mapping, cond)"""

    def __init__(self, mapping, cond):
        self.mapping, self.cond = mapping, cond


class TargetAt:
    """hg.targetAt(graph, i): link -> its i-th target."""

    def __init__(self, snapshot, pos):
        self.snapshot, self.pos = snapshot, int(pos)

    def __call__(self, link):
        tg = self.snapshot.targets(link)
        return int(tg[self.pos]) if self.pos < len(tg) else None


class BFSCondition:
    def __init__(self, start, link_predicate=None, return_preceding=True, return_succeeding=True,
                 reverse_order=False, max_distance=None, sibling_predicate=None):
        self.start = int(start)
        self.link_predicate = link_predicate
        self.sibling_predicate = sibling_predicate   # not accelerated here: find_all raises HGXUnsupported
        self.flags = (return_preceding, return_succeeding, reverse_order)
        self.max_distance = max_distance


class hg:
    """The subset of HGQuery.hg on the accelerated path."""

    @staticmethod
    def type(t):
        return AtomTypeCondition(t)

    @staticmethod
    def incident(h):
        return IncidentCondition(h)

    @staticmethod
    def orderedLink(*targets):
        return OrderedLinkCondition(*targets)

    @staticmethod
    def anyHandle():
        return ANY

    @staticmethod
    def link(*targets):
        return LinkCondition(*targets)

    @staticmethod
    def incidentAt(target, lower, upper=None):
        return PositionedIncidentCondition(target, lower, upper, False)

    @staticmethod
    def incidentNotAt(target, lower, upper=None):
        return PositionedIncidentCondition(target, lower, upper, True)

    @staticmethod
    def arity(k):
        return ArityCondition(k)

    @staticmethod
    def typePlus(types):
        return types if isinstance(types, TypePlusCondition) else TypePlusCondition(types)

    @staticmethod
    def and_(*conds):
        return And(conds)

    @staticmethod
    def or_(*conds):
        return Or(conds)

    @staticmethod
    def not_(pred):
        return Not(pred)

    @staticmethod
    def bfs(start, link_predicate=None, return_preceding=True, return_succeeding=True, reverse_order=False,
            sibling_predicate=None):
        return BFSCondition(start, link_predicate, return_preceding, return_succeeding, reverse_order,
                            sibling_predicate=sibling_predicate)

    @staticmethod
    def subsumed(general, subsumes_type):
        """descendants: BFS(G) over HGSubsumes links, preceding=False, succeeding=True (ToQueryMap.java:340-370)"""
        return BFSCondition(general, AtomTypeCondition(subsumes_type), False, True, False)

    @staticmethod
    def subsumes(specific, subsumes_type):
        """ancestors: the same with reverseOrder=True (ToQueryMap.java:282-312)"""
        return BFSCondition(specific, AtomTypeCondition(subsumes_type), False, True, True)

    @staticmethod
    def apply(mapping, cond):
        return MapCondition(mapping, cond)

    @staticmethod
    def targetAt(snapshot, pos):
        return TargetAt(snapshot, pos)


def _flatten(cond, out):
    if isinstance(cond, And):
        for c in cond:
            _flatten(c, out)
    else:
        out.append(cond)
    return out


_LEAVES = (AtomTypeCondition, TypePlusCondition, IncidentCondition, LinkCondition, PositionedIncidentCondition,
           OrderedLinkCondition, ArityCondition)


def normalize(cond):
    """The accelerated And shapes after ExpressionBasedQuery.expand + toDNF, as a dict
    {types (sorted list, [] = no type condition), inc, pos [(target, lb, ub, complement)],
    patterns [tuple], arity (-1 = none)} -- or "empty" when the conjunction can match nothing
    (two different exact types, two different arities).  Any other shape raises HGXUnsupported
    (a Java shim delegates those to AndToQuery)."""
    if isinstance(cond, _LEAVES):
        cond = And([cond])
    if not isinstance(cond, And):
        raise HGXUnsupported(_lib.HGX_E_UNSUPPORTED, f"not an And: {cond!r}")
    subs = _flatten(cond, [])
    if not all(isinstance(c, _LEAVES) for c in subs):
        raise HGXUnsupported(_lib.HGX_E_UNSUPPORTED, f"shape not accelerated: {cond!r}")
    tset = None
    for c in subs:   # every type condition must hold: intersect their type sets
        if isinstance(c, AtomTypeCondition):
            tset = {c.type} if tset is None else tset & {c.type}
        elif isinstance(c, TypePlusCondition):
            tset = set(c.types) if tset is None else tset & set(c.types)
    arities = {c.arity for c in subs if isinstance(c, ArityCondition)}
    if (tset is not None and not tset) or len(arities) > 1:
        return "empty"
    inc = [c.target for c in subs if isinstance(c, IncidentCondition)]
    for c in subs:
        if isinstance(c, LinkCondition):
            inc.extend(t for t in c.targets if t != ANY)
    return {"types": sorted(tset) if tset is not None else [], "inc": inc,
            "pos": [c.record() for c in subs if isinstance(c, PositionedIncidentCondition)],
            "patterns": [c.targets for c in subs if isinstance(c, OrderedLinkCondition)],
            "arity": arities.pop() if arities else -1}


def _from_tuple(q):
    """legacy (type, incident, pattern-or-None) -> the normalised dict"""
    t, inc, pat = q
    return {"types": [] if t is None or t < 0 else [int(t)], "inc": list(inc), "pos": [],
            "patterns": [] if pat is None else [tuple(pat)], "arity": -1}


MAX_DNF_CLAUSES = 4096


def to_dnf(cond) -> "Or":
    """ExpressionBasedQuery.toDNF (ExpressionBasedQuery.java:94-167) + the part of simplify that matters
    here: the condition as an Or of Ands of leaf conditions.  Nested And / Or are flattened (:106-111,
    :144-149), And is distributed over Or (:112-125), a sub-condition repeated inside a clause and a clause
    repeated inside the Or are dropped (the HashSets of :100 and :138).  A clause that normalize() reports
    as "empty" (it can match nothing) is dropped, as simplify removes Nothing from an Or.  A clause holding
    anything but the accelerated leaves raises HGXUnsupported, and so do more than MAX_DNF_CLAUSES clauses
    (the distribution is exponential; the caller falls back to the CPU's OrToQuery).
    A Not over a tree of the accelerated leaves is a leaf too: toDNF does not look inside it (no De Morgan
    step), distributes and dedupes it like the others (Not.java:46-57); whether a clause is "empty" is
    decided by its positive leaves alone."""
    def cap(clauses):
        if len(clauses) > MAX_DNF_CLAUSES:
            raise HGXUnsupported(_lib.HGX_E_UNSUPPORTED, f"more than {MAX_DNF_CLAUSES} clauses in the DNF of {cond!r}")
        return clauses

    def dedupe(clauses):
        seen, out = set(), []
        for c in clauses:
            k = frozenset(c)
            if k not in seen:
                seen.add(k)
                out.append(c)
        return out

    def dnf(c):   # -> list of clauses, a clause = tuple of distinct leaves in first-seen order
        if isinstance(c, And):
            acc = [()]
            for sub in c:
                acc = cap(dedupe([a + tuple(x for x in b if x not in a) for a in acc for b in dnf(sub)]))
            return acc
        if isinstance(c, Or):
            acc = []
            for sub in c:
                acc = cap(dedupe(acc + dnf(sub)))
            return acc
        if isinstance(c, Not):
            _nnf(c.negated, True)   # raises HGXUnsupported on anything but And / Or / Not over the leaves
        elif not isinstance(c, _LEAVES):
            raise HGXUnsupported(_lib.HGX_E_UNSUPPORTED, f"shape not accelerated: {c!r}")
        return [(c,)]

    return Or(And(cl) for cl in dnf(cond)
              if normalize(And([x for x in cl if not isinstance(x, Not)])) != "empty")


# --- hg.not: the negations of a clause, lowered on the host (include/hgx_not.h) ---------------------------

NOT_TYPE, NOT_INCIDENT, NOT_POSITIONED, NOT_ORDERED, NOT_LINK, NOT_ARITY = 1, 2, 3, 4, 5, 6


def _nnf(p, pol):
    """Negation normal form of ``p`` (``pol`` False: of its negation): nested Nots become the polarity of
    the literals -- ("lit", leaf, polarity) under ("and", [...]) / ("or", [...])."""
    if isinstance(p, Not):
        return _nnf(p.negated, not pol)
    if isinstance(p, (And, Or)):
        conj = isinstance(p, And) == pol   # De Morgan: a negated And is an Or of the negated operands
        return ("and" if conj else "or", [_nnf(c, pol) for c in p])
    if isinstance(p, _LEAVES):
        return ("lit", p, pol)
    raise HGXUnsupported(_lib.HGX_E_UNSUPPORTED, f"shape not accelerated inside a Not: {p!r}")


def lower_not(neg, max_terms=None):
    """``neg`` = Not(P) -> the terms of P: its negation normal form in disjunctive normal form, a list of
    tuples of (leaf, polarity) literals.  P holds iff every literal of some term does, so Not(P) holds iff
    every term has a failing literal.  No term: P is false (an empty Or); an empty term: P is true (an empty
    And).  More than ``max_terms`` (MAX_DNF_CLAUSES) terms raise HGXUnsupported."""
    limit = MAX_DNF_CLAUSES if max_terms is None else max_terms

    def cap(terms):
        if len(terms) > limit:
            raise HGXUnsupported(_lib.HGX_E_UNSUPPORTED, f"more than {limit} terms in the negations of {neg!r}")
        return terms

    def dedupe(terms):
        seen, out = set(), []
        for t in terms:
            k = frozenset(t)
            if k not in seen:
                seen.add(k)
                out.append(t)
        return out

    def terms(node):
        if node[0] == "lit":
            return [((node[1], node[2]),)]
        if node[0] == "or":
            acc = []
            for sub in node[1]:
                acc = cap(dedupe(acc + terms(sub)))
            return acc
        acc = [()]
        for sub in node[1]:
            acc = cap(dedupe([a + tuple(x for x in b if x not in a) for a in acc for b in terms(sub)]))
        return acc

    return terms(_nnf(neg.negated, True))


def raw_satisfies(leaf, targets, type_) -> bool:
    """The leaf's own satisfies() on a link with these targets and this type key -- what a Not negates, not
    the leaf's query translation (the kinds of include/hgx_not.h; the kernel of hgx_not.hip restates them)."""
    tg = [int(t) for t in targets]
    if isinstance(leaf, AtomTypeCondition):          # AtomTypeCondition.java:121-135
        return type_ == leaf.type
    if isinstance(leaf, TypePlusCondition):          # TypePlusCondition.java:63-71
        return type_ in leaf.types
    if isinstance(leaf, IncidentCondition):          # IncidentCondition.java:63-76
        return leaf.target in tg
    if isinstance(leaf, PositionedIncidentCondition):   # PositionedIncidentCondition.java:123-177
        n, (x, lb, ub, comp) = len(tg), leaf.record()
        ub, lb = (ub + n if ub < 0 else ub), (lb + n if lb < 0 else lb)
        if lb > ub or lb < 0 or ub < 0 or lb >= n or ub >= n:
            return False
        return any(t == x and ((lb <= i <= ub) != bool(comp)) for i, t in enumerate(tg))
    if isinstance(leaf, OrderedLinkCondition):       # OrderedLinkCondition.java:92-124: [] satisfies every link
        j = 0
        for t in tg:
            if j < len(leaf.targets) and leaf.targets[j] in (ANY, t):
                j += 1
        return j == len(leaf.targets)
    if isinstance(leaf, LinkCondition):              # LinkCondition.java:101-140: positions counted, not members
        members = set(leaf.targets)
        return sum(t in members for t in tg) == len(members)
    if isinstance(leaf, ArityCondition):             # ArityCondition.java:49-67
        return len(tg) == leaf.arity
    raise TypeError(leaf)


def terms_hold(terms, targets, type_) -> bool:
    """P of lower_not on one link: some term has every literal holding."""
    return any(all(raw_satisfies(leaf, targets, type_) == pol for leaf, pol in term) for term in terms)


def _literal(leaf):
    """(kind, operands) of include/hgx_not.h"""
    if isinstance(leaf, AtomTypeCondition):
        return NOT_TYPE, [leaf.type]
    if isinstance(leaf, TypePlusCondition):
        return NOT_TYPE, sorted(leaf.types)
    if isinstance(leaf, IncidentCondition):
        return NOT_INCIDENT, [leaf.target]
    if isinstance(leaf, PositionedIncidentCondition):
        return NOT_POSITIONED, list(leaf.record())
    if isinstance(leaf, OrderedLinkCondition):
        return NOT_ORDERED, list(leaf.targets)
    if isinstance(leaf, LinkCondition):
        return NOT_LINK, list(dict.fromkeys(leaf.targets))   # the reference's target set: each member once
    return NOT_ARITY, [leaf.arity]


def normalize_clause(clause):
    """One clause of to_dnf -> (normalize(And(its positive leaves)), [lower_not(n) for its Nots]).  The
    terms of one clause are capped together at MAX_DNF_CLAUSES (HGXUnsupported beyond)."""
    leaves = _flatten(clause if isinstance(clause, And) else And([clause]), [])
    negs = [lower_not(c) for c in leaves if isinstance(c, Not)]
    if sum(len(t) for t in negs) > MAX_DNF_CLAUSES:
        raise HGXUnsupported(_lib.HGX_E_UNSUPPORTED, f"more than {MAX_DNF_CLAUSES} terms in the negations of {clause!r}")
    return normalize(And([c for c in leaves if not isinstance(c, Not)])), negs


def encode_negations(clause_negs):
    """[per clause: [per negation: terms of lower_not]] -> (neg_off, term_off, lit_off, lit, ops) of
    hgx_pattern_batch_dnf_not."""
    neg_off, term_off, lit_off, lit, ops = [0], [0], [0], [], []
    for negs in clause_negs:
        for terms in negs:
            for term in terms:
                for leaf, pol in term:
                    kind, operands = _literal(leaf)
                    lit.extend((kind, int(bool(pol)), len(ops), len(ops) + len(operands)))
                    ops.extend(operands)
                lit_off.append(len(lit) // 4)
            term_off.append(len(lit_off) - 1)
        neg_off.append(len(term_off) - 1)
    return (np.array(neg_off, np.int64), np.array(term_off, np.int64), np.array(lit_off, np.int64),
            np.array(lit, np.int32), np.array(ops, np.int32))


def decode_negations(neg_off, term_off, lit_off, lit, ops):
    """The inverse of encode_negations up to the leaf classes: literals come back as
    (kind, polarity, operand tuple)."""
    return [[[tuple((int(lit[4 * l]), int(lit[4 * l + 1]), tuple(int(x) for x in ops[lit[4 * l + 2]:lit[4 * l + 3]]))
                    for l in range(lit_off[t], lit_off[t + 1]))
              for t in range(term_off[g], term_off[g + 1])]
             for g in range(neg_off[c], neg_off[c + 1])]
            for c in range(len(neg_off) - 1)]


class QueryResult:
    def __init__(self, offsets, ids, ms=None, union=None, negation=None, scan=None, join=None, atoms=None):
        self.offsets, self.ids, self.ms = offsets, ids, ms
        # pattern_batch_atoms: {"queries_filtered", "values_tested", "values_rejected", "ms_filter", "bytes_filter"}
        # (hgx_query_result_atoms_stats; all zero on any other result)
        self.atoms = atoms
        # pattern_batch_join: {"parts", "hits_projected", "values_distinct", "kept", "ms_join", "bytes_join"}
        # (hgx_query_result_join_stats; all zero on a pattern_batch_dnf result)
        self.join = join
        # pattern_batch_dnf(type_scan=True): {"clauses_scanned", "rows_scanned", "rows_kept", "ms_scan",
        # "bytes_scan"} (hgx_query_result_scan_stats)
        self.scan = scan
        # pattern_batch_dnf: {"clause_hits", "kept", "ms_union", "bytes_union"} (hgx_query_result_union_stats)
        self.union = union
        # ... {"hits_tested", "hits_rejected", "ms_not", "bytes_not"} (hgx_query_result_not_stats)
        self.negation = negation

    def __len__(self):
        return len(self.offsets) - 1

    def __getitem__(self, q):
        return self.ids[self.offsets[q]:self.offsets[q + 1]]


def _read_result(h, n) -> QueryResult:
    try:
        off = np.empty(n + 1, np.int64)
        check(lib().hgx_query_result_offsets(h, ptr(off)))
        ids = np.empty(max(int(off[-1]), 1), np.int32)
        check(lib().hgx_query_result_ids(h, ptr(ids)))
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(lib().hgx_query_result_ms(h, C.byref(a), C.byref(b), C.byref(c)))
    finally:
        lib().hgx_query_result_free(h)
    return QueryResult(off, ids[: int(off[-1])], {"ms_total": a.value, "ms_match": b.value, "bytes_match": c.value})


class QuerySet:
    """A packed batch resident in device memory (hgx_query_set_create): uploaded once, run many times
    (``run(snapshot)``) without moving the queries again -- a fixed set of compiled queries re-executed
    by an application (TC/query/QueryCompilation.java:76-122)."""

    def __init__(self, snapshot, q_type, inc_off, inc, has_ordered, pat_off, pat):
        self._h = None
        arrs = [np.ascontiguousarray(q_type, np.int32), np.ascontiguousarray(inc_off, np.int64),
                np.ascontiguousarray(inc, np.int32), np.ascontiguousarray(has_ordered, np.int32),
                np.ascontiguousarray(pat_off, np.int64), np.ascontiguousarray(pat, np.int32)]
        self.n = len(arrs[0])
        h = C.c_void_p()
        check(lib().hgx_query_set_create(snapshot.handle, self.n, *(a.ctypes.data for a in arrs), C.byref(h)))
        self._h = h

    def run(self, snapshot) -> QueryResult:
        """hgx_pattern_batch_set on ``snapshot`` (or an execution context of it)."""
        h = C.c_void_p()
        check(lib().hgx_pattern_batch_set(snapshot.handle, self._h, C.byref(h)))
        return _read_result(h, self.n)

    def run_into(self, snapshot, offsets: np.ndarray, ids: np.ndarray, timing: np.ndarray | None = None) -> int:
        """hgx_pattern_batch_set_into: the results into caller arrays (``offsets``: int64[n + 1],
        ``ids``: int32); returns the number of hits.  ``ids`` holds them only when that number fits
        (``offsets`` is always filled, so a caller can size ``ids`` and run again).  ``timing``
        (float64[3], optional): device ms of the batch, ms and algorithmic bytes of the match kernel."""
        if timing is not None and (timing.dtype != np.float64 or timing.size < 3 or not timing.flags.c_contiguous):
            raise ValueError("timing must be a contiguous float64 array of 3 entries")
        if offsets.dtype != np.int64 or offsets.size < self.n + 1 or not offsets.flags.c_contiguous:
            raise ValueError(f"offsets must be a contiguous int64 array of at least {self.n + 1} entries")
        if ids.dtype != np.int32 or not ids.flags.c_contiguous:
            raise ValueError("ids must be a contiguous int32 array")
        n_ids = C.c_int64()
        check(lib().hgx_pattern_batch_set_into(snapshot.handle, self._h, offsets.ctypes.data, ids.ctypes.data,
                                               ids.size, C.byref(n_ids),
                                               None if timing is None else timing.ctypes.data))
        return n_ids.value

    def close(self):
        if self._h is not None:
            lib().hgx_query_set_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pattern_batch_arrays(snapshot, q_type, inc_off, inc, has_ordered, pat_off, pat) -> QueryResult:
    """Packed batch (hgx_pattern_batch_packed): query q = And(type(q_type[q]),
    incident(inc[inc_off[q]:inc_off[q+1]]...), orderedLink(pat[pat_off[q]:pat_off[q+1]]) if has_ordered[q])."""
    n = len(q_type)
    arrs = [np.ascontiguousarray(q_type, np.int32), np.ascontiguousarray(inc_off, np.int64),
            np.ascontiguousarray(inc, np.int32), np.ascontiguousarray(has_ordered, np.int32),
            np.ascontiguousarray(pat_off, np.int64), np.ascontiguousarray(pat, np.int32)]
    h = C.c_void_p()
    check(lib().hgx_pattern_batch_packed(snapshot.handle, n, *(a.ctypes.data for a in arrs), C.byref(h)))
    return _read_result(h, n)


def pattern_batch_ext_arrays(snapshot, type_off, types, inc_off, inc, pos_off, pos, pset_off, pat_off, pat,
                             arity) -> QueryResult:
    """Flat batch for hgx_pattern_batch_ext (see include/hgx.h)."""
    n = len(arity)
    arrs = [np.ascontiguousarray(type_off, np.int64), np.ascontiguousarray(types, np.int32),
            np.ascontiguousarray(inc_off, np.int64), np.ascontiguousarray(inc, np.int32),
            np.ascontiguousarray(pos_off, np.int64), np.ascontiguousarray(pos, np.int32),
            np.ascontiguousarray(pset_off, np.int64), np.ascontiguousarray(pat_off, np.int64),
            np.ascontiguousarray(pat, np.int32), np.ascontiguousarray(arity, np.int32)]
    h = C.c_void_p()
    check(lib().hgx_pattern_batch_ext(snapshot.handle, n, *(a.ctypes.data for a in arrs), C.byref(h)))
    try:
        off = np.zeros(n + 1, np.int64)
        check(lib().hgx_query_result_offsets(h, ptr(off)))
        ids = np.zeros(max(int(off[-1]), 1), np.int32)
        check(lib().hgx_query_result_ids(h, ptr(ids)))
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(lib().hgx_query_result_ms(h, C.byref(a), C.byref(b), C.byref(c)))
    finally:
        lib().hgx_query_result_free(h)
    return QueryResult(off, ids[: int(off[-1])], {"ms_total": a.value, "ms_match": b.value, "bytes_match": c.value})


def _ext_arrays(norm):
    """normalised dicts (or "empty") -> the flat arrays of hgx_pattern_batch_ext, in its argument order"""
    n = len(norm)
    type_off, inc_off, pos_off, pset_off = (np.zeros(n + 1, np.int64) for _ in range(4))
    types, inc, pos, pat, pat_off = [], [], [], [], [0]
    arity = np.full(n, -1, np.int32)
    for i, q in enumerate(norm):
        if q == "empty":   # nothing can match: run a NOP (an empty orderedLink) on a valid anchor
            q = {"types": [], "inc": [0], "pos": [], "patterns": [()], "arity": -1}
        types.extend(q["types"])
        type_off[i + 1] = len(types)
        inc.extend(q["inc"])
        inc_off[i + 1] = len(inc)
        for rec in q["pos"]:
            pos.extend(rec)
        pos_off[i + 1] = len(pos) // 4
        for p in q["patterns"]:
            pat.extend(p)
            pat_off.append(len(pat))
        pset_off[i + 1] = len(pat_off) - 1
        arity[i] = q["arity"]
    return (type_off, np.array(types or [0], np.int32), inc_off, np.array(inc or [0], np.int32), pos_off,
            np.array(pos or [0], np.int32), pset_off, np.array(pat_off, np.int64), np.array(pat or [0], np.int32),
            arity)


def pattern_batch_dnf_arrays(snapshot, clause_off, type_off, types, inc_off, inc, pos_off, pos, pset_off, pat_off,
                             pat, arity) -> QueryResult:
    """Flat DNF batch for hgx_pattern_batch_dnf (include/hgx_dnf.h): query q = Or over the clauses
    [clause_off[q], clause_off[q+1]) of the hgx_pattern_batch_ext arrays."""
    clause_off = np.ascontiguousarray(clause_off, np.int64)
    n = len(clause_off) - 1
    arrs = [np.ascontiguousarray(type_off, np.int64), np.ascontiguousarray(types, np.int32),
            np.ascontiguousarray(inc_off, np.int64), np.ascontiguousarray(inc, np.int32),
            np.ascontiguousarray(pos_off, np.int64), np.ascontiguousarray(pos, np.int32),
            np.ascontiguousarray(pset_off, np.int64), np.ascontiguousarray(pat_off, np.int64),
            np.ascontiguousarray(pat, np.int32), np.ascontiguousarray(arity, np.int32)]
    h = C.c_void_p()
    check(lib().hgx_pattern_batch_dnf(snapshot.handle, n, clause_off.ctypes.data, *(a.ctypes.data for a in arrs),
                                      C.byref(h)))
    return _read_dnf_result(h, n)


def _read_dnf_result(h, n, scan=False, atoms=False) -> QueryResult:
    qf, vt, vr, ms_f, by_f = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
    rc5 = lib().hgx_query_result_atoms_stats(h, C.byref(qf), C.byref(vt), C.byref(vr), C.byref(ms_f),
                                             C.byref(by_f)) if atoms else _lib.HGX_OK
    ch, kept, ms_u, by_u = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
    rc = lib().hgx_query_result_union_stats(h, C.byref(ch), C.byref(kept), C.byref(ms_u), C.byref(by_u))
    te, rj, ms_n, by_n = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
    rc2 = lib().hgx_query_result_not_stats(h, C.byref(te), C.byref(rj), C.byref(ms_n), C.byref(by_n))
    cs, rs, rk, ms_s, by_s = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
    rc3 = lib().hgx_query_result_scan_stats(h, C.byref(cs), C.byref(rs), C.byref(rk), C.byref(ms_s),
                                            C.byref(by_s)) if scan else _lib.HGX_OK
    pa, hp, vd, jk, ms_j, by_j = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
    rc4 = lib().hgx_query_result_join_stats(h, C.byref(pa), C.byref(hp), C.byref(vd), C.byref(jk), C.byref(ms_j),
                                            C.byref(by_j))
    r = _read_result(h, n)   # frees the result
    check(rc)
    check(rc2)
    check(rc3)
    check(rc4)
    check(rc5)
    if atoms:
        r.atoms = {"queries_filtered": qf.value, "values_tested": vt.value, "values_rejected": vr.value,
                   "ms_filter": ms_f.value, "bytes_filter": by_f.value}
    r.join = {"parts": pa.value, "hits_projected": hp.value, "values_distinct": vd.value, "kept": jk.value,
              "ms_join": ms_j.value, "bytes_join": by_j.value}
    if scan:
        r.scan = {"clauses_scanned": cs.value, "rows_scanned": rs.value, "rows_kept": rk.value, "ms_scan": ms_s.value,
                  "bytes_scan": by_s.value}
    r.union = {"clause_hits": ch.value, "kept": kept.value, "ms_union": ms_u.value, "bytes_union": by_u.value}
    r.negation = {"hits_tested": te.value, "hits_rejected": rj.value, "ms_not": ms_n.value, "bytes_not": by_n.value}
    return r


def pattern_batch_dnf_not_arrays(snapshot, clause_off, type_off, types, inc_off, inc, pos_off, pos, pset_off, pat_off,
                                 pat, arity, neg_off, term_off, lit_off, lit, ops) -> QueryResult:
    """Flat DNF batch with negations for hgx_pattern_batch_dnf_not (include/hgx_not.h): the arrays of
    pattern_batch_dnf_arrays, then the negation program of encode_negations (all five None: no program)."""
    clause_off = np.ascontiguousarray(clause_off, np.int64)
    n = len(clause_off) - 1
    if neg_off is None:
        neg_off = term_off = lit_off = np.zeros(0, np.int64)
        lit = ops = np.zeros(0, np.int32)
    arrs = [np.ascontiguousarray(type_off, np.int64), np.ascontiguousarray(types, np.int32),
            np.ascontiguousarray(inc_off, np.int64), np.ascontiguousarray(inc, np.int32),
            np.ascontiguousarray(pos_off, np.int64), np.ascontiguousarray(pos, np.int32),
            np.ascontiguousarray(pset_off, np.int64), np.ascontiguousarray(pat_off, np.int64),
            np.ascontiguousarray(pat, np.int32), np.ascontiguousarray(arity, np.int32),
            np.ascontiguousarray(neg_off, np.int64), np.ascontiguousarray(term_off, np.int64),
            np.ascontiguousarray(lit_off, np.int64), np.ascontiguousarray(lit, np.int32),
            np.ascontiguousarray(ops, np.int32)]
    h = C.c_void_p()
    check(lib().hgx_pattern_batch_dnf_not(snapshot.handle, n, clause_off.ctypes.data,
                                          *(a.ctypes.data if a.size else None for a in arrs), len(arrs[-1]),
                                          C.byref(h)))
    return _read_dnf_result(h, n)


def pattern_batch_dnf_scan_arrays(snapshot, clause_off, type_off, types, inc_off, inc, pos_off, pos, pset_off, pat_off,
                                  pat, arity, neg_off=None, term_off=None, lit_off=None, lit=None,
                                  ops=None) -> QueryResult:
    """Flat DNF batch for hgx_pattern_batch_dnf_scan (include/hgx_scan.h): the arrays of
    pattern_batch_dnf_not_arrays; a clause without an incidence anchor and with exactly one type is scanned
    over the type index (its LINK atoms of that type).  ``result.scan`` holds the scan statistics."""
    clause_off = np.ascontiguousarray(clause_off, np.int64)
    n = len(clause_off) - 1
    if neg_off is None:
        neg_off = term_off = lit_off = np.zeros(0, np.int64)
        lit = ops = np.zeros(0, np.int32)
    arrs = [np.ascontiguousarray(type_off, np.int64), np.ascontiguousarray(types, np.int32),
            np.ascontiguousarray(inc_off, np.int64), np.ascontiguousarray(inc, np.int32),
            np.ascontiguousarray(pos_off, np.int64), np.ascontiguousarray(pos, np.int32),
            np.ascontiguousarray(pset_off, np.int64), np.ascontiguousarray(pat_off, np.int64),
            np.ascontiguousarray(pat, np.int32), np.ascontiguousarray(arity, np.int32),
            np.ascontiguousarray(neg_off, np.int64), np.ascontiguousarray(term_off, np.int64),
            np.ascontiguousarray(lit_off, np.int64), np.ascontiguousarray(lit, np.int32),
            np.ascontiguousarray(ops, np.int32)]
    h = C.c_void_p()
    check(lib().hgx_pattern_batch_dnf_scan(snapshot.handle, n, clause_off.ctypes.data,
                                           *(a.ctypes.data if a.size else None for a in arrs), len(arrs[-1]),
                                           C.byref(h)))
    return _read_dnf_result(h, n, scan=True)


def is_anchored(norm) -> bool:
    """A normalised clause has an incidence anchor: an incident target, a positioned target or a non-ANY
    pattern target (ExpressionBasedQuery.expand adds incident(x) for it)."""
    return bool(norm["inc"] or norm["pos"] or any(t != ANY for p in norm["patterns"] for t in p))


def split_type_scan(norm, negs):
    """One normalised clause of normalize_clause -> the clauses hgx_pattern_batch_dnf_scan takes for it.  A
    clause without an anchor and with k >= 1 types becomes k one-type clauses with the negations repeated:
    expand turns a TypePlusCondition into an Or of AtomTypeConditions (ExpressionBasedQuery.java:606-627) and
    toDNF distributes it.  An anchored clause, an "empty" one and a clause with neither anchor nor type (the
    engine refuses that one: nothing to scan) pass through untouched."""
    if norm == "empty" or is_anchored(norm) or len(norm["types"]) <= 1:
        return [(norm, negs)]
    return [(dict(norm, types=[t]), negs) for t in norm["types"]]


def _lower_dnf_query(q, type_scan, norm, negs):
    """One query of pattern_batch_dnf -- a condition, or a list of normalised clauses -- appended to ``norm`` /
    ``negs`` as the clauses the engine takes."""
    for c in (q if type(q) in (list, tuple) else [normalize_clause(c) for c in to_dnf(q)]):
        c, ng = c if type(c) is tuple else (c, [])
        for c1, ng1 in (split_type_scan(c, ng) if type_scan else [(c, ng)]):
            norm.append(c1)
            negs.append([] if c1 == "empty" else ng1)   # (an "empty" clause runs as a NOP: nothing to filter)


# --- hg.apply(hg.targetAt): projections of pattern hits and their intersection (include/hgx_join.h) --------

JOIN_SELF = _lib.HGX_JOIN_SELF


def _same_store(a, b) -> bool:
    """``a`` and ``b`` are one snapshot or execution contexts of one (they share the host mirror)."""
    mirror = getattr(a, "tgt_off", None)
    return a is b or (mirror is not None and mirror is getattr(b, "tgt_off", None))


def _check_part(c, whole):
    if isinstance(c, (MapCondition, BFSCondition)):
        raise HGXUnsupported(_lib.HGX_E_UNSUPPORTED, f"{type(c).__name__} inside a part of {whole!r}")
    if isinstance(c, (And, Or)):
        for x in c:
            _check_part(x, whole)
    elif isinstance(c, Not):
        _check_part(c.negated, whole)


def join_parts(cond, snapshot=None):
    """``cond`` -> the parts [(pos, condition)] of one join query of pattern_batch_join (pos None: the link atom
    itself), or HGXUnsupported.  Accepted: hg.apply(hg.targetAt(graph, i), c), or an And of those and of plain
    sub-conditions; the plain sub-conditions together form one part without a projection.  Refused: a mapping
    that is not a TargetAt (or one with a negative position), TargetAts of different snapshots or of another
    one than ``snapshot``, a MapCondition nested inside a part, a BFSCondition, an Or of maps, and a condition
    without any projection (that one is a plain pattern_batch_dnf query)."""
    subs = [cond] if isinstance(cond, MapCondition) else _flatten(cond, []) if isinstance(cond, And) else None
    if subs is None or not any(isinstance(c, MapCondition) for c in subs):
        raise HGXUnsupported(_lib.HGX_E_UNSUPPORTED, f"not a projection or an And of projections: {cond!r}")
    parts, rest = [], []
    for c in subs:
        if not isinstance(c, MapCondition):
            _check_part(c, cond)
            rest.append(c)
            continue
        m = c.mapping
        if not isinstance(m, TargetAt) or m.pos < 0:
            raise HGXUnsupported(_lib.HGX_E_UNSUPPORTED, f"mapping not accelerated: {m!r}")
        if snapshot is None:
            snapshot = m.snapshot
        if not _same_store(m.snapshot, snapshot):
            raise HGXUnsupported(_lib.HGX_E_UNSUPPORTED, "a targetAt of another snapshot")
        _check_part(c.cond, cond)
        parts.append((m.pos, c.cond))
    if rest:
        parts.append((None, rest[0] if len(rest) == 1 else And(rest)))
    return parts


def pattern_batch_join_arrays(snapshot, part_off, part_pos, clause_off, type_off, types, inc_off, inc, pos_off, pos,
                              pset_off, pat_off, pat, arity, neg_off=None, term_off=None, lit_off=None, lit=None,
                              ops=None, type_scan=False) -> QueryResult:
    """Flat join batch for hgx_pattern_batch_join (include/hgx_join.h): join query j owns the parts
    [part_off[j], part_off[j+1]); part s is query s of the pattern_batch_dnf_scan_arrays arrays that follow,
    projected to target position part_pos[s] (-1: the link atom itself).  ``result.join`` holds the
    statistics."""
    part_off = np.ascontiguousarray(part_off, np.int64)
    part_pos = np.ascontiguousarray(part_pos, np.int32)
    clause_off = np.ascontiguousarray(clause_off, np.int64)
    n = len(part_off) - 1
    if neg_off is None:
        neg_off = term_off = lit_off = np.zeros(0, np.int64)
        lit = ops = np.zeros(0, np.int32)
    arrs = [np.ascontiguousarray(type_off, np.int64), np.ascontiguousarray(types, np.int32),
            np.ascontiguousarray(inc_off, np.int64), np.ascontiguousarray(inc, np.int32),
            np.ascontiguousarray(pos_off, np.int64), np.ascontiguousarray(pos, np.int32),
            np.ascontiguousarray(pset_off, np.int64), np.ascontiguousarray(pat_off, np.int64),
            np.ascontiguousarray(pat, np.int32), np.ascontiguousarray(arity, np.int32),
            np.ascontiguousarray(neg_off, np.int64), np.ascontiguousarray(term_off, np.int64),
            np.ascontiguousarray(lit_off, np.int64), np.ascontiguousarray(lit, np.int32),
            np.ascontiguousarray(ops, np.int32)]
    h = C.c_void_p()
    check(lib().hgx_pattern_batch_join(snapshot.handle, n, part_off.ctypes.data,
                                       part_pos.ctypes.data if part_pos.size else None, clause_off.ctypes.data,
                                       *(a.ctypes.data if a.size else None for a in arrs), len(arrs[-1]),
                                       _lib.HGX_JOIN_TYPE_SCAN if type_scan else 0, C.byref(h)))
    return _read_dnf_result(h, n, scan=True)


def pattern_batch_join(snapshot, queries, type_scan=False) -> QueryResult:
    """From links to the atoms they connect, in one device call: every query is a list of (pos, cond) parts
    (pos None: the link atoms of cond themselves) or a condition join_parts lowers to one --
    hg.apply(hg.targetAt(graph, pos), cond), or an And of those and of plain sub-conditions.  Each part's cond
    (a condition, or a list of normalised clauses as pattern_batch_dnf takes) goes through to_dnf /
    normalize_clause / split_type_scan exactly as in pattern_batch_dnf; its hits are projected to their target at
    ``pos`` -- a link too short for it contributes nothing -- and the values of a query's parts are intersected
    on the device: ascending, each atom once.  A query without parts is empty.  ``type_scan`` as in
    pattern_batch_dnf (opt-in, the same rule).  ``result.join``: {"parts", "hits_projected", "values_distinct",
    "kept", "ms_join", "bytes_join"} (hgx_query_result_join_stats); ``result.union`` / ``negation`` / ``scan``
    describe the parts' evaluation."""
    part_off, part_pos, clause_off, norm, negs = [0], [], [0], [], []
    for q in queries:
        for pos, cond in (q if type(q) in (list, tuple) else join_parts(q, snapshot)):
            if pos is not None and pos < 0:
                raise ValueError(f"bad target position {pos}")
            part_pos.append(JOIN_SELF if pos is None else int(pos))
            _lower_dnf_query(cond, type_scan, norm, negs)
            clause_off.append(len(norm))
        part_off.append(len(part_pos))
    return pattern_batch_join_arrays(snapshot, part_off, part_pos, clause_off, *_ext_arrays(norm),
                                     *(encode_negations(negs) if any(negs) else (None,) * 5), type_scan=type_scan)


# --- the pattern path over every atom: atom-index scans and a predicate on projected atoms (include/hgx_atoms.h) ---

def node_satisfies(leaf, type_) -> bool:
    """The leaf's own satisfies() on a NODE atom of this type key (include/hgx_atoms.h): arity(k) holds iff
    k == 0 (ArityCondition.java:54-55); every leaf that reads targets is false, an empty orderedLink() / link()
    included (OrderedLinkCondition.java:100-101, LinkCondition.java:119-120, PositionedIncidentCondition.java:
    134-135, IncidentCondition.java:71-75) -- raw_satisfies makes those two true on a link without targets, so a
    node is not an arity-0 link."""
    if isinstance(leaf, (AtomTypeCondition, TypePlusCondition)):
        return raw_satisfies(leaf, (), type_)
    if isinstance(leaf, ArityCondition):
        return leaf.arity == 0
    if isinstance(leaf, (IncidentCondition, PositionedIncidentCondition, OrderedLinkCondition, LinkCondition)):
        return False
    raise TypeError(leaf)


def is_type_tree(c) -> bool:
    """``c`` is an And / Or / Not tree over hg.type / hg.typePlus alone: what an AtomPredicate evaluates."""
    if isinstance(c, (And, Or)):
        return len(c) > 0 and all(is_type_tree(x) for x in c)
    if isinstance(c, Not):
        return is_type_tree(c.negated)
    return isinstance(c, (AtomTypeCondition, TypePlusCondition))


def atom_parts(cond, snapshot=None):
    """``cond`` -> (parts, tree) of one query of pattern_batch_atoms: the parts [(pos, condition)] as join_parts
    makes them, and the type tree that becomes the query's predicate (None: no predicate).  As join_parts, with
    one addition: when the And has at least one projection, its sub-conditions that are pure type trees (And /
    Or / Not over hg.type / hg.typePlus) form the predicate instead of a scanned plain part.  A condition
    without any projection is one plain part (a DNF query over the atoms) and has no predicate."""
    subs = [cond] if isinstance(cond, MapCondition) else _flatten(cond, []) if isinstance(cond, And) else None
    if subs is None or not any(isinstance(c, MapCondition) for c in subs):
        _check_part(cond, cond)
        return [(None, cond)], None
    trees = [c for c in subs if not isinstance(c, MapCondition) and is_type_tree(c)]
    others = [c for c in subs if isinstance(c, MapCondition) or not is_type_tree(c)]
    parts = join_parts(others[0] if len(others) == 1 else And(others), snapshot)
    return parts, (None if not trees else trees[0] if len(trees) == 1 else And(trees))


def pattern_batch_atoms_arrays(snapshot, part_off, part_pos, keep, clause_off, type_off, types, inc_off, inc, pos_off,
                               pos, pset_off, pat_off, pat, arity, neg_off=None, term_off=None, lit_off=None, lit=None,
                               ops=None, type_scan=True) -> QueryResult:
    """Flat batch for hgx_pattern_batch_atoms (include/hgx_atoms.h): the arrays of pattern_batch_join_arrays, and
    ``keep``: None, or one AtomPredicate or None per join query -- the query's result is restricted to the atoms
    the predicate keeps.  ``type_scan``: clauses without an anchor scan the ATOM index (nodes and links of the
    type).  ``result.atoms`` holds the filter's statistics."""
    part_off = np.ascontiguousarray(part_off, np.int64)
    part_pos = np.ascontiguousarray(part_pos, np.int32)
    clause_off = np.ascontiguousarray(clause_off, np.int64)
    n = len(part_off) - 1
    keep_arr = None
    if keep is not None:
        if len(keep) != n:
            raise ValueError("keep must have one entry per query")
        keep_arr = (C.c_void_p * max(n, 1))(*[None if k is None else k.handle for k in keep])
    if neg_off is None:
        neg_off = term_off = lit_off = np.zeros(0, np.int64)
        lit = ops = np.zeros(0, np.int32)
    arrs = [np.ascontiguousarray(type_off, np.int64), np.ascontiguousarray(types, np.int32),
            np.ascontiguousarray(inc_off, np.int64), np.ascontiguousarray(inc, np.int32),
            np.ascontiguousarray(pos_off, np.int64), np.ascontiguousarray(pos, np.int32),
            np.ascontiguousarray(pset_off, np.int64), np.ascontiguousarray(pat_off, np.int64),
            np.ascontiguousarray(pat, np.int32), np.ascontiguousarray(arity, np.int32),
            np.ascontiguousarray(neg_off, np.int64), np.ascontiguousarray(term_off, np.int64),
            np.ascontiguousarray(lit_off, np.int64), np.ascontiguousarray(lit, np.int32),
            np.ascontiguousarray(ops, np.int32)]
    h = C.c_void_p()
    check(lib().hgx_pattern_batch_atoms(snapshot.handle, n, part_off.ctypes.data,
                                        part_pos.ctypes.data if part_pos.size else None,
                                        None if keep_arr is None else C.cast(keep_arr, C.c_void_p),
                                        clause_off.ctypes.data, *(a.ctypes.data if a.size else None for a in arrs),
                                        len(arrs[-1]), _lib.HGX_ATOMS_TYPE_SCAN if type_scan else 0, C.byref(h)))
    return _read_dnf_result(h, n, scan=True, atoms=True)


def pattern_batch_atoms(snapshot, queries, keep=None, type_scan=True) -> QueryResult:
    """pattern_batch_join over every atom, in one device call (include/hgx_atoms.h).  Every query is a list of
    (pos, cond) parts or a condition atom_parts lowers -- its type trees next to projections become the query's
    predicate.  ``keep``: None, or per query an AtomPredicate, a raw tree over hg.type / hg.typePlus, or None;
    the query's result is restricted to the atoms it keeps (together with the tree atom_parts found, if any).  A
    raw tree is compiled once per distinct tree per call against the snapshot's atom types and released on
    return.  ``type_scan`` (on by default here): a clause without an incidence anchor is split into one clause
    per type and scanned over the atom index -- every atom of the type that passes, NODE atoms included, by the
    node rules of node_satisfies; it needs the atom types (HGXUnsupported without them).  A query without parts
    is empty.  ``result.atoms``: {"queries_filtered", "values_tested", "values_rejected", "ms_filter",
    "bytes_filter"}; ``result.join`` / ``union`` / ``negation`` / ``scan`` as for pattern_batch_join
    (values_distinct before the filter, kept after it; rows_scanned counts atom-index rows)."""
    queries = list(queries)
    if keep is not None and len(keep) != len(queries):
        raise ValueError("keep must have one entry per query")
    part_off, part_pos, clause_off, norm, negs, preds = [0], [], [0], [], [], []
    for j, q in enumerate(queries):
        parts, tree = (q, None) if type(q) in (list, tuple) else atom_parts(q, snapshot)
        k = None if keep is None else keep[j]
        if tree is not None and k is not None:
            if isinstance(k, AtomPredicate):
                raise ValueError(f"query {j}: an AtomPredicate next to the type tree {tree!r} (pass a raw tree)")
            k = And([tree, k])
        preds.append(tree if k is None else k)
        for pos, cond in parts:
            if pos is not None and pos < 0:
                raise ValueError(f"bad target position {pos}")
            part_pos.append(JOIN_SELF if pos is None else int(pos))
            _lower_dnf_query(cond, type_scan, norm, negs)
            clause_off.append(len(norm))
        part_off.append(len(part_pos))
    compiled = {}
    try:
        handles = None
        if any(p is not None for p in preds):
            handles = []
            for p in preds:
                if p is not None and not isinstance(p, AtomPredicate):
                    key = _tree_key(p)
                    if key not in compiled:
                        compiled[key] = AtomPredicate(snapshot, p)
                    p = compiled[key]
                handles.append(p)
        return pattern_batch_atoms_arrays(snapshot, part_off, part_pos, handles, clause_off, *_ext_arrays(norm),
                                          *(encode_negations(negs) if any(negs) else (None,) * 5),
                                          type_scan=type_scan)
    finally:
        for p in compiled.values():
            p.close()


def pattern_batch_dnf(snapshot, queries, type_scan=False) -> QueryResult:
    """Evaluate many And / Or trees over the accelerated leaves in one device call: every query goes
    through to_dnf, its clauses run as one hgx_pattern_batch_ext-shaped batch and are united on the device
    (ascending, each link atom once).  ``queries``: conditions, or lists of normalised clauses -- a dict, or
    a (dict, negations) pair of normalize_clause.  A clause's Nots filter its hits on the device before the
    union (hgx_pattern_batch_dnf_not); a batch without any goes through hgx_pattern_batch_dnf as before.
    ``result.union`` / ``result.negation`` hold the statistics.
    ``type_scan=True`` (off by default: without it a clause without an incidence anchor raises HGXUnsupported, as
    ever) also takes clauses without an anchor that have a type: each is split into one clause per type
    (split_type_scan) and the batch runs through hgx_pattern_batch_dnf_scan, which scans the type index.  Such a
    clause delivers the LINK atoms of its type that pass -- the snapshot holds no node types, so it equals the
    reference's indexByType scan only for a type whose instances are all links.  ``result.scan`` holds the scan
    statistics."""
    clause_off, norm, negs = [0], [], []
    for q in queries:
        _lower_dnf_query(q, type_scan, norm, negs)
        clause_off.append(len(norm))
    if type_scan:
        return pattern_batch_dnf_scan_arrays(snapshot, clause_off, *_ext_arrays(norm),
                                             *(encode_negations(negs) if any(negs) else ()))
    if not any(negs):
        return pattern_batch_dnf_arrays(snapshot, clause_off, *_ext_arrays(norm))
    return pattern_batch_dnf_not_arrays(snapshot, clause_off, *_ext_arrays(norm), *encode_negations(negs))


def pattern_batch(snapshot, queries) -> QueryResult:
    """Evaluate many accelerated And queries in one GPU launch sequence.  ``queries``: conditions,
    normalised dicts, or legacy (type, incident, pattern) tuples (pattern None = no orderedLink)."""
    norm = []
    for q in queries:
        if isinstance(q, tuple):
            q = _from_tuple(q)
        elif not isinstance(q, dict) and q != "empty":
            q = normalize(q)
        norm.append(q)
    n = len(norm)
    empty = np.array([q == "empty" for q in norm], bool)
    r = pattern_batch_ext_arrays(snapshot, *_ext_arrays(norm))
    if empty.any():
        parts = [np.empty(0, np.int32) if empty[i] else r[i] for i in range(n)]
        off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        return QueryResult(off, np.concatenate(parts).astype(np.int32), r.ms)
    return r


class QueryMetaData:
    """C/query/cond2qry/QueryMetaData.java -- ORACCESS for the accelerated And."""

    def __init__(self, ordered=True, random_access=True, predicate_cost=-1):
        self.ordered, self.randomAccess, self.predicateCost = ordered, random_access, predicate_cost


class GpuAndToQuery:
    """ConditionToQuery for And, registered with HGQueryConfiguration.addCompiler(And, ...)."""

    def getQuery(self, snapshot, cond):
        if _has_not(cond):   # the Nots filter the And's hits on the device: one clause of the DNF path
            return GpuOrToQuery().getQuery(snapshot, cond)
        norm = normalize(cond)

        class _Q:
            def execute(_self):
                return list(pattern_batch(snapshot, [norm])[0].tolist())

        return _Q()

    def getMetaData(self, snapshot, cond):
        if _has_not(cond):
            return GpuOrToQuery().getMetaData(snapshot, cond)
        normalize(cond)
        return QueryMetaData(True, True, -1)


class GpuOrToQuery:
    """ConditionToQuery for Or (and for an And holding an Or), registered with
    HGQueryConfiguration.addCompiler(Or, ...): the condition's DNF as one device batch."""

    def getQuery(self, snapshot, cond):
        clauses = [normalize_clause(c) for c in to_dnf(cond)]

        class _Q:
            def execute(_self):
                return list(pattern_batch_dnf(snapshot, [clauses])[0].tolist())

        return _Q()

    def getMetaData(self, snapshot, cond):
        """OrToQuery.getMetaData (OrToQuery.java:44-76): ordered and random-access when every operand
        is -- every accelerated clause is (GpuAndToQuery.getMetaData)."""
        try:
            to_dnf(cond)
        except HGXUnsupported:
            return QueryMetaData(False, False, -1)
        return QueryMetaData(True, True, -1)


class GpuScanToQuery:
    """ConditionToQuery for And and Or that also takes clauses without an incidence anchor, by a scan of the
    device type index (include/hgx_scan.h).  Opt-in: a caller registers it with
    HGQueryConfiguration.addCompiler(And, GpuScanToQuery()) and (Or, ...) for a graph whose scanned types have
    link instances only -- a scanned clause delivers the LINK atoms of its type, the reference's indexByType
    scan also the nodes of that type.  Without it find_all keeps refusing such a clause."""

    def getQuery(self, snapshot, cond):
        clauses = [normalize_clause(c) for c in to_dnf(cond)]

        class _Q:
            def execute(_self):
                return list(pattern_batch_dnf(snapshot, [clauses], type_scan=True)[0].tolist())

        return _Q()

    def getMetaData(self, snapshot, cond):
        """Ordered and random-access: every clause's run ascends and the union keeps the order (AndToQuery
        over one ordered set, OrToQuery.java:44-76)."""
        try:
            to_dnf(cond)
        except HGXUnsupported:
            return QueryMetaData(False, False, -1)
        return QueryMetaData(True, True, -1)


class GpuMapToQuery:
    """ConditionToQuery for MapCondition, registered with HGQueryConfiguration.addCompiler(MapCondition, ...):
    hg.apply(hg.targetAt(graph, i), cond) as one device join batch (include/hgx_join.h).  getMetaData reports
    ordered and random-access, which the result is (the sorted set of the projected atoms); the reference's
    MapCondition translator reports neither (ToQueryMap.java:417-426: its ResultMapQuery delivers the values
    in the inner order, duplicates included)."""

    def getQuery(self, snapshot, cond):
        parts = join_parts(cond, snapshot)

        class _Q:
            def execute(_self):
                return list(pattern_batch_join(snapshot, [parts])[0].tolist())

        return _Q()

    def getMetaData(self, snapshot, cond):
        try:
            for _, c in join_parts(cond, snapshot):
                to_dnf(c)
        except HGXUnsupported:
            return QueryMetaData(False, False, -1)
        return QueryMetaData(True, True, -1)


class HGQueryConfiguration:
    """Per-graph compiler registry (C/query/HGQueryConfiguration.java:37-66)."""

    def __init__(self):
        self._compilers = {}

    def addCompiler(self, cls, compiler):
        self._compilers[cls] = compiler

    def compiler(self, cls):
        return self._compilers.get(cls)


def _has_or(cond):
    return isinstance(cond, Or) or (isinstance(cond, And) and any(_has_or(c) for c in cond))


def _has_not(cond):
    return isinstance(cond, Not) or (isinstance(cond, (And, Or)) and any(_has_not(c) for c in cond))


def _find_all_join(snapshot, cond):
    """find_all's And of mapped sub-queries on the device (pattern_batch_join), or None when join_parts or
    the engine refuses it (the caller keeps its host path)."""
    try:
        return list(pattern_batch_join(snapshot, [join_parts(cond, snapshot)])[0].tolist())
    except HGXUnsupported:
        return None


def find_all(snapshot, cond, config: HGQueryConfiguration | None = None):
    """hg.findAll(graph, cond) for the accelerated shapes.  On a snapshot with atom types
    (``snapshot.set_atom_types``), and only there, two shapes every other route refuses go through
    pattern_batch_atoms: a condition whose DNF has a typed clause without an incidence anchor (the scan then
    delivers the nodes of the type too), and an And of type trees with projections."""
    try:
        return _find_all(snapshot, cond, config)
    except HGXUnsupported:
        if getattr(snapshot, "atom_type", None) is None or isinstance(cond, BFSCondition):
            raise
        try:
            return list(pattern_batch_atoms(snapshot, [cond])[0].tolist())
        except HGXUnsupported:
            pass
        raise


def _find_all(snapshot, cond, config):
    if isinstance(cond, BFSCondition):
        # TraversalBasedQuery(traversal, ReturnType.targets) (ToQueryMap.java:313-319): the atoms
        # in HGBreadthFirstTraversal.next() order
        gen = DefaultALGenerator(snapshot, cond.link_predicate, cond.sibling_predicate, *cond.flags)
        seq = bfs_sequence(snapshot, [cond.start], cond.max_distance, gen)
        return seq.pairs(0)[1].tolist()
    if isinstance(cond, MapCondition):
        compiler = (config.compiler(MapCondition) if config else None) or GpuMapToQuery()
        try:
            return compiler.getQuery(snapshot, cond).execute()
        except HGXUnsupported:
            pass   # a mapping or an inner condition the join does not take: the host path below
        return sorted({v for v in (cond.mapping(x) for x in _find_all(snapshot, cond.cond, config)) if v is not None})
    if isinstance(cond, Or) or (isinstance(cond, And) and _has_or(cond)) or _has_not(cond):
        compiler = (config.compiler(Or) if config else None) or GpuOrToQuery()
        try:
            return compiler.getQuery(snapshot, cond).execute()
        except HGXUnsupported:
            if _has_not(cond):
                raise   # a Not over anything but the accelerated leaves, or without an anchor: the CPU's query
            # a part the pattern engine does not take (Map / BFS sub-conditions): host set algebra
        if isinstance(cond, Or):
            return sorted(set().union(*(_find_all(snapshot, c, config) for c in cond)))
        joined = _find_all_join(snapshot, cond)
        if joined is not None:
            return joined
        subs = _flatten(cond, [])
        own = (MapCondition, BFSCondition, Or)
        sets = [set(_find_all(snapshot, c, config)) for c in subs if isinstance(c, own)]
        rest = [c for c in subs if not isinstance(c, own)]
        if rest:
            sets.append(set(_find_all(snapshot, And(rest), config)))
        return sorted(set.intersection(*sets))
    if isinstance(cond, And):
        subs = _flatten(cond, [])
        if any(isinstance(c, (MapCondition, BFSCondition)) for c in subs):
            # And of mapped / traversal sub-queries: one device join batch when every part is a projection or
            # plain, else set intersection of the parts
            joined = _find_all_join(snapshot, cond)
            if joined is not None:
                return joined
            sets = [set(_find_all(snapshot, c, config)) for c in subs if isinstance(c, (MapCondition, BFSCondition))]
            rest = [c for c in subs if not isinstance(c, (MapCondition, BFSCondition))]
            if rest:
                sets.append(set(_find_all(snapshot, And(rest), config)))
            return sorted(set.intersection(*sets))
    compiler = (config.compiler(And) if config else None) or GpuAndToQuery()
    return compiler.getQuery(snapshot, cond).execute()
