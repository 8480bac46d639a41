"""TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Reference side of the atom tests (no GPU): the pattern path over EVERY atom of a snapshot whose atoms all carry a
type key (include/hgx_atoms.h), by brute force.

A condition tree is evaluated on one atom at a time, links and nodes alike, by direct recursion over And / Or /
Not -- no DNF, no anchors, no scans, no index:
  * on a link atom a leaf outside a Not means its query translation (dnf_ref.satisfies) and inside a Not its raw
    satisfies (not_ref.raw), as in not_ref;
  * on a NODE atom a leaf takes the reference's own satisfies (C = core/src/java/org/hypergraphdb/query):
    arity(k) holds iff k == 0 (C/ArityCondition.java:54-55); incident, incidentAt / incidentNotAt, orderedLink and
    link are false (C/IncidentCondition.java:71-75, C/PositionedIncidentCondition.java:134-135,
    C/OrderedLinkCondition.java:100-101, C/LinkCondition.java:119-120) -- a node's store record has no targets --
    and that includes the EMPTY orderedLink() / link() under a Not, which not_ref.raw makes true on a link without
    targets: a node is not an arity-0 link.
A part of a join query projects its atoms to a target position (a node, like a link too short, contributes
nothing), the parts' values are intersected, and the query's predicate -- a type tree by sibling_ref.holds, or a
per-atom mask -- restricts what is left.

The model reads one type per atom (``atom_type``).  A link row WITHOUT a type (link_type < 0) is answered by the
engine from atom_type in a scanned clause and from link_type in an anchored one (the one documented difference of
include/hgx_atoms.h); the model does not know that split, so the hand graph keeps its untyped row away from the
anchors of typed clauses and the tests pin it in scans only."""
from __future__ import annotations

import numpy as np

import dnf_ref as D
import not_ref as N
import scan_ref as S
import sibling_ref as SR
from hypergraphdb_amd.algorithms import AtomTypeCondition
from hypergraphdb_amd.query import (And, ArityCondition, IncidentCondition, LinkCondition, Not, Or,
                                    OrderedLinkCondition, PositionedIncidentCondition, TypePlusCondition, to_dnf)


class AtomGraph:
    """Every atom of a snapshot: ``links`` {link atom: targets}, ``atom_type`` one key per atom."""

    def __init__(self, g, atom_type):
        off, tg = g["tgt_off"], g["tgt_idx"]
        self.A = int(g["num_atoms"])
        self.links = {int(a): [int(x) for x in tg[off[i]:off[i + 1]]] for i, a in enumerate(g["link_atom"])}
        self.atom_type = [int(t) for t in atom_type]
        assert len(self.atom_type) == self.A


def node_raw(leaf, type_) -> bool:
    """satisfies(graph, node) of a leaf class on a node atom of this type (the rules of the module docstring)."""
    if isinstance(leaf, AtomTypeCondition):
        return type_ == leaf.type
    if isinstance(leaf, TypePlusCondition):
        return type_ in leaf.types
    if isinstance(leaf, ArityCondition):
        return leaf.arity == 0
    if isinstance(leaf, (IncidentCondition, PositionedIncidentCondition, OrderedLinkCondition, LinkCondition)):
        return False
    raise TypeError(leaf)


def raw(ag, cond, atom) -> bool:
    """What a Not negates, on any atom."""
    if isinstance(cond, And):
        return all(raw(ag, c, atom) for c in cond)
    if isinstance(cond, Or):
        return any(raw(ag, c, atom) for c in cond)
    if isinstance(cond, Not):
        return not raw(ag, cond.negated, atom)
    if atom in ag.links:
        return N.raw(cond, ag.links[atom], ag.atom_type[atom])
    return node_raw(cond, ag.atom_type[atom])


def satisfies(ag, cond, atom) -> bool:
    """Does the atom belong to the result of the query the tree compiles to?"""
    if isinstance(cond, And):
        return all(satisfies(ag, c, atom) for c in cond)
    if isinstance(cond, Or):
        return any(satisfies(ag, c, atom) for c in cond)
    if isinstance(cond, Not):
        return not raw(ag, cond.negated, atom)
    if atom in ag.links:
        return D.satisfies(cond, ag.links[atom], ag.atom_type[atom])
    return node_raw(cond, ag.atom_type[atom])   # (an empty orderedLink is a NOP on a link and false on a node)


_atoms = {}   # (id(ag), id(cond)) -> (ag, cond, atoms): one brute-force pass per part, shared by the tests


def evaluate(ag, cond) -> list:
    """The sorted atoms, nodes and links, of the result."""
    k = (id(ag), id(cond))
    if k not in _atoms:
        _atoms[k] = (ag, cond, [a for a in range(ag.A) if satisfies(ag, cond, a)])
    return _atoms[k][2]


def project(ag, atoms, pos) -> set:
    if pos is None:
        return set(atoms)
    return {ag.links[a][pos] for a in atoms if a in ag.links and len(ag.links[a]) > pos}


def keeps(ag, keep, atom) -> bool:
    """``keep``: None, a type tree, or a mask (one truth value per atom)."""
    if keep is None:
        return True
    if isinstance(keep, (And, Or, Not, AtomTypeCondition, TypePlusCondition)):
        return SR.holds(keep, ag.atom_type[atom])
    return bool(keep[atom])


def join(ag, parts, keep=None) -> list:
    """One query [(pos, cond)] with its predicate: no parts, no result."""
    if not parts:
        return []
    vals = set.intersection(*(project(ag, evaluate(ag, c), p) for p, c in parts))
    return sorted(v for v in vals if keeps(ag, keep, v))


def stats(ag, queries, keeps_=None) -> dict:
    """What the join and atoms statistics of a batch must report.  The filter tests the distinct values of each
    filtered query's driver part: the part with the fewest atoms, the lowest index among equals."""
    parts = hits = distinct = kept = filtered = tested = rejected = 0
    for j, q in enumerate(queries):
        k = None if keeps_ is None else keeps_[j]
        parts += len(q)
        sizes = [len(evaluate(ag, c)) for _, c in q]
        hits += sum(sizes)
        distinct += sum(len(project(ag, evaluate(ag, c), p)) for p, c in q)
        kept += len(join(ag, q, k))
        if k is not None:
            filtered += 1
            if q:
                p, c = q[sizes.index(min(sizes))]
                vals = project(ag, evaluate(ag, c), p)
                tested += len(vals)
                rejected += sum(not keeps(ag, k, v) for v in vals)
    return {"join": {"parts": parts, "hits_projected": hits, "values_distinct": distinct, "kept": kept},
            "atoms": {"queries_filtered": filtered, "values_tested": tested, "values_rejected": rejected}}


def type_count(ag) -> dict:
    keys, cnt = np.unique(np.asarray(ag.atom_type), return_counts=True)
    return {int(k): int(c) for k, c in zip(keys, cnt)}


def scan_counts(ag, conds) -> dict:
    """clauses_scanned / rows_scanned / rows_kept of a batch of part conditions: scan_ref.scan_counts over the
    atoms -- an anchor-free clause counts once per type key it allows and, unless a NOP, covers every ATOM of
    each."""
    tc = type_count(ag)
    clauses = rows = kept = 0
    for cond in conds:
        for cl in to_dnf(cond):
            if not S.is_scanned(cl):
                continue
            ts = S.clause_types(cl)
            clauses += len(ts)
            if not S.is_nop(cl):
                rows += sum(tc.get(k, 0) for k in ts)
                kept += sum(satisfies(ag, And(cl), a) for a in range(ag.A))
    return {"clauses_scanned": clauses, "rows_scanned": rows, "rows_kept": kept}


def random_type_tree(rng, n_types, depth=2):
    """A tree over hg.type / hg.typePlus, an absent key (n_types) among the operands."""
    from hypergraphdb_amd.query import hg
    if depth == 0 or rng.random() < 0.4:
        if rng.random() < 0.5:
            return hg.type(int(rng.integers(0, n_types + 1)))
        return hg.typePlus({int(t) for t in rng.integers(0, n_types + 1, 2)})
    k = rng.random()
    if k < 0.25:
        return Not(random_type_tree(rng, n_types, depth - 1))
    kids = [random_type_tree(rng, n_types, depth - 1) for _ in range(int(rng.integers(1, 4)))]
    return Or(kids) if k < 0.65 else And(kids)


def hand_graph():
    """About 400 atoms whose type segments are 1, 63, 64, 65 and 129 atoms long (a wave handles 64 index
    entries), ids interleaved.  Returns (arrays, atom_type, names)."""
    import kat_graphs as K
    T = dict(ONE=10, NODE=11, LINK=12, MIX=13, BIG=14, ABSENT=15, PAD=16)
    b = K.Builder()
    at = {}

    def node(name, t):
        a = b.node(name)
        at[a] = t
        return a

    def link(name, t, *tg, typed=True):
        a = b.link(name, t if typed else -1, *tg)
        at[a] = t
        return a

    a = node("a", T["NODE"])                       # the anchor of the incident queries
    one = node("one", T["ONE"])                    # a type with a single atom
    nodes = [node(f"n{i}", T["NODE"]) for i in range(20)]
    link("empty", T["MIX"])                        # an arity-0 link
    inner = link("inner", T["MIX"], a, nodes[0])
    link("outer", T["MIX"], nodes[1], inner)       # a link whose target is a link
    link("untyped", T["MIX"], nodes[3], nodes[2], typed=False)   # a link row without a type: indexed under its atom type
    for i in range(31):                            # MIX: 4 + 31 links + 30 nodes = 65
        link(f"m{i}", T["MIX"], *([a] if i % 3 == 0 else []), nodes[i % 20], one if i % 5 == 0 else nodes[(i + 7) % 20])
        if i < 30:
            node(f"mn{i}", T["MIX"])
    for i in range(64):                            # LINK: link-only, arities 1..3
        link(f"l{i}", T["LINK"], *[nodes[(i + k) % 20] for k in range(1 + i % 3)])
        if i < 42:
            node(f"nn{i}", T["NODE"])              # NODE: 1 + 20 + 42 = 63, node-only
    for i in range(129):                           # BIG: 60 links, 69 nodes
        if i % 2 == 0 and i < 120:
            link(f"b{i}", T["BIG"], nodes[i % 20], a if i % 8 == 0 else nodes[(i + 3) % 20])
        else:
            node(f"bn{i}", T["BIG"])
    for i in range(78):
        node(f"p{i}", T["PAD"])
    g = b.arrays()
    atom_type = np.array([at[x] for x in range(g["num_atoms"])], np.int32)
    cnt = type_count(AtomGraph(g, atom_type))
    assert [cnt[T[k]] for k in ("ONE", "NODE", "LINK", "MIX", "BIG", "PAD")] == [1, 63, 64, 65, 129, 78]
    assert g["num_atoms"] == 400 and T["ABSENT"] not in cnt
    return g, atom_type, T
