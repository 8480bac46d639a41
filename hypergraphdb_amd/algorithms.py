"""GPU traversal behind the reference's HGTraversal / HGALGenerator API.

Reference (C = core/src/java/org/hypergraphdb):
  * HGTraversal                (C/algorithms/HGTraversal.java:36-63)
  * HGBreadthFirstTraversal    (C/algorithms/HGBreadthFirstTraversal.java:29-164)
  * DefaultALGenerator         (C/algorithms/DefaultALGenerator.java:73-593)
  * AtomTypeCondition as link predicate (C/query/AtomTypeCondition.java:121-135)

``bfs_batch`` is the batched entry (many start atoms per launch) the GPU engine is built for.
``HGBreadthFirstTraversal`` keeps the single-seed iterator contract (hasNext/next/isVisited/
reset, remove() unsupported) on top of one batch of size 1.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import HGXError, check, lib, ptr


class HGException(RuntimeError):
    """org.hypergraphdb.HGException"""


class AtomTypeCondition:
    """hg.type(T): exact type equality (no subtypes), C/query/AtomTypeCondition.java:121-135."""

    def __init__(self, type_key: int):
        self.type = int(type_key)

    def __eq__(self, o):
        return isinstance(o, AtomTypeCondition) and o.type == self.type

    def __hash__(self):
        return hash(("type", self.type))

    def __repr__(self):
        return f"type({self.type})"


class LinkPredicate:
    """A link predicate of a DefaultALGenerator, evaluated once per link row on the snapshot's device
    (hgx_link_predicate, include/hgx_linkpred.h): any tree of hg.and_ / hg.or_ / hg.not_ over the accelerated
    leaves -- type, typePlus, incident, incidentAt / incidentNotAt, orderedLink, link, arity.  Anything else in
    the tree raises HGXUnsupported.  Reusable across calls and across the snapshot's contexts; a result made
    with it keeps it alive, so closing it first is fine.  While one lives the snapshot refuses updates."""

    def __init__(self, snapshot, cond):
        self._h = None
        lit_off, lit, ops = encode_link_predicate(lower_link_predicate(cond))
        h = C.c_void_p()
        check(lib().hgx_link_predicate_create(snapshot.handle, len(lit_off) - 1, ptr(lit_off), ptr(lit), ptr(ops),
                                              len(ops), C.byref(h)))
        self._h = h
        self.snapshot = snapshot
        self.cond = cond
        self.num_links, self.num_satisfied, self._ms, self._bytes = self._info()

    def _info(self):
        m, ns, ms, by = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
        check(lib().hgx_link_predicate_info(self.handle, C.byref(m), C.byref(ns), C.byref(ms), C.byref(by)))
        return m.value, ns.value, ms.value, by.value

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("link predicate closed")
        return self._h

    def flags(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """uint8 per link row of [first, first + n): 1 = the row satisfies the predicate."""
        n = self.num_links - first if n is None else n
        out = np.empty(max(n, 1), np.uint8)
        check(lib().hgx_link_predicate_flags(self.handle, int(first), int(n), ptr(out) if n else None))
        return out[:n]

    def stats(self) -> dict:
        """Device ms of the evaluation and projection kernels (timing enabled) and their algorithmic bytes."""
        return {"num_links": self.num_links, "num_satisfied": self.num_satisfied, "ms_eval": self._ms,
                "bytes_eval": self._bytes}

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().hgx_link_predicate_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AtomPredicate:
    """A sibling predicate of a DefaultALGenerator, evaluated once per atom on the snapshot's device
    (hgx_atom_predicate, include/hgx_sibling.h), one bit an atom: any tree of hg.and_ / hg.or_ / hg.not_ over
    hg.type / hg.typePlus, evaluated against the snapshot's atom types (``snapshot.set_atom_types``); anything else
    in the tree raises HGXUnsupported.  ``from_mask``: any predicate the caller evaluated per atom.  Reusable
    across calls and across the snapshot's contexts; a result made with it keeps it alive, so closing it first is
    fine.  While one lives the snapshot refuses updates."""

    def __init__(self, snapshot, cond):
        self._h = None
        lit_off, lit, ops = encode_link_predicate(lower_sibling_predicate(cond))
        h = C.c_void_p()
        check(lib().hgx_atom_predicate_create(snapshot.handle, len(lit_off) - 1, ptr(lit_off), ptr(lit), ptr(ops),
                                              len(ops), C.byref(h)))
        self._attach(snapshot, h, cond)

    @classmethod
    def from_mask(cls, snapshot, keep):
        """``keep``: one truth value per atom, or a callable atom -> bool evaluated once per atom."""
        if callable(keep):
            keep = [bool(keep(a)) for a in range(snapshot.A)]
        k = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
        if k.shape != (snapshot.A,):
            raise ValueError("keep must have one entry per atom")
        self = cls.__new__(cls)
        self._h = None
        h = C.c_void_p()
        check(lib().hgx_atom_predicate_create_mask(snapshot.handle, ptr(k), C.byref(h)))
        self._attach(snapshot, h, None)
        return self

    def _attach(self, snapshot, h, cond):
        self._h = h
        self.snapshot = snapshot
        self.cond = cond
        a, nk, ms, by = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
        check(lib().hgx_atom_predicate_info(h, C.byref(a), C.byref(nk), C.byref(ms), C.byref(by)))
        self.num_atoms, self.num_kept, self._ms, self._bytes = a.value, nk.value, ms.value, by.value

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("atom predicate closed")
        return self._h

    def flags(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """uint8 per atom of [first, first + n): 1 = the atom satisfies the predicate."""
        n = self.num_atoms - first if n is None else n
        out = np.empty(max(n, 1), np.uint8)
        check(lib().hgx_atom_predicate_flags(self.handle, int(first), int(n), ptr(out) if n else None))
        return out[:n]

    def stats(self) -> dict:
        """Device ms of the evaluation kernel (timing enabled) and its algorithmic bytes."""
        return {"num_atoms": self.num_atoms, "num_kept": self.num_kept, "ms_eval": self._ms,
                "bytes_eval": self._bytes}

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().hgx_atom_predicate_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lower_sibling_predicate(cond):
    """A sibling tree -> the terms of its disjunctive normal form (``lower_link_predicate``), every literal a
    hg.type / hg.typePlus leaf; any other leaf raises HGXUnsupported (on a node atom those leaves have rules of
    their own in the reference: evaluate them per atom and use ``AtomPredicate.from_mask``)."""
    from .query import TypePlusCondition
    terms = lower_link_predicate(cond)
    for term in terms:
        for leaf, _ in term:
            if not isinstance(leaf, (AtomTypeCondition, TypePlusCondition)):
                raise _lib.HGXUnsupported(_lib.HGX_E_UNSUPPORTED, f"sibling predicate leaf {leaf!r}: only hg.type / "
                                                                  "hg.typePlus are evaluated on atoms")
    return terms


def lower_link_predicate(cond):
    """A condition tree -> the terms of its disjunctive normal form, tuples of (leaf, polarity) literals: the
    lowering of a negated tree (query.lower_not) applied to the tree itself, without the outer Not."""
    from .query import Not, lower_not   # (query imports this module)
    return lower_not(Not(cond))


def encode_link_predicate(terms):
    """terms -> (lit_off, lit, ops) of hgx_link_predicate_create."""
    from .query import _literal
    lit_off, lit, ops = [0], [], []
    for term in terms:
        for leaf, pol in term:
            kind, operands = _literal(leaf)
            lit.extend((kind, int(bool(pol)), len(ops), len(ops) + len(operands)))
            ops.extend(operands)
        lit_off.append(len(lit) // 4)
    return np.array(lit_off, np.int64), np.array(lit, np.int32), np.array(ops, np.int32)


def decode_link_predicate(lit_off, lit, ops):
    """The inverse of encode_link_predicate up to the leaf classes: (kind, polarity, operand tuple) literals."""
    return [[(int(lit[4 * l]), int(lit[4 * l + 1]), tuple(int(x) for x in ops[lit[4 * l + 2]:lit[4 * l + 3]]))
             for l in range(lit_off[t], lit_off[t + 1])] for t in range(len(lit_off) - 1)]


class DefaultALGenerator:
    """Adjacency-list generator configuration.  linkPredicate: None, an AtomTypeCondition (both through the
    type key of hgx_algen_opts), a LinkPredicate, or a raw tree of hg.and_ / hg.or_ / hg.not_ over the
    accelerated leaves, which every call compiles into a LinkPredicate of its own and releases when it returns
    (include/hgx_linkpred.h).  siblingPredicate (include/hgx_sibling.h; bfs_batch, hop_paths, shortest_paths and
    GraphClassics.dijkstra only -- ``options()`` / ``compiled()`` and so every other caller keep refusing it): None,
    an AtomPredicate, a raw tree over hg.type / hg.typePlus compiled per call against the snapshot's atom types,
    or a callable atom -> bool evaluated once per atom into a mask."""

    def __init__(self, graph, link_predicate=None, sibling_predicate=None, return_preceding=True,
                 return_succeeding=True, reverse_order=False, return_source=None):
        if return_source is None:
            # the 6-argument constructor rejects both false (DefaultALGenerator.java:451-452)
            if not return_preceding and not return_succeeding:
                raise HGException("DefaultALGenerator: attempt to construct with both returnSucceeding and "
                                  "returnPreceeding set to false.")
            return_source = False
        self.graph = graph
        self.link_predicate = link_predicate
        self.sibling_predicate = sibling_predicate
        self.return_preceding = bool(return_preceding)
        self.return_succeeding = bool(return_succeeding)
        self.reverse_order = bool(reverse_order)
        self.return_source = bool(return_source)

    def options(self) -> _lib.AlgenOpts:
        if self.sibling_predicate is not None:
            raise _lib.HGXUnsupported(_lib.HGX_E_UNSUPPORTED, "siblingPredicate is not accelerated")
        if self.link_predicate is None:
            lt = _lib.HGX_NO_TYPE
        elif isinstance(self.link_predicate, AtomTypeCondition):
            lt = self.link_predicate.type
        else:
            raise _lib.HGXUnsupported(_lib.HGX_E_UNSUPPORTED, f"link predicate {self.link_predicate!r}")
        return _lib.AlgenOpts(lt, int(self.return_preceding), int(self.return_succeeding),
                              int(self.reverse_order), int(self.return_source))

    def compiled(self, snapshot):
        """(options, LinkPredicate or None, owned): what a traversal call hands to the engine.  None and an
        AtomTypeCondition go through ``options()``; a LinkPredicate is used as it is; any other tree is
        compiled now (owned = True: the caller closes it when its call returns)."""
        lp = self.link_predicate
        if lp is None or isinstance(lp, AtomTypeCondition):
            return self.options(), None, False
        if self.sibling_predicate is not None:
            raise _lib.HGXUnsupported(_lib.HGX_E_UNSUPPORTED, "siblingPredicate is not accelerated")
        opts = _lib.AlgenOpts(_lib.HGX_NO_TYPE, int(self.return_preceding), int(self.return_succeeding),
                              int(self.reverse_order), int(self.return_source))
        if isinstance(lp, LinkPredicate):
            return opts, lp, False
        return opts, LinkPredicate(snapshot, lp), True

    def compiled_sibling(self, snapshot):
        """(options, LinkPredicate or None, AtomPredicate or None, owned): ``compiled`` for the entry points
        that take a sibling predicate (hgx_bfs_batch_sib, hgx_shortest_paths_sib).  owned: the predicates made
        for this call, which the caller closes when its call returns."""
        sp = self.sibling_predicate
        if sp is None:
            opts, lp, owned = self.compiled(snapshot)
            return opts, lp, None, ([lp] if owned else [])
        bare = DefaultALGenerator(self.graph, self.link_predicate, None, self.return_preceding,
                                  self.return_succeeding, self.reverse_order, self.return_source)
        opts, lp, owned = bare.compiled(snapshot)
        made = [lp] if owned else []
        try:
            if isinstance(sp, AtomPredicate):
                return opts, lp, sp, made
            ap = AtomPredicate.from_mask(snapshot, sp) if callable(sp) else AtomPredicate(snapshot, sp)
        except BaseException:
            for p in made:
                p.close()
            raise
        return opts, lp, ap, made + [ap]


class BfsResult:
    """Per-seed, per-distance visited sets of a batched traversal (device resident)."""

    def __init__(self, snapshot, handle, seeds):
        self.snapshot = snapshot
        self._h = handle
        self.seeds = np.asarray(seeds, np.int32)
        ns, nl = C.c_int32(), C.c_int32()
        check(lib().hgx_bfs_result_info(handle, C.byref(ns), C.byref(nl)))
        self.n_seeds, self.n_levels = ns.value, nl.value
        self._counts = None

    def counts(self) -> np.ndarray:
        """[n_seeds, n_levels] |V_d| per seed (V_0 = {seed})."""
        if self._counts is None:
            out = np.zeros(self.n_seeds * self.n_levels, np.int64)
            check(lib().hgx_bfs_result_counts(self._h, ptr(out)))
            self._counts = out.reshape(self.n_seeds, self.n_levels)
        return self._counts

    def visited(self, seed_index: int, depth: int) -> np.ndarray:
        """V_depth of seed ``seed_index``: ascending atom ids."""
        n = C.c_int64()
        check(lib().hgx_bfs_result_visited(self._h, int(seed_index), int(depth), None, 0, C.byref(n)))
        out = np.empty(max(n.value, 1), np.int32)
        check(lib().hgx_bfs_result_visited(self._h, int(seed_index), int(depth), ptr(out), n.value, C.byref(n)))
        return out[: n.value]

    def levels(self, seed_index: int):
        return [self.visited(seed_index, d) for d in range(self.n_levels)]

    def depth_of(self, seed_index: int, atom: int) -> int:
        d = C.c_int32()
        check(lib().hgx_bfs_result_depth_of(self._h, int(seed_index), int(atom), C.byref(d)))
        return d.value

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("result closed")
        return self._h

    def paths(self, seed_indices, goals) -> "HopPaths":
        """The shortest hop path from seed ``seed_indices[i]`` to ``goals[i]`` for every i (hgx_hops.h):
        what GraphClassics.dijkstra(seed, goal, generator) finds with the default weight, rule R
        predecessors.  The generator is the one this result was made with."""
        si = np.ascontiguousarray(seed_indices, np.int32)
        go = np.ascontiguousarray(goals, np.int32)
        if si.shape != go.shape or si.ndim != 1:
            raise ValueError("seed_indices and goals: two 1-d sequences of one length")
        h = C.c_void_p()
        check(lib().hgx_bfs_result_paths(self.handle, ptr(si), ptr(go), len(si), C.byref(h)))
        return HopPaths(h, self.seeds[si] if len(si) else np.zeros(0, np.int32), go, owner=self)

    def depths(self, seed_index: int, first: int = 0, n: int | None = None) -> np.ndarray:
        """The distanceMatrix row of one seed over atoms [first, first + n): -1 = not reached."""
        n = self.snapshot.A - first if n is None else n
        out = np.empty(max(n, 1), np.int32)
        check(lib().hgx_bfs_result_depth_row(self.handle, int(seed_index), int(first), int(n), ptr(out)))
        return out[:n]

    def predecessors(self, seed_index: int, first: int = 0, n: int | None = None):
        """(predecessor atoms, their links) of one seed over atoms [first, first + n): -1 for the seed
        and for atoms not reached (the predecessorMatrix row, rule R)."""
        n = self.snapshot.A - first if n is None else n
        pa = np.empty(max(n, 1), np.int32)
        pl = np.empty(max(n, 1), np.int32)
        check(lib().hgx_bfs_result_predecessor_row(self.handle, int(seed_index), int(first), int(n), ptr(pa), ptr(pl)))
        return pa[:n], pl[:n]

    def sets(self, seed_indices=None, min_depth=0, max_depth=None, where=None, depths=False, count_only=False,
             max_entries=None) -> "VisitedSets":
        """The visited sets of many seeds in one device pass (hgx_sets.h): set i = the ascending atoms the
        traversal of seed ``seed_indices[i]`` (None: every seed) reached at a depth in [min_depth, max_depth]
        (None: to the last level; min_depth 0 includes the seed), and that satisfy ``where`` -- an AtomPredicate,
        a tree over hg.type / hg.typePlus (compiled for this call), or one truth value per atom.  ``where``
        filters what is reported, not what the traversal expanded.  ``depths``: keep each entry's depth;
        ``count_only``: the offsets alone; ``max_entries``: refuse (HGX_E_NOMEM) a larger result."""
        si = np.arange(self.n_seeds, dtype=np.int32) if seed_indices is None else \
            np.ascontiguousarray(seed_indices, np.int32)
        if si.ndim != 1:
            raise ValueError("seed_indices: a 1-d sequence")
        owned = None
        if where is None or isinstance(where, AtomPredicate):
            ap = where
        elif isinstance(where, (np.ndarray, list, tuple)):
            ap = owned = AtomPredicate.from_mask(self.snapshot, where)
        else:
            ap = owned = AtomPredicate(self.snapshot, where)
        flags = (_lib.HGX_SETS_DEPTHS if depths else 0) | (_lib.HGX_SETS_COUNT_ONLY if count_only else 0)
        md = _lib.HGX_UNBOUNDED if max_depth is None or max_depth >= 2**31 - 1 else int(max_depth)
        h = C.c_void_p()
        try:
            check(lib().hgx_bfs_result_sets(self.handle, ptr(si), len(si), int(min_depth), md,
                                            None if ap is None else ap.handle, flags,
                                            -1 if max_entries is None else int(max_entries), C.byref(h)))
        finally:
            if owned is not None:
                owned.close()   # the call held its own reference
        return VisitedSets(h, self.seeds[si] if len(si) else np.zeros(0, np.int32), owner=self)

    def stats(self, accounting=True, raw=False):
        """Kernel timings (timing enabled), algorithmic bytes; with ``accounting`` also the
        TEPS numerator, |U_d| and the SURVEY.md 8(d) bytes (runs the accounting kernels).
        ``raw``: the hgx_bfs_stats struct itself (``.as_dict()`` later, outside a timed loop)."""
        s = _lib.BfsStats()
        check(lib().hgx_bfs_result_stats(self._h, 1 if accounting else 0, C.byref(s)))
        return s if raw else s.as_dict()

    def close(self):
        if self._h is not None:
            lib().hgx_bfs_result_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HopPaths:
    """Shortest hop paths of a batch of (seed, goal) pairs (hgx_hop_paths, host resident).
    ``hops[i]``: links on pair i's path (-1: not reached); ``reached``; ``path(i)``."""

    def __init__(self, handle, starts, goals, owner=None):
        self._h = handle
        self.starts, self.goals = starts, goals
        self.owner = owner          # the BfsResult the paths were read from
        self.owns_result = False    # hop_paths: the BfsResult was made for this object and closes with it
        n, tot = C.c_int32(), C.c_int64()
        check(lib().hgx_hop_paths_info(handle, C.byref(n), C.byref(tot)))
        self.n_pairs, self.total_atoms = n.value, tot.value
        self.offsets = np.zeros(self.n_pairs + 1, np.int64)
        self.hops = np.zeros(self.n_pairs, np.int32)
        check(lib().hgx_hop_paths_offsets(handle, ptr(self.offsets), ptr(self.hops)))
        self.reached = self.hops >= 0
        self._link_off = self.offsets[:-1] - np.concatenate(([0], np.cumsum(self.reached)[:-1])) if self.n_pairs else \
            np.zeros(0, np.int64)
        self._atoms = self._links = None

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("result closed")
        return self._h

    def _read(self):
        if self._atoms is None:
            atoms = np.empty(max(self.total_atoms, 1), np.int32)
            links = np.empty(max(self.total_atoms, 1), np.int32)
            check(lib().hgx_hop_paths_read(self.handle, ptr(atoms), ptr(links)))
            self._atoms, self._links = atoms, links

    def path(self, i: int):
        """(atoms, links) of pair ``i``: atoms = start .. goal, links[k] joins atoms[k] and atoms[k + 1];
        two empty arrays when the goal was not reached."""
        self._read()
        h = int(self.hops[i])
        if h < 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        o, lo = int(self.offsets[i]), int(self._link_off[i])
        return self._atoms[o:o + h + 1], self._links[lo:lo + h]

    def stats(self) -> dict:
        s, e, p = C.c_int64(), C.c_int64(), C.c_int64()
        ms, by = C.c_double(), C.c_double()
        check(lib().hgx_hop_paths_stats(self.handle, C.byref(s), C.byref(e), C.byref(p), C.byref(ms), C.byref(by)))
        return {"steps": s.value, "entries": e.value, "probes": p.value, "ms_total": ms.value, "bytes": by.value}

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().hgx_hop_paths_free(self._h)
            self._h = None
            if self.owns_result and self.owner is not None:
                self.owner.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bfs_batch(snapshot, seeds, max_depth=None, generator: DefaultALGenerator | None = None) -> BfsResult:
    """HGBreadthFirstTraversal(seeds[i], generator, max_depth) for every i, run together on the GPU."""
    gen = generator or DefaultALGenerator(snapshot)
    opts, pred, apred, owned = gen.compiled_sibling(snapshot)
    s = np.ascontiguousarray(seeds, np.int32)
    md = _lib.HGX_UNBOUNDED if max_depth is None or max_depth >= 2**31 - 1 else int(max_depth)
    h = C.c_void_p()
    try:
        if apred is not None:
            check(lib().hgx_bfs_batch_sib(snapshot.handle, ptr(s), len(s), md, C.byref(opts),
                                          None if pred is None else pred.handle, apred.handle, C.byref(h)))
        elif pred is None:
            check(lib().hgx_bfs_batch(snapshot.handle, ptr(s), len(s), md, C.byref(opts), C.byref(h)))
        else:
            check(lib().hgx_bfs_batch_pred(snapshot.handle, ptr(s), len(s), md, C.byref(opts), pred.handle, C.byref(h)))
    finally:
        for p in owned:
            p.close()   # the result holds its own references
    return BfsResult(snapshot, h, s)


class VisitedSets:
    """The visited sets of a selection of seeds as one CSR (hgx_visited_sets; device resident until read).
    ``offsets`` [n + 1], ``counts`` [n], ``total``; ``self[i]``: set i's ascending atoms, or (atoms, depths) when
    made with depths; ``flat()``: the flat arrays.  A count-only object has offsets and counts alone."""

    def __init__(self, handle, starts, owner=None):
        self._h = handle
        self.starts = starts
        self.owner = owner          # the BfsResult the sets were read from
        self.owns_result = False    # reachable_batch: the BfsResult was made for this object and closes with it
        n, tot, fl = C.c_int32(), C.c_int64(), C.c_uint32()
        check(lib().hgx_visited_sets_info(handle, C.byref(n), C.byref(tot), C.byref(fl)))
        self.n_sets, self.total = n.value, tot.value
        self.with_depths = bool(fl.value & _lib.HGX_SETS_DEPTHS)
        self.count_only = bool(fl.value & _lib.HGX_SETS_COUNT_ONLY)
        self.offsets = np.zeros(self.n_sets + 1, np.int64)
        check(lib().hgx_visited_sets_offsets(handle, ptr(self.offsets)))
        self.counts = np.diff(self.offsets)
        self._atoms = self._depths = None

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("result closed")
        return self._h

    def read(self, first: int = 0, n: int | None = None):
        """The entries [first, first + n) of the flat arrays (cut at the end): atoms, or (atoms, depths)."""
        n = self.total - first if n is None else n
        k = max(min(n, self.total - first), 0)
        atoms = np.empty(max(k, 1), np.int32)
        deps = np.empty(max(k, 1), np.int32) if self.with_depths else None
        check(lib().hgx_visited_sets_read(self.handle, int(first), int(n), ptr(atoms),
                                          None if deps is None else ptr(deps)))
        return (atoms[:k], deps[:k]) if self.with_depths else atoms[:k]

    def flat(self):
        """The flat arrays, read once: atoms, or (atoms, depths)."""
        if self._atoms is None:
            got = self.read()
            self._atoms, self._depths = got if self.with_depths else (got, None)
        return (self._atoms, self._depths) if self.with_depths else self._atoms

    def __len__(self):
        return self.n_sets

    def __getitem__(self, i: int):
        if not -self.n_sets <= i < self.n_sets:
            raise IndexError(i)
        self.flat()
        i %= self.n_sets
        o, e = int(self.offsets[i]), int(self.offsets[i + 1])
        return (self._atoms[o:e], self._depths[o:e]) if self.with_depths else self._atoms[o:e]

    def stats(self) -> dict:
        rr, ts = C.c_int64(), C.c_int64()
        ms, by = C.c_double(), C.c_double()
        check(lib().hgx_visited_sets_stats(self.handle, C.byref(rr), C.byref(ts), C.byref(ms), C.byref(by)))
        return {"rows_read": rr.value, "tiles_skipped": ts.value, "ms_total": ms.value, "bytes": by.value}

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().hgx_visited_sets_free(self._h)
            self._h = None
            if self.owns_result and self.owner is not None:
                self.owner.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def reachable_batch(snapshot, starts, generator: DefaultALGenerator | None = None, max_depth=None, where=None,
                    include_start=False, **kw) -> VisitedSets:
    """For every start: ``find_all(snapshot, hg.and_(where, hg.bfs(start, ...)))`` as a sorted set -- the atoms a
    breadth-first traversal of ``generator`` reaches from it within ``max_depth`` that satisfy ``where`` -- for
    many starts at once: ``bfs_batch`` followed by ``BfsResult.sets`` in one call.  ``include_start``: the start
    itself is a member (subject to ``where``); a traversal never returns it.  ``kw``: depths, count_only,
    max_entries of ``BfsResult.sets``.  The traversal's result closes with the returned object."""
    res = bfs_batch(snapshot, starts, max_depth, generator)
    try:
        vs = res.sets(None, 0 if include_start else 1, None, where, **kw)
    except BaseException:
        res.close()
        raise
    vs.owns_result = True
    return vs


class SequenceResult:
    """Order-exact traversal result: per seed, the (link, atom) pairs next() returns, in order,
    with each atom's distance (host arrays)."""

    def __init__(self, handle, seeds):
        self.seeds = np.asarray(seeds, np.int32)
        try:
            ns, npairs, nl = C.c_int32(), C.c_int64(), C.c_int32()
            check(lib().hgx_seq_result_info(handle, C.byref(ns), C.byref(npairs), C.byref(nl)))
            self.n_seeds, self.n_levels = ns.value, nl.value
            self.offsets = np.zeros(self.n_seeds + 1, np.int64)
            check(lib().hgx_seq_result_offsets(handle, ptr(self.offsets)))
            n = npairs.value
            self.links = np.empty(max(n, 1), np.int32)
            self.atoms = np.empty(max(n, 1), np.int32)
            self.dists = np.empty(max(n, 1), np.int32)
            check(lib().hgx_seq_result_pairs(handle, ptr(self.links), ptr(self.atoms), ptr(self.dists)))
            self.links, self.atoms, self.dists = self.links[:n], self.atoms[:n], self.dists[:n]
            ms, tr = C.c_double(), C.c_double()
            check(lib().hgx_seq_result_stats(handle, C.byref(ms), C.byref(tr)))
            self.ms_total, self.traversed_edges = ms.value, tr.value
            nb, nl, mb, bb = C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
            check(lib().hgx_seq_result_engine_stats(handle, C.byref(nb), C.byref(nl), C.byref(mb), C.byref(bb)))
            # seeds finished by the workgroup-per-seed engine / the level-synchronous reruns, and the
            # workgroup launches' device ms and algorithmic bytes
            self.n_block, self.n_level, self.ms_block, self.bytes_block = nb.value, nl.value, mb.value, bb.value
            ml, bl, pl = C.c_double(), C.c_double(), C.c_int64()
            check(lib().hgx_seq_result_level_stats(handle, C.byref(ml), C.byref(bl), C.byref(pl)))
            # the level-synchronous engine: device ms, algorithmic bytes, levels that ran as pulls
            self.ms_level, self.bytes_level, self.pull_levels = ml.value, bl.value, pl.value
            nc, mc, bc = C.c_int32(), C.c_double(), C.c_double()
            check(lib().hgx_seq_result_grid_stats(handle, C.byref(nc), C.byref(mc), C.byref(bc)))
            # the order-exact grid stage: seeds it finished, device ms, algorithmic bytes
            self.n_coop, self.ms_coop, self.bytes_coop = nc.value, mc.value, bc.value
        finally:
            lib().hgx_seq_result_free(handle)

    def pairs(self, seed_index: int):
        """(links, atoms, dists) of seed ``seed_index`` in next() order."""
        a, b = self.offsets[seed_index], self.offsets[seed_index + 1]
        return self.links[a:b], self.atoms[a:b], self.dists[a:b]


def bfs_sequence(snapshot, seeds, max_depth=None, generator: DefaultALGenerator | None = None) -> SequenceResult:
    """The exact next() sequence of HGBreadthFirstTraversal(seeds[i], generator, max_depth) for
    every i (FIFO order and discovering links as in the reference), computed on the GPU."""
    gen = generator or DefaultALGenerator(snapshot)
    opts, pred, owned = gen.compiled(snapshot)
    s = np.ascontiguousarray(seeds, np.int32)
    md = _lib.HGX_UNBOUNDED if max_depth is None or max_depth >= 2**31 - 1 else int(max_depth)
    h = C.c_void_p()
    try:
        if pred is None:
            check(lib().hgx_bfs_sequence(snapshot.handle, ptr(s), len(s), md, C.byref(opts), C.byref(h)))
        else:
            check(lib().hgx_bfs_sequence_pred(snapshot.handle, ptr(s), len(s), md, C.byref(opts), pred.handle,
                                              C.byref(h)))
    finally:
        if owned:
            pred.close()
    return SequenceResult(h, s)


class HGBreadthFirstTraversal:
    """HGTraversal (C/algorithms/HGTraversal.java:36-63) for one start atom, backed by the GPU
    order-exact traversal: next() returns the same (link, atom) pairs in the same order as
    HGBreadthFirstTraversal.next() (:143-156), None once exhausted; isVisited(h) is true for the
    start atom and for every atom already returned (:137-141); remove() is unsupported (:98-101)."""

    def __init__(self, start, adj_list_generator: DefaultALGenerator, max_distance=None):
        self.start = int(start)
        self.gen = adj_list_generator
        self.max_distance = max_distance
        self.snapshot = adj_list_generator.graph
        self.reset()

    def reset(self):
        seq = bfs_sequence(self.snapshot, [self.start], self.max_distance, self.gen)
        self._links, self._atoms, self._dists = (x.tolist() for x in seq.pairs(0))
        self._returned = {self.start}
        self._pos = 0

    def hasNext(self):
        return self._pos < len(self._atoms)

    def next(self):
        if not self.hasNext():
            return None
        i = self._pos
        self._pos += 1
        self._returned.add(self._atoms[i])
        return (self._links[i], self._atoms[i])

    def distance(self):
        """distance of the atom returned by the last next() (the queue entry's Integer)"""
        return self._dists[self._pos - 1] if self._pos else 0

    def isVisited(self, handle):
        return int(handle) in self._returned

    def remove(self):
        raise NotImplementedError("UnsupportedOperationException")

    def __iter__(self):
        while self.hasNext():
            yield self.next()
