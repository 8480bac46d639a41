"""GPU shortest paths behind the reference's GraphClassics API (include/hgx_paths.h).

Reference (C = core/src/java/org/hypergraphdb):
  * GraphClassics.dijkstra     (C/algorithms/GraphClassics.java:126-209)
  * DefaultALGenerator         (C/algorithms/DefaultALGenerator.java:73-593)

``shortest_paths`` is the batched entry (many (start, goal) pairs per call) the GPU engine is built
for; ``GraphClassics.dijkstra`` keeps the reference's single-pair signature on top of a batch of one.
``hop_paths`` is the batched unit-weight form (the reference's 3-argument dijkstra, GraphClassics.java:80-83):
one batched BFS over the distinct starts and the backtrace of include/hgx_hops.h.  It is the faster way from a
few tens of pairs a call; a single pair is faster on the relaxation engine, so ``GraphClassics.dijkstra``
stays there.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib, ptr
from .algorithms import DefaultALGenerator, HopPaths, LinkPredicate, bfs_batch  # noqa: F401

NO_GOAL = _lib.HGX_NO_GOAL


class LinkWeights:
    """One weight per link row, validated and resident on the snapshot's device (hgx_link_weights):
    the reference's ``Mapping<HGHandle, Double> weight`` evaluated once per link.  Reusable across
    calls; refused after a snapshot update that changes the link count."""

    def __init__(self, snapshot, weights):
        self._h = None
        w = np.ascontiguousarray(weights, np.float64)
        if w.shape != (snapshot.M,):
            raise ValueError(f"weights: expected {snapshot.M} values (one per link row), got {w.shape}")
        h = C.c_void_p()
        check(lib().hgx_link_weights_create(snapshot.handle, w.ctypes.data, C.byref(h)))
        self._h = h
        self.snapshot = snapshot

    @classmethod
    def from_mapping(cls, snapshot, weight):
        """``weight``: callable link atom -> float, evaluated once per link (Mapping.eval)."""
        return cls(snapshot, np.array([float(weight(int(l))) for l in snapshot.link_atom], np.float64))

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("weights closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().hgx_link_weights_free(self._h)
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


class ShortestPathsResult:
    """Distances, paths and (for NO_GOAL pairs) whole distance / predecessor rows of one batch."""

    def __init__(self, snapshot, handle, starts, goals):
        self.snapshot = snapshot
        self._h = handle
        self.starts, self.goals = starts, goals
        n = C.c_int32()
        check(lib().hgx_sp_result_info(handle, C.byref(n)))
        self.n_pairs = n.value
        self.distance = np.zeros(self.n_pairs, np.float64)      # d*(goal), +inf when not connected
        reached = np.zeros(self.n_pairs, np.uint8)
        check(lib().hgx_sp_result_distances(handle, ptr(self.distance), ptr(reached)))
        self.reached = reached.astype(bool)

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("result closed")
        return self._h

    def path(self, i: int):
        """(atoms, links) of pair ``i``: atoms = start .. goal, links[k] joins atoms[k] and atoms[k + 1];
        two empty arrays when the goal is not connected (and for NO_GOAL pairs)."""
        n = C.c_int64()
        check(lib().hgx_sp_result_path(self.handle, int(i), None, None, 0, C.byref(n)))
        atoms = np.empty(max(n.value, 1), np.int32)
        links = np.empty(max(n.value, 1), np.int32)
        check(lib().hgx_sp_result_path(self.handle, int(i), ptr(atoms), ptr(links), n.value, C.byref(n)))
        return atoms[: n.value], links[: max(n.value - 1, 0)]

    def distances(self, i: int, first: int = 0, n: int | None = None) -> np.ndarray:
        """The distance row of NO_GOAL pair ``i`` over atoms [first, first + n): +inf = not reached."""
        n = self.snapshot.A - first if n is None else n
        out = np.empty(max(n, 1), np.float64)
        check(lib().hgx_sp_result_distance_row(self.handle, int(i), int(first), int(n), ptr(out)))
        return out[:n]

    def predecessors(self, i: int, first: int = 0, n: int | None = None):
        """(predecessor atoms, their links) of NO_GOAL pair ``i`` over atoms [first, first + n): -1 for
        the start and for atoms not reached."""
        n = self.snapshot.A - first if n is None else n
        pa = np.empty(max(n, 1), np.int32)
        pl = np.empty(max(n, 1), np.int32)
        check(lib().hgx_sp_result_predecessor_row(self.handle, int(i), int(first), int(n), ptr(pa), ptr(pl)))
        return pa[:n], pl[:n]

    def stats(self) -> dict:
        r, e, x, m = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        ms, by = C.c_double(), C.c_double()
        check(lib().hgx_sp_result_stats(self.handle, C.byref(r), C.byref(e), C.byref(x), C.byref(m), C.byref(ms),
                                        C.byref(by)))
        return {"rounds": r.value, "expanded": e.value, "relaxed": x.value, "improved": m.value,
                "ms_total": ms.value, "bytes": by.value}

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().hgx_sp_result_free(self._h)
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


def shortest_paths(snapshot, starts, goals, generator: DefaultALGenerator | None = None,
                   weights=None) -> ShortestPathsResult:
    """GraphClassics.dijkstra(starts[i], goals[i], generator, weights) for every i, run together on the
    GPU.  ``goals[i]`` None / NO_GOAL: distances from starts[i] to every reachable atom.  ``weights``:
    None (1.0 per link), an array with one value per link row, a LinkWeights, or a callable
    link atom -> float (evaluated once per link)."""
    gen = generator or DefaultALGenerator(snapshot)
    s = np.ascontiguousarray(starts, np.int32)
    g = np.ascontiguousarray([NO_GOAL if x is None else int(x) for x in goals], np.int32)
    if s.shape != g.shape or s.ndim != 1:
        raise ValueError("starts and goals: two 1-d sequences of one length")
    own = None
    if weights is None:
        wh = None
    elif isinstance(weights, LinkWeights):
        wh = weights.handle
    else:
        own = LinkWeights.from_mapping(snapshot, weights) if callable(weights) else LinkWeights(snapshot, weights)
        wh = own.handle
    owned = []
    try:
        opts, pred, apred, owned = gen.compiled_sibling(snapshot)
        h = C.c_void_p()
        if apred is not None:
            check(lib().hgx_shortest_paths_sib(snapshot.handle, ptr(s), ptr(g), len(s), C.byref(opts), wh,
                                               None if pred is None else pred.handle, apred.handle, C.byref(h)))
        elif pred is None:
            check(lib().hgx_shortest_paths(snapshot.handle, ptr(s), ptr(g), len(s), C.byref(opts), wh, C.byref(h)))
        else:
            check(lib().hgx_shortest_paths_pred(snapshot.handle, ptr(s), ptr(g), len(s), C.byref(opts), wh,
                                                pred.handle, C.byref(h)))
    finally:
        if own is not None:
            own.close()
        for p in owned:
            p.close()   # the result holds its own references
    return ShortestPathsResult(snapshot, h, s, g)


def hop_paths(snapshot, starts, goals, generator: DefaultALGenerator | None = None, max_depth=None) -> HopPaths:
    """GraphClassics.dijkstra(starts[i], goals[i], generator) with the default weight (1.0 per link,
    C/algorithms/GraphClassics.java:80-83) for every i: one batched BFS over the distinct starts and the
    backtrace of include/hgx_hops.h over its level rows.  ``max_depth`` bounds the BFS: goals beyond it
    are reported as not reached.  The returned HopPaths keeps the BfsResult alive (``.owner``)."""
    s = np.ascontiguousarray(starts, np.int32)
    g = np.ascontiguousarray(goals, np.int32)
    if s.shape != g.shape or s.ndim != 1:
        raise ValueError("starts and goals: two 1-d sequences of one length")
    distinct, index = np.unique(s, return_inverse=True)
    res = bfs_batch(snapshot, distinct, max_depth, generator)
    try:
        hp = res.paths(index.astype(np.int32), g)
    except Exception:
        res.close()
        raise
    hp.owns_result = True
    return hp


class GraphClassics:
    """org.hypergraphdb.algorithms.GraphClassics (the accelerated part: dijkstra)."""

    @staticmethod
    def dijkstra(start, goal, generator: DefaultALGenerator, weight=None, distance_matrix=None,
                 predecessor_matrix=None):
        """GraphClassics.dijkstra (C/algorithms/GraphClassics.java:126-209): the distance between
        ``start`` and ``goal`` as a float, or None when they are not connected.  ``weight``: as
        ``shortest_paths``'s weights (None = 1.0 per link, the reference's default Mapping).

        Deviation: ``distance_matrix`` / ``predecessor_matrix`` (dicts), when given, receive the entries
        of the atoms ON THE RETURNED PATH (exact values).  The reference also leaves entries -- some of
        them tentative -- for the other atoms it touched before it reached the goal.  ``goal=None``
        gives the complete, exact maps: every reachable atom's distance and predecessor (which is what
        the reference's maps hold when the goal is never reached); the call then returns None."""
        snap = generator.graph
        with shortest_paths(snap, [int(start)], [goal], generator, weight) as r:
            if goal is None:
                if distance_matrix is not None or predecessor_matrix is not None:
                    d = r.distances(0)
                    pa, _ = r.predecessors(0)
                    for a in np.nonzero(np.isfinite(d))[0].tolist():
                        if distance_matrix is not None:
                            distance_matrix[a] = float(d[a])
                        if predecessor_matrix is not None and pa[a] >= 0:
                            predecessor_matrix[a] = int(pa[a])
                return None
            if not r.reached[0]:
                if distance_matrix is not None:
                    distance_matrix[int(start)] = 0.0
                return None
            if distance_matrix is not None or predecessor_matrix is not None:
                atoms, links = r.path(0)
                w = _weights_of(snap, weight, links)
                d = 0.0
                for k, a in enumerate(atoms.tolist()):
                    if k:
                        d = d + w[k - 1]        # the left-to-right sum the engine computed
                        if predecessor_matrix is not None:
                            predecessor_matrix[a] = int(atoms[k - 1])
                    if distance_matrix is not None:
                        distance_matrix[a] = d
            return float(r.distance[0])


def _weights_of(snap, weight, links):
    """Host-side weights of the given link atoms (for the distance entries along a path)."""
    if weight is None:
        return [1.0] * len(links)
    if isinstance(weight, LinkWeights):
        raise ValueError("dijkstra: filling the maps needs the weights as an array or a callable")
    if callable(weight):
        return [float(weight(int(l))) for l in links]
    w = np.asarray(weight, np.float64)
    return [float(w[snap.row_of(int(l))]) for l in links]
