"""hypergraphdb_amd -- MI355X-native engine for HyperGraphDB's data-parallel query path.

Native engine: libhgx.so (HIP kernels for gfx950 + the C ABI of include/hgx.h).
This package is the host-side mirror of the reference interfaces on that path:
  snapshot.HyperGraphSnapshot   the store snapshot (bipartite CSR on the device)
  algorithms                    DefaultALGenerator / HGBreadthFirstTraversal / bfs_batch; LinkPredicate: any tree of
                                hg.and_ / or_ / not_ over the accelerated leaves as a generator's link predicate
                                (include/hgx_linkpred.h); AtomPredicate: a type tree or a per-atom mask as its
                                sibling predicate (include/hgx_sibling.h); BfsResult.sets / reachable_batch ->
                                VisitedSets: the visited sets of many seeds, optionally filtered by an atom
                                predicate, as one CSR built on the device (include/hgx_sets.h)
  query                         hg.and/or/type/incident/orderedLink, GpuAndToQuery, GpuOrToQuery, pattern_batch,
                                pattern_batch_dnf (include/hgx_dnf.h); hg.not_ on its clauses (include/hgx_not.h);
                                opt-in type-index scans of clauses without an anchor: pattern_batch_dnf(...,
                                type_scan=True), GpuScanToQuery (include/hgx_scan.h); hg.apply(hg.targetAt) and
                                the And of such projections on the device: pattern_batch_join, join_parts,
                                GpuMapToQuery (include/hgx_join.h); over every atom, with the atom types set
                                (snapshot.set_atom_types): pattern_batch_atoms, atom_parts -- type scans that
                                deliver node atoms too and a type tree or mask on the projected atoms
                                (include/hgx_atoms.h)
  classics                      GraphClassics.dijkstra / shortest_paths (include/hgx_paths.h);
                                hop_paths -> HopPaths, BfsResult.paths / depths / predecessors: unit-weight
                                shortest paths read out of a batched BFS (include/hgx_hops.h)
"""
from ._lib import HGXError, HGXUnsupported, lib  # noqa: F401
from .algorithms import (AtomPredicate, AtomTypeCondition, BfsResult, DefaultALGenerator, HGBreadthFirstTraversal,  # noqa: F401
                         HopPaths, LinkPredicate, SequenceResult, VisitedSets, bfs_sequence,
                         HGException, bfs_batch, reachable_batch)
from .classics import GraphClassics, LinkWeights, ShortestPathsResult, hop_paths, shortest_paths  # noqa: F401
from .query import (And, ArityCondition, GpuAndToQuery, GpuMapToQuery, GpuOrToQuery, GpuScanToQuery,  # noqa: F401
                    HGQueryConfiguration, LinkCondition, MapCondition, Not, Or, PositionedIncidentCondition, TargetAt,
                    TypePlusCondition, atom_parts, find_all, hg, join_parts, pattern_batch, pattern_batch_atoms, pattern_batch_dnf,
                    pattern_batch_join,
                    to_dnf)
from .snapshot import HyperGraphSnapshot, export_store, rank_handles, read_snapshot, write_snapshot  # noqa: F401

__version__ = "0.1.0"
