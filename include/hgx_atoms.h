/*
 * hgx_atoms.h -- the pattern path over every atom: type scans that deliver node atoms as well as link atoms, and
 * a type (or any per-atom) condition on the atoms a join projects to (an extension of hgx_join.h and
 * hgx_sibling.h: same conventions -- int status, hgx_last_error, nothing thrown across the ABI, one graph mutex).
 *
 * Reference interface replaced (C = core/src/java/org/hypergraphdb):
 *   hgx_pattern_batch_atoms with HGX_ATOMS_TYPE_SCAN
 *                            <- a scan of indexByType.find(T) over ALL atoms of the type, wrapped in one
 *                               PredicateBasedFilter per remaining condition (C/query/cond2qry/AndToQuery.java:
 *                               120-294).  hgx_scan.h delivers the LINK atoms of T only; here the scan runs over an
 *                               index of every atom keyed by the atom-type column (hgx_graph_set_atom_types).
 *   hgx_pattern_batch_atoms with keep
 *                            <- and(type(Person), apply(targetAt(g, 1), and(type(Knows), orderedLink(a, ANY)))):
 *                               a condition on the projected atom next to the projections of hgx_join.h.  Any
 *                               hgx_atom_predicate serves (a type tree or a per-atom mask).
 *
 * NODE ATOMS UNDER THE ACCELERATED LEAVES take the reference's own satisfies rules:
 *   - arity(k) holds iff k == 0 (ArityCondition.java:54-55);
 *   - incident, incidentAt / incidentNotAt, orderedLink and link are false (IncidentCondition.java:71-75,
 *     PositionedIncidentCondition.java:134-135, OrderedLinkCondition.java:100-101, LinkCondition.java:119-120):
 *     a node's store record has no targets;
 *   - this includes an EMPTY orderedLink() / link() under a Not.  The negation validator (hgx_not.h) accepts
 *     empty patterns under a Not, and on a link without targets they hold, so a node is NOT an arity-0 link: the
 *     atom index marks its node records and the scan evaluates the negations of a node by the rules above;
 *   - a positive clause keeps the rules of hgx_scan.h: an all-ANY pattern of length m > 0 needs arity >= m (a
 *     node fails it), arity(0) keeps the nodes, an empty pattern makes the clause a NOP;
 *   - a node atom projected to a position >= 0 contributes nothing: the deviation hgx_join.h documents for a
 *     link too short for the position, extended to atoms without targets.
 *
 * ONE DIFFERENCE FROM hgx_scan.h: a link row without a type (link_type < 0) is indexed under its atom_type, so a
 * scan of that type delivers it here; anchored clauses are unchanged (they compare link_type).
 *
 * Cost: the atom index is 16 bytes per atom of device memory, built on the first use and dropped whenever the
 * atom-type column changes (hgx_graph_set_atom_types, hgx_graph_update).  Not accelerated: partition shards.
 */
#ifndef HGX_ATOMS_H
#define HGX_ATOMS_H

#include "hgx_join.h"
#include "hgx_sibling.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HGX_ATOMS_TYPE_SCAN 1     /* flags: scan anchor-free clauses over the atom index (nodes and links) */

/* out_counts[i] = the atoms, nodes and links, whose type key is types[i] (0 for an absent key), from the
 * histogram of the atom index (built when absent).  HGX_E_UNSUPPORTED: the snapshot has no atom-type column, or
 * g is a partition shard. */
int hgx_graph_type_atoms(hgx_graph *g, const int32_t *types, int64_t n, int64_t *out_counts);

/* hgx_pattern_batch_join with two additions.
 * keep: NULL, or n_queries pointers, each NULL or an atom predicate made on g's snapshot (g: the snapshot or one
 *   of its contexts; a predicate of another graph is HGX_E_INVALID, the message names the join query).
 *   result(j) is additionally restricted to the atoms whose bit is set in keep[j]; a query without parts stays
 *   empty.  One predicate may serve many queries.  The bits are read before the call returns: the result holds
 *   no reference on the predicate.  A mask predicate needs no atom-type column.
 * flags: 0 or HGX_ATOMS_TYPE_SCAN.  With the flag a clause without an incidence anchor and with exactly one type
 *   T is scanned over the ATOM index: its result is every atom of type T that passes the clause, node atoms
 *   included, ascending (the node rules above).  Without the flag such a clause is refused as by
 *   hgx_pattern_batch_dnf_not.  With the flag and no atom-type column: HGX_E_UNSUPPORTED.  An unknown flag:
 *   HGX_E_INVALID.
 * With keep == NULL and flags == 0 the call is exactly hgx_pattern_batch_join: same result, same launches, same
 * statistics.  Every other check, status and behaviour (execution contexts, which borrow the snapshot's index;
 * the rerun after a workspace overflow; HGX_E_UNSUPPORTED on a partition shard) is that of hgx_pattern_batch_join.
 * hgx_query_result_scan_stats of the result counts atom-index rows in rows_scanned; in
 * hgx_query_result_join_stats values_distinct is counted before the filter and kept after it. */
int hgx_pattern_batch_atoms(hgx_graph *g, int32_t n_queries, const int64_t *part_off, const int32_t *part_pos,
                            hgx_atom_predicate *const *keep,
                            const int64_t *clause_off,
                            const int64_t *type_off, const int32_t *types,
                            const int64_t *inc_off, const int32_t *inc,
                            const int64_t *pos_off, const int32_t *pos,
                            const int64_t *pset_off, const int64_t *pat_off, const int32_t *pat,
                            const int32_t *arity,
                            const int64_t *neg_off, const int64_t *term_off, const int64_t *lit_off,
                            const int32_t *lit, const int32_t *ops, int64_t n_ops,
                            int32_t flags, hgx_query_result **out);

/* The join queries that carry a predicate, the values whose bit was tested (the distinct values of the driver
 * part of those queries), the values the bit rejected, device ms of the join's keep kernel, which holds the
 * filter (timing enabled, hgx_set_timing), and the filter's algorithmic bytes.  All zero for a
 * result of another entry point, and for a batch without a predicate.  Any output may be NULL. */
int hgx_query_result_atoms_stats(const hgx_query_result *r, int64_t *queries_filtered, int64_t *values_tested,
                                 int64_t *values_rejected, double *ms_filter, double *bytes_filter);

#ifdef __cplusplus
}
#endif
#endif
