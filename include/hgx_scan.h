/*
 * hgx_scan.h -- clauses without an incidence anchor on the MI355X pattern engine: a scan of the type index
 * (an extension of hgx_not.h: same conventions -- int status, hgx_last_error, nothing thrown across the ABI,
 * one graph mutex).
 *
 * Reference interface replaced (C = core/src/java/org/hypergraphdb):
 *   hgx_pattern_batch_dnf_scan <- an And whose only ordered set is a type condition.  AndToQuery.getQuery
 *                            (C/query/cond2qry/AndToQuery.java:120-294) then scans indexByType.find(T) and
 *                            wraps the scan in one PredicateBasedFilter per remaining condition (:279-294);
 *                            with neither an ordered set nor a type it throws "No query condition translatable
 *                            into a scannable result set" (:262-263).  TypePlusCondition reaches it as an Or of
 *                            AtomTypeConditions (C/query/cond2qry/ExpressionBasedQuery.java:606-627) that toDNF
 *                            distributes, so a clause has one type.
 *                            Here: a wave per 64 entries of the type's segment of a device type index tests
 *                            the predicates and compacts the rows that pass in order.
 *   hgx_graph_type_links   <- the size of indexByType.find(T) a ConditionToQuery.getMetaData reports as
 *                            sizeExpected (C/query/cond2qry/QueryMetaData.java).
 *
 * THE SNAPSHOT KNOWS THE TYPES OF LINK ATOMS ONLY (hgx_graph_desc.link_type).  The result of a scanned clause
 * is the LINK atoms of the type that pass the predicates; indexByType.find(T) also returns node atoms of type
 * T.  The two are equal whenever T has no node instances, and the caller opts in knowing that: no other entry
 * point routes a clause to the scan (hgx_pattern_batch* and hgx_pattern_batch_dnf* keep returning
 * HGX_E_UNSUPPORTED for a clause without an anchor).
 */
#ifndef HGX_SCAN_H
#define HGX_SCAN_H

#include "hgx_not.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hgx_pattern_batch_dnf_not that also takes clauses without an incidence anchor.  The arguments are those of
 * hgx_pattern_batch_dnf_not; the five negation arrays may be NULL (no negation in the batch).
 * A clause is SCANNED when it has no incidence anchor (no incident target, no positioned target, no non-ANY
 * pattern target) and exactly one type T.  Its result: the link atoms L with link_type[L] == T for which
 *   - arity(L) == arity[c] when that is >= 0,
 *   - arity(L) >= m for every ordered pattern of length m > 0 (all its entries are HGX_ANY_HANDLE: the greedy
 *     subsequence match of C/query/OrderedLinkCondition.java:92-124),
 *   - no Not(P) of the clause holds (hgx_not.h),
 * ascending.  An empty ordered pattern makes the clause a NOP (HGQuery.NOP), as on the anchored path.  Every
 * other clause is evaluated as by hgx_pattern_batch_dnf_not; the runs of both kinds are united per query,
 * each link atom once.  A batch without a scanned clause is exactly hgx_pattern_batch_dnf_not: the same
 * launches and statistics.
 * Checked on the host before any launch; the message names the query and the clause.
 * HGX_E_INVALID: what hgx_pattern_batch_dnf_not rejects, a negative type key.
 * HGX_E_UNSUPPORTED: a clause with neither an anchor nor a type, a clause without an anchor and with more
 * than one type (split it into one clause per type), the limits of hgx_pattern_batch_dnf_not, or g is a
 * partition shard.
 * The first scanned batch builds the type index of the snapshot (16 bytes per link; execution contexts share
 * it, hgx_graph_update drops it). */
int hgx_pattern_batch_dnf_scan(hgx_graph *g, int32_t n_queries, const int64_t *clause_off,
                               const int64_t *type_off, const int32_t *types,
                               const int64_t *inc_off, const int32_t *inc,
                               const int64_t *pos_off, const int32_t *pos,
                               const int64_t *pset_off, const int64_t *pat_off, const int32_t *pat,
                               const int32_t *arity,
                               const int64_t *neg_off, const int64_t *term_off, const int64_t *lit_off,
                               const int32_t *lit, const int32_t *ops, int64_t n_ops,
                               hgx_query_result **out);
/* The scanned clauses of the batch (NOP clauses and absent types included), the index rows they covered (the
 * sum of the segment lengths of the scanned clauses that are no NOP), the rows that passed (the scan's hits
 * before the union), device ms of the scan stage (timing enabled, hgx_set_timing) and its algorithmic bytes
 * (DESIGN.md 3.6.2).  All zero for a result of another entry point or of a batch without a scanned clause.
 * Any output may be NULL.  hgx_query_result_not_stats of such a result counts the hits of anchored clauses
 * only: a scanned row is tested by the scan, never by the filter; hgx_query_result_union_stats counts the
 * hits of both kinds. */
int hgx_query_result_scan_stats(const hgx_query_result *r, int64_t *clauses_scanned, int64_t *rows_scanned,
                                int64_t *rows_kept, double *ms_scan, double *bytes_scan);
/* out_counts[i] = the number of link atoms of type key types[i] (0 for an absent or negative key), from the
 * histogram of the type index (built when absent). */
int hgx_graph_type_links(hgx_graph *g, const int32_t *types, int64_t n, int64_t *out_counts);

#ifdef __cplusplus
}
#endif
#endif
