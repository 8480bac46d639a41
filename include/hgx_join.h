/*
 * hgx_join.h -- from link atoms to the atoms they connect on the MI355X pattern engine: the hits of a DNF query
 * projected to a target position and the projections of several queries intersected on the device
 * (an extension of hgx_scan.h: same conventions -- int status, hgx_last_error, nothing thrown across the ABI,
 * one graph mutex).
 *
 * Reference interface replaced (C = core/src/java/org/hypergraphdb, TC = testcore/test/java/hgtest):
 *   hgx_pattern_batch_join <- hg.apply(hg.targetAt(graph, i), cond) (C/HGQuery.java:1167-1222): a MapCondition
 *                            that ToQueryMap compiles to a ResultMapQuery over the query of cond
 *                            (C/query/cond2qry/ToQueryMap.java:409-427), whose mapping is a deref followed by
 *                            LinkProjectionMapping.eval = link.getTargetAt(i) (C/query/impl/
 *                            LinkProjectionMapping.java:33-36); and the And of such conditions, the reference's
 *                            own pattern test: and(apply(targetAt(0), orderedLink(ANY, A)),
 *                            apply(targetAt(0), orderedLink(ANY, B))) == {C1, C4}
 *                            (TC/query/PatternTests.java:20-61).
 *                            Here: one more stage behind the union of hgx_pattern_batch_dnf_scan keys every hit
 *                            with (part, projected atom), sorts the keys and keeps the values of the smallest
 *                            part that every other part of the join query holds.
 *
 * DEVIATIONS FROM THE REFERENCE, both documented and tested:
 *   - Order and duplicates.  ResultMapQuery maps the inner result set element by element: it delivers a value
 *     once per link that projects to it, in the inner query's order, and ToQueryMap.java:417-426 declares the
 *     result neither ordered nor random-access.  This engine delivers the SET of values, ascending, each atom
 *     once -- what find_all has always returned for a MapCondition.
 *   - A position beyond a link's arity.  LinkProjectionMapping.eval calls getTargetAt(i), which indexes the
 *     link's target array (HGPlainLink.getTargetAt: outgoingSet[i]) and so throws
 *     ArrayIndexOutOfBoundsException out of the result set.  Here a link too short for the position contributes
 *     nothing (the rule of the Python mirror's TargetAt).
 */
#ifndef HGX_JOIN_H
#define HGX_JOIN_H

#include "hgx_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HGX_JOIN_SELF (-1)        /* part_pos: the link atom itself, no projection */
#define HGX_JOIN_TYPE_SCAN 1      /* flags: take anchor-free clauses as hgx_pattern_batch_dnf_scan does */

/* n_queries join queries over n_parts = part_off[n_queries] parts.  Join query j owns the parts
 * [part_off[j], part_off[j+1]).  Part s is exactly one query of hgx_pattern_batch_dnf_scan: its clauses are
 * [clause_off[s], clause_off[s+1]) of the arrays that follow (clause_off has n_parts + 1 entries), negations
 * included; the five negation arrays may be NULL (no negation in the batch).
 *   U_s       = the part's DNF result (link atoms),
 *   value(s)  = { targets(L)[p] : L in U_s, arity(L) > p }   with p = part_pos[s] >= 0
 *             = U_s                                           with p == HGX_JOIN_SELF,
 *   result(j) = the intersection of value(s) over the parts of j, ascending, each atom once.
 * One part gives the projection alone; no parts give an empty result.  A link too short for p contributes
 * nothing (see the deviations above).  The result is read with the hgx_query_result_* readers: n_queries + 1
 * offsets, ids that are ATOMS (nodes or links), no longer link atoms only.  hgx_query_result_union_stats,
 * _not_stats and _scan_stats of the result describe the parts' DNF evaluation as for hgx_pattern_batch_dnf_scan
 * (kept = the summed sizes of the U_s).
 * flags: 0, or HGX_JOIN_TYPE_SCAN.  Without the flag a clause without an incidence anchor is refused as by
 * hgx_pattern_batch_dnf_not; with it the opt-in rule of hgx_scan.h carries over unchanged (a scanned clause
 * delivers the LINK atoms of its type).  No other entry point routes here.
 * Checked on the host before any launch; the message names the join query and the part.
 * HGX_E_INVALID: part_off does not start at 0 or decreases, part_pos < -1, an unknown flag, whatever
 * hgx_pattern_batch_dnf_scan rejects.
 * HGX_E_UNSUPPORTED: what hgx_pattern_batch_dnf_not refuses (an anchor-free clause without HGX_JOIN_TYPE_SCAN
 * among it), the limits of hgx_pattern_batch_dnf_scan, or g is a partition shard.
 * The graph mutex, execution contexts, hgx_set_timing and the rerun after a workspace overflow behave as for a
 * DNF batch: one synchronisation per batch, and the hits never cross the host link before the join. */
int hgx_pattern_batch_join(hgx_graph *g, int32_t n_queries, const int64_t *part_off, const int32_t *part_pos,
                           const int64_t *clause_off,
                           const int64_t *type_off, const int32_t *types,
                           const int64_t *inc_off, const int32_t *inc,
                           const int64_t *pos_off, const int32_t *pos,
                           const int64_t *pset_off, const int64_t *pat_off, const int32_t *pat,
                           const int32_t *arity,
                           const int64_t *neg_off, const int64_t *term_off, const int64_t *lit_off,
                           const int32_t *lit, const int32_t *ops, int64_t n_ops,
                           int32_t flags, hgx_query_result **out);
/* The parts of the batch, the hits projected (the summed sizes of the parts' DNF results), the distinct values
 * of the parts (summed over the parts, a missing position not counted), the ids kept (the result's total),
 * device ms of the join stage (timing enabled, hgx_set_timing) and its algorithmic bytes.
 * All zero for a result of another entry point.  Any output may be NULL. */
int hgx_query_result_join_stats(const hgx_query_result *r, int64_t *parts, int64_t *hits_projected,
                                int64_t *values_distinct, int64_t *kept, double *ms_join, double *bytes_join);

#ifdef __cplusplus
}
#endif
#endif
