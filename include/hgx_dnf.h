/*
 * hgx_dnf.h -- Or over the accelerated And shapes on the MI355X pattern engine (an extension of hgx.h:
 * same conventions -- int status, hgx_last_error, nothing thrown across the ABI, one graph mutex).
 *
 * Reference interface replaced (C = core/src/java/org/hypergraphdb):
 *   hgx_pattern_batch_dnf <- ExpressionBasedQuery compiling simplify(toDNF(expand(cond)))
 *                            (C/query/cond2qry/ExpressionBasedQuery.java:863, toDNF :94-167): every And / Or
 *                            tree becomes an Or of Ands; OrToQuery (C/query/cond2qry/OrToQuery.java:14-43)
 *                            chains UnionResults (C/query/impl/UnionResult.java): an ordered union without
 *                            duplicates.  The clauses are the Ands hgx_pattern_batch_ext accelerates; the
 *                            union runs on the device, the clause hits never reach the host.
 */
#ifndef HGX_DNF_H
#define HGX_DNF_H

#include "hgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Query q = Or over the clauses [clause_off[q], clause_off[q+1]); clause c is exactly one query of
 * hgx_pattern_batch_ext (the same arrays, indexed by clause: type_off/types, inc_off/inc, pos_off/pos,
 * pset_off/pat_off/pat, arity; n_clauses = clause_off[n_queries], clause_off[0] = 0).  Result of q: the
 * link atoms matched by at least one of its clauses, ascending, each once.  A query with no clauses has an
 * empty result (OrToQuery: HGQuery.NOP).  The result is read with the hgx_query_result_* readers of hgx.h
 * (n_queries offsets + 1).
 * HGX_E_INVALID: an id out of range, clause_off not monotone or not starting at 0.  HGX_E_UNSUPPORTED: a
 * clause without an incidence anchor or beyond the condition limits, or g is a partition shard.  The
 * message names the query and the clause.  The call takes the graph mutex itself (it does not go through
 * the cross-thread coalescer of hgx_pattern_batch_packed); execution contexts (hgx_graph_context) work. */
int hgx_pattern_batch_dnf(hgx_graph *g, int32_t n_queries, const int64_t *clause_off,
                          const int64_t *type_off, const int32_t *types,
                          const int64_t *inc_off, const int32_t *inc,
                          const int64_t *pos_off, const int32_t *pos,
                          const int64_t *pset_off, const int64_t *pat_off, const int32_t *pat,
                          const int32_t *arity, hgx_query_result **out);
/* Clause hits before the union, ids kept by it, device ms of the union kernels (timing enabled,
 * hgx_set_timing) and their algorithmic bytes.  All zero for a result of another entry
 * point.  Any output may be NULL. */
int hgx_query_result_union_stats(const hgx_query_result *r, int64_t *clause_hits, int64_t *kept,
                                 double *ms_union, double *bytes_union);

#ifdef __cplusplus
}
#endif
#endif
