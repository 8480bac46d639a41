/*
 * hgx_not.h -- Not over the accelerated leaves on the MI355X pattern engine (an extension of hgx_dnf.h:
 * same conventions -- int status, hgx_last_error, nothing thrown across the ABI, one graph mutex).
 *
 * Reference interface replaced (C = core/src/java/org/hypergraphdb):
 *   hgx_pattern_batch_dnf_not <- a Not inside an And.  ExpressionBasedQuery.toDNF
 *                            (C/query/cond2qry/ExpressionBasedQuery.java:94-167) keeps a Not as an opaque leaf,
 *                            no ConditionToQuery is registered for it, so AndToQuery.getQuery
 *                            (C/query/cond2qry/AndToQuery.java:126-135) puts it into the predicate list and
 *                            wraps the intersection of the clause in a PredicateBasedFilter (:279-294) calling
 *                            Not.satisfies = !negated.satisfies(graph, candidate) (C/query/Not.java:33-36).
 *                            Here: a lane per clause hit evaluates the clause's negations between the clause
 *                            stage and the union, all on the device.
 */
#ifndef HGX_NOT_H
#define HGX_NOT_H

#include "hgx_dnf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Literal kinds: the raw satisfies() of the leaf on the candidate link L (targets t[0..n), type key ty), NOT
 * its query translation.  Operands are ops[op_beg, op_end). */
#define HGX_NOT_TYPE        1  /* ty is one of the operands.  AtomTypeCondition.satisfies (C/query/
                                  AtomTypeCondition.java:121-135) with one operand, TypePlusCondition.satisfies
                                  (C/query/TypePlusCondition.java:63-71) with the base and its subtypes. */
#define HGX_NOT_INCIDENT    2  /* one operand x: some t[i] == x (C/query/IncidentCondition.java:63-76). */
#define HGX_NOT_POSITIONED  3  /* four operands (x, lower, upper, complement), negative bounds count from the
                                  end: false when the bounds leave [0, n) or cross, else x sits at a position
                                  inside [lower, upper] (complement: outside it)
                                  (C/query/PositionedIncidentCondition.java:123-177). */
#define HGX_NOT_ORDERED     4  /* the operands (HGX_ANY_HANDLE = any) are a subsequence pattern of t, matched
                                  greedily left to right (C/query/OrderedLinkCondition.java:92-124).  No operand:
                                  true for every link (TC/query/Queries.java:178-206, [] => true) -- unlike the
                                  positive clause leaf, which compiles to HGQuery.NOP. */
#define HGX_NOT_LINK        5  /* the operands are a duplicate-free set S: the number of POSITIONS i with t[i] in
                                  S equals |S| (C/query/LinkCondition.java:101-140).  For a link without repeated
                                  targets that is "every member of S is a target"; a link that repeats a member
                                  of S counts it twice and fails, and HGX_ANY_HANDLE in S equals no target, so
                                  it fails every link -- as the reference does. */
#define HGX_NOT_ARITY       6  /* one operand k: n == k (C/query/ArityCondition.java:49-67). */

/* hgx_pattern_batch_dnf with negated predicates on the clause hits.  The first thirteen arguments are those
 * of hgx_pattern_batch_dnf (n_clauses = clause_off[n_queries]).  The negation program, clause -> negations ->
 * terms -> literals:
 *   neg_off  [n_clauses + 1]  clause c owns the negations [neg_off[c], neg_off[c+1])      (n_negs = neg_off[n_clauses])
 *   term_off [n_negs + 1]     negation g = Not(P) owns the terms [term_off[g], term_off[g+1]): P in disjunctive
 *                             normal form over literals (And.java:66-76, Or.java:67-78 after pushing every
 *                             inner Not down to a polarity bit)                          (n_terms = term_off[n_negs])
 *   lit_off  [n_terms + 1]    term t owns the literals [lit_off[t], lit_off[t+1])         (n_lits = lit_off[n_terms])
 *   lit      [4 * n_lits]     (kind, polarity, op_beg, op_end) per literal: it holds iff the kind's satisfies
 *                             == (polarity != 0)
 *   ops      [n_ops]          the operands
 * A term holds iff all its literals hold (none: it holds); P holds iff one of its terms holds (none: it does
 * not); a clause hit is delivered iff no P of its clause holds.  Result of query q: the link atoms that at
 * least one of its clauses matches AND keeps, ascending, each once -- the filter of a clause applies before
 * the union, so an id an earlier clause rejects is still delivered by a later clause that keeps it.
 * neg_off == NULL or n_negs == 0: exactly hgx_pattern_batch_dnf.
 * Checked on the host before any launch; the message names the query, the clause and the negation.
 * HGX_E_INVALID: offsets not monotone or not starting at 0, an operand range outside ops or of the wrong
 * length for its kind, an atom id out of range, a repeated member of a HGX_NOT_LINK set, an unknown kind.
 * HGX_E_UNSUPPORTED: more than 64 operands of a HGX_NOT_ORDERED / HGX_NOT_LINK literal or 65536 of a
 * HGX_NOT_TYPE one, a clause hgx_pattern_batch_dnf refuses (no incidence anchor -- a Not is no anchor --
 * or beyond the condition limits), or g is a partition shard.
 * The union statistics (hgx_query_result_union_stats) of such a result count the hits the filter kept. */
int hgx_pattern_batch_dnf_not(hgx_graph *g, int32_t n_queries, const int64_t *clause_off,
                              const int64_t *type_off, const int32_t *types,
                              const int64_t *inc_off, const int32_t *inc,
                              const int64_t *pos_off, const int32_t *pos,
                              const int64_t *pset_off, const int64_t *pat_off, const int32_t *pat,
                              const int32_t *arity,
                              const int64_t *neg_off, const int64_t *term_off, const int64_t *lit_off,
                              const int32_t *lit, const int32_t *ops, int64_t n_ops,
                              hgx_query_result **out);
/* Hits of clauses with a negation the filter tested, those it rejected, device ms of the filter kernels
 * (timing enabled, hgx_set_timing) and their algorithmic bytes.  All zero for a result of
 * another entry point or of a batch without a negation.  Any output may be NULL. */
int hgx_query_result_not_stats(const hgx_query_result *r, int64_t *hits_tested, int64_t *hits_rejected,
                               double *ms_not, double *bytes_not);

#ifdef __cplusplus
}
#endif
#endif
