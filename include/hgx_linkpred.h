/*
 * hgx_linkpred.h -- traversals over any accelerated link predicate (an extension of hgx_not.h, hgx_paths.h and
 * hgx_hops.h: same conventions -- int status, hgx_last_error, nothing thrown across the ABI, one graph mutex).
 *
 * Reference interface replaced (C = core/src/java/org/hypergraphdb):
 *   hgx_link_predicate         <- the linkPredicate of a DefaultALGenerator, any HGAtomPredicate: generate()
 *                                 calls linkPredicate.satisfies(graph, link) once per incident link and nothing
 *                                 else (C/algorithms/DefaultALGenerator.java:300-308).  Here the predicate is a
 *                                 tree of And / Or / Not over the leaves whose raw satisfies hgx_not.h restates
 *                                 (AtomTypeCondition.java:121-135, TypePlusCondition.java:63-71,
 *                                 IncidentCondition.java:63-76, PositionedIncidentCondition.java:123-177,
 *                                 OrderedLinkCondition.java:92-124, LinkCondition.java:101-140,
 *                                 ArityCondition.java:49-67; And.java:66-76, Or.java:67-78, Not.java:33-36),
 *                                 lowered by the host to disjunctive normal form.  A link predicate is a
 *                                 property of the link row alone: it is evaluated once per link row on the
 *                                 device when the object is made, and every traversal streams the flags
 *                                 (DESIGN.md 3.8).
 *   hgx_bfs_batch_pred, hgx_bfs_sequence_pred, hgx_shortest_paths_pred
 *                              <- the traversals of hgx.h / hgx_paths.h with such a generator.
 *
 * A siblingPredicate goes through hgx_sibling.h (the types of node atoms are an optional column there).  Not
 * accelerated: partition shards (hgx_pbfs_batch keeps the single link type).
 */
#ifndef HGX_LINKPRED_H
#define HGX_LINKPRED_H

#include "hgx_hops.h"
#include "hgx_not.h"
#include "hgx_paths.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hgx_link_predicate hgx_link_predicate;   /* evaluated, device-resident, reusable, reference counted */

/* The predicate P in disjunctive normal form over the literals of hgx_not.h -- the inside of one negation of
 * hgx_pattern_batch_dnf_not, without the outer Not:
 *   lit_off [n_terms + 1]  term t owns the literals [lit_off[t], lit_off[t+1])     (n_lits = lit_off[n_terms])
 *   lit     [4 * n_lits]   (kind, polarity, op_beg, op_end): the literal holds iff the kind's satisfies == (polarity != 0)
 *   ops     [n_ops]        the operands
 * A term holds iff all its literals hold (none: it holds); P holds iff one of its terms holds.  n_terms == 0: P
 * is false on every link (lit_off may be NULL); an empty term: P is true on every link.
 * Evaluates P on every link row of g's snapshot (g may be one of its execution contexts).  The object holds a
 * reference on the snapshot: while it lives, hgx_graph_update is refused.
 * Checked on the host before any launch, as hgx_pattern_batch_dnf_not checks a negation program; the message
 * names the term and the literal.  HGX_E_INVALID: offsets not monotone or not starting at 0, an operand range
 * outside ops or of the wrong length for its kind, an atom id out of range, a repeated member of a HGX_NOT_LINK
 * set, an unknown kind.  HGX_E_UNSUPPORTED: more than 64 operands of a HGX_NOT_ORDERED / HGX_NOT_LINK literal or
 * 65536 of a HGX_NOT_TYPE one, or g is a partition shard. */
int  hgx_link_predicate_create(hgx_graph *g, int64_t n_terms, const int64_t *lit_off, const int32_t *lit,
                               const int32_t *ops, int64_t n_ops, hgx_link_predicate **out);
/* Drops the caller's handle.  Results made with the predicate hold references of their own, so freeing it
 * before them is legal; its device memory goes with the last reference. */
void hgx_link_predicate_free(hgx_link_predicate *p);
/* Link rows, rows that satisfy P (counted on the device), device ms of the evaluation and projection kernels
 * (timing enabled, hgx_set_timing) and their algorithmic bytes.  Any output may be NULL. */
int  hgx_link_predicate_info(const hgx_link_predicate *p, int64_t *num_links, int64_t *num_satisfied,
                             double *ms_eval, double *bytes_eval);
/* out[i] = 1 iff link row first + i satisfies P, else 0, for i in [0, n).  Rows outside [0, num_links):
 * HGX_E_INVALID. */
int  hgx_link_predicate_flags(hgx_link_predicate *p, int64_t first, int64_t n, uint8_t *out);

/* hgx_bfs_batch / hgx_bfs_sequence / hgx_shortest_paths with the link predicate p: generate() follows exactly
 * the incident links that satisfy P (DefaultALGenerator.java:300-308).  p == NULL: exactly the entry point
 * without _pred.  Otherwise opts->link_type must be HGX_NO_TYPE (a type belongs inside P; anything else is
 * HGX_E_INVALID) and p must have been made on g's snapshot (g: the snapshot or one of its contexts; any other
 * graph is HGX_E_INVALID).  The results are ordinary results: every reader of hgx.h, hgx_paths.h and hgx_hops.h
 * works on them, and each holds a reference on p. */
int  hgx_bfs_batch_pred(hgx_graph *g, const int32_t *seeds, int32_t n_seeds, int32_t max_depth,
                        const hgx_algen_opts *opts, hgx_link_predicate *p, hgx_bfs_result **out);
int  hgx_bfs_sequence_pred(hgx_graph *g, const int32_t *seeds, int32_t n_seeds, int32_t max_depth,
                           const hgx_algen_opts *opts, hgx_link_predicate *p, hgx_seq_result **out);
int  hgx_shortest_paths_pred(hgx_graph *g, const int32_t *starts, const int32_t *goals, int32_t n_pairs,
                             const hgx_algen_opts *opts, const hgx_link_weights *w, hgx_link_predicate *p,
                             hgx_sp_result **out);

#ifdef __cplusplus
}
#endif
#endif
