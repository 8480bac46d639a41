/*
 * hgx_sibling.h -- batched traversals with a sibling predicate (an extension of hgx_linkpred.h: same conventions
 * -- int status, hgx_last_error, nothing thrown across the ABI, one graph mutex).
 *
 * Reference interface replaced (C = core/src/java/org/hypergraphdb):
 *   hgx_atom_predicate         <- the siblingPredicate of a DefaultALGenerator, any HGAtomPredicate: the iterator
 *                                 yields the adjacency list of generate(src) without every target h for which
 *                                 siblingPredicate.satisfies(graph, h) is false, the focus atom under returnSource
 *                                 included (C/algorithms/DefaultALGenerator.java:120-150, 207-237; call sites
 *                                 156-157, 188-189, 251-252, 272-273).  An element-wise filter of the adjacency
 *                                 list: the start atom is never tested, an atom that fails is never reached and
 *                                 so never expanded.  A sibling predicate is a property of the atom alone: it is
 *                                 evaluated once per atom when the object is made, one bit an atom, and every
 *                                 traversal reads the bits.
 *   hgx_bfs_batch_sib, hgx_shortest_paths_sib
 *                              <- the traversals of hgx.h / hgx_paths.h with such a generator.
 *
 * Not accelerated with a sibling predicate: the order-exact sequence (hgx_bfs_sequence*), partition shards and the
 * JNI shim.  (Node atoms in type scans read the atom-type column of this header through hgx_atoms.h.)
 */
#ifndef HGX_SIBLING_H
#define HGX_SIBLING_H

#include "hgx_linkpred.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hgx_atom_predicate hgx_atom_predicate;   /* evaluated, device-resident, reusable, reference counted */

/* The type key of every atom of the snapshot g, link atoms and node atoms alike: an optional device-resident
 * column next to link_type, deep-copied from atom_type[num_atoms]; a second call replaces it, NULL drops it.
 * hgx_graph_update drops the column (the id space may have grown): the caller sets it again afterwards.  The
 * .hgcsr file does not hold it.
 * HGX_E_INVALID: g is an execution context, a value is negative, atom_type[link_atom[r]] differs from the stored
 * link_type[r] of a link row r that has a type (link_type[r] >= 0; the message names the row), or an atom
 * predicate made from the column (hgx_atom_predicate_create) is alive.  HGX_E_UNSUPPORTED: a partition shard. */
int  hgx_graph_set_atom_types(hgx_graph *g, const int32_t *atom_type);

/* The predicate P over the atoms in the disjunctive normal form of hgx_link_predicate_create, restricted to
 * HGX_NOT_TYPE literals (type / typePlus with either polarity: every And / Or / Not tree over hg.type /
 * hg.typePlus), evaluated on the device against the atom-type column of g's snapshot (g may be one of its
 * contexts).  n_terms == 0: P is false on every atom; an empty term: P is true on every atom.
 * The object holds a reference on the snapshot: while it lives, hgx_graph_update is refused.
 * Checked on the host before any launch as hgx_link_predicate_create checks its program (same statuses; the
 * message names the term and the literal).  HGX_E_UNSUPPORTED: a literal of any other kind (on a node atom those
 * leaves have rules of their own in the reference, e.g. ArityCondition.java:54-55; evaluate them per atom and
 * use hgx_atom_predicate_create_mask), no atom-type column, or g is a partition shard. */
int  hgx_atom_predicate_create(hgx_graph *g, int64_t n_terms, const int64_t *lit_off, const int32_t *lit,
                               const int32_t *ops, int64_t n_ops, hgx_atom_predicate **out);
/* Any HGAtomPredicate the caller evaluated once per atom: keep[a] != 0 iff atom a satisfies it
 * (keep[num_atoms]).  Needs no atom-type column.  HGX_E_UNSUPPORTED: g is a partition shard. */
int  hgx_atom_predicate_create_mask(hgx_graph *g, const uint8_t *keep, hgx_atom_predicate **out);
/* Drops the caller's handle.  Results made with the predicate hold references of their own, so freeing it
 * before them is legal; its device memory goes with the last reference. */
void hgx_atom_predicate_free(hgx_atom_predicate *p);
/* Atoms, atoms that satisfy P (counted on the device), device ms of the evaluation kernel (timing enabled,
 * hgx_set_timing) and its algorithmic bytes.  Any output may be NULL. */
int  hgx_atom_predicate_info(const hgx_atom_predicate *p, int64_t *num_atoms, int64_t *num_kept, double *ms_eval,
                             double *bytes_eval);
/* out[i] = 1 iff atom first + i satisfies P, else 0, for i in [0, n).  Atoms outside [0, num_atoms):
 * HGX_E_INVALID. */
int  hgx_atom_predicate_flags(hgx_atom_predicate *p, int64_t first, int64_t n, uint8_t *out);

/* hgx_bfs_batch_pred / hgx_shortest_paths_pred with the sibling predicate ap: a target that fails it is never
 * yielded.  The start atoms are not tested; a start that fails is still expanded, and no other traversal of the
 * batch reaches it.  ap == NULL: exactly the _pred entry point (link_pred may be NULL as there).  ap must have
 * been made on g's snapshot (g: the snapshot or one of its contexts; any other graph is HGX_E_INVALID).  The
 * results are ordinary results: every reader of hgx.h, hgx_paths.h and hgx_hops.h works on them, and each holds
 * a reference on ap.  HGX_E_UNSUPPORTED: g is a partition shard. */
int  hgx_bfs_batch_sib(hgx_graph *g, const int32_t *seeds, int32_t n_seeds, int32_t max_depth,
                       const hgx_algen_opts *opts, hgx_link_predicate *link_pred, hgx_atom_predicate *ap,
                       hgx_bfs_result **out);
int  hgx_shortest_paths_sib(hgx_graph *g, const int32_t *starts, const int32_t *goals, int32_t n_pairs,
                            const hgx_algen_opts *opts, const hgx_link_weights *w, hgx_link_predicate *link_pred,
                            hgx_atom_predicate *ap, hgx_sp_result **out);

#ifdef __cplusplus
}
#endif
#endif
