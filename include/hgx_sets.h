/*
 * hgx_sets.h -- the visited sets of many seeds of a finished batched BFS in one device pass (an extension of
 * hgx_sibling.h: same conventions -- int status, hgx_last_error, nothing thrown across the ABI, one graph mutex).
 *
 * Reference interface replaced (C = core/src/java/org/hypergraphdb):
 *   hgx_bfs_result_sets   <- the set form of a TraversalBasedQuery over an HGBreadthFirstTraversal and of
 *                            And(cond, BFSCondition) (C/query/impl/TraversalBasedQuery.java; the translation in
 *                            C/query/cond2qry/ToQueryMap.java:282-370), for many start atoms at once: every atom
 *                            the traversal of a start reaches within a depth range, ascending, optionally only
 *                            those that satisfy an atom condition.  With HGX_SETS_COUNT_ONLY: their hg.count.
 *
 * The traversal is not changed.  `where` filters what is REPORTED, not what is expanded: an atom that fails it is
 * still reached, still expanded, and the atoms behind it are still reported.  That is what separates it from the
 * sibling predicate of hgx_bfs_batch_sib, under which such an atom is never reached at all.
 *
 * Results of partition shards hold owned atoms only: hgx_bfs_result_sets refuses them (HGX_E_UNSUPPORTED), as the
 * readers of hgx_hops.h do.
 */
#ifndef HGX_SETS_H
#define HGX_SETS_H

#include "hgx_sibling.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hgx_visited_sets hgx_visited_sets;
#define HGX_SETS_DEPTHS     1   /* keep the depth of every entry */
#define HGX_SETS_COUNT_ONLY 2   /* offsets only: no atoms are written or allocated */

/* Set i = the ascending atoms v with min_depth <= depth_i(v) <= max_depth in the traversal of the seed with index
 * seed_index[i] of r (max_depth HGX_UNBOUNDED: to the last level), and where(v) when where is given.  The sets
 * come in the order of seed_index, as one CSR: offsets plus flat atoms (plus their depths with HGX_SETS_DEPTHS).
 * min_depth == 0 includes the seed itself, still subject to where.  n_sets == 0 is an empty result.
 * Every error is decided on the host before any launch, except the entry cap:
 *   HGX_E_INVALID      null r or out; n_sets < 0; min_depth < 0; max_depth < min_depth and not HGX_UNBOUNDED;
 *                      unknown flag bits; a repeated seed index (the message names both places); where was made
 *                      on another snapshot;
 *   HGX_E_NOTFOUND     a seed index outside the result;
 *   HGX_E_UNSUPPORTED  r is the result of a partition shard;
 *   HGX_E_NOMEM        max_entries >= 0 and the counted total exceeds it (max_entries < 0: no cap): decided after
 *                      the count pass and before anything is written, no object is made, r stays usable, and the
 *                      message names the total so that the caller can page by seeds.
 * where is referenced for the duration of the call only: the object copies what it needs.  The object stays on the
 * device of r's graph until it is read; it must be freed before r and before the graph. */
int  hgx_bfs_result_sets(hgx_bfs_result *r, const int32_t *seed_index, int32_t n_sets,
                         int32_t min_depth, int32_t max_depth /* HGX_UNBOUNDED: to the last level */,
                         const hgx_atom_predicate *where /* may be NULL */, uint32_t flags,
                         int64_t max_entries /* < 0: no cap */, hgx_visited_sets **out);
/* total = the entries of all sets.  Any output may be NULL. */
int  hgx_visited_sets_info(const hgx_visited_sets *s, int32_t *n_sets, int64_t *total, uint32_t *flags);
/* off[i], off[i + 1]: set i's entries in the flat arrays. */
int  hgx_visited_sets_offsets(const hgx_visited_sets *s, int64_t *off /*[n_sets + 1]*/);
/* Copies the entries [first, first + n) of the flat arrays; entries past total are not written (first > total,
 * first < 0 or n < 0: HGX_E_INVALID).  Either output may be NULL.  HGX_E_INVALID: depths of an object made
 * without HGX_SETS_DEPTHS; any read of a count-only object. */
int  hgx_visited_sets_read(const hgx_visited_sets *s, int64_t first, int64_t n, int32_t *atoms, int32_t *depths);
/* Atom rows loaded and (64-atom tile, level) pairs skipped by the level-bitmap test, both over the count and the
 * write pass; device ms of the passes (timing enabled, hgx_set_timing) and algorithmic bytes.
 * Any output may be NULL. */
int  hgx_visited_sets_stats(const hgx_visited_sets *s, int64_t *rows_read, int64_t *tiles_skipped,
                            double *ms_total, double *bytes);
void hgx_visited_sets_free(hgx_visited_sets *s);

#ifdef __cplusplus
}
#endif
#endif
