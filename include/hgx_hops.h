/*
 * hgx_hops.h -- shortest hop paths and predecessor rows read out of a finished batched BFS (an extension of
 * hgx.h: same conventions -- int status, hgx_last_error, nothing thrown across the ABI, one graph mutex).
 *
 * Reference interface replaced (C = core/src/java/org/hypergraphdb):
 *   hgx_bfs_result_paths            <- GraphClassics.dijkstra(start, goal, HGALGenerator), the "simplified
 *                                      interface" in which every link weighs 1.0 (C/algorithms/GraphClassics.java:80-83),
 *                                      which runs the general algorithm (GraphClassics.java:126-209), for many
 *                                      (start, goal) pairs at once;
 *   hgx_bfs_result_depth_row        <- its distanceMatrix (GraphClassics.java:133-135,191) of one start;
 *   hgx_bfs_result_predecessor_row  <- its predecessorMatrix (GraphClassics.java:193-194,202-203) of one start.
 *
 * With unit weights the distance of an atom is its BFS depth, and every relaxation is strictly inflationary,
 * so rule R of hgx_paths.h is exactly the reference's final predecessorMatrix entry.  It then reads: the
 * predecessor of n at depth d >= 1 is the lowest-rank atom a != n of level d - 1 (of the same seed) whose
 * generate(a) yields n; the reported link is the lowest link atom among a's qualifying links to n.  The
 * generator (mode, link type) is the one the BFS result was made with.
 *
 * Results of partition shards hold owned atoms only: every reader here refuses them (HGX_E_UNSUPPORTED).
 */
#ifndef HGX_HOPS_H
#define HGX_HOPS_H

#include "hgx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hgx_hop_paths hgx_hop_paths;

/* For every i: the shortest hop path from the seed with index seed_index[i] of r to goal[i] -- what
 * GraphClassics.dijkstra(seed, goal, gen) (GraphClassics.java:80-83,126-209) returns with the default weight,
 * with rule R predecessors (hgx_paths.h).  A goal that r did not reach (not connected, or beyond r's
 * max_depth) has hops -1.  goal == seed: hops 0, path {seed}.  n_pairs == 0 is an empty result.
 * goal outside [0, num_atoms): HGX_E_INVALID; seed_index outside the result: HGX_E_NOTFOUND. */
int  hgx_bfs_result_paths(hgx_bfs_result *r, const int32_t *seed_index, const int32_t *goal, int32_t n_pairs,
                          hgx_hop_paths **out);
/* total_atoms = the atoms of all paths (hops + 1 of every reached pair). */
int  hgx_hop_paths_info(const hgx_hop_paths *p, int32_t *n_pairs, int64_t *total_atoms);
/* hops[i] (-1: not reached); off[i], off[i + 1]: pair i's atoms in the flat atom array (hops + 1 atoms; its
 * hops links start at off[i] - the reached pairs before i).  Either may be NULL. */
int  hgx_hop_paths_offsets(const hgx_hop_paths *p, int64_t *off /*[n_pairs + 1]*/, int32_t *hops /*[n_pairs]*/);
/* atoms: start .. goal per pair (total_atoms); links: per pair links[k] joins atoms[k] and atoms[k + 1]
 * (flat, total_atoms - reached pairs).  Following predecessorMatrix from the goal (GraphClassics.java:120-122).
 * Either may be NULL. */
int  hgx_hop_paths_read(const hgx_hop_paths *p, int32_t *atoms, int32_t *links);
/* Step launches of the backtrace, incidence entries walked, membership probes (level-bitmap words or table
 * searches), device ms (timing enabled, hgx_set_timing) and algorithmic bytes.  Any output
 * may be NULL. */
int  hgx_hop_paths_stats(const hgx_hop_paths *p, int64_t *steps, int64_t *entries, int64_t *probes,
                         double *ms_total, double *bytes);
void hgx_hop_paths_free(hgx_hop_paths *p);

/* distanceMatrix / predecessorMatrix rows of one seed over the atoms [first, first + n)
 * (GraphClassics.java:133-135,191-194): depth -1 = not reached; predecessor -1 for the seed and for
 * unreached atoms.  The rows of the last seed asked for stay on the result until it is freed. */
int  hgx_bfs_result_depth_row(hgx_bfs_result *r, int32_t seed_index, int64_t first, int64_t n, int32_t *depth);
int  hgx_bfs_result_predecessor_row(hgx_bfs_result *r, int32_t seed_index, int64_t first, int64_t n,
                                    int32_t *pred_atom, int32_t *pred_link);

#ifdef __cplusplus
}
#endif
#endif
