/*
 * hgx_paths.h -- batched weighted shortest paths on the MI355X engine (an extension of hgx.h: same
 * conventions -- int status, hgx_last_error, nothing thrown across the ABI, one graph mutex).
 *
 * Reference interface replaced (C = core/src/java/org/hypergraphdb):
 *   hgx_shortest_paths    <- GraphClassics.dijkstra(start, goal, HGALGenerator, weight, distanceMatrix,
 *                            predecessorMatrix) (C/algorithms/GraphClassics.java:126-209) over a
 *                            DefaultALGenerator (C/algorithms/DefaultALGenerator.java:437-502), for many
 *                            (start, goal) pairs at once.
 *
 * Edges.  Atom a has an edge to n through link L, of weight w[row(L)], iff DefaultALGenerator.generate(a)
 * yields (L, n): the per-mode reachability predicate of the set-mode BFS plus the link-type filter.
 *
 * Distance.  d*(n) = the minimum over generator paths start = a0 -> a1 -> ... -> n of the left-to-right
 * double sum ((0 + w1) + w2) + ...; for finite weights >= 0 IEEE addition is monotone and inflationary,
 * so this is exactly what the reference's Dijkstra returns, bit for bit, whatever the relaxation order
 * (DESIGN.md 3.5).  "Not connected" is the reference's null.
 *
 * Predecessors (rule R).  For every atom n != start with a final distance the predecessor is the atom
 * a != n that minimises (d*(a), rank a) among the atoms with an edge to n and d*(a) + w == d*(n)
 * bitwise; the reported link is the lowest link atom id among a's qualifying links to n (the link is
 * this engine's addition: the reference's map stores the atom only).  When every relaxation of the run
 * is strictly inflationary (d + w > d: e.g. weights >= 1 on integer-valued distances) this is exactly the
 * reference's final predecessorMatrix entry.  With zero or absorbed weights (d + w == d) the reference's
 * tie-break depends on its insertion history; the engine then still returns A shortest path: among
 * predecessors at the same distance as n it takes one that is one zero-weight step closer to a strictly
 * nearer atom, so the chain always ends at the start.
 */
#ifndef HGX_PATHS_H
#define HGX_PATHS_H

#include "hgx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HGX_NO_GOAL (-1)   /* goal of a single-source pair: distances from the start to every atom */

typedef struct hgx_link_weights hgx_link_weights;   /* validated, device-resident, reusable (like hgx_query_set) */
typedef struct hgx_sp_result hgx_sp_result;

/* One weight per LINK ROW (aligned with link_atom / link_type of hgx_graph_desc): the reference's
 * Mapping<HGHandle, Double> evaluated once per link (GraphClassics.java:167-168,188).  Weights must be
 * finite and >= 0 (-0.0 is taken as 0.0); a negative, NaN or infinite weight is HGX_E_INVALID (the
 * reference documents negative weights as unsupported, GraphClassics.java:104-106).  The object belongs
 * to the device of g and holds no reference on it: after an hgx_graph_update that changes the link
 * count it is refused (HGX_E_INVALID). */
int  hgx_link_weights_create(hgx_graph *g, const double *w /*[num_links]*/, hgx_link_weights **out);
void hgx_link_weights_free(hgx_link_weights *w);

/* GraphClassics.dijkstra(starts[i], goals[i], DefaultALGenerator(opts), w) for every i
 * (GraphClassics.java:126-209).  goals[i] == HGX_NO_GOAL computes the distances from starts[i] to every
 * reachable atom (what the reference's distanceMatrix holds when the goal is never reached).  w == NULL is
 * weight 1.0 for every link (the reference's default Mapping).  Ids out of range: HGX_E_INVALID;
 * partition shards: HGX_E_UNSUPPORTED.  A live result blocks hgx_graph_update, as BFS results do. */
int  hgx_shortest_paths(hgx_graph *g, const int32_t *starts, const int32_t *goals, int32_t n_pairs,
                        const hgx_algen_opts *opts, const hgx_link_weights *w, hgx_sp_result **out);
int  hgx_sp_result_info(const hgx_sp_result *r, int32_t *n_pairs);
/* dist[i] = d*(goals[i]) (+inf when not connected; 0 for HGX_NO_GOAL pairs), reached[i] = 0 / 1
 * (the Double / null of GraphClassics.java:178,208; 1 for HGX_NO_GOAL pairs).  Either may be NULL. */
int  hgx_sp_result_distances(const hgx_sp_result *r, double *dist, uint8_t *reached);
/* The path of a goal pair: atoms[0, n) = start .. goal and links[0, n - 1), links[k] joining atoms[k] and
 * atoms[k + 1]; *n_out = the path's atoms even when > cap (then cap atoms and cap - 1 links are written);
 * 0 when not connected and for HGX_NO_GOAL pairs.  Following predecessorMatrix from the goal
 * (GraphClassics.java:120-122,193-194,202-203). */
int  hgx_sp_result_path(hgx_sp_result *r, int32_t pair, int32_t *atoms, int32_t *links, int64_t cap, int64_t *n_out);
/* HGX_NO_GOAL pairs only (else HGX_E_NOTFOUND): the distanceMatrix / predecessorMatrix rows over the
 * atoms [first, first + n) (GraphClassics.java:133-135,191-194).  Unreached entries are +inf and -1; the
 * start's predecessor is -1. */
int  hgx_sp_result_distance_row(hgx_sp_result *r, int32_t pair, int64_t first, int64_t n, double *out);
int  hgx_sp_result_predecessor_row(hgx_sp_result *r, int32_t pair, int64_t first, int64_t n,
                                   int32_t *pred_atom, int32_t *pred_link);
/* Relaxation rounds (launches), frontier items expanded, edges relaxed (the reference's inner loop,
 * GraphClassics.java:182-205), strict improvements, device ms (timing enabled, hgx_set_timing) and the
 * algorithmic bytes of the relaxation.  Any output may be NULL. */
int  hgx_sp_result_stats(const hgx_sp_result *r, int64_t *rounds, int64_t *expanded, int64_t *relaxed,
                         int64_t *improved, double *ms_total, double *bytes);
void hgx_sp_result_free(hgx_sp_result *r);
/* hgx_set_option: device bytes of the per-pair working arrays of hgx_shortest_paths (dijkstra's dm /
 * unsettled state, GraphClassics.java:133-172, one copy per pair); the pairs of a call run in chunks
 * that fit, at least one pair at a time (default 48 GiB). */
#define HGX_OPT_SP_BUDGET 22

#ifdef __cplusplus
}
#endif
#endif
