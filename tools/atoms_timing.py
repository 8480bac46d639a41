#!/usr/bin/env python3
"""Cost of the pattern path over every atom (include/hgx_atoms.h) on the config-3 graph (10M nodes, 50M links, 64
link types at scale 1) with synthesised node types: nodes whose id is no multiple of 4 get the type key NODE_BIG
(7.5M atoms at scale 1), the others NODE_SMALL; a link atom keeps its link type.  The graph, its indexes and the
compiled predicate are resident in HBM, timing on, the legs alternating inside every round:

  node_scan    type(NODE_BIG) through hgx_pattern_batch_atoms: the segment of a node type copied out in order
  link_new     type(T) for a link-only type through hgx_pattern_batch_atoms (the atom index)
  link_old     the same condition through hgx_pattern_batch_dnf_scan (the link index): both run hgx_scan_eval /
               hgx_scan_emit over 16-byte records, so the two scan stages should cost the same
  join_plain   N projections apply(targetAt(1), and(type(T), incident(a))) of the bench's queries, no predicate
  join_keep    the same batch with the predicate type(NODE_BIG) on every query

  python tools/atoms_timing.py [--scale 1.0] [--calls 10] [--warmup 3] [--queries 4096] [--out FILE]

Reported: the index build (wall ms of the first hgx_graph_type_atoms call, which builds it; 16 A bytes); per scan
leg the device ms of the batch and ms_scan from the engine's events (median, min, max over the timed calls),
rows_scanned / ms_scan, bytes_scan / ms_scan and that rate's share of the HBM peak of the microarchitecture notes
(8.0 TB/s) -- a WHOLE-STAGE figure over ALGORITHMIC bytes, not a kernel's counter
figure; per join leg ms_join, the keep kernel's ms_filter and the device ms.  Every result is checked against a
numpy pass on the host.  One JSON line is printed (and appended to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def med(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 5:
        ap.error("--calls: at least 5 timed calls")
    import hypergraphdb_amd as H
    from hypergraphdb_amd import hg, synth

    g = synth.config3(scale=args.scale, n_queries=args.queries)
    A, ty = int(g["num_atoms"]), g["link_type"]
    is_link = np.zeros(A, bool)
    is_link[g["link_atom"]] = True
    node_big, node_small = int(ty.max()) + 1, int(ty.max()) + 2
    at = np.where(np.arange(A) % 4 != 0, node_big, node_small).astype(np.int32)
    at[g["link_atom"]] = ty
    snap = H.HyperGraphSnapshot(A, g["link_atom"], g["tgt_off"], g["tgt_idx"], ty)
    snap.set_timing(True)
    snap.set_atom_types(at)
    types = np.unique(ty).tolist()
    t1 = types[len(types) // 2]
    t0 = time.perf_counter()
    counts = snap.type_atoms([node_big, node_small, t1])
    build_ms = (time.perf_counter() - t0) * 1e3   # (the first call builds the index)
    assert counts.tolist() == np.bincount(at, minlength=node_small + 1)[[node_big, node_small, t1]].tolist()
    snap.type_links([t1])                          # (and the link index, for link_old)

    Q = g["queries"]
    parts = [[(1, hg.and_(hg.type(int(Q["type"][i])), hg.incident(int(Q["a"][i]))))] for i in range(args.queries)]
    pred = H.AtomPredicate(snap, hg.type(node_big))
    legs = {
        "node_scan": lambda: H.pattern_batch_atoms(snap, [[(None, hg.type(node_big))]]),
        "link_new": lambda: H.pattern_batch_atoms(snap, [[(None, hg.type(t1))]]),
        "link_old": lambda: H.pattern_batch_dnf(snap, [hg.type(t1)], type_scan=True),
        "join_plain": lambda: H.pattern_batch_atoms(snap, parts, type_scan=False),
        "join_keep": lambda: H.pattern_batch_atoms(snap, parts, keep=[pred] * len(parts), type_scan=False),
    }
    dev, stage, filt, res = ({k: [] for k in legs} for _ in range(4))
    for i in range(args.warmup + args.calls):
        for k, run in legs.items():
            r = run()
            res[k] = r
            if i >= args.warmup:
                dev[k].append(r.ms["ms_total"])
                stage[k].append(r.scan["ms_scan"] if "join" not in k else r.join["ms_join"])
                if k == "join_keep":
                    filt[k].append(r.atoms["ms_filter"])
    # the host pass
    if not np.array_equal(res["node_scan"][0], np.nonzero(at == node_big)[0]):
        raise SystemExit("node_scan differs from the host pass")
    of_t1 = g["link_atom"][ty == t1]
    if not (np.array_equal(res["link_new"][0], of_t1) and np.array_equal(res["link_old"][0], of_t1)):
        raise SystemExit("the link-only type differs from the host pass")
    for q in range(args.queries):
        if not np.array_equal(res["join_keep"][q], [v for v in res["join_plain"][q] if at[v] == node_big]):
            raise SystemExit(f"join_keep: query {q} differs from the host filter of join_plain")
    rec = {"what": "atoms_timing", "scale": args.scale, "calls": args.calls, "warmup": args.warmup,
           "num_atoms": A, "num_links": int(len(ty)), "index_bytes": 16 * A, "index_build_wall_ms": round(build_ms, 2),
           "hbm_peak_gb_per_s": HBM_PEAK_GBS, "queries": args.queries}
    for k in ("node_scan", "link_new", "link_old"):
        r, ms = res[k], float(np.median(stage[k]))
        gbs = r.scan["bytes_scan"] / max(ms, 1e-9) / 1e6
        rec[k] = {"ms_device": med(dev[k]), "ms_scan": med(stage[k]), "rows_scanned": r.scan["rows_scanned"],
                  "rows_kept": r.scan["rows_kept"], "rows_per_s": round(r.scan["rows_scanned"] / max(ms, 1e-9) * 1e3, 1),
                  "bytes_scan": r.scan["bytes_scan"], "stage_algorithmic_gb_per_s": round(gbs, 1),
                  "stage_algorithmic_share_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
    for k in ("join_plain", "join_keep"):
        r = res[k]
        rec[k] = {"ms_device": med(dev[k]), "ms_join": med(stage[k]), "join": {x: r.join[x] for x in
                  ("parts", "hits_projected", "values_distinct", "kept")}}
    rec["join_keep"]["ms_filter"] = med(filt["join_keep"])
    rec["join_keep"]["atoms"] = {x: res["join_keep"].atoms[x] for x in
                                 ("queries_filtered", "values_tested", "values_rejected", "bytes_filter")}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    pred.close()
    snap.close()


if __name__ == "__main__":
    main()
