#!/usr/bin/env python3
"""Cost of the device join (hgx_pattern_batch_join) against the host path it replaces, on the config-3 graph
(50M links, 64 types, arity 3..6 at scale 1) resident in HBM, timing on.

10,000 join queries of two parts, built from the config's own pattern queries hg.and(hg.type(T), hg.incident(a),
hg.orderedLink(x, ANY, y)): the queries are sorted by type and neighbours sharing a type are paired; join query i =
and(apply(targetAt(1), part 2i), apply(targetAt(1), part 2i+1)).  Two legs, alternating inside every round:

  pattern   the parts are the config's queries as they are (a hit or none per part)
  typed     the parts without their orderedLink: and(type(T), incident(a)) -- every link of the type at a, so hub
            atoms give long runs and the projections fold duplicates

  python tools/join_timing.py [--scale 1.0] [--joins 10000] [--calls 10] [--host-calls 3] [--warmup 3] [--out FILE]

Each leg runs on an execution context of its own (hgx_graph_context): the hit workspace is per context and only
grows, and the join's sort and scan run over its capacity -- on one context the small leg would
sort the large leg's workspace.  ``--shared`` runs both legs on the snapshot itself and shows exactly that.

Per leg and per call: wall ms of pattern_batch_join (host lowering included), the device ms of the batch and of its
clause, union and join stages from the engine's events, the join stage's algorithmic bytes --
medians over the timed calls with their min and max.  The comparison (timed in the first --host-calls timed rounds
only: on the typed leg one host pass takes tens of seconds) is the best path without the join stage for
the same conditions: pattern_batch_dnf over all parts, then on the host a vectorised numpy projection
(tgt_idx[tgt_off[row] + 1]), np.unique and np.intersect1d per query -- wall ms, alternating with the join inside
the round.  The two results are checked against each other.  One JSON line is printed (and appended to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stat(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--joins", type=int, default=10_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--shared", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 5 or not 1 <= args.host_calls <= args.calls:
        ap.error("--calls: at least 5 timed calls; --host-calls: between 1 and --calls")
    import hypergraphdb_amd as H
    from hypergraphdb_amd import synth

    g = synth.config3(scale=args.scale, n_queries=4 * args.joins)
    Q = g["queries"]
    # pairs of queries sharing a type: sort by type, pair neighbours, keep the pairs whose types agree
    order = np.argsort(Q["type"], kind="stable")
    a, b = order[0::2], order[1::2]
    same = Q["type"][a] == Q["type"][b]
    a, b = a[same][:args.joins], b[same][:args.joins]
    if len(a) < args.joins:
        raise SystemExit(f"only {len(a)} pairs share a type")
    idx = np.stack([a, b], 1).ravel()   # part 2i, 2i+1

    def clause(i, pattern):
        return {"types": [int(Q["type"][i])], "inc": [int(Q["a"][i])], "pos": [],
                "patterns": [(int(Q["x"][i]), -1, int(Q["y"][i]))] if pattern else [], "arity": -1}

    legs = {"pattern": [[clause(i, True)] for i in idx], "typed": [[clause(i, False)] for i in idx]}
    link_atom, tgt_off, tgt_idx = g["link_atom"], g["tgt_off"], g["tgt_idx"]

    def host_path(snap, parts):
        """pattern_batch_dnf over the parts, projection / unique / intersection on the host"""
        r = H.pattern_batch_dnf(snap, parts)
        row = np.searchsorted(link_atom, r.ids)
        has = tgt_off[row + 1] - tgt_off[row] > 1
        val = np.where(has, tgt_idx[np.minimum(tgt_off[row] + 1, len(tgt_idx) - 1)], -1)
        off = r.offsets
        out = []
        for j in range(len(parts) // 2):
            u = np.unique(val[off[2 * j]:off[2 * j + 1]])
            v = np.unique(val[off[2 * j + 1]:off[2 * j + 2]])
            w = np.intersect1d(u, v, assume_unique=True)
            out.append(w[w >= 0])
        return out, r

    snap = H.HyperGraphSnapshot(g["num_atoms"], link_atom, tgt_off, tgt_idx, g["link_type"])
    snap.set_timing(True)
    keys = ("wall_join", "dev_total", "dev_union", "dev_join", "wall_host", "dev_host_dnf")
    t = {k: {x: [] for x in keys} for k in legs}
    last = {}
    ctx = {k: snap if args.shared else snap.context() for k in legs}
    for c in ctx.values():
        c.set_timing(True)
    for i in range(args.warmup + args.calls):
        for k, parts in legs.items():
            joins = [[(1, parts[2 * j]), (1, parts[2 * j + 1])] for j in range(args.joins)]
            t0 = time.perf_counter()
            r = H.pattern_batch_join(ctx[k], joins)
            t1 = time.perf_counter()
            if i >= args.warmup:
                t[k]["wall_join"].append((t1 - t0) * 1e3)
                t[k]["dev_total"].append(r.ms["ms_total"])
                t[k]["dev_union"].append(r.union["ms_union"])
                t[k]["dev_join"].append(r.join["ms_join"])
            if i == 0 or args.warmup <= i < args.warmup + args.host_calls:   # (round 0: the check and the warm-up)
                t1 = time.perf_counter()
                exp, rd = host_path(ctx[k], parts)
                t2 = time.perf_counter()
                last[k] = (r, exp, rd)
                if i >= args.warmup:
                    t[k]["wall_host"].append((t2 - t1) * 1e3)
                    t[k]["dev_host_dnf"].append(rd.ms["ms_total"])
    rec = {"what": "join_timing", "scale": args.scale, "joins": args.joins, "calls": args.calls,
           "host_calls": args.host_calls, "warmup": args.warmup, "shared_workspace": bool(args.shared), "num_links": int(len(link_atom))}
    for k in legs:
        r, exp, rd = last[k]
        for j, e in enumerate(exp):
            if not np.array_equal(r[j], e):
                raise SystemExit(f"{k}: join query {j} differs from the host path")
        clause_ms = [a - b - c for a, b, c in zip(t[k]["dev_total"], t[k]["dev_union"], t[k]["dev_join"])]
        ms_join = float(np.median(t[k]["dev_join"]))
        rec[k] = {"wall_ms_join": stat(t[k]["wall_join"]), "device_ms_total": stat(t[k]["dev_total"]),
                  "device_ms_clause_stage": stat(clause_ms), "device_ms_union": stat(t[k]["dev_union"]),
                  "device_ms_join": stat(t[k]["dev_join"]), "bytes_join": r.join["bytes_join"],
                  "join_stage_algorithmic_gb_per_s": round(r.join["bytes_join"] / max(ms_join, 1e-9) / 1e6, 1),
                  "hits_projected": r.join["hits_projected"], "values_distinct": r.join["values_distinct"],
                  "kept": r.join["kept"], "wall_ms_host_path": stat(t[k]["wall_host"]),
                  "device_ms_host_path_dnf": stat(t[k]["dev_host_dnf"]),
                  "host_over_join_wall": round(float(np.median(t[k]["wall_host"])) / float(np.median(t[k]["wall_join"])), 2)}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    for c in ctx.values():
        if c is not snap:
            c.close()
    snap.close()


if __name__ == "__main__":
    main()
