#!/usr/bin/env python3
"""Or-query timing on the config-3 graph: hgx_pattern_batch_dnf (clauses + union in one device call)
against what a caller could do without it -- hgx_pattern_batch_ext over the same clauses and a union on
the host (one np.unique over (query, id) keys for the whole batch, the fastest host form).

  python tools/dnf_timing.py [--scale 1.0] [--calls 10] [--warmup 2] [--out FILE] [--baseline-only]

Legs (clauses from the bench's 10K config-3 queries: type T, incident(a), orderedLink(x, _, y)):
  a  10,000 one-clause queries
  b  2,500 queries of 4 consecutive config-3 clauses (mostly disjoint)
  c  2,500 queries of 4 clauses sharing an anchor: incident(a) | type T ^ incident(a) |
     incident(a) ^ orderedLink(x, _, y) | incident(a) ^ arity 3 (heavy overlap)
Per leg: ms per call from a host clock around the call (both paths), the device ms of the batch, ms_union and
its share of the device time, bytes_union / ms_union.  The two paths must return identical results, or the
tool fails.  --baseline-only uses nothing newer than hgx_pattern_batch_ext (it runs on an older build).
One JSON line per leg is printed (and appended to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def legs(Q, n):
    """leg -> (clause_off, the hgx_pattern_batch_ext arrays over the clauses)"""
    T, a, x, y = (np.asarray(Q[k][:n], np.int32) for k in ("type", "a", "x", "y"))
    any_ = np.full(n, -1, np.int32)
    full = dict(type_off=np.arange(n + 1, dtype=np.int64), types=T, inc_off=np.arange(n + 1, dtype=np.int64), inc=a,
                pos_off=np.zeros(n + 1, np.int64), pos=np.zeros(1, np.int32), pset_off=np.arange(n + 1, dtype=np.int64),
                pat_off=np.arange(0, 3 * n + 1, 3, dtype=np.int64), pat=np.stack([x, any_, y], 1).reshape(-1),
                arity=np.full(n, -1, np.int32))
    order = ("type_off", "types", "inc_off", "inc", "pos_off", "pos", "pset_off", "pat_off", "pat", "arity")
    out = {"a": (np.arange(n + 1, dtype=np.int64), tuple(full[k] for k in order)),
           "b": (np.arange(0, n + 1, 4, dtype=np.int64), tuple(full[k] for k in order))}
    m = n // 4                                    # leg c: clause 4 i + j of query i, all anchored on a[i]
    has_t = np.tile([0, 1, 0, 0], m)
    has_p = np.tile([0, 0, 1, 0], m)
    c = dict(type_off=np.concatenate([[0], np.cumsum(has_t)]).astype(np.int64), types=T[:m],
             inc_off=np.arange(4 * m + 1, dtype=np.int64), inc=np.repeat(a[:m], 4),
             pos_off=np.zeros(4 * m + 1, np.int64), pos=np.zeros(1, np.int32),
             pset_off=np.concatenate([[0], np.cumsum(has_p)]).astype(np.int64),
             pat_off=np.arange(0, 3 * m + 1, 3, dtype=np.int64), pat=np.stack([x[:m], any_[:m], y[:m]], 1).reshape(-1),
             arity=np.tile([-1, -1, -1, 3], m).astype(np.int32))
    out["c"] = (np.arange(0, 4 * m + 1, 4, dtype=np.int64), tuple(c[k] for k in order))
    return out


def host_union(clause_off, r):
    """The per-query sorted union of the clause results: one np.unique over (query, id) keys."""
    n_clauses = len(r.offsets) - 1
    q_of_clause = np.searchsorted(clause_off, np.arange(n_clauses), side="right") - 1
    q_of_hit = np.repeat(q_of_clause, np.diff(r.offsets))
    keys = np.unique((q_of_hit.astype(np.int64) << 32) | r.ids.astype(np.int64))
    off = np.searchsorted(keys >> 32, np.arange(len(clause_off)), side="left")
    return off.astype(np.int64), (keys & 0xFFFFFFFF).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    import hypergraphdb_amd as H
    from hypergraphdb_amd import synth
    from hypergraphdb_amd.query import pattern_batch_ext_arrays

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    t0 = time.perf_counter()
    g = synth.config3(scale=args.scale, n_queries=args.queries)
    snap = H.HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"])
    snap.set_timing(True)
    emit({"what": "setup", "scale": args.scale, "num_atoms": int(g["num_atoms"]), "num_links": int(len(g["link_atom"])),
          "baseline_only": args.baseline_only, "seconds": round(time.perf_counter() - t0, 2)})
    n = len(g["queries"]["type"]) // 4 * 4
    for name, (clause_off, arrs) in legs(g["queries"], n).items():
        if name not in args.legs.split(","):
            continue
        rec = {"what": "leg", "leg": name, "queries": int(len(clause_off) - 1), "clauses": int(clause_off[-1]),
               "calls": args.calls, "warmup": args.warmup}
        wall, dev, ref = [], [], None
        for i in range(args.warmup + args.calls):       # the baseline: clause batch + host union
            t = time.perf_counter()
            r = pattern_batch_ext_arrays(snap, *arrs)
            ref = host_union(clause_off, r)
            el = (time.perf_counter() - t) * 1e3
            if i >= args.warmup:
                wall.append(el)
                dev.append(r.ms["ms_total"])
        rec.update({"base_ms_wall_median": round(float(np.median(wall)), 4), "base_ms_wall_min": round(min(wall), 4),
                    "base_ms_device_median": round(float(np.median(dev)), 4), "clause_hits": int(len(r.ids)),
                    "kept": int(len(ref[1]))})
        if not args.baseline_only:
            from hypergraphdb_amd.query import pattern_batch_dnf_arrays
            wall, dev, un, bw = [], [], [], []
            for i in range(args.warmup + args.calls):
                t = time.perf_counter()
                r = pattern_batch_dnf_arrays(snap, clause_off, *arrs)
                el = (time.perf_counter() - t) * 1e3
                if not (np.array_equal(r.offsets, ref[0]) and np.array_equal(r.ids, ref[1])):
                    raise SystemExit(f"leg {name}: the device union differs from the host union")
                if i >= args.warmup:
                    wall.append(el)
                    dev.append(r.ms["ms_total"])
                    un.append(r.union["ms_union"])
                    bw.append(r.union["bytes_union"] / max(r.union["ms_union"], 1e-9) / 1e6)
            assert r.union["clause_hits"] == rec["clause_hits"] and r.union["kept"] == rec["kept"]
            rec.update({"dnf_ms_wall_median": round(float(np.median(wall)), 4), "dnf_ms_wall_min": round(min(wall), 4),
                        "dnf_ms_device_median": round(float(np.median(dev)), 4),
                        "ms_union_median": round(float(np.median(un)), 4),
                        "union_share_of_device": round(float(np.median(un)) / float(np.median(dev)), 3),
                        "union_gb_per_s": round(float(np.median(bw)), 2),
                        "bytes_union": r.union["bytes_union"]})
        emit(rec)
    snap.close()


if __name__ == "__main__":
    main()
