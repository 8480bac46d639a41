#!/usr/bin/env python3
"""Cost of the type-index scan on the config-3 graph (50M links, 64 types, arity 3..6 at scale 1), the graph and
its type index resident in HBM, timing on, three batches alternating inside every round:

  arity_all   and(type(T), arity(k)) for each of the graph's types, k = 3 + T % 4: every index record streamed once
  type_one    type(T) alone for one type: the segment copied out in order
  not_hub     and(type(T), not(incident(hub))), hub = the atom with the longest incidence set: every row's
              targets gathered

  python tools/scan_timing.py [--scale 1.0] [--calls 10] [--warmup 3] [--out FILE]

Per leg: the device ms of the batch and ms_scan from the engine's events (medians over the timed calls),
rows_scanned, bytes_scan / ms_scan, and that rate's share of the HBM peak of the microarchitecture notes
(8.0 TB/s) -- a WHOLE-STAGE figure over ALGORITHMIC bytes (five launches, the eval kernel among
them), not a kernel's counter figure.  For comparison a single-thread numpy pass over link_type and the arities on
the host: a generous stand-in for the reference's per-candidate filter (AndToQuery's PredicateBasedFilter loads
every candidate atom; numpy streams two flat arrays).  The results are checked against that pass.  One JSON line
is printed (and appended to --out).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 5:
        ap.error("--calls: at least 5 timed calls")
    import hypergraphdb_amd as H
    from hypergraphdb_amd import hg, synth

    g = synth.config3(scale=args.scale, n_queries=64)
    snap = H.HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"])
    snap.set_timing(True)
    ty, arity = g["link_type"], np.diff(g["tgt_off"]).astype(np.int32)
    types = np.unique(ty).tolist()
    hub = int(np.bincount(g["tgt_idx"], minlength=g["num_atoms"]).argmax())
    t1 = types[len(types) // 2]
    legs = {"arity_all": [hg.and_(hg.type(t), hg.arity(3 + t % 4)) for t in types],
            "type_one": [hg.type(t1)],
            "not_hub": [hg.and_(hg.type(t1), hg.not_(hg.incident(hub)))]}
    t0 = time.perf_counter()
    assert snap.type_links(types).tolist() == np.bincount(ty, minlength=max(types) + 1)[types].tolist()
    build_ms = (time.perf_counter() - t0) * 1e3   # (the first call builds the index)

    # the host pass: one thread over the flat arrays
    def host_arity_all():
        return [g["link_atom"][(ty == t) & (arity == 3 + t % 4)] for t in types]

    t0 = time.perf_counter()
    exp_arity = host_arity_all()
    host_ms = (time.perf_counter() - t0) * 1e3
    of_t1 = g["link_atom"][ty == t1]
    has_hub = np.zeros(len(ty), bool)
    has_hub[np.searchsorted(g["tgt_off"], np.nonzero(g["tgt_idx"] == hub)[0], side="right") - 1] = True
    exp = {"arity_all": exp_arity, "type_one": [of_t1], "not_hub": [g["link_atom"][(ty == t1) & ~has_hub]]}

    dev, scan, res = ({k: [] for k in legs} for _ in range(3))
    for i in range(args.warmup + args.calls):
        for k, trees in legs.items():
            r = H.pattern_batch_dnf(snap, trees, type_scan=True)
            res[k] = r
            if i >= args.warmup:
                dev[k].append(r.ms["ms_total"])
                scan[k].append(r.scan["ms_scan"])
    rec = {"what": "scan_timing", "scale": args.scale, "calls": args.calls, "warmup": args.warmup,
           "num_links": int(len(ty)), "types": len(types), "index_bytes": 16 * int(len(ty)), "index_build_ms": round(build_ms, 2),
           "host_numpy_arity_all_ms": round(host_ms, 2), "hbm_peak_gb_per_s": HBM_PEAK_GBS}
    for k in legs:
        r = res[k]
        for q, e in enumerate(exp[k]):
            if not np.array_equal(r[q], e):
                raise SystemExit(f"{k}: query {q} differs from the host pass")
        ms = float(np.median(scan[k]))
        gbs = r.scan["bytes_scan"] / max(ms, 1e-9) / 1e6
        rec[k] = {"ms_device_median": round(float(np.median(dev[k])), 4), "ms_scan_median": round(ms, 4),
                  "ms_scan_min": round(min(scan[k]), 4), "ms_scan_max": round(max(scan[k]), 4),
                  "rows_scanned": r.scan["rows_scanned"], "rows_kept": r.scan["rows_kept"],
                  "bytes_scan": r.scan["bytes_scan"], "stage_algorithmic_gb_per_s": round(gbs, 1),
                  "stage_algorithmic_share_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    snap.close()


if __name__ == "__main__":
    main()
