#!/usr/bin/env python3
"""Sibling predicate timing (include/hgx_sibling.h) on config 2.

  python tools/sibling_timing.py [--scale 1.0] [--calls 10] [--warmup 2] [--plain-only] [--out FILE]

  (i)  the evaluation (hgx_sibling_eval) of a type program, typePlus of half the node types, and of a byte mask:
       device ms from the predicate's own events, its algorithmic bytes and the rate they give;
  (ii) one BFS step (hgx_bfs_batch over the config's 1024 sources to its depth, the result's counts read out)
       without a sibling predicate against the same step with a mask that keeps every atom (the prologue alone:
       nothing is saturated, so the levels are the plain ones), about half of the atoms and about a tenth.  The
       legs alternate call by call in one session -- plain, everything, half, tenth, plain again -- so the spread
       between the two plain legs is the run-to-run noise the others are judged against.  With a sibling
       predicate every seed runs on the rows engine (the workgroup engine is skipped), on config 2 as without one:
       its seeds outgrow a workgroup.
--plain-only runs the two plain legs alone (a build without the sibling entry points: the parent commit's step
under the same harness).  The tool fails unless the keep-everything step's counts equal the plain step's.  One
JSON line per measurement is printed (and appended to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(x):
    return round(float(np.median(x)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    import hypergraphdb_amd as H
    from hypergraphdb_amd import _lib, hg, synth

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    n_all = args.warmup + args.calls
    t0 = time.perf_counter()
    g = synth.config2(scale=args.scale)
    A, M, depth = int(g["num_atoms"]), len(g["link_atom"]), int(g["depth"])
    snap = H.HyperGraphSnapshot(A, g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"], keep_host=False)
    snap.set_timing(True)
    seeds = np.asarray(g["seeds"], np.int32)
    emit({"what": "setup", "graph": "config2", "scale": args.scale, "num_atoms": A, "num_links": int(M),
          "pins": int(len(g["tgt_idx"])), "seeds": int(len(seeds)), "depth": depth, "plain_only": args.plain_only,
          "seconds": round(time.perf_counter() - t0, 2)})

    def timed(fn):
        _lib.device_synchronize(snap.device)
        t = time.perf_counter()
        r = fn()
        _lib.device_synchronize(snap.device)
        return r, (time.perf_counter() - t) * 1e3

    rng = np.random.default_rng(13)
    preds = {}
    if not args.plain_only:
        # (i) the evaluation: ten node types, the link atoms keep their link type
        n_types = 10
        types = rng.integers(0, n_types, A).astype(np.int32)
        types[np.asarray(g["link_atom"])] = np.asarray(g["link_type"], np.int32)
        snap.set_atom_types(types)
        half = rng.random(A) < 0.5
        for prog, make in (("typePlus_of_5", lambda: H.AtomPredicate(snap, hg.typePlus(list(range(n_types // 2))))),
                           ("not_type", lambda: H.AtomPredicate(snap, hg.not_(hg.type(3)))),
                           ("mask", lambda: H.AtomPredicate.from_mask(snap, half))):
            dev, wall, st = [], [], None
            for i in range(n_all):
                p, el = timed(make)
                st = p.stats()
                p.close()
                if i >= args.warmup:
                    dev.append(st["ms_eval"])
                    wall.append(el)
            emit({"what": "eval", "program": prog, "calls": args.calls, "warmup": args.warmup,
                  "ms_device_median": med(dev), "ms_device_min": round(min(dev), 3), "ms_device_max": round(max(dev), 3),
                  "ms_wall_median": med(wall), "algorithmic_mb": round(st["bytes_eval"] / 1e6, 3),
                  "gb_per_s": round(st["bytes_eval"] / (med(dev) * 1e-3) / 1e9, 1) if med(dev) > 0 else None,
                  "num_kept": st["num_kept"], "num_atoms": st["num_atoms"]})
        preds = {"everything": H.AtomPredicate.from_mask(snap, np.ones(A, bool)),
                 "half": H.AtomPredicate.from_mask(snap, half),
                 "tenth": H.AtomPredicate.from_mask(snap, rng.random(A) < 0.1)}

    # (ii) the BFS step
    gens = {"plain_a": None, **{k: H.DefaultALGenerator(snap, None, p) for k, p in preds.items()}, "plain_b": None}

    def step(gn):
        r = H.bfs_batch(snap, seeds, depth, gn)
        c = r.counts().copy()                      # the step's readout
        st = r.stats(accounting=False)
        r.close()
        levels[0] = {"kind": st["level_sparse"][:st["n_levels_expanded"]], "new_atoms": st["level_new"][:st["n_levels_expanded"]],
                     "ms": [round(x, 3) for x in st["level_ms"][:st["n_levels_expanded"]]]}
        return c, st["ms_total"]

    levels = [None]                                # the last step's level kinds, new atoms and device ms per level
    last = {}
    wall = {k: [] for k in gens}
    devs = {k: [] for k in gens}
    first = {}
    ok = True
    for i in range(n_all):
        for leg, gn in gens.items():
            (c, dms), el = timed(lambda: step(gn))
            last[leg] = levels[0]
            if leg not in first:
                first[leg] = c
            ok = ok and np.array_equal(c, first[leg])
            if i >= args.warmup:
                wall[leg].append(el)
                devs[leg].append(dms)
    same = all(np.array_equal(first[k], first["plain_a"]) for k in ("plain_b", "everything") if k in first)
    spread = max(max(devs[k]) - min(devs[k]) for k in ("plain_a", "plain_b"))
    plain_med = (med(devs["plain_a"]) + med(devs["plain_b"])) / 2
    emit({"what": "step", "calls": args.calls, "warmup": args.warmup,
          **{f"{k}_ms_device_median": med(v) for k, v in devs.items()},
          **{f"{k}_ms_device_min": round(min(v), 3) for k, v in devs.items()},
          **{f"{k}_ms_device_max": round(max(v), 3) for k, v in devs.items()},
          **{f"{k}_ms_wall_median": med(v) for k, v in wall.items()},
          "plain_legs_median_difference_ms": round(abs(med(devs["plain_a"]) - med(devs["plain_b"])), 3),
          "plain_legs_largest_spread_ms": round(spread, 3),
          **{f"{k}_minus_plain_ms": round(med(devs[k]) - plain_med, 3) for k in preds},
          **{f"{k}_atoms_reached": int(first[k][:, 1:].sum()) for k in first},
          "steps_repeat": bool(ok), "everything_equals_plain": bool(same)})
    for leg, lv in last.items():
        emit({"what": "levels", "leg": leg, **lv})
    for p in preds.values():
        p.close()
    snap.close()
    if not (ok and same):
        raise SystemExit("a step's counts differ")


if __name__ == "__main__":
    main()
