#!/usr/bin/env python3
"""Link predicate timing (include/hgx_linkpred.h) on config 5 and config 2.

  python tools/linkpred_timing.py [--c5-scale 1.0] [--c2-scale 1.0] [--calls 10] [--warmup 2] [--out FILE]

Per graph:
  (i)  the evaluation (hgx_linkpred_eval + hgx_linkpred_project) of a type-only program, type(T), and of a
       target-reading program, and(type(T), not(incident(hub))): device ms from the predicate's own events,
       its algorithmic bytes and the rate they give;
  (ii) one BFS step (hgx_bfs_batch over the graph's sources, the result's counts read out) with the predicate
       type(T) against the typed generator AtomTypeCondition(T) on the same seeds.  The typed generator runs
       the kernels and the host code it ran before link predicates existed, and the predicate step runs the
       same kernels over the predicate's flag arrays instead of link_type / inc_type.  Three legs alternate
       call by call in one session -- typed, predicate, typed again -- so the spread between the two typed
       legs is the run-to-run noise the predicate leg is judged against.
Config 5: T = the subsumes type, the step = the closures of the sources in both directions (unbounded depth).
Config 2: one link type (0), so type(0) accepts every link; the step = the symmetric BFS to the config's depth.
The tool fails unless the predicate step's counts equal the typed step's.  One JSON line per measurement is
printed (and appended to --out).
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
    ap.add_argument("--c5-scale", type=float, default=1.0)
    ap.add_argument("--c2-scale", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("config5", "config2"), default=None)
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

    ok = True
    n_all = args.warmup + args.calls
    for name in ("config5", "config2"):
        if args.only and args.only != name:
            continue
        t0 = time.perf_counter()
        if name == "config5":
            g = synth.config5(scale=args.c5_scale)
            T, depth = int(g["subsumes_type"]), None
            modes = [(False, True, False, False), (False, True, True, False)]
        else:
            g = synth.config2(scale=args.c2_scale)
            T, depth = 0, int(g["depth"])
            modes = [(True, True, False, False)]
        M = len(g["link_atom"])
        hub = int(np.argmax(np.bincount(g["tgt_idx"], minlength=g["num_atoms"])))
        snap = H.HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"],
                                    keep_host=False)
        snap.set_timing(True)
        seeds = np.asarray(g["seeds"], np.int32)
        emit({"what": "setup", "graph": name, "num_atoms": int(g["num_atoms"]), "num_links": int(M),
              "pins": int(len(g["tgt_idx"])), "type": T, "seeds": int(len(seeds)),
              "seconds": round(time.perf_counter() - t0, 2)})

        def timed(fn):
            _lib.device_synchronize(snap.device)
            t = time.perf_counter()
            r = fn()
            _lib.device_synchronize(snap.device)
            return r, (time.perf_counter() - t) * 1e3

        # (i) the evaluation
        for prog, tree in (("type_only", hg.type(T)), ("target_reading", hg.and_(hg.type(T), hg.not_(hg.incident(hub))))):
            dev, wall, st = [], [], None
            for i in range(n_all):
                p, el = timed(lambda: H.LinkPredicate(snap, tree))
                st = p.stats()
                p.close()
                if i >= args.warmup:
                    dev.append(st["ms_eval"])
                    wall.append(el)
            emit({"what": "eval", "graph": name, "program": prog, "calls": args.calls, "warmup": args.warmup,
                  "ms_device_median": med(dev), "ms_device_min": round(min(dev), 3), "ms_device_max": round(max(dev), 3),
                  "ms_wall_median": med(wall), "algorithmic_mb": round(st["bytes_eval"] / 1e6, 3),
                  "gb_per_s": round(st["bytes_eval"] / (med(dev) * 1e-3) / 1e9, 1) if med(dev) > 0 else None,
                  "num_satisfied": st["num_satisfied"], "num_links": st["num_links"]})

        # (ii) the BFS step: typed, predicate, typed again -- alternating
        pred = H.LinkPredicate(snap, hg.type(T))
        gens = {"typed": [H.DefaultALGenerator(snap, H.AtomTypeCondition(T), None, *m) for m in modes],
                "predicate": [H.DefaultALGenerator(snap, pred, None, *m) for m in modes]}

        def step(kind):
            out, dev_ms = [], 0.0
            for gn in gens[kind]:
                r = H.bfs_batch(snap, seeds, depth, gn)
                out.append(r.counts().copy())          # the step's readout
                dev_ms += r.stats(accounting=False)["ms_total"]
                r.close()
            return out, dev_ms

        legs = {"typed_a": [], "predicate": [], "typed_b": []}
        devs = {"typed_a": [], "predicate": [], "typed_b": []}
        ref = None
        for i in range(n_all):
            for leg, kind in (("typed_a", "typed"), ("predicate", "predicate"), ("typed_b", "typed")):
                (cnt, dms), el = timed(lambda: step(kind))
                if ref is None:
                    ref = cnt
                same = len(cnt) == len(ref) and all(np.array_equal(a, b) for a, b in zip(cnt, ref))
                ok = ok and same
                if i >= args.warmup:
                    legs[leg].append(el)
                    devs[leg].append(dms)
        pred.close()
        noise = abs(med(legs["typed_a"]) - med(legs["typed_b"]))
        spread = max(max(legs[k]) - min(legs[k]) for k in ("typed_a", "typed_b"))
        typed_med = (med(legs["typed_a"]) + med(legs["typed_b"])) / 2
        emit({"what": "step", "graph": name, "calls": args.calls, "warmup": args.warmup, "traversals_per_step": len(modes),
              **{f"{k}_ms_wall_median": med(v) for k, v in legs.items()},
              **{f"{k}_ms_wall_min": round(min(v), 3) for k, v in legs.items()},
              **{f"{k}_ms_wall_max": round(max(v), 3) for k, v in legs.items()},
              **{f"{k}_ms_device_median": med(v) for k, v in devs.items()},
              "typed_legs_median_difference_ms": round(noise, 3), "typed_legs_largest_spread_ms": round(spread, 3),
              "predicate_minus_typed_ms": round(med(legs["predicate"]) - typed_med, 3),
              "within_typed_spread": bool(abs(med(legs["predicate"]) - typed_med) <= spread),
              "counts_equal": bool(ok), "atoms_reached": int(sum(int(c[:, 1:].sum()) for c in ref))})
        snap.close()
    if not ok:
        raise SystemExit("the predicate step's counts differ from the typed step's")


if __name__ == "__main__":
    main()
