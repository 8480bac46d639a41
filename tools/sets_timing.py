#!/usr/bin/env python3
"""Readout timing of the visited sets of a batched BFS: hgx_bfs_result_sets (include/hgx_sets.h, one device pass
for many seeds) against the loop of hgx_bfs_result_visited over (seed, depth), the only way to the same data
before, called the way BfsResult.visited calls it (twice per set: the size, then the data).  Both read the same
bfs_batch result in one process.

  python tools/sets_timing.py [--scale5 0.02] [--scale2 0.02] [--bfs-block 1] [--calls 5] [--warmup 1] [--out FILE]

Cases:
  config5  a scaled config 5: the subsumption closures of 1024 classes (unbounded, HGSubsumes links only), every
           seed read
  config2  a scaled config 2: 1024 seeds, depth 4; 64 of the 1024 seeds read (every 16th), all depths
Per case, alternating call by call after --warmup calls of each: the reader loop, the batched readout without a
predicate, with a predicate that keeps half of the atoms, and count-only.  Times are from a host clock around work
that ends in a device synchronise; medians over --calls calls.  Printed per case: the times, the ratio batched /
loop (below 1: the batched readout is faster), and the stage's GB/s from its algorithmic bytes over its wall time.
The tool fails unless the batched readout returns exactly the loop's sets, or if a ratio is not below 1.
--bfs-block 0 keeps every seed on the rows engine, so the kernels serve the readout; 1 is the default engine
choice, where the workgroup stages finish the small traversals and the host lists serve their seeds.
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
    ap.add_argument("--scale5", type=float, default=0.02)
    ap.add_argument("--scale2", type=float, default=0.02)
    ap.add_argument("--bfs-block", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 3 or args.warmup < 1:
        ap.error("at least 3 timed calls and 1 warm-up call")
    import hypergraphdb_amd as H
    from hypergraphdb_amd import _lib, synth

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    ok = True
    for case in ("config5", "config2"):
        t0 = time.perf_counter()
        if case == "config5":
            g = synth.config5(scale=args.scale5)
            make_gen = lambda s: H.DefaultALGenerator(s, H.AtomTypeCondition(g["subsumes_type"]), None, False, True, False)  # noqa: E731
            maxd, pick = None, None
        else:
            g = synth.config2(scale=args.scale2)
            make_gen = lambda s: None  # noqa: E731
            maxd, pick = g["depth"], np.arange(0, len(g["seeds"]), 16, dtype=np.int32)
        snap = H.HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"])
        snap.set_option(_lib.HGX_OPT_BFS_BLOCK, args.bfs_block)
        A = int(g["num_atoms"])
        keep = np.random.default_rng(3).random(A) < 0.5
        res = H.bfs_batch(snap, g["seeds"], maxd, make_gen(snap))
        res.counts()
        sel = np.arange(res.n_seeds, dtype=np.int32) if pick is None else pick
        st = res.stats(accounting=False)
        emit({"what": "setup", "case": case, "num_atoms": A, "num_links": int(len(g["link_atom"])), "seeds": res.n_seeds,
              "levels": res.n_levels, "sets_read": int(len(sel)), "bfs_block": args.bfs_block,
              "block_seeds": st["block_seeds"], "block_rerun": st["block_rerun"], "block_coop": st["block_coop"],
              "seconds": round(time.perf_counter() - t0, 2)})

        def timed(fn):
            _lib.device_synchronize(snap.device)
            t = time.perf_counter()
            r = fn()
            _lib.device_synchronize(snap.device)
            return r, (time.perf_counter() - t) * 1e3

        def loop():   # the reader loop: every depth of every selected seed, as BfsResult.levels does
            return [[res.visited(int(i), d) for d in range(res.n_levels)] for i in sel]

        def batched(**kw):
            vs = res.sets(sel, **kw)
            if not vs.count_only:
                vs.flat()
            return vs

        with H.AtomPredicate.from_mask(snap, keep) as half:
            variants = {"plain": {}, "half": {"where": half}, "count_only": {"count_only": True}}
            t_loop, t_var, stats = [], {k: [] for k in variants}, {}
            for i in range(args.warmup + args.calls):
                lv, el = timed(loop)
                if i >= args.warmup:
                    t_loop.append(el)
                for name, kw in variants.items():
                    vs, el = timed(lambda: batched(**kw))
                    if i >= args.warmup:
                        t_var[name].append(el)
                    if i == 0:   # the same data as the loop's
                        exp = [np.sort(np.concatenate(x)) for x in lv]
                        if name == "half":
                            exp = [x[keep[x]] for x in exp]
                        same = np.array_equal(vs.counts, [len(x) for x in exp])
                        if same and name != "count_only":
                            same = np.array_equal(vs.flat(), np.concatenate(exp) if exp else np.zeros(0, np.int32))
                        ok = ok and bool(same)
                        stats[name] = dict(vs.stats(), total=int(vs.total), equal_to_loop=bool(same))
                    vs.close()
        rec = {"what": "case", "case": case, "bfs_block": args.bfs_block, "calls": args.calls, "warmup": args.warmup,
               "sets_read": int(len(sel)), "levels": res.n_levels,
               "reader_calls_of_the_loop": int(2 * len(sel) * res.n_levels), "loop_ms_wall_median": med(t_loop),
               "loop_ms_wall_min": round(min(t_loop), 3), "loop_ms_wall_max": round(max(t_loop), 3)}
        for name in variants:
            m = med(t_var[name])
            s = stats[name]
            rec[name] = {"ms_wall_median": m, "ms_wall_min": round(min(t_var[name]), 3),
                         "ms_wall_max": round(max(t_var[name]), 3), "ratio_to_loop": round(m / med(t_loop), 4),
                         "entries": s["total"], "rows_read": s["rows_read"], "tiles_skipped": s["tiles_skipped"],
                         "algorithmic_mb": round(s["bytes"] / 1e6, 3),
                         "gb_per_s_over_wall": round(s["bytes"] / (m * 1e-3) / 1e9, 3) if m > 0 else None,
                         "equal_to_loop": s["equal_to_loop"]}
            ok = ok and m < med(t_loop)
        emit(rec)
        res.close()
        snap.close()
    if not ok:
        raise SystemExit("the batched readout differs from the reader loop, or is not faster than it")


if __name__ == "__main__":
    main()
