#!/usr/bin/env python3
"""Hop-path timing on the config-2 graph: hop_paths (one batched BFS + the backtrace of include/hgx_hops.h)
against hgx_shortest_paths with unit weights, the only way to these paths before.  The sibling of
tools/sp_timing.py: the same graph and the same pairs.

  python tools/hop_timing.py [--scale 1.0] [--calls 10] [--warmup 2] [--out FILE]

Cases (64 random (start, goal) pairs over nodes with incidence, seeds 7 / 8; symmetric generator), (a) and (b)
alternating call by call in one session:
  a  shortest_paths(weights=None) on the 64 pairs
  b  hop_paths on the same pairs, split into the forward BFS and the backtrace
  c  hop_paths on 1024 pairs (1024 distinct starts)
  d  one depths + predecessors row
  e  one pair, both ways (alternating)
Per case: ms per call from device events and from a host clock around a device synchronise.  The tool fails
unless (a) and (b) agree -- bitwise distances, identical atoms and links -- and the first --cpu-pairs pairs
agree with the single-thread Dijkstra of tools/native/sp_cpu.cc.  One JSON line per case is printed (and
appended to --out).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sp_timing import cpu_lib  # noqa: E402


def med(x):
    return round(float(np.median(x)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--many", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-pairs", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    import hypergraphdb_amd as H
    from hypergraphdb_amd import _lib, synth

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def timed(fn):
        _lib.device_synchronize(snap.device)
        t = time.perf_counter()
        r = fn()
        _lib.device_synchronize(snap.device)
        return r, (time.perf_counter() - t) * 1e3

    t0 = time.perf_counter()
    g = synth.config2(scale=args.scale, n_sources=16)
    A, M = g["num_atoms"], len(g["link_atom"])
    starts = synth.sources(g, args.pairs, 7)
    goals = synth.sources(g, args.pairs, 8)
    snap = H.HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"],
                                keep_host=False)
    snap.set_timing(True)
    emit({"what": "setup", "scale": args.scale, "num_atoms": int(A), "num_links": int(M), "pins": int(len(g["tgt_idx"])),
          "seconds": round(time.perf_counter() - t0, 2)})
    n_all = args.warmup + args.calls
    ok = True

    # (a) / (b), alternating
    a_dev, a_wall, b_wall, b_bfs, b_back, a_st, b_st = [], [], [], [], [], None, None
    sp_dist = sp_paths = hp_hops = hp_paths = None
    for i in range(n_all):
        sp, el_a = timed(lambda: H.shortest_paths(snap, starts, goals))
        a_st = sp.stats()
        if i == 0:
            sp_dist = sp.distance.copy()
            sp_paths = [tuple(x.tolist() for x in sp.path(k)) for k in range(len(starts))]
        sp.close()
        hp, el_b = timed(lambda: H.hop_paths(snap, starts, goals))
        b_st = hp.stats()
        bfs_ms = hp.owner.stats(accounting=False)["ms_total"]
        if i == 0:
            hp_hops = hp.hops.copy()
            hp_paths = [tuple(x.tolist() for x in hp.path(k)) for k in range(len(starts))]
            levels = hp.owner.n_levels
        hp.close()
        if i >= args.warmup:
            a_dev.append(a_st["ms_total"])
            a_wall.append(el_a)
            b_wall.append(el_b)
            b_bfs.append(bfs_ms)
            b_back.append(b_st["ms_total"])
    exp = np.where(hp_hops >= 0, hp_hops.astype(np.float64), np.inf)
    agree = bool(np.array_equal(exp.view(np.uint64), sp_dist.view(np.uint64)) and sp_paths == hp_paths)
    ok = ok and agree
    emit({"what": "case", "case": "a", "engine": "shortest_paths(weights=None)", "pairs": int(len(starts)),
          "calls": args.calls, "warmup": args.warmup, "ms_device_median": med(a_dev), "ms_device_min": round(min(a_dev), 3),
          "ms_device_max": round(max(a_dev), 3), "ms_wall_median": med(a_wall), "ms_per_pair": round(med(a_wall) / len(starts), 3),
          "rounds": a_st["rounds"], "relaxed": a_st["relaxed"], "reached_goals": int(np.isfinite(sp_dist).sum())})
    back = med(b_back)
    emit({"what": "case", "case": "b", "engine": "hop_paths", "pairs": int(len(starts)), "calls": args.calls,
          "warmup": args.warmup, "ms_wall_median": med(b_wall), "ms_wall_min": round(min(b_wall), 3),
          "ms_per_pair": round(med(b_wall) / len(starts), 3), "bfs_ms_device_median": med(b_bfs),
          "backtrace_ms_device_median": back, "backtrace_ms_device_min": round(min(b_back), 3),
          "backtrace_share_of_wall": round(back / med(b_wall), 4), "bfs_levels": int(levels),
          "max_hops": int(hp_hops.max()), "step_launches": b_st["steps"], "entries": b_st["entries"], "probes": b_st["probes"],
          "probes_per_second": round(b_st["probes"] / (back * 1e-3), 1) if back > 0 else None,
          "algorithmic_mb": round(b_st["bytes"] / 1e6, 3), "agrees_with_a": agree,
          "speedup_over_a_wall": round(med(a_wall) / med(b_wall), 2)})

    # the CPU baseline on the first pairs
    ncpu = min(args.cpu_pairs, len(starts))
    if ncpu:
        L = cpu_lib()
        tg = np.ascontiguousarray(g["tgt_idx"], np.int32)
        cpu = L.sp_cpu_build(A, M, g["tgt_off"].ctypes.data, tg.ctypes.data, g["link_type"].ctypes.data)
        cs, cq = np.ascontiguousarray(starts[:ncpu], np.int32), np.ascontiguousarray(goals[:ncpu], np.int32)
        cd = np.zeros(ncpu)
        nrel = C.c_int64()
        secs = L.sp_cpu_run(cpu, 0, -1, None, cs.ctypes.data, cq.ctypes.data, ncpu, cd.ctypes.data, None, C.byref(nrel))
        L.sp_cpu_free(cpu)
        cpu_ok = bool(np.array_equal(cd.view(np.uint64), exp[:ncpu].view(np.uint64)))
        ok = ok and cpu_ok
        emit({"what": "cpu", "cpu_pairs": ncpu, "cpu_ms_per_pair": round(secs * 1e3 / ncpu, 3), "bitwise_equal_cpu": cpu_ok})

    # (c) many pairs, as many distinct starts
    ms_, mg_ = synth.sources(g, args.many, 7), synth.sources(g, args.many, 8)
    wall, bfs, backs, st = [], [], [], None
    for i in range(n_all):
        hp, el = timed(lambda: H.hop_paths(snap, ms_, mg_))
        st = hp.stats()
        if i >= args.warmup:
            wall.append(el)
            bfs.append(hp.owner.stats(accounting=False)["ms_total"])
            backs.append(st["ms_total"])
        reached, mh, ns = int(hp.reached.sum()), int(hp.hops.max()), hp.owner.n_seeds
        hp.close()
    back = med(backs)
    emit({"what": "case", "case": "c", "engine": "hop_paths", "pairs": int(len(ms_)), "distinct_starts": int(ns),
          "calls": args.calls, "warmup": args.warmup, "ms_wall_median": med(wall), "ms_per_pair": round(med(wall) / len(ms_), 4),
          "bfs_ms_device_median": med(bfs), "backtrace_ms_device_median": back,
          "backtrace_share_of_wall": round(back / med(wall), 4), "reached_goals": reached, "max_hops": mh,
          "step_launches": st["steps"], "entries": st["entries"], "probes": st["probes"],
          "probes_per_second": round(st["probes"] / (back * 1e-3), 1) if back > 0 else None,
          "algorithmic_mb": round(st["bytes"] / 1e6, 3)})

    # (d) one depth row and one predecessor row (a fresh seed per call: the rows are cached per seed)
    res = H.bfs_batch(snap, starts, None)
    dw, pw = [], []
    for i in range(n_all):
        k = i % len(starts)
        _, el_d = timed(lambda: res.depths(k))
        _, el_p = timed(lambda: res.predecessors(k))
        if i >= args.warmup:
            dw.append(el_d)
            pw.append(el_p)
    res.close()
    emit({"what": "case", "case": "d", "calls": args.calls, "warmup": args.warmup, "depth_row_ms_wall_median": med(dw),
          "predecessor_row_ms_wall_median": med(pw), "row_atoms": int(A)})

    # (e) one pair, both ways
    ea, eb = [], []
    for i in range(n_all):
        sp, el_a = timed(lambda: H.shortest_paths(snap, starts[:1], goals[:1]))
        d1 = float(sp.distance[0])
        sp.close()
        hp, el_b = timed(lambda: H.hop_paths(snap, starts[:1], goals[:1]))
        h1 = int(hp.hops[0])
        hp.close()
        ok = ok and (d1 == (float(h1) if h1 >= 0 else np.inf))
        if i >= args.warmup:
            ea.append(el_a)
            eb.append(el_b)
    spread = max(ea) - min(ea)
    emit({"what": "case", "case": "e", "pairs": 1, "calls": args.calls, "warmup": args.warmup,
          "shortest_paths_ms_wall_median": med(ea), "shortest_paths_ms_wall_min": round(min(ea), 3),
          "shortest_paths_ms_wall_max": round(max(ea), 3), "hop_paths_ms_wall_median": med(eb),
          "hop_paths_ms_wall_min": round(min(eb), 3), "hop_paths_ms_wall_max": round(max(eb), 3),
          "hop_paths_faster_by_more_than_the_spread": bool(med(ea) - med(eb) > spread)})
    snap.close()
    if not ok:
        raise SystemExit("hop_paths disagrees with shortest_paths or with the CPU baseline")


if __name__ == "__main__":
    main()
