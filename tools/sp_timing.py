#!/usr/bin/env python3
"""Shortest-path timing on the config-2 graph: hgx_shortest_paths against a single-thread binary-heap
Dijkstra (tools/native/sp_cpu.cc) and, for unit weights, against hgx_bfs_batch unbounded + depth_of.

  python tools/sp_timing.py [--scale 1.0] [--calls 10] [--warmup 2] [--out FILE]

Cases (64 random pairs over nodes with incidence, seed 7 / 8):
  a  unit weights, goal-terminated
  b  random integer weights 1..16, goal-terminated
  c  4 HGX_NO_GOAL sources, weights of b
Per case: ms per call from device events and from a host clock around a device synchronise, rounds,
edges relaxed, improvements.  The CPU baseline runs on the first --cpu-pairs pairs (--cpu-sources for c:
one full single-source run over this graph examines ~10^9 edges) and the GPU distances of those pairs must
equal it bitwise, or the tool fails.  One JSON line per case is printed (and appended to --out).
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


def cpu_lib():
    L = C.CDLL(os.path.join(ROOT, "tools", "native", "build", "libsp_cpu.so"))
    vp = C.c_void_p
    L.sp_cpu_build.argtypes = [C.c_int64, C.c_int64, vp, vp, vp]
    L.sp_cpu_build.restype = vp
    L.sp_cpu_free.argtypes = [vp]
    L.sp_cpu_run.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, C.POINTER(C.c_int64)]
    L.sp_cpu_run.restype = C.c_double
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-pairs", type=int, default=2)
    ap.add_argument("--cpu-sources", type=int, default=1)
    ap.add_argument("--cases", default="a,b,c")
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

    t0 = time.perf_counter()
    g = synth.config2(scale=args.scale, n_sources=16)
    A, M = g["num_atoms"], len(g["link_atom"])
    starts = synth.sources(g, args.pairs, 7)
    goals = synth.sources(g, args.pairs, 8)
    rng = np.random.default_rng(9)
    w16 = rng.integers(1, 17, M).astype(np.float64)
    snap = H.HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"],
                                keep_host=False)
    snap.set_timing(True)
    L = cpu_lib()
    tg = np.ascontiguousarray(g["tgt_idx"], np.int32)
    cpu = L.sp_cpu_build(A, M, g["tgt_off"].ctypes.data, tg.ctypes.data, g["link_type"].ctypes.data)
    emit({"what": "setup", "scale": args.scale, "num_atoms": int(A), "num_links": int(M), "pins": int(len(tg)),
          "seconds": round(time.perf_counter() - t0, 2)})
    lw16 = H.LinkWeights(snap, w16)
    nog = np.full(args.sources, _lib.HGX_NO_GOAL, np.int32)
    cases = {"a": (starts, goals, None, None, args.cpu_pairs),
             "b": (starts, goals, lw16, w16, args.cpu_pairs),
             "c": (starts[:args.sources], nog, lw16, w16, args.cpu_sources)}
    for name in args.cases.split(","):
        s, q, lw, w, ncpu = cases[name]
        dev, wall, st, dist, rows = [], [], None, None, None
        for i in range(args.warmup + args.calls):
            _lib.device_synchronize(snap.device)
            t = time.perf_counter()
            res = H.shortest_paths(snap, s, q, None, lw)
            _lib.device_synchronize(snap.device)
            el = (time.perf_counter() - t) * 1e3
            st = res.stats()
            if i == 0:
                dist = res.distance.copy()
                if name == "c":
                    rows = [res.distances(k) for k in range(min(ncpu, len(s)))]
            else:
                assert np.array_equal(dist.view(np.uint64), res.distance.view(np.uint64)), "calls differ"
            res.close()
            if i >= args.warmup:
                dev.append(st["ms_total"])
                wall.append(el)
        rec = {"what": "case", "case": name, "pairs": int(len(s)), "calls": args.calls, "warmup": args.warmup,
               "gpu_ms_device_median": round(float(np.median(dev)), 3), "gpu_ms_device_min": round(min(dev), 3),
               "gpu_ms_wall_median": round(float(np.median(wall)), 3), "gpu_ms_wall_min": round(min(wall), 3),
               "gpu_ms_per_pair": round(float(np.median(wall)) / len(s), 3),
               "rounds": st["rounds"], "expanded": st["expanded"], "relaxed": st["relaxed"], "improved": st["improved"],
               "reached_goals": int(np.isfinite(dist).sum()), "algorithmic_gb": round(st["bytes"] / 1e9, 3)}
        # CPU baseline on the first ncpu pairs, compared bitwise
        ncpu = min(ncpu, len(s))
        cs, cq = np.ascontiguousarray(s[:ncpu], np.int32), np.ascontiguousarray(q[:ncpu], np.int32)
        cd = np.zeros(ncpu)
        crow = np.zeros(ncpu * A if name == "c" else 1)
        nrel = C.c_int64()
        secs = L.sp_cpu_run(cpu, 0, -1, None if w is None else w.ctypes.data, cs.ctypes.data, cq.ctypes.data, ncpu,
                            cd.ctypes.data, crow.ctypes.data if name == "c" else None, C.byref(nrel))
        rec.update({"cpu_pairs": ncpu, "cpu_ms_per_pair": round(secs * 1e3 / ncpu, 3), "cpu_relaxed": nrel.value})
        ok = np.array_equal(cd.view(np.uint64), dist[:ncpu].view(np.uint64))
        if name == "c":
            for k in range(ncpu):
                ok = ok and np.array_equal(crow[k * A:(k + 1) * A].view(np.uint64), rows[k].view(np.uint64))
        rec["bitwise_equal_cpu"] = bool(ok)
        if name == "a":   # what a user could do before: BFS to exhaustion + depth_of (unit weights only, no path)
            bw = []
            depth = None
            for i in range(args.warmup + args.calls):
                _lib.device_synchronize(snap.device)
                t = time.perf_counter()
                br = H.bfs_batch(snap, s, None)
                depth = [br.depth_of(k, int(q[k])) for k in range(len(s))]
                _lib.device_synchronize(snap.device)
                if i >= args.warmup:
                    bw.append((time.perf_counter() - t) * 1e3)
                br.close()
            exp = np.array([np.inf if d < 0 else float(d) for d in depth])
            rec.update({"bfs_ms_wall_median": round(float(np.median(bw)), 3),
                        "bfs_equal": bool(np.array_equal(exp, dist))})
            ok = ok and rec["bfs_equal"]
        emit(rec)
        if not ok:
            raise SystemExit(f"case {name}: the GPU distances differ from the baseline")
    L.sp_cpu_free(cpu)
    lw16.close()
    snap.close()


if __name__ == "__main__":
    main()
