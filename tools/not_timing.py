#!/usr/bin/env python3
"""Cost of hg.not on the config-3 graph: the bench's 10K config-3 queries (type T, incident(a),
orderedLink(x, _, y)) as one-clause DNF queries, the graph resident in HBM, run three ways, the three
alternating inside every round:

  plain         as they are, through hgx_pattern_batch_dnf
  not_incident  each with not(incident(r)) added, r a random node (seed 45): few hits are rejected
  not_type      each with not(type(T)) added, T the query's own type: every hit is rejected

  python tools/not_timing.py [--scale 1.0] [--calls 20] [--warmup 3] [--out FILE] [--baseline-only]

Per leg: ms per call from a host clock around the call (the call ends in the engine's synchronisation),
the device ms of the batch and ms_not / ms_union from the engine's events, medians over the timed calls, and
bytes_not / ms_not.  The not_incident and not_type results are checked against the plain one filtered on the
host.  --baseline-only runs the plain leg alone and uses nothing newer than hgx_pattern_batch_dnf, so it runs
on an older build (HGX_LIB_VARIANT) for the comparison against it.  One JSON line is printed (and appended to
--out).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 10:
        ap.error("--calls: at least 10 timed calls")
    import hypergraphdb_amd as H
    from hypergraphdb_amd import _lib, synth
    from hypergraphdb_amd.query import _read_result

    g = synth.config3(scale=args.scale, n_queries=args.queries)
    snap = H.HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"])
    snap.set_timing(True)
    Q, n = g["queries"], len(g["queries"]["type"])
    T, a, x, y = (np.asarray(Q[k], np.int32) for k in ("type", "a", "x", "y"))
    one = np.arange(n + 1, dtype=np.int64)
    dnf = (one, one, T, one, a, np.zeros(n + 1, np.int64), np.zeros(1, np.int32), one,
           np.arange(0, 3 * n + 1, 3, dtype=np.int64), np.stack([x, np.full(n, -1, np.int32), y], 1).reshape(-1),
           np.full(n, -1, np.int32))
    L = _lib.lib()

    def leg(entry, arrays, tail=()):
        """The C entry itself and the readers of its header: the same thin host path for every leg and build."""
        ptrs = [v.ctypes.data for v in arrays]

        def run():
            h, ms_u = C.c_void_p(), C.c_double()
            _lib.check(entry(snap.handle, n, *ptrs, *tail, C.byref(h)))
            rc = L.hgx_query_result_union_stats(h, None, None, C.byref(ms_u), None)
            neg = None
            if tail:
                te, rj, ms_n, by_n = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
                rc = rc or L.hgx_query_result_not_stats(h, C.byref(te), C.byref(rj), C.byref(ms_n), C.byref(by_n))
                neg = {"hits_tested": te.value, "hits_rejected": rj.value, "ms_not": ms_n.value, "bytes_not": by_n.value}
            r = _read_result(h, n)   # frees the result
            _lib.check(rc)
            r.union, r.negation = {"ms_union": ms_u.value}, neg
            return r

        return run

    legs = {"plain": leg(L.hgx_pattern_batch_dnf, dnf)}
    if not args.baseline_only:
        from hypergraphdb_amd.query import NOT_INCIDENT, NOT_TYPE
        r_node = np.random.default_rng(45).integers(0, g["n_nodes"], n).astype(np.int32)

        def program(kind, operand):   # one negation of one term of one positive literal per clause
            lit = np.stack([np.full(n, kind, np.int32), np.ones(n, np.int32), np.arange(n, dtype=np.int32),
                            np.arange(1, n + 1, dtype=np.int32)], 1).reshape(-1)
            return one, one, one, lit, operand

        p_inc, p_type = program(NOT_INCIDENT, r_node), program(NOT_TYPE, T)
        legs["not_incident"] = leg(L.hgx_pattern_batch_dnf_not, dnf + p_inc, (n,))
        legs["not_type"] = leg(L.hgx_pattern_batch_dnf_not, dnf + p_type, (n,))
    wall, res = {k: [] for k in legs}, {}
    dev, msn, msu = ({k: [] for k in legs} for _ in range(3))
    for i in range(args.warmup + args.calls):
        for k, run in legs.items():
            t = time.perf_counter()
            r = run()
            el = (time.perf_counter() - t) * 1e3
            res[k] = r
            if i >= args.warmup:
                wall[k].append(el)
                dev[k].append(r.ms["ms_total"])
                msu[k].append(r.union["ms_union"])
                msn[k].append(r.negation["ms_not"] if r.negation else 0.0)
    plain = res["plain"]
    rec = {"what": "not_timing", "variant": _lib.LIB_VARIANT or "product", "scale": args.scale, "queries": n,
           "calls": args.calls, "warmup": args.warmup, "num_links": int(len(g["link_atom"])), "hits": int(len(plain.ids)),
           "result_crc": zlib.crc32(plain.ids.tobytes(), zlib.crc32(plain.offsets.tobytes()))}
    if not args.baseline_only:
        # the filtered results, from the plain one on the host
        row = np.searchsorted(g["link_atom"], plain.ids)
        off, tg = g["tgt_off"], g["tgt_idx"]
        q_of = np.repeat(np.arange(n), np.diff(plain.offsets))
        has_r = np.array([r_node[q] in tg[off[w]:off[w + 1]] for q, w in zip(q_of, row)], bool)
        ri = res["not_incident"]
        if not (np.array_equal(ri.ids, plain.ids[~has_r]) and
                np.array_equal(np.diff(ri.offsets), np.bincount(q_of[~has_r], minlength=n))):
            raise SystemExit("not_incident differs from the plain result filtered on the host")
        if len(res["not_type"].ids) or res["not_type"].offsets.any():
            raise SystemExit("not_type kept a hit")
    for k in legs:
        r = res[k]
        rec[k] = {"ms_wall_median": round(float(np.median(wall[k])), 4), "ms_wall_min": round(min(wall[k]), 4),
                  "ms_wall_p90": round(float(np.percentile(wall[k], 90)), 4),
                  "ms_device_median": round(float(np.median(dev[k])), 4),
                  "ms_union_median": round(float(np.median(msu[k])), 4), "ms_not_median": round(float(np.median(msn[k])), 4),
                  "kept": int(len(r.ids))}
        if r.negation and r.negation["hits_tested"]:
            rec[k].update({"hits_tested": r.negation["hits_tested"], "hits_rejected": r.negation["hits_rejected"],
                           "bytes_not": r.negation["bytes_not"],
                           "not_gb_per_s": round(r.negation["bytes_not"] / max(float(np.median(msn[k])), 1e-9) / 1e6, 2)})
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    snap.close()


if __name__ == "__main__":
    main()
