"""Sweep of HGX_OPT_HUB_MASK on the config-2 headline step: T and the hub pull's test
schedule.  One snapshot, per setting one warm-up and `--steps` timed batches; prints one JSON line per setting
with the host wall per step, the device ms of the level-1 hub pull (hgx_atom_pull_heavy's slot of the statistics)
and of the gather, and the two hub-mask counters.

  python tools/hub_mask_sweep.py [--scale 1.0] [--steps 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import hypergraphdb_amd as H
    from hypergraphdb_amd import _lib, synth
    g = synth.config2(scale=args.scale, n_sources=1024)
    snap = H.HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"])
    snap.set_timing(True)
    settings = [("off", 0, 0, 0)]
    settings += [(f"T{t}", 1, t, 0) for t in (8, 16, 32, 64)]
    settings += [(f"sched{s:#x}", 1, 32, s) for s in (0xFFFF, 0x5555, 0x1, 0x3, 0xB, 0x8B, 0x808B)]
    settings += [("forced", 2, 32, 0), ("off again", 0, 0, 0)]
    out = open(args.out, "a") if args.out else None
    for name, mode, t, sched in settings:
        snap.set_option(_lib.HGX_OPT_HUB_MASK, mode + (t << 8) + (sched << 16))
        H.bfs_batch(snap, g["seeds"], 4).close()
        wall, heavy, gather, pull = [], [], [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            res = H.bfs_batch(snap, g["seeds"], 4)
            res.counts()
            wall.append((time.perf_counter() - t0) * 1e3)
            st = res.stats(accounting=False)
            heavy.append(st["kernels"]["hgx_atom_pull_heavy"]["ms"])
            gather.append(st["kernels"]["hgx_link_gather"]["ms"])
            pull.append(st["kernels"]["hgx_atom_pull"]["ms"])
            res.close()
        line = json.dumps({"setting": name, "mode": mode, "T": t, "sched": sched,
                           "wall_ms": round(sorted(wall)[len(wall) // 2], 3), "wall_min": round(min(wall), 3),
                           "hub_pull_ms": round(sorted(heavy)[len(heavy) // 2], 3),
                           "gather_ms": round(sorted(gather)[len(gather) // 2], 3),
                           "light_pull_ms": round(sorted(pull)[len(pull) // 2], 3),
                           "hub_mask_entries": st["hub_mask_entries"], "hub_mask_skipped": st["hub_mask_skipped"],
                           "hub_rows_read": int(st["level_rows"][1][5])})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    snap.close()


if __name__ == "__main__":
    main()
