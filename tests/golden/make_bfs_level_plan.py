"""Records tests/golden/bfs_level_plan.json: the level plan of every case of tests/test_gpu_bfs_level_plan.py as
the build in the tree runs it (needs the GPU).  The committed fixture was recorded on the commit before the level
loop was split into one routine per level kind, and is kept as recorded; record a build twice and compare the two
files before trusting a field (a field that differs between them belongs in DROPPED of the test).
Usage:  python tests/golden/make_bfs_level_plan.py [out.json]
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import test_gpu_bfs_level_plan as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    rec = {}
    for name in sorted(T.CASES):
        rec[name] = T.run_case(name)
        r = rec[name][0]
        print(name, r["level_sparse"][:12], "levels", r["n_levels_expanded"], "pass", r["count_pass_levels"],
              "hint", r["nf_hint_atoms_nonzero"], "mask", r["hub_mask_entries_nonzero"], flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("written:", out)


if __name__ == "__main__":
    main()
