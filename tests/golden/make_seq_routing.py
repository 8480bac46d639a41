"""Records tests/golden/seq_routing.json: the routing of every case of tests/test_gpu_seq_routing.py as the build
in the tree runs it (needs the GPU).  The committed fixture was recorded on the commit before the order-exact
traversal's host code was split into one routine per stage, and is kept as recorded; record a build twice and
compare the two files before trusting a field (a field that differs between them belongs in DROPPED of the test).
Usage:  python tests/golden/make_seq_routing.py [out.json]
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import test_gpu_seq_routing as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
    rec = {}
    for name in sorted(T.CASES):
        rec[name] = T.run_case(name)
        for c in rec[name]:
            if "n_block" in c:
                print(name, "seeds", c["n_seeds"], "block", c["n_block"], "level", c["n_level"], "coop",
                      c["n_coop"], "pulls", c["pull_levels"], "levels", c["n_levels"], "pairs", c["n_pairs"], flush=True)
            else:
                print(name, "batch: block", c["block_seeds"], "rerun", c["block_rerun"], "coop", c["block_coop"],
                      "fallbacks", c["coop_fallbacks"], flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("written:", out)


if __name__ == "__main__":
    main()
