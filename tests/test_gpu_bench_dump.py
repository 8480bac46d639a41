"""A plain `bench.py --gpus 1` run is the headline alone (the other legs wait for --full), and
`--dump-outputs DIR` writes the last timed step's results: the whole counts readout and the sampled
visited sets, both equal to the oracle's on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_headline_and_dumps_its_outputs(tmp_path):
    from hypergraphdb_amd import synth
    from oracle_ctypes import OracleGraph
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--scale", "0.002", "--sources", "64", "--depth", "3", "--dump-outputs", out], env=env,
                       capture_output=True, text=True, timeout=100)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "TEPS" and line["higher_is_better"] is True
    for leg in ("cpu_baseline", "pattern", "subsumption", "dropin"):
        assert line[leg] is None
    assert "config4" not in line

    g = synth.config2(scale=0.002, n_sources=64)
    orc = OracleGraph(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g["link_type"])
    counts = np.load(os.path.join(out, "counts.npy"))
    index = np.load(os.path.join(out, "visited_index.npy"))
    atoms = np.load(os.path.join(out, "visited_atoms.npy"))
    assert counts.dtype == index.dtype == atoms.dtype == np.float64
    nl = counts.shape[1]   # the levels the batch reached: depth + 1 at most
    assert counts.shape[0] == 64 and 2 <= nl <= 4
    oc, _ = orc.bfs_many(g["seeds"], 3, 4)
    assert np.array_equal(counts, oc[:, :nl]) and not oc[:, nl:].any()
    assert len(index) == 8 * nl and int(index[:, 3].sum()) == len(atoms)
    assert len(np.unique(index[:, 0])) == 8
    at = 0
    for i, d, n, k in index.astype(np.int64):
        assert n == counts[i, d] and k == n   # sets this small are written whole
        levels = orc.bfs_levels(int(g["seeds"][i]), 3)
        assert np.array_equal(atoms[at:at + k], levels[d] if d < len(levels) else [])
        at += k
