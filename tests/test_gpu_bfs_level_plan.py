"""The level plan of the batched BFS, pinned: which kind of level the rows engine runs at every depth, and the
launches, rows and bytes that follow from it.  Every level kind is exact, so a wrong choice passes every oracle
test and only gets slower; this file compares the choice with a recording (tests/golden/bfs_level_plan.json,
written by tests/golden/make_bfs_level_plan.py from the commit before the level loop was split into one routine
per kind).

Each case runs one bfs_batch with HGX_OPT_BFS_BLOCK = 0 and compares, from stats(accounting=False):
  level_sparse, level_new, n_levels_expanded, count_pass_levels;
  kernels[*]["launches"];
  whether nf_hint_atoms and hub_mask_entries are nonzero;
  level_rows and kernels[*]["bytes"].
Two recordings of the same build agreed on every one of these fields but two, which are dropped from the
comparison (DROPPED): kernels["hgx_fc_pull"]["bytes"] and kernels["hgx_fc_pull_heavy"]["bytes"], which differed
in the two unbounded cases with frontier-code levels (their formulas use level counters beyond the eight that
level_rows holds).  level_rows agreed in every field.  The two-part case compares the stats
of both parts.

Cases: the symmetric mode, after-first and a typed generator; 64, 512 and 1024 seeds (rows of 1, 8 and 16 words:
both sides of the 4-lane group); HGX_OPT_BFS_FLAGS 0x3BE, 0x0, 0x1BE, 0x39E, 0x3FE and 0x203BE; HGX_OPT_NF_PULL
0 / 1 / 2, HGX_OPT_NF_HINT 0 / 1, HGX_OPT_HUB_MASK 0 / 2, HGX_OPT_COUNT_FUSED 0 / 1; unbounded depth and depth 1;
chains of more than 64 levels (the counter blocks are cleared 64 levels at a time); two parts over the in-process
transport."""
import functools
import json
import os

import numpy as np
import pytest

import deep_graphs as D
import kat_graphs as K

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfs_level_plan.json")
DROPPED = ("hgx_fc_pull", "hgx_fc_pull_heavy")   # kernels whose bytes differed between two recordings of one build

SYM, AFTER_FIRST = K.ALGEN_MODES[0], K.ALGEN_MODES[1]
DEFAULTS = dict(mode=SYM, lt=-1, maxd=None, flags=0x3BE, nf_pull=1, nf_hint=1, hub_mask=0, fused=1, parts=1)

# name -> graph, seeds and what differs from DEFAULTS
CASES = {
    "pl_1024": dict(graph="power_law", S=1024),
    "pl_1024_nf2": dict(graph="power_law", S=1024, nf_pull=2),
    "pl_1024_nf2_nohint": dict(graph="power_law", S=1024, nf_pull=2, nf_hint=0),
    "pl_512_nf0_unfused": dict(graph="power_law", S=512, nf_pull=0, fused=0),
    "pl_64": dict(graph="power_law", S=64),
    "pl_1024_flags0": dict(graph="power_law", S=1024, flags=0x0),
    "pl_1024_flags1be": dict(graph="power_law", S=1024, flags=0x1BE),
    "pl_64_flags39e": dict(graph="power_law", S=64, flags=0x39E),
    "pl_1024_flags3fe": dict(graph="power_law", S=1024, flags=0x3FE),
    "pl_1024_fc_nf0": dict(graph="power_law", S=1024, flags=0x203BE, nf_pull=0),
    "pl_512_fc": dict(graph="power_law", S=512, flags=0x203BE),
    "pl_512_fc_depth1": dict(graph="power_law", S=512, flags=0x203BE, maxd=1),
    "pl_1024_after_first": dict(graph="power_law", S=1024, mode=AFTER_FIRST),
    "pl_64_after_first_flags1be": dict(graph="power_law", S=64, mode=AFTER_FIRST, flags=0x1BE),
    "pl_1024_typed": dict(graph="power_law", S=1024, lt=1),
    "pl_1024_depth1": dict(graph="power_law", S=1024, maxd=1),
    "hubs_1024_nf0": dict(graph="hubs", S=1024, nf_pull=0),
    "hubs_1024_nf0_unfused": dict(graph="hubs", S=1024, nf_pull=0, fused=0),
    "hub_1024_mask2": dict(graph="hub_graph", S=1024, nf_pull=0, hub_mask=2),
    "hub_512_mask2": dict(graph="hub_graph", S=512, nf_pull=0, hub_mask=2),
    "band_64": dict(graph="band", S=64),
    "band_64_flags39e": dict(graph="band", S=64, flags=0x39E),
    "path_64_fwd": dict(graph="path", S=64, mode=D.FWD),
    "path_64_fwd_flags1be": dict(graph="path", S=64, mode=D.FWD, flags=0x1BE),
    "pl_512_two_parts": dict(graph="power_law", S=512, parts=2),
}


@functools.lru_cache(maxsize=None)
def graph_and_seeds(name, S, lt):
    """The small graphs the other BFS tests build, and S seeds on them (built once, left unchanged)."""
    if name == "power_law":
        from test_gpu_bfs_direct_pull import power_law
        g, has = power_law(21)
        return g, np.random.default_rng(5).choice(has[lt], S, replace=False).astype(np.int32)
    if name == "hubs":
        from test_gpu_bfs_fused_counts import graph
        g, _, has = graph("hubs")
        return g, np.random.default_rng(15).choice(has[lt], S, replace=False).astype(np.int32)
    if name == "hub_graph":
        from test_gpu_bfs_hub_mask import hub_graph
        return hub_graph(4096, S)
    if name == "band":      # 104 levels in the symmetric mode
        g = D.band(200, hubs=2, rng=np.random.default_rng(2024))
    else:                   # "path": 149 levels walked in link order
        g = D.path(150)
    seeds = np.resize(g["pos"][:3], S).astype(np.int32)
    return g, seeds


def observe(st):
    """The compared part of one stats() dict."""
    return {
        "level_sparse": st["level_sparse"], "level_new": st["level_new"],
        "n_levels_expanded": st["n_levels_expanded"], "count_pass_levels": st["count_pass_levels"],
        "launches": {k: v["launches"] for k, v in sorted(st["kernels"].items())},
        "nf_hint_atoms_nonzero": st["nf_hint_atoms"] > 0, "hub_mask_entries_nonzero": st["hub_mask_entries"] > 0,
        "level_rows": st["level_rows"],
        "bytes": {k: v["bytes"] for k, v in sorted(st["kernels"].items())},
    }


def run_case(name):
    """One bfs_batch of the case on the rows engine: a list of observe() dicts, one per part."""
    from hypergraphdb_amd import _lib, bfs_batch
    from test_gpu_bfs import gen, snapshot
    c = dict(DEFAULTS, **CASES[name])
    g, seeds = graph_and_seeds(c["graph"], c["S"], c["lt"])
    if c["parts"] > 1:
        from hypergraphdb_amd.partition import pbfs_batch_group
        from test_gpu_partition import parts
        snaps = parts(g, c["parts"])
    else:
        snaps = [snapshot(g)]
    for s in snaps:
        s.set_option(_lib.HGX_OPT_BFS_BLOCK, 0)
        s.set_option(_lib.HGX_OPT_BFS_FLAGS, c["flags"])
        s.set_option(_lib.HGX_OPT_NF_PULL, c["nf_pull"])
        s.set_option(_lib.HGX_OPT_NF_HINT, c["nf_hint"])
        s.set_option(_lib.HGX_OPT_HUB_MASK, c["hub_mask"])
        s.set_option(_lib.HGX_OPT_COUNT_FUSED, c["fused"])
    if c["parts"] > 1:
        res = pbfs_batch_group(snaps, seeds, c["maxd"], gen(None, c["mode"], c["lt"]))
        out = [observe(st) for st in res.stats(accounting=False)]
    else:
        res = bfs_batch(snaps[0], seeds, c["maxd"], gen(snaps[0], c["mode"], c["lt"]))
        out = [observe(res.stats(accounting=False))]
    res.close()
    for s in snaps:
        s.close()
    return out


@functools.lru_cache(maxsize=None)
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def without_dropped(obs):
    return dict(obs, bytes={k: v for k, v in obs["bytes"].items() if k not in DROPPED})


@pytest.mark.parametrize("name", sorted(CASES))
def test_level_plan_is_the_recorded_one(name):
    want = recorded()[name]
    got = json.loads(json.dumps(run_case(name)))   # (tuples and numpy scalars as JSON holds them)
    assert len(got) == len(want)
    for p, (gp, wp) in enumerate(zip(got, want)):
        gp, wp = without_dropped(gp), without_dropped(wp)
        for key in wp:
            assert gp[key] == wp[key], (name, p, key, gp[key], wp[key])
        assert sorted(gp) == sorted(wp)


def test_the_recording_covers_every_level_kind():
    rec = recorded()
    assert sorted(rec) == sorted(CASES)
    runs = [part for name in rec for part in rec[name]]
    kinds = set().union(*(r["level_sparse"] for r in runs))
    assert kinds >= {0, 1, 2, 3, 4}, kinds
    assert any(r["hub_mask_entries_nonzero"] for r in runs)
    assert any(r["nf_hint_atoms_nonzero"] for r in runs)
    assert any(r["count_pass_levels"] == 0 and 0 in r["level_sparse"] for r in runs)
    assert any(r["n_levels_expanded"] > 64 for r in runs)   # crosses a boundary of the counter blocks' clearing
