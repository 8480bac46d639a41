"""The routing of the order-exact traversal, pinned: which engine finishes which seeds of hgx_bfs_sequence (the
workgroup stage, the chained or unchained grid stage, the level engine and its key-array fallback) and of the
workgroup stage of hgx_bfs_batch.  Every engine is exact, so seeds sent to the wrong one pass every oracle test
and only get slower; this file compares the routing with a recording (tests/golden/seq_routing.json, written by
tests/golden/make_seq_routing.py from the commit before the traversal's host code was split into one routine per
stage).

A case is a list of calls on one snapshot.  Per hgx_bfs_sequence call, from SequenceResult: n_levels, the offsets
(their count, their last entry and a SHA-256 of the int64 array: 1101 numbers a call would make the fixture large), a
SHA-256 of links / atoms / dists, n_block, n_level, n_coop, pull_levels, traversed_edges, bytes_block, bytes_level
and bytes_coop.  Per hgx_bfs_batch call, from stats(accounting=False): block_seeds, block_rerun, block_coop (the
seeds the grid stage took), coop_fallbacks, the bytes of hgx_bfs_block and hgx_bfs_coop, n_levels_expanded and
traversed_edges, next to a SHA-256 of counts().

Two recordings of the same build agreed on every field of every call but two, which are dropped from the
comparison (DROPPED): bytes_block and bytes_coop, of hgx_bfs_sequence and of hgx_bfs_batch alike.  Both are sums
over racing workgroups: a seed that outgrows its workgroup stops at a point that depends on the interleaving, and
the grid stage's blocks share a level's work differently from run to run.  They differed by up to 3% in 25 of the
91 calls; bytes_level, traversed_edges and every count agreed in all of them.

Sequence cases: engines 0, 1 and 2; 1, 63, 64, 65 (both sides of kSeqChainMin) and 1100 (> kSbChunk) seeds; a few
seeds that outgrow a workgroup among small ones (at most kMaxCoSeeds of them: the grid stage; more: the level
engine); every generator mode and a typed generator (the symmetric mode without a type has no yield adjacency:
no grid stage); reverse_order; HGX_OPT_SEQ_PULL 0, 1 and 2; HGX_OPT_SEQ_SMALL 1; HGX_OPT_SEQ_TLIMIT 2000 (chunks
split down to single seeds, which then run on the key-array engine); HGX_OPT_SEQ_PACK_MIN 1 (only with A <= 2^24,
3-byte atoms: a graph of more than 2^24 atoms is not affordable at test size); depth limits 0, 1 and unbounded;
two calls on one snapshot (the capacities kept on the graph carry over).  Batch cases: HGX_OPT_BFS_BLOCK 1 and 2
with HGX_CO_CHAIN unset.  No case forces a barrier timeout (test_order_exact_grid_stage_vs_oracle does)."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import kat_graphs as K

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_routing.json")
DROPPED = ("bytes_block", "bytes_coop")   # fields that differed between two recordings of one build
NEVER_DROPPED = ("n_block", "n_level", "n_coop", "pull_levels", "n_levels", "n_seeds", "n_pairs", "offsets_sha256",
                 "pairs_sha256")

SYM, AFTER_FIRST = K.ALGEN_MODES[0], K.ALGEN_MODES[1]
SUBSUMED, SUBSUMES = (False, True, False, False), (False, True, True, False)   # config 5: lt = the subsumes type
SEQ_OPTS = {"engine": "HGX_OPT_SEQ_ENGINE", "pull": "HGX_OPT_SEQ_PULL", "small": "HGX_OPT_SEQ_SMALL",
            "tlimit": "HGX_OPT_SEQ_TLIMIT", "pack_min": "HGX_OPT_SEQ_PACK_MIN", "block": "HGX_OPT_BFS_BLOCK"}


def seq(mode=AFTER_FIRST, lt=-1, maxd=None, **opts):
    return dict(kind="seq", mode=mode, lt=lt, maxd=maxd, opts=opts)


def batch(block, mode=AFTER_FIRST, lt=-1, maxd=None):
    return dict(kind="batch", mode=mode, lt=lt, maxd=maxd, opts={"block": block})


# name -> graph, seeds (see graph_and_seeds) and the calls made on one snapshot
CASES = {
    # seed counts around kSeqChainMin and past kSbChunk; three seeds outgrow a workgroup
    **{f"dag_{s}": dict(graph="dag", seeds=("mix", 3, s - 3 if s > 3 else 0), calls=[seq(SUBSUMED, "T")])
       for s in (63, 64, 65, 1100)},
    "dag_1_big": dict(graph="dag", seeds=("mix", 1, 0), calls=[seq(SUBSUMED, "T")]),
    "dag_1_small": dict(graph="dag", seeds=("mix", 0, 1), calls=[seq(SUBSUMED, "T")]),
    "dag_few_big": dict(graph="dag", seeds=("mix", 8, 40), calls=[seq(SUBSUMED, "T")]),
    "dag_few_big_chained": dict(graph="dag", seeds=("mix", 8, 100), calls=[seq(SUBSUMED, "T")]),
    "dag_depths": dict(graph="dag", seeds=("mix", 4, 96), calls=[seq(SUBSUMED, "T", maxd=d) for d in (0, 1, 3, None)]),
    "dag_reverse": dict(graph="dag", seeds=("mix", 4, 96), calls=[seq(SUBSUMES, "T"), seq(SUBSUMES, "T", maxd=2)]),
    "dag_engines": dict(graph="dag", seeds=("mix", 3, 30), calls=[seq(SUBSUMED, "T", engine=e) for e in (1, 2, 0)]),
    # the power-law graph: node seeds reach most of the graph, link atoms reach nothing
    "pl_few_big": dict(graph="power_law", seeds=("mix", 5, 40), calls=[seq(), seq(lt=2)]),
    "pl_many_big": dict(graph="power_law", seeds=("mix", 80, 40), calls=[seq()]),
    "pl_many_big_unchained": dict(graph="power_law", seeds=("mix", 40, 10), calls=[seq()]),
    "pl_sym_no_adjacency": dict(graph="power_law", seeds=("mix", 5, 70), calls=[seq(SYM), seq(SYM, lt=1)]),
    "pl_pull": dict(graph="power_law", seeds=("rand", 130), calls=[seq(SYM, engine=2, pull=p) for p in (0, 1, 2)]),
    "pl_pull_after_first": dict(graph="power_law", seeds=("rand", 70),
                                calls=[seq(engine=2, pull=p, maxd=d) for p in (0, 1, 2) for d in (None, 2)]),
    "pl_small": dict(graph="power_law", seeds=("rand", 6), calls=[seq(SYM, engine=2, small=1),
                                                                  seq(SYM, engine=2, small=1, pull=2)]),
    "pl_small_depths": dict(graph="power_law", seeds=("rand", 6),
                            calls=[seq(SYM, engine=2, small=1, maxd=d) for d in (0, 1, None)]),
    "pl_tlimit": dict(graph="power_law", seeds=("hubs", 4, 20), calls=[seq(SYM, engine=2, tlimit=2000, maxd=3),
                                                                       seq(SYM, engine=2, tlimit=200000, maxd=3)]),
    "pl_packed": dict(graph="power_law", seeds=("rand", 70), calls=[seq(SYM, engine=2, pack_min=1),
                                                                    seq(engine=2, pack_min=1, maxd=2)]),
    "pl_two_calls": dict(graph="power_law", seeds=("rand", 40), calls=[seq(SYM, engine=2, small=1), seq(SYM, engine=2),
                                                                       seq(SYM, engine=2, small=1, maxd=2)]),
    "pl_key_array": dict(graph="power_law", seeds=("rand", 9), calls=[seq(SYM, engine=1), seq(engine=1, maxd=2)]),
    "kat_modes": dict(graph="kat", seeds=("rand", 70), calls=[seq(m) for m in K.ALGEN_MODES]),
    "kat_modes_typed": dict(graph="kat", seeds=("rand", 130), calls=[seq(m, lt=1) for m in K.ALGEN_MODES]),
    "kat_modes_level_engine": dict(graph="kat", seeds=("rand", 70), calls=[seq(m, engine=2) for m in K.ALGEN_MODES]),
    # hgx_bfs_batch: the workgroup stage with the chained grid stage (1) and every seed to the grid stage (2)
    "batch_dag": dict(graph="dag", seeds=("mix", 8, 200), calls=[batch(1, SUBSUMED, "T"), batch(1, SUBSUMED, "T", 2)]),
    "batch_dag_grid_only": dict(graph="dag", seeds=("mix", 4, 20), calls=[batch(2, SUBSUMED, "T")]),
    "batch_pl": dict(graph="power_law", seeds=("mix", 5, 200), calls=[batch(1, SYM), batch(1), batch(1, SYM, maxd=1)]),
    "batch_pl_many_big": dict(graph="power_law", seeds=("mix", 80, 40), calls=[batch(1, SYM)]),
    "batch_pl_grid_only": dict(graph="power_law", seeds=("mix", 3, 30), calls=[batch(2, SYM), batch(2)]),
}


@functools.lru_cache(maxsize=None)
def graph(name):
    """The small graphs the other traversal tests build (built once, left unchanged)."""
    from hypergraphdb_amd import synth
    if name == "power_law":    # test_power_law_hubs_and_chunking
        return synth.hypergraph(3000, 20000, 2, 8, 2.1, 3, seed=21)
    if name == "kat":
        return K.random_graph(np.random.default_rng(40), 3000, 2000, max_arity=9, link_targets=True, n_types=3)
    return synth.config5(scale=0.05, n_sources=40)   # "dag": test_order_exact_grid_stage_vs_oracle


@functools.lru_cache(maxsize=None)
def dag_big():
    """Classes of the DAG whose hg.subsumed closure outgrows the workgroup engine (> 2046 pairs) but stays below
    the grid stage's per-level key space, as test_order_exact_grid_stage_vs_oracle picks them."""
    from hypergraphdb_amd import bfs_batch
    from test_gpu_bfs import gen, snapshot
    g = graph("dag")
    snap = snapshot(g)
    cand = np.concatenate([np.arange(4000, dtype=np.int32), np.asarray(g["seeds"], np.int32)])
    r = bfs_batch(snap, cand, None, gen(snap, SUBSUMED, int(g["subsumes_type"])))
    size = r.counts()[:, 1:].sum(1)
    r.close()
    snap.close()
    return cand[(size > 2100) & (size < 30000)][:8]


def graph_and_seeds(name, spec):
    g = graph(name)
    A = g["num_atoms"]
    if spec[0] == "rand":
        return g, np.random.default_rng(41).integers(0, A, spec[1]).astype(np.int32)
    if spec[0] == "hubs":      # test_level_engine_chunk_split_on_wide_keys
        deg = np.bincount(np.asarray(g["tgt_idx"]), minlength=A)
        return g, np.concatenate([np.argsort(-deg, kind="stable")[:spec[1]], np.arange(100, 100 + spec[2])]).astype(np.int32)
    n_big, n_small = spec[1:]
    if name == "dag":
        big, small = np.resize(dag_big(), n_big), np.resize(np.asarray(g["seeds"], np.int32), n_small)
    else:                      # nodes 0..2999 (hubs first), then the link atoms
        big, small = np.arange(n_big, dtype=np.int32), np.arange(A - n_small, A, dtype=np.int32)
    seeds = np.concatenate([big, small]).astype(np.int32)
    return g, seeds[np.random.default_rng(7).permutation(len(seeds))]   # the big ones anywhere in the batch


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def observe_seq(r):
    return {"n_levels": r.n_levels, "n_seeds": r.n_seeds, "n_pairs": int(r.offsets[-1]),
            "offsets_sha256": sha(np.asarray(r.offsets, np.int64)), "pairs_sha256": sha(r.links, r.atoms, r.dists),
            "n_block": r.n_block, "n_level": r.n_level, "n_coop": r.n_coop, "pull_levels": r.pull_levels,
            "traversed_edges": r.traversed_edges, "bytes_block": r.bytes_block, "bytes_level": r.bytes_level,
            "bytes_coop": r.bytes_coop}


def observe_batch(res):
    st = res.stats(accounting=False)
    k = st["kernels"]
    return {"block_seeds": st["block_seeds"], "block_rerun": st["block_rerun"], "block_coop": st["block_coop"],
            "coop_fallbacks": st["coop_fallbacks"], "n_levels_expanded": st["n_levels_expanded"],
            "traversed_edges": st["traversed_edges"],
            "bytes_block": k["hgx_bfs_block"]["bytes"] if "hgx_bfs_block" in k else None,
            "bytes_coop": k["hgx_bfs_coop"]["bytes"] if "hgx_bfs_coop" in k else None,
            "counts_sha256": sha(res.counts())}


def run_case(name):
    """The calls of the case on one fresh snapshot: a list of observe_*() dicts."""
    from hypergraphdb_amd import _lib, bfs_batch, bfs_sequence
    from test_gpu_bfs import gen, snapshot
    assert not os.environ.get("HGX_CO_CHAIN")
    c = CASES[name]
    g, seeds = graph_and_seeds(c["graph"], c["seeds"])
    snap = snapshot(g)
    out = []
    for call in c["calls"]:
        lt = int(g["subsumes_type"]) if call["lt"] == "T" else call["lt"]
        for k, v in call["opts"].items():
            snap.set_option(getattr(_lib, SEQ_OPTS[k]), int(v))
        if call["kind"] == "seq":
            out.append(observe_seq(bfs_sequence(snap, seeds, call["maxd"], gen(snap, call["mode"], lt))))
        else:
            res = bfs_batch(snap, seeds, call["maxd"], gen(snap, call["mode"], lt))
            out.append(observe_batch(res))
            res.close()
        for k in call["opts"]:   # back to the defaults (what the graph has learnt stays)
            snap.set_option(getattr(_lib, SEQ_OPTS[k]), {"pull": 1, "block": 1}.get(k, 0))
    snap.close()
    return out


@functools.lru_cache(maxsize=None)
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_routing_is_the_recorded_one(name):
    want = recorded()[name]
    got = json.loads(json.dumps(run_case(name)))   # (numpy scalars as JSON holds them)
    assert len(got) == len(want)
    for i, (gc, wc) in enumerate(zip(got, want)):
        assert sorted(gc) == sorted(wc)
        for key in wc:
            if key not in DROPPED:
                assert gc[key] == wc[key], (name, i, key, gc[key], wc[key])


def test_the_recording_covers_every_route():
    rec = recorded()
    assert sorted(rec) == sorted(CASES) and not set(DROPPED) & set(NEVER_DROPPED)
    sq = {n: [c for c in rec[n] if "n_block" in c] for n in rec}
    calls = [c for n in sq for c in sq[n]]
    # the workgroup stage alone; the grid stage unchained (< kSeqChainMin seeds) and chained; the level engine
    # behind the workgroup stage (more than kMaxCoSeeds handed over, or no yield adjacency) and alone
    assert any(c["n_level"] == 0 and c["n_block"] > 0 for c in calls)
    assert sq["dag_63"][0]["n_coop"] > 0 and sq["dag_63"][0]["n_block"] > 0
    assert sq["dag_1_big"][0]["n_coop"] == 1 and sq["dag_1_small"][0]["n_block"] == 1
    for n in ("dag_64", "dag_65", "dag_1100", "dag_few_big_chained"):
        assert sq[n][0]["n_coop"] > 0 and sq[n][0]["n_coop"] == sq[n][0]["n_level"], n
    assert sq["pl_many_big"][0]["n_level"] > 64 and sq["pl_many_big"][0]["n_coop"] == 0
    assert all(c["n_coop"] == 0 and c["n_level"] > 0 and c["n_block"] > 0 for c in sq["pl_sym_no_adjacency"])
    assert all(c["n_block"] == 0 for c in sq["pl_pull"] + sq["pl_key_array"])
    assert sq["pl_pull"][0]["pull_levels"] == 0 < sq["pl_pull"][2]["pull_levels"]
    bt = [c for n in rec for c in rec[n] if "block_coop" in c]
    assert any(c["block_coop"] > 0 and c["block_seeds"] > 0 for c in bt)
    assert any(c["block_coop"] == c["block_seeds"] > 0 for c in bt)             # HGX_OPT_BFS_BLOCK 2
    assert any(c["block_rerun"] > 64 and c["block_coop"] == 0 for c in bt)      # more than the grid stage takes
    assert all(c["coop_fallbacks"] == 0 for c in bt)                            # no barrier timed out
