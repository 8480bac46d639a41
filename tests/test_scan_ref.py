"""CPU tests of the type-scan layer (include/hgx_scan.h): libhgx.so exports the header's boundary, the host
lowering of clauses without an incidence anchor (split_type_scan), the brute-force evaluator of tests/not_ref.py
on hand-written anchor-free trees, and the properties of the random trees the GPU test relies on.  No GPU
compute."""
import os
import re

import numpy as np

import dnf_ref as D
import kat_graphs as K
import not_ref as N
import scan_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_abi_exported_and_bound():
    import hypergraphdb_amd
    from hypergraphdb_amd import _lib
    src = open(os.path.join(ROOT, "include", "hgx_scan.h")).read()
    # the header's comments may name entries of the headers it extends
    declared = sorted(set(re.findall(r"\b(hgx_[a-z_]+)\s*\(", src)) - set(_lib.EXPORTED) - set(_lib.EXPORTED_DNF) -
                      set(_lib.EXPORTED_NOT))
    assert declared == sorted(_lib.EXPORTED_SCAN) and len(declared) == 3
    for other in ("hgx.h", "hgx_dnf.h", "hgx_not.h"):    # an extension header: the others do not grow
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(s in text for s in declared), other
    out = os.popen(f"nm -D --defined-only {os.path.join(ROOT, 'hypergraphdb_amd', 'libhgx.so')}").read()
    L = _lib.lib()
    for s in declared:
        assert re.search(rf"\sT {s}$", out, re.M), s
        assert getattr(L, s).argtypes is not None
    assert hypergraphdb_amd.GpuScanToQuery is hypergraphdb_amd.query.GpuScanToQuery
    # null arguments: a status, never a crash, without touching a device
    assert L.hgx_query_result_scan_stats(None, None, None, None, None, None) == _lib.HGX_E_INVALID
    assert L.hgx_graph_type_links(None, None, 0, None) == _lib.HGX_E_INVALID
    assert L.hgx_pattern_batch_dnf_scan(None, 0, None, *[None] * 15, 0, None) == _lib.HGX_E_INVALID


def test_lowering_of_clauses_without_an_anchor():
    from hypergraphdb_amd import hg, to_dnf
    from hypergraphdb_amd.query import is_anchored, normalize, normalize_clause, split_type_scan
    a = hg.incident(3)
    # and(typePlus{1,2}, not(incident a)): two one-type clauses with the same negation
    norm, negs = normalize_clause(hg.and_(hg.typePlus([1, 2]), hg.not_(a)))
    assert norm["types"] == [1, 2] and not is_anchored(norm) and len(negs) == 1
    got = split_type_scan(norm, negs)
    assert [c["types"] for c, _ in got] == [[1], [2]]
    assert all(ng is negs for _, ng in got)
    assert all({k: v for k, v in c.items() if k != "types"} == {k: v for k, v in norm.items() if k != "types"}
               for c, _ in got)
    # and(type 1, type 2) can match nothing: "empty", dropped from the DNF
    assert normalize(hg.and_(hg.type(1), hg.type(2))) == "empty"
    assert split_type_scan("empty", []) == [("empty", [])]
    assert len(to_dnf(hg.and_(hg.type(1), hg.type(2)))) == 0
    # an anchored clause is untouched, with several types too
    for tree in (hg.and_(hg.typePlus([1, 2]), a, hg.not_(hg.arity(2))), hg.and_(hg.typePlus([1, 2]), hg.orderedLink(-1, 4)),
                 hg.and_(hg.typePlus([1, 2]), hg.incidentAt(5, 0))):
        norm, negs = normalize_clause(tree)
        assert is_anchored(norm) and split_type_scan(norm, negs) == [(norm, negs)]
    # one type: nothing to split; an all-ANY pattern and an arity are no anchors
    norm, negs = normalize_clause(hg.and_(hg.type(2), hg.arity(2), hg.orderedLink(-1, -1)))
    assert not is_anchored(norm) and split_type_scan(norm, negs) == [(norm, negs)]
    # neither type nor anchor: passed through for the engine to refuse
    for tree in (hg.arity(2), hg.not_(a), hg.and_(hg.orderedLink(-1), hg.not_(a))):
        norm, negs = normalize_clause(tree)
        assert norm["types"] == [] and not is_anchored(norm)
        assert split_type_scan(norm, negs) == [(norm, negs)]


def test_the_evaluator_on_hand_written_anchor_free_trees():
    """The hand results of tests/test_gpu_scan.py are the evaluator's (the reference's: a scan of the type's
    atoms filtered by the other conditions, AndToQuery.java:120-294)."""
    from test_gpu_scan import hand_cases
    g = K.queries_graph()
    pg = D.graph_of(g)
    n = g["names"]
    cases = hand_cases(g)
    for tree, exp in cases:
        assert N.evaluate(pg, tree) == exp, tree
    assert cases[0][1] == [n["linkH"], n["linkH1"], n["empty"], n["link5"]]
    assert cases[0][1] == g["link_atom"][g["link_type"] == K.T_TESTLINK].tolist()
    assert S.is_scanned(cases[0][0:1]) and not S.is_scanned([cases[5][0][0]])


def test_random_scan_trees_have_the_properties_the_gpu_test_relies_on():
    from test_gpu_scan import SEED, random_case
    g, pg, trees, exp = random_case(SEED)
    assert len(trees) == 300
    props = np.array([S.properties(pg, t) for t in trees])
    nonempty, split, shared = props.sum(axis=0)
    assert nonempty >= 75 and split >= 38 and shared >= 38, (nonempty, split, shared)
    # every clause has an anchor or a type: the engine refuses anything else
    from hypergraphdb_amd import to_dnf
    for t in trees:
        for cl in to_dnf(t):
            assert not S.is_scanned(cl) or S.clause_types(cl)
    # the statistics the batch must report are not trivial
    clauses, rows, kept = S.scan_counts(pg, S.type_count(g), trees)
    assert clauses > 100 and rows > kept > 0
    # arities beyond the 8 register targets, links as targets, repeated targets
    arity = np.diff(g["tgt_off"])
    is_link = np.zeros(g["num_atoms"], bool)
    is_link[g["link_atom"]] = True
    assert (arity > 8).sum() >= 400 and is_link[g["tgt_idx"]].sum() >= 1000
