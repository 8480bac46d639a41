"""CPU tests of the join layer (include/hgx_join.h): libhgx.so exports the header's boundary, the evaluator of
tests/join_ref.py on the reference's pattern test, the lowering of conditions to parts (join_parts), and the
properties of the random join queries the GPU test relies on.  No GPU compute."""
import os
import re

import numpy as np
import pytest

import dnf_ref as D
import join_ref as J
import kat_graphs as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_join_abi_exported_and_bound():
    import hypergraphdb_amd
    from hypergraphdb_amd import _lib
    src = open(os.path.join(ROOT, "include", "hgx_join.h")).read()
    # the header's comments may name entries of the headers it extends
    declared = sorted(set(re.findall(r"\b(hgx_[a-z_]+)\s*\(", src)) - set(_lib.EXPORTED) - set(_lib.EXPORTED_DNF) -
                      set(_lib.EXPORTED_NOT) - set(_lib.EXPORTED_SCAN))
    assert declared == sorted(_lib.EXPORTED_JOIN) and len(declared) == 2
    for other in ("hgx.h", "hgx_dnf.h", "hgx_not.h", "hgx_scan.h"):    # an extension header: the others do not grow
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(s in text for s in declared), other
    assert re.search(r"#define HGX_JOIN_SELF \(-1\)", src) and _lib.HGX_JOIN_SELF == -1
    assert re.search(r"#define HGX_JOIN_TYPE_SCAN 1\b", src) and _lib.HGX_JOIN_TYPE_SCAN == 1
    out = os.popen(f"nm -D --defined-only {os.path.join(ROOT, 'hypergraphdb_amd', 'libhgx.so')}").read()
    L = _lib.lib()
    for s in declared:
        assert re.search(rf"\sT {s}$", out, re.M), s
        assert getattr(L, s).argtypes is not None
    assert hypergraphdb_amd.GpuMapToQuery is hypergraphdb_amd.query.GpuMapToQuery
    assert hypergraphdb_amd.pattern_batch_join is hypergraphdb_amd.query.pattern_batch_join
    assert hypergraphdb_amd.join_parts is hypergraphdb_amd.query.join_parts
    # null arguments: a status, never a crash, without touching a device
    assert L.hgx_query_result_join_stats(None, None, None, None, None, None, None) == _lib.HGX_E_INVALID
    assert L.hgx_pattern_batch_join(None, 0, None, None, None, *[None] * 15, 0, 0, None) == _lib.HGX_E_INVALID


def test_the_evaluator_on_the_reference_pattern_test():
    """TC/query/PatternTests.java:20-61: and(apply(targetAt(0), orderedLink(ANY, A)),
    apply(targetAt(0), orderedLink(ANY, B))) == {C1, C4}."""
    from hypergraphdb_amd import hg
    g = K.pattern_graph()
    pg, n = D.graph_of(g), g["names"]
    a, b = hg.orderedLink(hg.anyHandle(), n["A"]), hg.orderedLink(hg.anyHandle(), n["B"])
    assert J.evaluate(pg, [(0, a), (0, b)]) == [n["C1"], n["C4"]]
    assert len(J.part_links(pg, b)) == 4                    # (C5, B) exists twice ...
    assert J.evaluate(pg, [(0, b)]) == [n["C1"], n["C4"], n["C5"]]   # ... and C5 is delivered once
    assert J.evaluate(pg, [(1, hg.incident(n["C1"]))]) == sorted([n["A"], n["B"], n["C2"]])
    assert J.evaluate(pg, [(2, hg.incident(n["C1"]))]) == [] and J.evaluate(pg, []) == []
    assert J.stats(pg, [[(0, a), (0, b)], [(2, b)]]) == {"parts": 3, "hits_projected": 3 + 4 + 4, "values_distinct": 3 + 3,
                                                         "kept": 2}
    # the hand results of the GPU test are the evaluator's
    from test_gpu_join import pattern_cases, queries_cases
    for parts, exp in pattern_cases(g):
        assert J.evaluate(pg, parts) == exp, parts
    g = K.queries_graph()
    pg = D.graph_of(g)
    assert sorted(len(tg) for _, tg in pg.links.values()) == [0, 2, 3, 5, 10]
    for parts, exp, _ in queries_cases(g):
        assert J.evaluate(pg, parts) == exp, parts


def test_join_parts_lowering():
    from hypergraphdb_amd import HGXUnsupported, hg, join_parts

    class Snap:   # join_parts only compares snapshots
        tgt_off = None

    s1, s2 = Snap(), Snap()
    a, b, c = hg.incident(1), hg.orderedLink(-1, 2), hg.type(3)
    t0, t1 = hg.targetAt(s1, 0), hg.targetAt(s1, 1)
    assert join_parts(hg.apply(t0, a)) == [(0, a)]
    assert join_parts(hg.apply(t1, hg.or_(a, b)), s1) == [(1, hg.or_(a, b))]
    assert join_parts(hg.and_(hg.apply(t0, a), hg.apply(t1, b))) == [(0, a), (1, b)]
    # nested Ands flatten; the plain sub-conditions together form one part without a projection, after the others
    got = join_parts(hg.and_(a, hg.and_(hg.apply(t0, b), c), hg.apply(t0, hg.and_(a, hg.not_(c)))))
    assert got == [(0, b), (0, hg.and_(a, hg.not_(c))), (None, hg.and_(a, c))]
    assert join_parts(hg.and_(hg.apply(t0, a), b)) == [(0, a), (None, b)]
    assert join_parts(hg.and_(hg.apply(t0, a), hg.or_(a, b))) == [(0, a), (None, hg.or_(a, b))]
    for bad in (hg.apply(lambda x: x, a),                                   # a mapping that is no TargetAt
                hg.apply(hg.targetAt(s1, -1), a),
                hg.and_(hg.apply(t0, a), hg.apply(hg.targetAt(s2, 0), b)),  # a TargetAt of another snapshot
                hg.apply(t0, hg.apply(t1, a)),                              # a nested MapCondition
                hg.apply(t0, hg.and_(a, hg.apply(t1, b))),
                hg.and_(hg.apply(t0, a), hg.bfs(1)),                        # a BFSCondition
                hg.apply(t0, hg.bfs(1)),
                hg.or_(hg.apply(t0, a), hg.apply(t0, b)),                   # an Or of maps
                hg.and_(hg.apply(t0, a), hg.or_(b, hg.apply(t0, b))),
                hg.and_(hg.apply(t0, a), hg.not_(hg.apply(t0, b))),
                hg.and_(a, b), a):                                          # no projection at all
        with pytest.raises(HGXUnsupported):
            join_parts(bad)
    with pytest.raises(HGXUnsupported):
        join_parts(hg.apply(t0, a), s2)


def test_random_join_queries_have_the_properties_the_gpu_test_relies_on():
    from test_gpu_join import N_RANDOM, random_case
    for scan in (False, True):
        g, pg, qs, exp = random_case(scan)
        assert len(qs) == N_RANDOM and all(1 <= len(q) <= 4 or len(q) == 8 for q in qs)
        nonempty, smaller = J.properties(pg, qs)
        assert nonempty >= N_RANDOM // 3 + 1 and smaller >= N_RANDOM // 10, (scan, nonempty, smaller)
        assert nonempty == sum(bool(e) for e in exp)
        sizes = {len(q) for q in qs}
        assert sizes >= {1, 2, 3, 4, 8}
        poss = {p for q in qs for p, _ in q}
        assert poss == {None, 0, 1, 2, 3}
        # links too short for their position, and duplicates the projection folds
        st = J.stats(pg, qs)
        assert st["hits_projected"] > st["values_distinct"] > st["kept"] > 0
        assert any(p is not None and any(len(pg.links[l][1]) <= p for l in J.part_links(pg, c)) for q in qs for p, c in q)
        if scan:                                            # some part has a clause without an anchor
            import scan_ref as S
            from hypergraphdb_amd import to_dnf
            assert sum(any(S.is_scanned(cl) for cl in to_dnf(c)) for q in qs for _, c in q) >= 50
