"""hg.apply(hg.targetAt) on the GPU pattern path (hgx_pattern_batch_join, include/hgx_join.h): the hits of each
part projected to a target position and the parts of a join query intersected on the device.  Expected results:
tests/join_ref.py (not_ref's brute-force evaluator per part, projected and intersected with Python sets),
compared as exact id lists with offsets."""
import threading

import numpy as np
import pytest

import dnf_ref as D
import join_ref as J
import kat_graphs as K

pytestmark = pytest.mark.gpu

SEED = 2100   # test_gpu_not.py's: the same graph; the properties of the queries are checked in test_join_ref.py
N_RANDOM = 200
SIZES = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025]   # test_gpu_scan.py's segment sizes


def snapshot(g):
    from hypergraphdb_amd import HyperGraphSnapshot
    return HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g.get("link_type"))


def check(r, expected):
    """ids and offsets of a batch against the per-query expected lists"""
    assert len(r) == len(expected)
    assert r.offsets.tolist() == np.concatenate([[0], np.cumsum([len(e) for e in expected])]).tolist()
    assert r.ids.tolist() == [x for e in expected for x in e]


_cases = {}


def random_case(scan):
    """(graph, its pyref form, N_RANDOM join queries, their expected results); ``scan``: parts with clauses
    without an anchor.  Computed once per process and left unchanged."""
    if scan not in _cases:
        rng = np.random.default_rng(SEED)
        g = K.random_graph(rng, 600, 2500, max_arity=12, n_types=3)
        pg = D.graph_of(g)
        qs = J.random_queries(np.random.default_rng(SEED + 1 + int(scan)), g, pg, N_RANDOM, scan=scan)
        _cases[scan] = (g, pg, qs, [J.evaluate(pg, q) for q in qs])
    return _cases[scan]


def pattern_cases(g):
    """(parts, expected) on PatternTests' graph"""
    from hypergraphdb_amd import hg
    n = g["names"]
    a, b = hg.orderedLink(hg.anyHandle(), n["A"]), hg.orderedLink(hg.anyHandle(), n["B"])
    return [
        ([(0, a), (0, b)], [n["C1"], n["C4"]]),                                  # TC/query/PatternTests.java:20-61
        ([(0, b)], [n["C1"], n["C4"], n["C5"]]),                                 # (C5, B) exists twice: C5 once
        ([(1, hg.incident(n["C1"]))], sorted([n["A"], n["B"], n["C2"]])),
        ([(2, hg.incident(n["C1"]))], []),                                       # beyond every arity
        ([(0, a), (0, b), (0, hg.orderedLink(hg.anyHandle(), n["C2"]))], [n["C1"]]),
        ([(0, a), (1, a)], []),                                                  # {C1, C2, C4} and {A}
    ]


def queries_cases(g):
    """(parts, expected, needs type_scan) on the queries graph: arities 0, 2, 3, 5, 10"""
    from hypergraphdb_amd import hg
    n = g["names"]
    inc = [hg.incident(n[f"n{i}"]) for i in range(7)]
    T = hg.type(K.T_TESTLINK)
    return [
        ([(10, inc[2])], [], False),                                             # beyond every arity
        ([(3, inc[2])], sorted([n["n3"], n["n2"]]), False),                      # linkH1 is too short
        ([(4, inc[2])], sorted([n["n4"], n["linkH1"]]), False),
        ([(2, inc[2])], sorted([n["n2"], n["linkH"], n["n6"]]), False),
        ([(None, inc[0]), (2, inc[2])], [n["linkH"]], False),                    # the link atom itself: linkH1 = (.., linkH)
        ([(None, hg.and_(inc[2], T)), (4, inc[4])], [n["linkH1"]], False),       # link5 = (.., linkH1)
        ([(0, hg.and_(inc[2], hg.not_(inc[3])))], [n["n4"]], False),             # a part with a Not
        ([(1, hg.or_(inc[0], inc[4]))], sorted([n["n1"], n["n5"]]), False),      # a part that is an Or
        ([], [], False),                                                         # no parts
        ([(0, T)], sorted([n["n0"], n["n2"], n["n4"]]), True),                   # scanned; the empty link is too short
        ([(0, T), (0, inc[3])], sorted([n["n0"], n["n2"]]), True),               # scanned and anchored parts joined
        ([(None, inc[2])], sorted([n["valuelink"], n["linkH1"], n["link5"]]), False),
    ]


def test_hand_cases_in_one_batch_and_one_by_one():
    from hypergraphdb_amd import HGXUnsupported, pattern_batch_join
    from hypergraphdb_amd.query import _ext_arrays, pattern_batch_join_arrays
    g = K.pattern_graph()
    snap, pg = snapshot(g), D.graph_of(g)
    cases = pattern_cases(g)
    for parts, exp in cases:
        assert J.evaluate(pg, parts) == exp, parts            # the hand results are the reference's
    check(pattern_batch_join(snap, [c[0] for c in cases]), [c[1] for c in cases])
    for parts, exp in cases:
        check(pattern_batch_join(snap, [parts]), [exp])
    snap.close()
    g = K.queries_graph()
    snap, pg = snapshot(g), D.graph_of(g)
    cases = queries_cases(g)
    for parts, exp, _ in cases:
        assert J.evaluate(pg, parts) == exp, parts
    check(pattern_batch_join(snap, [c[0] for c in cases], type_scan=True), [c[1] for c in cases])
    plain = [c for c in cases if not c[2]]
    check(pattern_batch_join(snap, [c[0] for c in plain]), [c[1] for c in plain])
    for parts, exp, scan in cases:
        check(pattern_batch_join(snap, [parts], type_scan=scan), [exp])
        if scan:                                                # the opt-in rule of hgx_scan.h carries over
            with pytest.raises(HGXUnsupported):
                pattern_batch_join(snap, [parts])
    # a batch of 0 queries, and the raw arrays entry without any part
    r = pattern_batch_join(snap, [])
    assert len(r) == 0 and r.offsets.tolist() == [0]
    r = pattern_batch_join_arrays(snap, [0, 0, 0], [], [0], *_ext_arrays([]))
    assert r.offsets.tolist() == [0, 0, 0] and len(r.ids) == 0 and r.join["parts"] == 0
    snap.close()


def test_find_all_goes_through_the_device_entry(monkeypatch):
    import hypergraphdb_amd.query as Q
    from hypergraphdb_amd import HGQueryConfiguration, MapCondition, find_all, hg
    g = K.pattern_graph()
    snap, n = snapshot(g), g["names"]
    calls = []
    real = Q.pattern_batch_join

    def spy(*a, **k):
        calls.append(a)
        return real(*a, **k)

    monkeypatch.setattr(Q, "pattern_batch_join", spy)
    t0 = hg.targetAt(snap, 0)
    a, b = hg.orderedLink(hg.anyHandle(), n["A"]), hg.orderedLink(hg.anyHandle(), n["B"])
    kat = hg.and_(hg.apply(t0, a), hg.apply(t0, b))
    assert find_all(snap, kat) == [n["C1"], n["C4"]] and len(calls) == 1
    assert find_all(snap, hg.apply(t0, b)) == [n["C1"], n["C4"], n["C5"]] and len(calls) == 2
    cfg = HGQueryConfiguration()
    cfg.addCompiler(MapCondition, Q.GpuMapToQuery())
    assert find_all(snap, hg.apply(hg.targetAt(snap, 1), hg.incident(n["C1"])), cfg) == sorted([n["A"], n["B"], n["C2"]])
    assert len(calls) == 3
    md = Q.GpuMapToQuery().getMetaData(snap, hg.apply(t0, b))
    assert md.ordered and md.randomAccess
    # a mapping that is a lambda, alone and next to a projection: the host path, the same results
    lam = hg.apply(lambda link: int(snap.targets(link)[0]), b)
    assert find_all(snap, lam) == [n["C1"], n["C4"], n["C5"]] and len(calls) == 3
    assert find_all(snap, hg.and_(hg.apply(t0, a), lam)) == [n["C1"], n["C4"]]
    # a plain sub-condition next to projections: the link atoms themselves -- no link of this graph is a target
    assert find_all(snap, hg.and_(hg.apply(t0, a), hg.incident(n["C1"]))) == []
    snap.close()


def boundary_graph():
    """An anchor atom per size in SIZES with that many incident links of arity 2 and 3 over a pool of 7 second
    targets (anchor k uses 1 + k % 7 of them: heavy duplicates, value sets that differ), the pool's first member
    being the graph's highest atom id."""
    b = K.Builder()
    anchors = [b.node(f"a{n}") for n in SIZES]
    pool = [b.node(f"s{i}") for i in range(6)]
    for k, n in enumerate(SIZES):
        m = 1 + k % 7
        for i in range(n):
            tg = [anchors[k], (i % m)]                    # (an index into the pool, resolved below)
            if i % 3 == 0:
                tg.append((3 * i + k) % 7)
            b.link(None, i % 3, *tg)
    pool.insert(0, b.node("top"))                        # pool[0]: every anchor with a link projects to it
    for _, _, tg in b.links:
        tg[1:] = [pool[x] for x in tg[1:]]
    g = b.arrays()
    assert g["names"]["top"] == g["num_atoms"] - 1
    return g, anchors


def test_boundary_sizes_single_parts_pairs_and_eight_parts():
    from hypergraphdb_amd import hg, pattern_batch_join
    g, anchors = boundary_graph()
    deg = np.bincount(g["tgt_idx"], minlength=g["num_atoms"])
    assert [int(deg[a]) for a in anchors] == SIZES
    snap, pg = snapshot(g), D.graph_of(g)
    inc = [hg.incident(a) for a in anchors]               # one object per anchor: join_ref evaluates each once
    K_ = len(SIZES)
    qs = [[(1, inc[i])] for i in range(K_)] + [[(2, inc[i])] for i in range(K_)]
    qs += [[(1, inc[i]), (2 if (i + j) % 3 == 0 else 1, inc[j])] for i in range(K_) for j in range(K_)]
    qs.append([(1 + k % 2, inc[4 + k]) for k in range(8)])
    exp = [J.evaluate(pg, q) for q in qs]
    top = g["names"]["top"]
    assert sum(top in e for e in exp) >= 20 and sum(not e for e in exp) >= 20 and exp[-1]
    # every ordered pair: the driver (the part with the fewest hits) is the first part in some, the second in others
    r = pattern_batch_join(snap, qs)
    check(r, exp)
    assert r.join == dict(r.join, **J.stats(pg, qs))
    for q, e in list(zip(qs, exp))[::17]:
        check(pattern_batch_join(snap, [q]), [e])
    snap.close()


def test_hub_graph_projections():
    from hypergraphdb_amd import hg, pattern_batch_join
    from test_gpu_not import hub_graph
    g = hub_graph(1500)
    snap, pg, n = snapshot(g), D.graph_of(g), g["names"]
    h = hg.incident(n["h"])
    xs = [n[f"x{i}"] for i in range(7)]
    by_type = [(1, hg.and_(h, hg.type(t))) for t in range(3)]
    qs = [[(1, h)], [(0, h)], [(2, h)], by_type]
    r = pattern_batch_join(snap, qs)
    check(r, [xs, [n["h"]], [], J.evaluate(pg, by_type)])
    assert r[3].tolist() == xs                              # every x is reached through every type
    assert r.join["hits_projected"] == 3 * 1500 + 1500 and r.join["values_distinct"] == 7 + 1 + 0 + 21
    snap.close()


def test_workspace_overflow_rerun():
    """A fresh snapshot starts with room for 16 n + 4096 candidates, which two parts over a 6,000-link hub
    outgrow: every stage does nothing after the overflow, the host grows the workspace and runs them again."""
    from hypergraphdb_amd import hg, pattern_batch_join
    from test_gpu_not import hub_graph
    g = hub_graph(6000)
    snap, pg, n = snapshot(g), D.graph_of(g), g["names"]
    h = hg.incident(n["h"])
    q = [(1, h), (1, hg.and_(h, hg.type(2), hg.not_(hg.incident(n["x3"]))))]
    assert 2 * 6000 > 16 * 2 + 4096
    exp = J.evaluate(pg, q)
    assert exp == [n[f"x{i}"] for i in range(7) if i != 3]
    for rep in range(2):
        r = pattern_batch_join(snap, [q])
        check(r, [exp])
        assert r.join["hits_projected"] == 6000 + 2000 - len(range(17, 6000, 21)) and r.join["kept"] == 6
    snap.close()


@pytest.mark.parametrize("scan", [False, True])
def test_random_join_queries_vs_brute_force(scan):
    from hypergraphdb_amd import pattern_batch_join
    g, pg, qs, exp = random_case(scan)
    snap = snapshot(g)
    r = pattern_batch_join(snap, qs, type_scan=scan)
    check(r, exp)
    if not scan:                                            # anchored parts: the flag changes nothing
        check(pattern_batch_join(snap, qs, type_scan=True), exp)
    assert r.join["kept"] == len(r.ids) and r.join["bytes_join"] > 0
    snap.close()


def test_statistics_equal_the_reference_counts():
    from hypergraphdb_amd import pattern_batch_dnf, pattern_batch_join
    g, pg, qs, exp = random_case(False)
    qs, exp = qs[:60], exp[:60]
    want = J.stats(pg, qs)
    assert want["parts"] > 60 and want["hits_projected"] > want["values_distinct"] > want["kept"] > 0
    snap = snapshot(g)
    snap.set_timing(True)
    r = pattern_batch_join(snap, qs)
    check(r, exp)
    assert {k: r.join[k] for k in want} == want and r.join["kept"] == len(r.ids)
    assert 0 < r.join["ms_join"] <= r.ms["ms_total"] and r.join["bytes_join"] > 0 and r.union["ms_union"] > 0
    # the union statistics still describe the parts: the clause hits, and the link atoms the parts kept
    assert r.union["clause_hits"] >= r.union["kept"] == want["hits_projected"]
    # a DNF batch carries no join statistics
    d = pattern_batch_dnf(snap, [c for q in qs for _, c in q])
    assert d.join == {"parts": 0, "hits_projected": 0, "values_distinct": 0, "kept": 0, "ms_join": 0.0, "bytes_join": 0.0}
    assert d.union["kept"] == want["hits_projected"] == len(d.ids)
    snap.close()


def test_errors_leave_the_graph_usable():
    from hypergraphdb_amd import HGXError, HGXUnsupported, _lib, hg, pattern_batch_join
    from hypergraphdb_amd.query import _ext_arrays, pattern_batch_join_arrays
    g = K.queries_graph()
    snap, n = snapshot(g), g["names"]
    inc2 = hg.incident(n["n2"])
    good = [(3, inc2)]

    def still_good():
        assert pattern_batch_join(snap, [good])[0].tolist() == sorted([n["n2"], n["n3"]])

    still_good()
    ok = {"types": [], "inc": [n["n2"]], "pos": [], "patterns": [], "arity": -1}
    with pytest.raises(HGXError) as e:                # part_off decreasing
        pattern_batch_join_arrays(snap, [0, 2, 1], [0, 0], [0, 1, 2], *_ext_arrays([ok, ok]))
    assert e.value.code == _lib.HGX_E_INVALID and "part_off" in str(e.value)
    still_good()
    with pytest.raises(HGXError) as e:                # part_off not starting at 0
        pattern_batch_join_arrays(snap, [1, 2], [0, 0], [0, 1, 2], *_ext_arrays([ok, ok]))
    assert e.value.code == _lib.HGX_E_INVALID
    with pytest.raises(HGXError) as e:                # a position below HGX_JOIN_SELF
        pattern_batch_join_arrays(snap, [0, 1, 2], [0, -2], [0, 1, 2], *_ext_arrays([ok, ok]))
    assert e.value.code == _lib.HGX_E_INVALID and "join query 1 part 0" in str(e.value)
    still_good()
    with pytest.raises(HGXError) as e:                # an atom id out of range inside a part
        pattern_batch_join(snap, [good, [(0, inc2), (1, hg.incident(g["num_atoms"] + 3))]])
    assert e.value.code == _lib.HGX_E_INVALID and "join query 1 part 1" in str(e.value)
    still_good()
    with pytest.raises(HGXUnsupported) as e:          # an anchor-free clause without the flag
        pattern_batch_join(snap, [good, [(0, hg.type(K.T_TESTLINK))]])
    assert "join query 1 part 0" in str(e.value)
    still_good()
    snap.close()
    from test_gpu_partition import parts
    sh = parts(g, 2)
    with pytest.raises(HGXUnsupported):               # a shard is not a whole snapshot
        pattern_batch_join(sh[0], [[(0, [{"types": [], "inc": [0], "pos": [], "patterns": [], "arity": -1}])]])
    for s in sh:
        s.close()


def test_two_threads_on_two_contexts():
    from hypergraphdb_amd import pattern_batch_join
    g, pg, qs, exp = random_case(False)
    snap = snapshot(g)
    ctxs = [snap.context() for _ in range(2)]
    out, errs = [None] * 2, []

    def work(i):
        try:
            for _ in range(3):
                out[i] = pattern_batch_join(ctxs[i], qs[:120] if i == 0 else qs[::-1][:150])
        except Exception as ex:   # noqa: BLE001
            errs.append(ex)

    ths = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs
    check(out[0], exp[:120])
    check(out[1], exp[::-1][:150])
    for c in ctxs:
        c.close()
    snap.close()
