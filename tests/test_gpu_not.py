"""hg.not on the GPU pattern path (hgx_pattern_batch_dnf_not, include/hgx_not.h): the Nots of a clause filter
its hits on the device between the clause stage and the union.  Expected results: the brute-force evaluator of
tests/not_ref.py (a Not negates the raw satisfies of its tree, Not.java:33-36), compared as exact lists."""
import threading

import numpy as np
import pytest

import dnf_ref as D
import kat_graphs as K
import not_ref as N

pytestmark = pytest.mark.gpu


def snapshot(g):
    from hypergraphdb_amd import HyperGraphSnapshot
    return HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g.get("link_type"))


def check(r, expected):
    """ids and offsets of a batch against the per-query expected lists"""
    assert len(r) == len(expected)
    assert r.offsets.tolist() == np.concatenate([[0], np.cumsum([len(e) for e in expected])]).tolist()
    assert r.ids.tolist() == [x for e in expected for x in e]


def hand_cases(g):
    """(tree, expected result) on the queries graph"""
    from hypergraphdb_amd import hg
    n = g["names"]
    inc = [hg.incident(n[f"n{i}"]) for i in range(7)]
    T, V = hg.type(K.T_TESTLINK), hg.type(K.T_VALUELINK)
    value, linkH, linkH1, link5 = n["valuelink"], n["linkH"], n["linkH1"], n["link5"]
    return [
        (hg.and_(inc[2], hg.not_(inc[3])), [link5]),                                   # one negation
        (hg.and_(inc[2], hg.not_(inc[4]), hg.not_(V)), [linkH1]),                      # two in one clause
        (hg.and_(inc[2], hg.not_(hg.or_(inc[3], inc[4]))), []),                        # Not(Or): every hit rejected
        (hg.and_(inc[2], hg.not_(hg.and_(inc[3], T))), sorted([value, link5])),        # Not(And)
        (hg.and_(inc[2], hg.not_(hg.not_(inc[3]))), sorted([value, linkH1])),          # Not(Not(incident))
        (hg.and_(inc[2], hg.not_(inc[2])), []),                                        # every hit rejected
        (hg.and_(hg.incident(n["n10"]), hg.not_(inc[0])), []),                         # no hit at all
        # the first clause contains valuelink and rejects it, the second accepts it
        (hg.or_(hg.and_(inc[2], hg.not_(inc[0])), hg.and_(inc[0], hg.not_(T))), sorted([value, linkH1, link5])),
        # both clauses accept linkH1: delivered once
        (hg.or_(hg.and_(inc[2], hg.not_(V)), hg.and_(inc[3], hg.not_(V))), sorted([linkH1, link5])),
        (hg.and_(inc[0], hg.not_(hg.orderedLink())), []),                              # [] satisfies every link
        (hg.and_(inc[0], hg.not_(hg.orderedLink(n["n1"], n["n0"]))), sorted([value, linkH])),
        (hg.and_(inc[0], hg.not_(hg.orderedLink(n["n0"], n["n1"]))), []),
        (hg.and_(inc[0], hg.not_(hg.arity(0))), sorted([value, linkH])),
        (hg.and_(inc[0], hg.not_(hg.arity(2))), [value]),
        (hg.and_(inc[2], hg.not_(hg.link(n["n2"], n["n3"]))), [link5]),
        (hg.and_(inc[2], hg.not_(hg.incidentAt(n["n2"], 0))), sorted([value, link5])),
        (hg.and_(inc[2], hg.not_(hg.typePlus([K.T_VALUELINK, 77]))), sorted([linkH1, link5])),
        (hg.and_(inc[2], hg.not_(hg.incident(linkH))), sorted([value, link5])),        # a link as a target
        (hg.and_(inc[2], T), sorted([linkH1, link5])),                                 # no Not next to Nots
    ]


def test_hand_cases_on_the_queries_graph():
    from hypergraphdb_amd import find_all, hg, pattern_batch_dnf
    g = K.queries_graph()
    snap, pg = snapshot(g), D.graph_of(g)
    cases = hand_cases(g)
    for tree, exp in cases:
        assert N.evaluate(pg, tree) == exp, tree            # the hand results are the reference's
    trees = [c[0] for c in cases]
    r = pattern_batch_dnf(snap, trees)
    check(r, [c[1] for c in cases])
    assert r.negation["hits_tested"] > r.negation["hits_rejected"] > 0
    for tree, exp in cases[:9]:
        assert find_all(snap, tree) == exp, tree
        assert pattern_batch_dnf(snap, [tree])[0].tolist() == exp
    # a query with 0 clauses between queries with Nots, and a batch of 0 queries
    r = pattern_batch_dnf(snap, [trees[0], [], trees[2], hg.or_(), trees[7]])
    check(r, [cases[0][1], [], cases[2][1], [], cases[7][1]])
    assert len(pattern_batch_dnf(snap, [])) == 0
    from hypergraphdb_amd.query import _ext_arrays, encode_negations, pattern_batch_dnf_not_arrays
    r = pattern_batch_dnf_not_arrays(snap, [0], *_ext_arrays([]), *encode_negations([]))
    assert len(r) == 0 and r.offsets.tolist() == [0]
    r = pattern_batch_dnf_not_arrays(snap, [0, 0, 0], *_ext_arrays([]), *encode_negations([]))
    assert r.offsets.tolist() == [0, 0, 0]
    snap.close()


SEED = 2100   # picked on the CPU: 94 of its 300 trees have a rejected and a kept hit (75 are asked for)


@pytest.fixture(scope="module")
def rand():
    rng = np.random.default_rng(SEED)
    g = K.random_graph(rng, 600, 2500, max_arity=12, n_types=3)
    pg = D.graph_of(g)
    trees = [N.random_tree(rng, g, pg=pg) for _ in range(300)]
    return g, pg, trees, [N.evaluate(pg, t) for t in trees]


def test_random_trees_vs_brute_force(rand):
    from hypergraphdb_amd import pattern_batch_dnf
    g, pg, trees, exp = rand
    # the input exercises what it should, from the graph and the reference alone
    arity = np.diff(g["tgt_off"])
    is_link = np.zeros(g["num_atoms"], bool)
    is_link[g["link_atom"]] = True
    assert (arity > 8).sum() >= 400 and is_link[g["tgt_idx"]].sum() >= 1000
    assert sum(len(set(tg)) < len(tg) for _, tg in pg.links.values()) >= 300
    both = sum(bool(e) and bool(set(N.evaluate(pg, N.strip_nots(t))) - set(e)) for t, e in zip(trees, exp))
    assert both >= len(trees) // 4, both
    snap = snapshot(g)
    r = pattern_batch_dnf(snap, trees)
    check(r, exp)
    assert r.union["kept"] == len(r.ids) and r.negation["bytes_not"] > 0
    snap.close()


def test_stats_equal_the_reference_counts(rand):
    from hypergraphdb_amd import pattern_batch_dnf, to_dnf
    g, pg, trees, exp = rand
    trees, exp = trees[:60], exp[:60]
    tested, rejected = map(sum, zip(*(N.filter_counts(pg, to_dnf(t)) for t in trees)))
    assert tested > rejected > 0
    snap = snapshot(g)
    snap.set_timing(True)
    r = pattern_batch_dnf(snap, trees)
    check(r, exp)
    assert (r.negation["hits_tested"], r.negation["hits_rejected"]) == (tested, rejected)
    assert 0 < r.negation["ms_not"] <= r.ms["ms_total"] and r.union["ms_union"] > 0
    # a batch without a Not: hgx_pattern_batch_dnf, whose results carry no filter statistics
    plain = [N.strip_nots(t) for t in trees]
    r = pattern_batch_dnf(snap, plain)
    assert r.negation == {"hits_tested": 0, "hits_rejected": 0, "ms_not": 0.0, "bytes_not": 0.0}
    assert [r[q].tolist() for q in range(len(plain))] == [N.evaluate(pg, t) for t in plain]
    snap.close()


def test_power_law_hub_long_runs():
    """1024 queries anchored on the hub of a power-law graph: runs of thousands of hits, many lanes share a
    clause.  On the fresh snapshot the first batch outgrows the initial workspace (16 n + 4096 candidates), so
    the clause stage, the filter and the union run twice."""
    from hypergraphdb_amd import hg, pattern_batch_dnf, synth
    g = synth.hypergraph(3000, 20000, 2, 8, 2.1, 3, seed=5)
    pg = D.graph_of(g)
    deg = np.bincount(g["tgt_idx"], minlength=g["num_atoms"])
    assert deg.argmax() == 0 and deg[0] > 5000
    hub, a, b, c = hg.incident(0), hg.incident(1), hg.incident(2), hg.incident(3)
    shapes = [hg.and_(hub, hg.not_(a)), hg.and_(hub, hg.not_(hg.or_(a, b))), hg.and_(hub, hg.type(1), hg.not_(hg.type(1))),
              hg.and_(hub, hg.not_(hg.not_(a))), hg.and_(hub, hg.not_(hg.arity(3)), hg.not_(hg.type(0))),
              hg.or_(hg.and_(hub, hg.not_(a)), hg.and_(a, hg.not_(b))), hg.and_(hub, hg.not_(hg.orderedLink(0, 1))),
              hg.and_(hub, hg.not_(hg.and_(hg.incidentAt(0, 0), hg.typePlus([0, 2])))),
              hg.or_(hg.and_(hub, hg.not_(hg.link(0, 1))), hg.and_(hub, hg.type(2), hg.not_(c)))]
    exp = [N.evaluate(pg, t) for t in shapes]
    assert all(len(e) > 0 for e in exp[:2] + exp[3:]) and exp[2] == [] and len(exp[1]) < len(exp[0]) < deg[0]
    idx = np.random.default_rng(4).integers(0, len(shapes), 1024)
    assert 1024 * deg[0] > 16 * 1024 + 4096
    snap = snapshot(g)
    for rep in range(2):
        r = pattern_batch_dnf(snap, [shapes[i] for i in idx])
        check(r, [exp[i] for i in idx])
    snap.close()


def hub_graph(n_links, n_types=3):
    b = K.Builder()
    h = b.node("h")
    xs = [b.node(f"x{i}") for i in range(7)]
    for i in range(n_links):
        b.link(None, i % n_types, h, xs[i % 7])
    return b.arrays()


def test_workspace_overflow_rerun_with_nots():
    """The engine has no option that shrinks the clause workspace; a fresh snapshot starts with room for
    16 n + 4096 candidates, which two clauses over a 6,000-link hub outgrow: the filter and the union do
    nothing after the overflow, the host grows the workspace and runs all three stages again."""
    from hypergraphdb_amd import hg, pattern_batch_dnf
    g = hub_graph(6000)
    snap, pg = snapshot(g), D.graph_of(g)
    h, x = g["names"]["h"], g["names"]["x3"]
    tree = hg.or_(hg.and_(hg.incident(h), hg.not_(hg.incident(x))), hg.and_(hg.incident(h), hg.type(2), hg.not_(hg.type(2))))
    assert 2 * 6000 > 16 * 2 + 4096
    exp = N.evaluate(pg, tree)
    assert len(exp) == 6000 - len(range(3, 6000, 7))
    for rep in range(2):
        r = pattern_batch_dnf(snap, [tree])
        check(r, [exp])
        assert r.negation["hits_tested"] == 8000 and r.negation["hits_rejected"] == 2000 + len(range(3, 6000, 7))
    snap.close()


def test_not_free_batch_contexts_and_threads(rand):
    from hypergraphdb_amd import pattern_batch_dnf, to_dnf
    from hypergraphdb_amd.query import (_ext_arrays, encode_negations, normalize, pattern_batch_dnf_arrays,
                                        pattern_batch_dnf_not_arrays)
    g, pg, trees, exp = rand
    snap = snapshot(g)
    # a Not-free batch through the new entry: hgx_pattern_batch_dnf's result, byte for byte
    clause_off, norm = [0], []
    for t in trees:
        norm += [normalize(c) for c in to_dnf(N.strip_nots(t))]
        clause_off.append(len(norm))
    ref = pattern_batch_dnf_arrays(snap, clause_off, *_ext_arrays(norm))
    assert len(ref.ids) > 1000
    no_negs = encode_negations([[] for _ in norm])
    for who in (snap, snap.context()):
        r = pattern_batch_dnf_not_arrays(who, clause_off, *_ext_arrays(norm), *no_negs)
        assert r.offsets.tobytes() == ref.offsets.tobytes() and r.ids.tobytes() == ref.ids.tobytes()
        assert r.union["clause_hits"] == ref.union["clause_hits"] and r.negation["hits_tested"] == 0
        r = pattern_batch_dnf_not_arrays(who, clause_off, *_ext_arrays(norm), None, None, None, None, None)   # no program
        assert r.offsets.tobytes() == ref.offsets.tobytes() and r.ids.tobytes() == ref.ids.tobytes()
        check(pattern_batch_dnf(who, trees), exp)       # with the Nots, through an execution context too
        if who is not snap:
            who.close()
    # from two threads on two contexts
    ctxs = [snap.context() for _ in range(2)]
    out, errs = [None] * 2, []

    def work(i):
        try:
            for _ in range(3):
                out[i] = pattern_batch_dnf(ctxs[i], trees if i == 0 else trees[::-1])
        except Exception as ex:   # noqa: BLE001
            errs.append(ex)

    ths = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs
    check(out[0], exp)
    check(out[1], exp[::-1])
    for c in ctxs:
        c.close()
    snap.close()


def test_errors_leave_the_graph_usable():
    import ctypes as C
    from hypergraphdb_amd import HGXError, HGXUnsupported, _lib, find_all, hg, pattern_batch_dnf
    from hypergraphdb_amd.query import _ext_arrays, encode_negations, lower_not, pattern_batch_dnf_not_arrays
    g = K.queries_graph()
    snap, n = snapshot(g), g["names"]
    inc0, inc2 = hg.incident(n["n0"]), hg.incident(n["n2"])
    good = hg.and_(inc2, hg.not_(hg.incident(n["n3"])))

    def still_good():
        assert pattern_batch_dnf(snap, [good])[0].tolist() == [n["link5"]]

    still_good()
    with pytest.raises(HGXError) as e:                # an atom id out of range inside a Not
        pattern_batch_dnf(snap, [good, hg.or_(inc0, hg.and_(inc2, hg.not_(inc0), hg.not_(hg.incident(g["num_atoms"] + 3))))])
    assert e.value.code == _lib.HGX_E_INVALID and "query 1 clause 1 negation 1" in str(e.value)
    still_good()
    ok = {"types": [], "inc": [n["n2"]], "pos": [], "patterns": [], "arity": -1}
    prog = encode_negations([[lower_not(hg.not_(inc0))], [lower_not(hg.not_(hg.or_(inc0, inc2)))]])
    for k, name in ((0, "neg_off"), (1, "term_off"), (2, "lit_off")):   # program offsets not monotone
        bad = [p.copy() for p in prog]
        bad[k][1] = bad[k][2] + 1
        with pytest.raises(HGXError) as e:
            pattern_batch_dnf_not_arrays(snap, [0, 1, 2], *_ext_arrays([ok, ok]), *bad)
        assert e.value.code == _lib.HGX_E_INVALID and name in str(e.value)
        assert "query 1 clause 0" in str(e.value)
        still_good()
    bad = [p.copy() for p in prog]
    bad[0][0] = 1                                     # not starting at 0
    with pytest.raises(HGXError) as e:
        pattern_batch_dnf_not_arrays(snap, [0, 1, 2], *_ext_arrays([ok, ok]), *bad)
    assert e.value.code == _lib.HGX_E_INVALID
    bad = [p.copy() for p in prog]
    bad[3][4] = 99                                    # an unknown kind in the second literal
    with pytest.raises(HGXError) as e:
        pattern_batch_dnf_not_arrays(snap, [0, 1, 2], *_ext_arrays([ok, ok]), *bad)
    assert e.value.code == _lib.HGX_E_INVALID and "query 1 clause 0 negation 0" in str(e.value)
    bad = [p.copy() for p in prog]
    bad[3][3] = len(prog[4]) + 1                      # an operand range outside ops
    with pytest.raises(HGXError) as e:
        pattern_batch_dnf_not_arrays(snap, [0, 1, 2], *_ext_arrays([ok, ok]), *bad)
    assert e.value.code == _lib.HGX_E_INVALID
    still_good()
    # a clause without an incidence anchor: a Not is none
    for tree in (hg.and_(hg.type(K.T_TESTLINK), hg.not_(inc0)), hg.not_(inc0),
                 hg.or_(good, hg.and_(hg.arity(2), hg.not_(inc0)))):
        with pytest.raises(HGXUnsupported):
            pattern_batch_dnf(snap, [tree])
        with pytest.raises(HGXUnsupported):
            find_all(snap, tree)
        still_good()
    with pytest.raises(HGXUnsupported):               # what the pattern engine does not negate
        find_all(snap, hg.and_(inc2, hg.not_(hg.bfs(n["n0"]))))
    with pytest.raises(HGXUnsupported):               # an ordered pattern beyond the condition limits
        pattern_batch_dnf(snap, [hg.and_(inc2, hg.not_(hg.orderedLink(*[n["n0"]] * 65)))])
    still_good()
    # null arguments: a status, never a crash
    L = _lib.lib()
    h = C.c_void_p()
    arrs = [a.ctypes.data for a in _ext_arrays([ok, ok])]
    off = np.array([0, 1, 2], np.int64)
    pr = [p.ctypes.data for p in prog]
    assert L.hgx_pattern_batch_dnf_not(snap.handle, 2, off.ctypes.data, *arrs, *pr, len(prog[4]), None) == _lib.HGX_E_INVALID
    assert L.hgx_pattern_batch_dnf_not(snap.handle, 2, None, *arrs, *pr, len(prog[4]), C.byref(h)) == _lib.HGX_E_INVALID
    assert L.hgx_pattern_batch_dnf_not(None, 2, off.ctypes.data, *arrs, *pr, len(prog[4]), C.byref(h)) == _lib.HGX_E_INVALID
    for k in range(1, 5):                             # a missing array of the program
        miss = list(pr)
        miss[k] = None
        assert L.hgx_pattern_batch_dnf_not(snap.handle, 2, off.ctypes.data, *arrs, *miss, len(prog[4]),
                                           C.byref(h)) == _lib.HGX_E_INVALID, k
    assert L.hgx_query_result_not_stats(None, None, None, None, None) == _lib.HGX_E_INVALID
    still_good()
    snap.close()
    from test_gpu_partition import parts
    sh = parts(g, 2)
    with pytest.raises(HGXUnsupported):               # a shard is not a whole snapshot
        pattern_batch_dnf(sh[0], [[({"types": [], "inc": [0], "pos": [], "patterns": [], "arity": -1},
                                    [lower_not(hg.not_(hg.incident(1)))])]])
    for s in sh:
        s.close()
