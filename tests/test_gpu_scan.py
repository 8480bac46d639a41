"""Type-index scans on the GPU pattern path (hgx_pattern_batch_dnf_scan, include/hgx_scan.h): a clause without
an incidence anchor and with a type is a scan of the type's segment of the device type index, opt-in through
pattern_batch_dnf(..., type_scan=True) and GpuScanToQuery.  Expected results: the brute-force evaluator of
tests/not_ref.py (it knows nothing of anchors, DNF or scans), compared as exact lists with offsets."""
import threading

import numpy as np
import pytest

import dnf_ref as D
import kat_graphs as K
import not_ref as N
import scan_ref as S
from test_gpu_not import check, hub_graph, snapshot

pytestmark = pytest.mark.gpu

ZERO_SCAN = {"clauses_scanned": 0, "rows_scanned": 0, "rows_kept": 0, "ms_scan": 0.0, "bytes_scan": 0.0}


def hand_cases(g):
    """(tree, expected result) on the queries graph"""
    from hypergraphdb_amd import hg
    n = g["names"]
    T, V = hg.type(K.T_TESTLINK), hg.type(K.T_VALUELINK)
    inc0 = hg.incident(n["n0"])
    value, linkH, linkH1, empty, link5 = n["valuelink"], n["linkH"], n["linkH1"], n["empty"], n["link5"]
    return [
        (T, [linkH, linkH1, empty, link5]),                                     # 0: the type alone
        (hg.and_(T, hg.arity(2)), [linkH]),
        (hg.and_(T, hg.orderedLink(-1, -1)), [linkH, linkH1, link5]),           # arity >= 2
        (hg.and_(T, hg.orderedLink()), []),                                     # a NOP
        (hg.and_(T, hg.not_(inc0)), [linkH1, empty, link5]),                    # 4: the tree test_gpu_not.py shows refused
        (hg.or_(inc0, T), [value, linkH, linkH1, empty, link5]),                # 5: linkH in both runs, delivered once
        (hg.typePlus([K.T_VALUELINK, K.T_TESTLINK, 77]), [value, linkH, linkH1, empty, link5]),
        (hg.type(77), []),                                                      # an absent type
        (hg.and_(V, T), []),                                                    # "empty"
        (hg.and_(T, hg.not_(T)), []),
        (hg.and_(T, hg.not_(hg.arity(2)), hg.not_(hg.incident(linkH1))), [linkH1, empty]),
        (hg.and_(hg.typePlus([K.T_VALUELINK, K.T_TESTLINK]), hg.not_(hg.orderedLink(n["n2"], n["n3"]))),
         [linkH, empty, link5]),
        (hg.or_(hg.and_(T, hg.arity(3)), hg.and_(hg.incident(n["n2"]), hg.not_(V))), [linkH1, link5]),
    ]


def test_hand_cases_on_the_queries_graph():
    from hypergraphdb_amd import GpuScanToQuery, HGQueryConfiguration, HGXUnsupported, find_all, hg, pattern_batch_dnf
    from hypergraphdb_amd.query import And, Or, _ext_arrays, pattern_batch_dnf_scan_arrays
    g = K.queries_graph()
    snap, pg = snapshot(g), D.graph_of(g)
    cases = hand_cases(g)
    trees, exp = [c[0] for c in cases], [c[1] for c in cases]
    assert exp[0] == g["link_atom"][g["link_type"] == K.T_TESTLINK].tolist()
    r = pattern_batch_dnf(snap, trees, type_scan=True)          # in one batch
    check(r, exp)
    clauses, rows, kept = S.scan_counts(pg, S.type_count(g), trees)
    assert (clauses, rows) == (15, 42) and kept > 20     # (typePlus counts once per type; "empty" not at all)
    assert (r.scan["clauses_scanned"], r.scan["rows_scanned"], r.scan["rows_kept"]) == (clauses, rows, kept)
    config = HGQueryConfiguration()
    config.addCompiler(And, GpuScanToQuery())
    config.addCompiler(Or, GpuScanToQuery())
    anchored = hg.and_(hg.incident(g["names"]["n2"]), hg.type(K.T_TESTLINK))
    for i, (tree, e) in enumerate(cases):                       # one by one
        check(pattern_batch_dnf(snap, [tree], type_scan=True), [e])
        assert find_all(snap, tree, config) == e, tree
        if i != 8:   # (and(V, T) is "empty" with or without the scan: no clause is left to refuse)
            with pytest.raises(HGXUnsupported):                 # no opt-in: refused as ever
                pattern_batch_dnf(snap, [tree])
            with pytest.raises(HGXUnsupported):
                find_all(snap, tree)
            with pytest.raises(HGXUnsupported):
                pattern_batch_dnf(snap, [anchored, tree])
    assert pattern_batch_dnf(snap, [trees[8]])[0].tolist() == []
    assert GpuScanToQuery().getMetaData(snap, trees[4]).ordered and GpuScanToQuery().getMetaData(snap, trees[4]).randomAccess
    assert find_all(snap, anchored, config) == find_all(snap, anchored) == [g["names"]["linkH1"], g["names"]["link5"]]
    # a query with no clauses between two scanned ones, and a batch of 0 queries
    r = pattern_batch_dnf(snap, [trees[0], [], trees[4], hg.or_(), trees[5]], type_scan=True)
    check(r, [exp[0], [], exp[4], [], exp[5]])
    r = pattern_batch_dnf(snap, [], type_scan=True)
    assert len(r) == 0 and r.scan == ZERO_SCAN
    r = pattern_batch_dnf_scan_arrays(snap, [0, 0, 0], *_ext_arrays([]))
    assert r.offsets.tolist() == [0, 0, 0] and r.scan == ZERO_SCAN
    assert snap.type_links([K.T_TESTLINK, K.T_VALUELINK, 77, K.T_NODE]).tolist() == [4, 1, 0, 0]
    snap.close()


SEGMENT_SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025)


@pytest.fixture(scope="module")
def segments():
    """Types with exactly SEGMENT_SIZES links (type key = 10 + its index; the first has none), the keys 0 and
    2_000_000_000 on top, their rows scattered over the row order by a fixed permutation; arities 0..12, some
    targets links, some repeated, node x a frequent target."""
    rng = np.random.default_rng(11)
    types = np.concatenate([np.full(s, 10 + i, np.int32) for i, s in enumerate(SEGMENT_SIZES)] +
                           [np.full(5, 0, np.int32), np.full(3, 2_000_000_000, np.int32)])
    types = types[rng.permutation(len(types))]
    b = K.Builder()
    nodes = [b.node(f"v{i}") for i in range(40)]
    x = nodes[7]
    made = []
    for i, t in enumerate(types):
        k = i % 13
        row = []
        for j in range(k):
            u = rng.random()
            if u < 0.25:
                row.append(x)
            elif u < 0.4 and made:
                row.append(made[int(rng.integers(0, len(made)))])     # a link as a target
            elif u < 0.5 and row:
                row.append(row[int(rng.integers(0, len(row)))])       # a repeated target
            else:
                row.append(nodes[int(rng.integers(0, len(nodes)))])
        made.append(b.link(None, int(t), *row))
        if i % 50 == 0:
            nodes.append(b.node(f"w{i}"))                             # link atoms are not contiguous
    g = b.arrays()
    g["x"] = x
    return g, D.graph_of(g)


def test_segment_boundaries(segments):
    from hypergraphdb_amd import hg, pattern_batch_dnf
    g, pg = segments
    keys = [10 + i for i in range(len(SEGMENT_SIZES))] + [0, 2_000_000_000]
    cnt = S.type_count(g)
    assert [cnt.get(k, 0) for k in keys] == list(SEGMENT_SIZES) + [5, 3]
    arity = np.diff(g["tgt_off"])
    assert arity.min() == 0 and arity.max() == 12 and (arity > 8).sum() > 500
    assert len(set(np.diff(np.nonzero(g["link_type"] == 21)[0]))) > 3     # rows of a type are scattered
    snap = snapshot(g)
    assert snap.type_links(keys).tolist() == [cnt.get(k, 0) for k in keys]
    assert snap.type_links(np.arange(40)).tolist() == np.bincount(g["link_type"][g["link_type"] < 40], minlength=40).tolist()
    trees = []
    for k in keys:
        T = hg.type(k)
        trees += [T, hg.and_(T, hg.arity(0)), hg.and_(T, hg.arity(8)), hg.and_(T, hg.arity(9)),
                  hg.and_(T, hg.not_(hg.incident(g["x"])))]
    exp = [N.evaluate(pg, t) for t in trees]
    assert exp[5 * 11] == g["link_atom"][g["link_type"] == 21].tolist() and len(exp[5 * 11]) == 1025
    assert 0 < len(exp[5 * 11 + 4]) < 1025 and len(exp[5 * 11 + 3]) > 0
    r = pattern_batch_dnf(snap, trees, type_scan=True)           # all in one batch
    check(r, exp)
    assert r.scan["clauses_scanned"] == len(trees) and r.scan["rows_scanned"] == 5 * len(g["link_atom"])
    assert r.scan["rows_kept"] == sum(map(len, exp))
    for t, e in zip(trees, exp):                                 # each alone
        check(pattern_batch_dnf(snap, [t], type_scan=True), [e])
    snap.close()


# picked on the CPU: of its 300 trees 146 have a scanned clause with a non-empty result (75 are asked for), 54 a
# scanned clause whose Nots reject some rows and keep others (38), 48 an id shared by a scanned and an anchored
# clause (38); tests/test_scan_ref.py asserts the shares without a GPU
SEED = 2102


def random_case(seed):
    rng = np.random.default_rng(seed)
    g = K.random_graph(rng, 600, 2500, max_arity=12, n_types=3)
    pg = D.graph_of(g)
    trees = [S.random_tree(rng, g, pg=pg) for _ in range(300)]
    return g, pg, trees, [N.evaluate(pg, t) for t in trees]


@pytest.fixture(scope="module")
def rand():
    return random_case(SEED)


def test_random_trees_vs_brute_force(rand):
    from hypergraphdb_amd import pattern_batch_dnf
    g, pg, trees, exp = rand
    props = np.array([S.properties(pg, t) for t in trees])
    nonempty, split, shared = props.sum(axis=0)
    assert nonempty >= len(trees) // 4 and split >= len(trees) // 8 + 1 and shared >= len(trees) // 8 + 1
    snap = snapshot(g)
    r = pattern_batch_dnf(snap, trees, type_scan=True)
    check(r, exp)
    assert r.union["kept"] == len(r.ids) and r.scan["bytes_scan"] > 0
    snap.close()


def test_workspace_growth():
    """A fresh snapshot has room for 16 n + 4096 hits: the scan's hits alone, or with an anchored clause's,
    outgrow it; the scan sets the overflow word, the union does nothing, the host grows the workspace and runs
    the batch once more."""
    from hypergraphdb_amd import hg, pattern_batch_dnf
    g = hub_graph(6000, n_types=1)
    pg = D.graph_of(g)
    h, x = g["names"]["h"], g["names"]["x3"]
    assert 6000 > 16 * 1 + 4096
    all_links = g["link_atom"].tolist()
    snap = snapshot(g)
    for rep in range(2):                                         # one type of 6,000 links, one clause, twice
        r = pattern_batch_dnf(snap, [hg.type(0)], type_scan=True)
        check(r, [all_links])
        assert r.scan["rows_scanned"] == r.scan["rows_kept"] == 6000
    snap.close()
    snap = snapshot(g)                                           # next to an anchored clause on the hub
    tree = hg.or_(hg.and_(hg.incident(h), hg.not_(hg.incident(x))), hg.and_(hg.type(0), hg.incident(x)), hg.type(0))
    assert N.evaluate(pg, tree) == all_links
    for rep in range(2):
        r = pattern_batch_dnf(snap, [tree], type_scan=True)
        check(r, [all_links])
        assert r.union["clause_hits"] == 6000 + 6000 and r.negation["hits_tested"] == 6000
    snap.close()
    g = hub_graph(64, n_types=1)                                 # 1,024 scanned clauses of one 64-link type
    snap = snapshot(g)
    assert 1024 * 64 > 16 * 1024 + 4096
    r = pattern_batch_dnf(snap, [hg.type(0)] * 1024, type_scan=True)
    check(r, [g["link_atom"].tolist()] * 1024)
    assert r.scan["clauses_scanned"] == 1024 and r.scan["rows_kept"] == 1024 * 64
    snap.close()


def test_stats_equal_the_reference_counts(rand):
    from hypergraphdb_amd import pattern_batch_dnf, to_dnf
    g, pg, trees, exp = rand
    trees, exp = trees[:60], exp[:60]
    clauses, rows, kept = S.scan_counts(pg, S.type_count(g), trees)
    tested, rejected = S.anchored_filter_counts(pg, trees)
    assert clauses > 0 and rows > kept > 0 and tested > rejected > 0
    snap = snapshot(g)
    snap.set_timing(True)
    r = pattern_batch_dnf(snap, trees, type_scan=True)
    check(r, exp)
    assert (r.scan["clauses_scanned"], r.scan["rows_scanned"], r.scan["rows_kept"]) == (clauses, rows, kept)
    assert 0 < r.scan["ms_scan"] <= r.ms["ms_total"] and r.scan["bytes_scan"] > 0
    # the filter's statistics count the hits of anchored clauses only
    assert (r.negation["hits_tested"], r.negation["hits_rejected"]) == (tested, rejected)
    assert r.union["clause_hits"] >= kept and r.union["kept"] == len(r.ids)
    # a batch without a scanned clause through type_scan=True: hgx_pattern_batch_dnf_not's statistics
    anch = [t for t in trees if not any(S.is_scanned(cl) for cl in to_dnf(t))]
    assert len(anch) >= 5
    a, b = pattern_batch_dnf(snap, anch, type_scan=True), pattern_batch_dnf(snap, anch)
    assert a.scan == ZERO_SCAN and b.scan is None
    assert a.offsets.tobytes() == b.offsets.tobytes() and a.ids.tobytes() == b.ids.tobytes()
    for k in ("clause_hits", "kept", "bytes_union"):
        assert a.union[k] == b.union[k], k
    for k in ("hits_tested", "hits_rejected", "bytes_not"):
        assert a.negation[k] == b.negation[k], k
    snap.close()


def test_errors_leave_the_graph_usable():
    import ctypes as C
    from hypergraphdb_amd import HGXError, HGXUnsupported, _lib, hg, pattern_batch_dnf
    from hypergraphdb_amd.query import _ext_arrays, encode_negations, lower_not, pattern_batch_dnf_scan_arrays
    g = K.queries_graph()
    snap, n = snapshot(g), g["names"]
    inc0, T = hg.incident(n["n0"]), hg.type(K.T_TESTLINK)
    good = hg.and_(T, hg.not_(inc0))

    def still_good():
        assert pattern_batch_dnf(snap, [good], type_scan=True)[0].tolist() == [n["linkH1"], n["empty"], n["link5"]]

    still_good()
    for tree in (hg.arity(2), hg.not_(inc0)):                    # neither a type nor an anchor
        with pytest.raises(HGXUnsupported) as e:
            pattern_batch_dnf(snap, [good, hg.or_(inc0, tree)], type_scan=True)
        assert "query 1 clause 1" in str(e.value)
        still_good()
    two = {"types": [K.T_VALUELINK, K.T_TESTLINK], "inc": [], "pos": [], "patterns": [], "arity": -1}
    one = {"types": [K.T_TESTLINK], "inc": [], "pos": [], "patterns": [], "arity": -1}
    with pytest.raises(HGXUnsupported) as e:                     # two types in an anchor-free clause, at the array level
        pattern_batch_dnf_scan_arrays(snap, [0, 2], *_ext_arrays([one, two]))
    assert "query 0 clause 1" in str(e.value)
    still_good()
    with pytest.raises(HGXError) as e:                           # an atom id out of range inside the Not of a scanned clause
        pattern_batch_dnf(snap, [good, hg.or_(inc0, hg.and_(T, hg.not_(inc0), hg.not_(hg.incident(g["num_atoms"] + 3))))],
                          type_scan=True)
    assert e.value.code == _lib.HGX_E_INVALID and "query 1 clause 1 negation 1" in str(e.value)
    still_good()
    with pytest.raises(HGXError) as e:                           # a negative type key
        pattern_batch_dnf_scan_arrays(snap, [0, 1], *_ext_arrays([dict(one, types=[-5])]))
    assert e.value.code == _lib.HGX_E_INVALID
    still_good()
    # null arguments: a status, never a crash
    L = _lib.lib()
    h = C.c_void_p()
    arrs = [a.ctypes.data for a in _ext_arrays([one, one])]
    off = np.array([0, 1, 2], np.int64)
    prog = encode_negations([[lower_not(hg.not_(inc0))], []])
    pr = [p.ctypes.data for p in prog]
    assert L.hgx_pattern_batch_dnf_scan(snap.handle, 2, off.ctypes.data, *arrs, *pr, len(prog[4]), None) == _lib.HGX_E_INVALID
    assert L.hgx_pattern_batch_dnf_scan(snap.handle, 2, None, *arrs, *pr, len(prog[4]), C.byref(h)) == _lib.HGX_E_INVALID
    assert L.hgx_pattern_batch_dnf_scan(None, 2, off.ctypes.data, *arrs, *pr, len(prog[4]), C.byref(h)) == _lib.HGX_E_INVALID
    for k in range(1, 5):                                        # a missing array of the program
        miss = list(pr)
        miss[k] = None
        assert L.hgx_pattern_batch_dnf_scan(snap.handle, 2, off.ctypes.data, *arrs, *miss, len(prog[4]),
                                            C.byref(h)) == _lib.HGX_E_INVALID, k
    assert L.hgx_pattern_batch_dnf_scan(snap.handle, 2, off.ctypes.data, *arrs, *[None] * 5, 0, C.byref(h)) == _lib.HGX_OK
    L.hgx_query_result_free(h)
    assert L.hgx_query_result_scan_stats(None, None, None, None, None, None) == _lib.HGX_E_INVALID
    assert L.hgx_graph_type_links(snap.handle, None, 3, None) == _lib.HGX_E_INVALID
    still_good()
    snap.close()
    from test_gpu_partition import parts
    sh = parts(g, 2)
    with pytest.raises(HGXUnsupported):                          # a shard is not a whole snapshot
        pattern_batch_dnf(sh[0], [[one]], type_scan=True)
    for s in sh:
        s.close()


def test_index_lifetime_contexts_and_the_plain_paths(rand):
    from hypergraphdb_amd import hg, pattern_batch, pattern_batch_dnf
    g, pg, trees, exp = rand
    snap = snapshot(g)
    # the paths that do not opt in return the same before and after a scanned batch
    anchored = [N.strip_nots(t) for t in N_trees(g, pg)]
    plain_q = [(int(g["link_type"][i]), [int(g["tgt_idx"][g["tgt_off"][i]])], None) for i in range(len(g["link_atom"]))
               if g["tgt_off"][i + 1] > g["tgt_off"][i]][:64]
    before = (pattern_batch(snap, plain_q), pattern_batch_dnf(snap, anchored))
    check(pattern_batch_dnf(snap, trees[:80], type_scan=True), exp[:80])
    after = (pattern_batch(snap, plain_q), pattern_batch_dnf(snap, anchored))
    for a, b in zip(before, after):
        assert a.offsets.tobytes() == b.offsets.tobytes() and a.ids.tobytes() == b.ids.tobytes()
    assert len(before[0].ids) > 0 and len(before[1].ids) > 0
    # the same batch from 4 threads, each on its own context
    ctxs = [snap.context() for _ in range(4)]
    out, errs = [None] * 4, []

    def work(i):
        try:
            for _ in range(2):
                out[i] = pattern_batch_dnf(ctxs[i], trees, type_scan=True)
        except Exception as ex:   # noqa: BLE001
            errs.append(ex)

    ths = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs
    for o in out:
        check(o, exp)
    for c in ctxs:
        c.close()
    # an update changes a type's membership: the index is dropped and the next scan rebuilds it
    la, ty = g["link_atom"], g["link_type"]
    t0 = [int(a) for a in la[ty == 0][:3]]
    t1 = [int(a) for a in la[ty == 1][:2]]
    free = [a for a in range(g["num_atoms"]) if a not in set(la.tolist())][:2]
    q = [hg.type(0), hg.and_(hg.type(1), hg.not_(hg.arity(2))), hg.type(2)]
    check(pattern_batch_dnf(snap, q, type_scan=True), [N.evaluate(pg, t) for t in q])
    snap.update(add={t1[0]: (0, [free[0], t0[2]]), free[1]: (0, [free[0]]), t1[1]: (1, [free[0], free[0]])},
                remove=t0[:2] + t1)
    g2 = dict(num_atoms=snap.A, link_atom=snap.link_atom, tgt_off=snap.tgt_off, tgt_idx=snap.tgt_idx, link_type=snap.link_type)
    pg2 = D.graph_of(g2)
    exp2 = [N.evaluate(pg2, t) for t in q]
    assert t1[0] in exp2[0] and free[1] in exp2[0] and t0[0] not in exp2[0] and t1[1] not in exp2[1]
    check(pattern_batch_dnf(snap, q, type_scan=True), exp2)
    assert snap.type_links([0, 1, 2]).tolist() == np.bincount(g2["link_type"], minlength=3).tolist()
    snap.close()


def N_trees(g, pg):
    """40 anchored trees of tests/not_ref.py (every clause has an anchor: the default path takes them)"""
    rng = np.random.default_rng(5)
    return [N.random_tree(rng, g, pg=pg) for _ in range(40)]
