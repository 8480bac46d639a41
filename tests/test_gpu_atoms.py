"""The pattern path over every atom (hgx_pattern_batch_atoms, include/hgx_atoms.h): type scans over the atom index,
which deliver node atoms too, and a predicate on the atoms a join projects to.  Expected results: tests/atoms_ref.py
(a brute force over all atoms with the reference's node rules), compared as exact id lists with offsets."""
import numpy as np
import pytest

import atoms_ref as AR
import kat_graphs as K
import sibling_ref as SR

pytestmark = pytest.mark.gpu

SEED = 3100
COUNTS = ("parts", "hits_projected", "values_distinct", "kept")
FILTER = ("queries_filtered", "values_tested", "values_rejected")
SCAN = ("clauses_scanned", "rows_scanned", "rows_kept")


def snapshot(g, atom_type=None):
    from hypergraphdb_amd import HyperGraphSnapshot
    s = HyperGraphSnapshot(g["num_atoms"], g["link_atom"], g["tgt_off"], g["tgt_idx"], g.get("link_type"))
    if atom_type is not None:
        s.set_atom_types(atom_type)
    return s


def check(r, expected):
    """ids and offsets of a batch against the per-query expected lists"""
    assert len(r) == len(expected)
    assert r.offsets.tolist() == np.concatenate([[0], np.cumsum([len(e) for e in expected])]).tolist()
    assert r.ids.tolist() == [x for e in expected for x in e]


_hand = {}


def hand():
    """(arrays, atom types, type keys, the model's graph): built once per process and left unchanged"""
    if not _hand:
        g, at, T = AR.hand_graph()
        _hand["v"] = (g, at, T, AR.AtomGraph(g, at))
    return _hand["v"]


def test_hand_graph_scans_deliver_nodes_and_links():
    from hypergraphdb_amd import hg, pattern_batch_atoms
    g, at, T, ag = hand()
    n = g["names"]
    a = n["a"]
    keys = sorted(T.values())
    conds = [hg.type(t) for t in keys]
    conds += [hg.and_(hg.type(t), hg.arity(0)) for t in keys]                 # nodes and the arity-0 link
    conds += [hg.and_(hg.type(t), hg.arity(2)) for t in keys]
    conds += [hg.and_(hg.type(t), hg.not_(hg.incident(a))) for t in keys]     # keeps the nodes
    conds += [hg.and_(hg.type(t), hg.not_(hg.arity(0))) for t in keys]
    conds += [hg.and_(hg.type(t), hg.not_(hg.orderedLink())) for t in keys]   # the empty pattern: nodes only
    conds += [hg.and_(hg.type(t), hg.not_(hg.link())) for t in keys]
    conds += [hg.and_(hg.type(t), hg.orderedLink(hg.anyHandle(), hg.anyHandle())) for t in keys]
    conds += [hg.or_(hg.type(T["NODE"]), hg.incident(a)),                     # scanned and anchored clauses united
              hg.or_(hg.type(T["ONE"]), hg.and_(hg.incident(a), hg.arity(2))),
              hg.typePlus({T["ONE"], T["MIX"], T["ABSENT"]}),                 # three keys, one absent
              hg.typePlus({T["NODE"], T["LINK"], T["BIG"]}),
              hg.and_(hg.type(T["BIG"]), hg.orderedLink())]                   # a NOP clause
    exp = [AR.evaluate(ag, c) for c in conds]
    by_type = dict(zip(keys, exp))
    for t in keys:                                                            # the model against numpy, type by type
        assert by_type[t] == np.nonzero(at == t)[0].tolist()
    node_only = exp[len(keys) + keys.index(T["NODE"])]
    assert node_only == by_type[T["NODE"]] and n["empty"] in exp[len(keys) + keys.index(T["MIX"])]
    assert exp[3 * len(keys) + keys.index(T["NODE"])] == by_type[T["NODE"]]   # not_(incident(a)) keeps every node
    assert n["empty"] not in exp[5 * len(keys) + keys.index(T["MIX"])] and n["mn0"] in exp[5 * len(keys) + keys.index(T["MIX"])]
    snap = snapshot(g, at)
    qs = [[(None, c)] for c in conds]
    r = pattern_batch_atoms(snap, qs)
    check(r, exp)
    assert {k: r.scan[k] for k in SCAN} == AR.scan_counts(ag, conds)
    assert {k: r.join[k] for k in COUNTS} == AR.stats(ag, qs)["join"]
    assert r.atoms == {"queries_filtered": 0, "values_tested": 0, "values_rejected": 0, "ms_filter": 0.0, "bytes_filter": 0.0}
    for q, e in list(zip(qs, exp))[::5]:
        check(pattern_batch_atoms(snap, [q]), [e])
    # a condition goes through atom_parts: no projection, one plain part
    check(pattern_batch_atoms(snap, conds[:len(keys)]), exp[:len(keys)])
    # the histogram of the index
    assert snap.type_atoms(keys + [99]).tolist() == np.bincount(at, minlength=100)[keys + [99]].tolist()
    # a link row without a type is indexed under its atom type: a scan of the type delivers it (the one
    # documented difference from hgx_scan.h)
    assert n["untyped"] in r[keys.index(T["MIX"])].tolist() and n["untyped"] in r[2 * len(keys) + keys.index(T["MIX"])].tolist()
    anchored = hg.and_(hg.type(T["MIX"]), hg.incident(a))
    check(pattern_batch_atoms(snap, [[(None, anchored)]]), [AR.evaluate(ag, anchored)])
    assert len(AR.evaluate(ag, anchored)) >= 5
    snap.close()


def filter_cases(g, T, snap):
    """(query: parts or a condition, keep: a raw tree or None, the parts for the model, the model's predicate)"""
    from hypergraphdb_amd import hg
    n = g["names"]
    a = n["a"]
    mix_a = hg.and_(hg.type(T["LINK"]), hg.orderedLink(n["n5"], hg.anyHandle()))
    person_knows = hg.and_(hg.type(T["NODE"]), hg.apply(hg.targetAt(snap, 1), mix_a))     # the introduction's query
    big = hg.and_(hg.type(T["BIG"]), hg.incident(a))
    m = hg.incident(n["n0"])
    cases = [
        (person_knows, None, [(1, mix_a)], hg.type(T["NODE"])),
        ([(1, big)], hg.type(T["NODE"]), [(1, big)], hg.type(T["NODE"])),
        ([(1, m)], hg.type(T["ONE"]), [(1, m)], hg.type(T["ONE"])),
        ([(1, m)], hg.type(T["ABSENT"]), [(1, m)], hg.type(T["ABSENT"])),                  # rejects everything
        ([(1, m), (0, hg.incident(a))], hg.not_(hg.type(T["MIX"])), [(1, m), (0, hg.incident(a))], hg.not_(hg.type(T["MIX"]))),
        ([(None, m)], hg.typePlus({T["MIX"], T["BIG"]}), [(None, m)], hg.typePlus({T["MIX"], T["BIG"]})),
        ([(1, m)], None, [(1, m)], None),
        ([], hg.type(T["NODE"]), [], hg.type(T["NODE"])),                                  # a predicate but no parts
        ([(0, hg.type(T["BIG"]))], hg.type(T["NODE"]), [(0, hg.type(T["BIG"]))], hg.type(T["NODE"])),   # a scanned part
    ]
    return cases


def test_filter_on_projected_atoms():
    from hypergraphdb_amd import AtomPredicate, hg, pattern_batch_atoms
    g, at, T, ag = hand()
    snap = snapshot(g, at)
    snap.set_timing(True)
    cases = filter_cases(g, T, snap)
    exp = [AR.join(ag, parts, tree) for _, _, parts, tree in cases]
    assert exp[0] == [g["names"]["n5"], g["names"]["n6"]] and exp[3] == [] and exp[7] == [] and sum(bool(e) for e in exp) >= 6
    plain = [AR.join(ag, parts) for _, _, parts, _ in cases]
    assert sum(len(e) < len(p) for e, p in zip(exp, plain)) >= 3              # the predicates reject something
    r = pattern_batch_atoms(snap, [c[0] for c in cases], keep=[c[1] for c in cases])
    check(r, exp)
    want = AR.stats(ag, [c[2] for c in cases], [c[3] for c in cases])
    assert {k: r.join[k] for k in COUNTS} == want["join"] and {k: r.atoms[k] for k in FILTER} == want["atoms"]
    assert want["atoms"]["values_tested"] > want["atoms"]["values_rejected"] > 0
    assert r.atoms["bytes_filter"] == 16.0 * want["atoms"]["values_tested"]
    assert 0 < r.atoms["ms_filter"] <= r.join["ms_join"]
    for c, e in zip(cases, exp):
        check(pattern_batch_atoms(snap, [c[0]], keep=[c[1]]), [e])
    # one compiled predicate serves many queries, next to another one and to None
    with AtomPredicate(snap, hg.type(T["NODE"])) as p1, AtomPredicate(snap, hg.not_(hg.type(T["NODE"]))) as p2:
        m = [(1, hg.incident(g["names"]["n0"]))]
        r = pattern_batch_atoms(snap, [m, m, m, m], keep=[p1, p2, None, p1])
        e1, e2 = AR.join(ag, m, hg.type(T["NODE"])), AR.join(ag, m, hg.not_(hg.type(T["NODE"])))
        assert e1 and e2 and sorted(e1 + e2) == AR.join(ag, m)
        check(r, [e1, e2, AR.join(ag, m), e1])
        assert r.atoms["queries_filtered"] == 3
    # the filter equals the same type written as a scanned self part: the two routes agree with the brute force
    for _, _, parts, tree in cases[1:6]:
        if parts and isinstance(tree, type(hg.type(0))):
            check(pattern_batch_atoms(snap, [parts + [(None, tree)]]), [AR.join(ag, parts, tree)])
    snap.close()


def test_mask_predicate_needs_no_atom_types():
    from hypergraphdb_amd import AtomPredicate, HGXUnsupported, hg, pattern_batch_atoms
    g, at, T, ag = hand()
    snap = snapshot(g)                                                        # no atom types
    mask = (np.arange(g["num_atoms"]) % 3 == 0).astype(np.uint8)
    m = [(1, hg.incident(g["names"]["n0"]))]
    exp = AR.join(ag, m, mask)
    assert exp and len(exp) < len(AR.join(ag, m))
    with AtomPredicate.from_mask(snap, mask) as p:
        check(pattern_batch_atoms(snap, [m, m], keep=[p, None], type_scan=False), [exp, AR.join(ag, m)])
        with pytest.raises(HGXUnsupported) as e:                              # the flag needs the column
            pattern_batch_atoms(snap, [m], keep=[p], type_scan=True)
        assert "atom types" in str(e.value)
    with pytest.raises(HGXUnsupported):                                       # and so does a raw type tree
        pattern_batch_atoms(snap, [m], keep=[hg.type(T["NODE"])], type_scan=False)
    with pytest.raises(HGXUnsupported):
        snap.type_atoms([T["NODE"]])
    snap.close()


def test_without_predicates_and_flag_it_is_the_join_entry():
    from hypergraphdb_amd import pattern_batch_atoms, pattern_batch_join
    from test_gpu_join import random_case
    g, pg, qs, exp = random_case(False)
    snap = snapshot(g)
    a = pattern_batch_atoms(snap, qs, keep=None, type_scan=False)
    j = pattern_batch_join(snap, qs)
    check(a, exp)
    check(j, exp)
    drop_ms = lambda d: {k: v for k, v in d.items() if not k.startswith("ms_")}   # noqa: E731
    assert drop_ms(a.join) == drop_ms(j.join) and drop_ms(a.union) == drop_ms(j.union)
    assert drop_ms(a.scan) == drop_ms(j.scan) and drop_ms(a.negation) == drop_ms(j.negation)
    assert a.atoms == {"queries_filtered": 0, "values_tested": 0, "values_rejected": 0, "ms_filter": 0.0, "bytes_filter": 0.0}
    snap.close()


def test_life_cycle_of_the_index():
    from hypergraphdb_amd import AtomPredicate, HGXError, HGXUnsupported, _lib, hg, pattern_batch_atoms
    g, at, T, ag = hand()
    snap = snapshot(g, at)
    q = [[(None, hg.type(T["NODE"]))], [(None, hg.and_(hg.type(T["PAD"]), hg.arity(0)))]]
    check(pattern_batch_atoms(snap, q), [AR.evaluate(ag, c) for (_, c), in q])
    # replacing the atom types changes the scan results: the index was rebuilt
    at2 = at.copy()
    at2[at == T["PAD"]] = T["NODE"]
    ag2 = AR.AtomGraph(g, at2)
    snap.set_atom_types(at2)
    exp2 = [AR.evaluate(ag2, c) for (_, c), in q]
    assert len(exp2[0]) == 63 + 78 and exp2[1] == []
    check(pattern_batch_atoms(snap, q), exp2)
    assert snap.type_atoms([T["NODE"], T["PAD"]]).tolist() == [141, 0]
    # an execution context borrows the snapshot's index, and follows a replaced column
    ctx = snap.context()
    check(pattern_batch_atoms(ctx, q), exp2)
    snap.set_atom_types(at)
    check(pattern_batch_atoms(ctx, q), [AR.evaluate(ag, c) for (_, c), in q])
    assert ctx.type_atoms([T["PAD"]]).tolist() == [78]
    ctx.close()
    # dropping the column: the flag is refused until it is set again; anchored batches go on
    snap.set_atom_types(None)
    with pytest.raises(HGXUnsupported):
        pattern_batch_atoms(snap, q)
    inc = [[(1, hg.incident(g["names"]["n0"]))]]
    check(pattern_batch_atoms(snap, inc, type_scan=False), [AR.join(ag, inc[0])])
    snap.set_atom_types(at)
    check(pattern_batch_atoms(snap, q), [AR.evaluate(ag, c) for (_, c), in q])
    # hgx_graph_update drops the column and the index with it
    snap.update(add={}, remove=[g["names"]["m1"]])
    with pytest.raises(HGXUnsupported):
        pattern_batch_atoms(snap, q)
    snap.set_atom_types(at)                                                   # (m1 is a node now; its type stays)
    r = pattern_batch_atoms(snap, [[(None, hg.and_(hg.type(T["MIX"]), hg.arity(0)))]])
    assert g["names"]["m1"] in r[0].tolist() and g["names"]["m0"] not in r[0].tolist()
    # a predicate of another snapshot is refused and the graph stays usable
    other = snapshot(g, at)
    with AtomPredicate(other, hg.type(T["NODE"])) as p:
        with pytest.raises(HGXError) as e:
            pattern_batch_atoms(snap, [inc[0], inc[0]], keep=[None, p])
        assert e.value.code == _lib.HGX_E_INVALID and "join query 1" in str(e.value)
    other.close()
    with pytest.raises(HGXError) as e:                                        # an unknown flag
        import ctypes as C
        h = C.c_void_p()
        off = np.zeros(1, np.int64)
        _lib.check(_lib.lib().hgx_pattern_batch_atoms(snap.handle, 0, off.ctypes.data, None, None, off.ctypes.data,
                                                      *([None] * 15), 0, 2, C.byref(h)))
    assert e.value.code == _lib.HGX_E_INVALID and "unknown flag" in str(e.value)
    snap.close()


def test_workspace_overflow_rerun_with_a_scanned_node_part():
    """test_gpu_join.py's 6,000-link hub, whose two anchored parts outgrow a fresh snapshot's workspace, with a
    scanned part over a node type and a predicate: every stage does nothing after the overflow and the rerun is
    exact."""
    from hypergraphdb_amd import hg, pattern_batch_atoms
    from test_gpu_not import hub_graph
    g = hub_graph(6000)
    n = g["names"]
    at = np.zeros(g["num_atoms"], np.int32)
    at[g["link_atom"]] = g["link_type"]
    at[n["h"]] = 9
    for i in range(7):
        at[n[f"x{i}"]] = 5 + i % 2
    ag = AR.AtomGraph(g, at)
    h = hg.incident(n["h"])
    q = [(1, h), (1, hg.and_(h, hg.type(2), hg.not_(hg.incident(n["x3"])))), (None, hg.type(5))]
    exp = AR.join(ag, q)
    assert exp == [n["x0"], n["x2"], n["x4"], n["x6"]] and 2 * 6000 > 16 * 3 + 4096
    snap = snapshot(g, at)
    for rep in range(2):
        r = pattern_batch_atoms(snap, [q, q], keep=[None, hg.not_(hg.type(5))])
        check(r, [exp, []])
        assert r.scan["rows_scanned"] == 2 * 4 and r.atoms["values_tested"] == 4 == r.atoms["values_rejected"]
    snap.close()


_random = {}


def random_case(i):
    """Graph i of the parity test with its atom types, queries, predicates and the model's results: computed once
    per process and left unchanged."""
    import dnf_ref as D
    import join_ref as J
    from hypergraphdb_amd import hg
    if i not in _random:
        rng = np.random.default_rng(SEED + i)
        n_links = int(rng.integers(20, 150))
        g = K.random_graph(rng, int(rng.integers(10, 300 - n_links)), n_links, max_arity=6, n_types=3)
        at = SR.atom_types(g, rng)
        pg, ag = D.graph_of(g), AR.AtomGraph(g, at)
        occ = J.occurrences(g)
        qs, keeps = [], []
        for _ in range(12):
            q = J.random_query(rng, g, pg, occ, scan=True) if occ else []
            if rng.random() < 0.3:                                            # a scanned self part next to the others
                q = q[:3] + [(None, hg.and_(hg.typePlus({0, 1, 2}), AR.random_type_tree(rng, 3, 1)))]
            qs.append(q)
            k = rng.random()
            keeps.append(None if k < 0.3 else (rng.random(g["num_atoms"]) < 0.5).astype(np.uint8) if k < 0.45
                         else AR.random_type_tree(rng, 3))
        _random[i] = (g, at, ag, qs, keeps, [AR.join(ag, q, k) for q, k in zip(qs, keeps)])
    return _random[i]


@pytest.mark.parametrize("i", range(20))
def test_random_graphs_vs_brute_force(i):
    from hypergraphdb_amd import AtomPredicate, pattern_batch_atoms
    g, at, ag, qs, keeps, exp = random_case(i)
    assert g["num_atoms"] <= 300
    snap = snapshot(g, at)
    masks = [AtomPredicate.from_mask(snap, k) if isinstance(k, np.ndarray) else k for k in keeps]
    r = pattern_batch_atoms(snap, qs, keep=masks)
    check(r, exp)
    want = AR.stats(ag, qs, keeps)
    assert {k: r.join[k] for k in COUNTS} == want["join"] and {k: r.atoms[k] for k in FILTER} == want["atoms"]
    assert {k: r.scan[k] for k in SCAN} == AR.scan_counts(ag, [c for q in qs for _, c in q])
    for m in masks:
        if isinstance(m, AtomPredicate):
            m.close()
    snap.close()


def test_random_cases_have_the_properties():
    """Over the twenty graphs: node atoms in results, predicates that reject and keep, empty and non-empty results."""
    nodes = rejected = nonempty = empty = 0
    for i in range(20):
        g, at, ag, qs, keeps, exp = random_case(i)
        st = AR.stats(ag, qs, keeps)["atoms"]
        rejected += st["values_rejected"] > 0 and st["values_tested"] > st["values_rejected"]
        for e in exp:
            nodes += any(x not in ag.links for x in e)
            nonempty += bool(e)
            empty += not e
    assert nodes >= 20 and rejected >= 10 and nonempty >= 40 and empty >= 20


def test_find_all_routes_the_two_shapes_with_atom_types():
    from hypergraphdb_amd import HGXUnsupported, find_all, hg
    g, at, T, ag = hand()
    n = g["names"]
    knows = hg.and_(hg.type(T["LINK"]), hg.orderedLink(n["n5"], hg.anyHandle()))
    snap = snapshot(g)
    person = lambda s: hg.and_(hg.type(T["NODE"]), hg.apply(hg.targetAt(s, 1), knows))   # noqa: E731
    scanned = [hg.type(T["NODE"]), hg.or_(hg.type(T["ONE"]), hg.incident(n["a"])),
               hg.and_(hg.type(T["MIX"]), hg.not_(hg.incident(n["a"])))]
    # without atom types every refusal stays
    for c in scanned + [person(snap)]:
        with pytest.raises(HGXUnsupported):
            find_all(snap, c)
    snap.set_atom_types(at)
    for c in scanned:
        assert find_all(snap, c) == AR.evaluate(ag, c), c
    assert find_all(snap, person(snap)) == [n["n5"], n["n6"]] == AR.join(ag, [(1, knows)], hg.type(T["NODE"]))
    # an anchored query keeps its route and its result
    assert find_all(snap, hg.and_(hg.type(T["BIG"]), hg.incident(n["a"]))) == AR.evaluate(ag, hg.and_(hg.type(T["BIG"]), hg.incident(n["a"])))
    snap.set_atom_types(None)
    with pytest.raises(HGXUnsupported):
        find_all(snap, scanned[0])
    snap.close()
