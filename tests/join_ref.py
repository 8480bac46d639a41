"""Reference side of the join tests (no GPU): hg.apply(hg.targetAt(graph, p), cond) and the And of such
projections, by plain Python sets.

Each part's links come from not_ref.evaluate -- the brute-force evaluator that knows nothing of DNF, anchors or
scans; they are projected to the target position (a link too short for it contributes nothing: the rule of
include/hgx_join.h, where the reference's LinkProjectionMapping.eval would throw) and the value sets of a query's
parts are intersected.  The reference delivers the mapped values as a stream with duplicates
(C/query/cond2qry/ToQueryMap.java:409-427); this engine and find_all deliver the sorted set, and so does this
file.  Also a generator of random join queries over not_ref.random_tree / scan_ref.random_tree parts."""
from __future__ import annotations

import numpy as np

import not_ref as N
import scan_ref as S
from hypergraphdb_amd.query import Or, hg


_links = {}   # (id(pg), id(cond)) -> (pg, cond, links): one brute-force pass per part, shared by the tests


def part_links(pg, cond) -> list:
    """U_s: the link atoms of the part's condition."""
    k = (id(pg), id(cond))
    if k not in _links:
        _links[k] = (pg, cond, N.evaluate(pg, cond))
    return _links[k][2]


def project(pg, links, pos) -> set:
    """value(s): the links themselves for pos None, else their targets at ``pos`` where they have one."""
    if pos is None:
        return set(links)
    return {pg.links[l][1][pos] for l in links if len(pg.links[l][1]) > pos}


def part_value(pg, pos, cond) -> set:
    return project(pg, part_links(pg, cond), pos)


def evaluate(pg, parts) -> list:
    """The result of one join query [(pos, cond)]: the sorted intersection of its parts' values; no parts,
    no result."""
    if not parts:
        return []
    return sorted(set.intersection(*(part_value(pg, p, c) for p, c in parts)))


def stats(pg, queries) -> dict:
    """What hgx_query_result_join_stats must report for a batch of join queries."""
    parts = hits = distinct = kept = 0
    for q in queries:
        parts += len(q)
        for p, c in q:
            links = part_links(pg, c)
            hits += len(links)
            distinct += len(project(pg, links, p))
        kept += len(evaluate(pg, q))
    return {"parts": parts, "hits_projected": hits, "values_distinct": distinct, "kept": kept}


def occurrences(g):
    """atom -> [(position, link row)] for the positions 0..3 it occupies, and the atoms that occur at all"""
    occ = {}
    off, tg = g["tgt_off"], g["tgt_idx"]
    for r in range(len(g["link_atom"])):
        for p in range(min(4, int(off[r + 1] - off[r]))):
            occ.setdefault(int(tg[off[r] + p]), []).append((p, r))
    return occ


def random_query(rng, g, pg, occ, scan=False, n_types=3, p_steer=0.75):
    """One join query of 1 to 4 parts, sometimes 8.  A part is (pos, tree) with pos in 0..3 or None and tree a
    not_ref.random_tree (``scan``: a scan_ref.random_tree, whose DNF has clauses without an anchor).  Random
    parts rarely share a value, so most queries are steered by a pivot atom v: a steered part's tree is
    Or(tree, incidentAt(v, pos)) for a position v occupies in some link -- v is then a value of the part -- or,
    for pos None and a pivot that is a link with targets, Or(tree, link(targets of v)), which v satisfies.  What
    the tests expect never comes from the steering: ``evaluate`` decides."""
    n_parts = 8 if rng.random() < 0.06 else int(rng.integers(1, 5))
    steer = rng.random() < p_steer
    atoms = list(occ)
    v = atoms[int(rng.integers(0, len(atoms)))]
    parts = []
    for _ in range(n_parts):
        tree = S.random_tree(rng, g, n_types=n_types, pg=pg) if scan else N.random_tree(rng, g, n_types=n_types, pg=pg)
        pos = None if rng.random() < 0.15 else int(rng.integers(0, 4))
        if steer and rng.random() < 0.9:
            if pos is None and v in pg.links and pg.links[v][1]:
                tree = Or([tree, hg.link(*dict.fromkeys(pg.links[v][1]))])
            else:
                pos = occ[v][int(rng.integers(0, len(occ[v])))][0]
                tree = Or([tree, hg.incidentAt(v, pos)])
        parts.append((pos, tree))
    return parts


def random_queries(rng, g, pg, n, scan=False, n_types=3):
    occ = occurrences(g)
    return [random_query(rng, g, pg, occ, scan, n_types) for _ in range(n)]


def properties(pg, queries):
    """(queries with a non-empty result, queries whose result is strictly smaller than the smallest of their
    parts' value sets) -- by the evaluator alone"""
    nonempty = smaller = 0
    for q in queries:
        res = evaluate(pg, q)
        nonempty += bool(res)
        smaller += bool(q) and len(res) < min(len(part_value(pg, p, c)) for p, c in q)
    return nonempty, smaller
