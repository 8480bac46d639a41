"""TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The unit-weight form of rule R (include/hgx_hops.h) over oracle_ctypes.OracleGraph.generate: BFS levels, and
for every reached atom n at depth d >= 1 the lowest-rank atom a != n of level d - 1 whose generate(a) yields
n, with a's lowest qualifying link.  tests/test_hop_ref.py checks it against the restatement of
GraphClassics.dijkstra in tests/sp_ref.py; the GPU tests compare the engine with it.
"""
from __future__ import annotations


def hop_rule(gen, start, max_depth=None):
    """``gen``: atom -> [(link, atom)] (sp_ref.memo_generate).  Returns (depth, pred): depth = {atom: level},
    pred = {n: (a, link)} for every reached n != start."""
    depth = {start: 0}
    pred = {}
    level = [start]
    d = 0
    while level and (max_depth is None or max_depth < 0 or d < max_depth):
        nxt = {}
        for a in sorted(level):                      # ascending rank: the first atom to reach n is the lowest
            for l, n in gen(a):
                l, n = int(l), int(n)
                if n == a or n in depth:
                    continue
                best = nxt.get(n)
                if best is None:
                    nxt[n] = (a, l)
                elif best[0] == a and l < best[1]:   # the same predecessor through a lower link
                    nxt[n] = (a, l)
        d += 1
        for n, k in nxt.items():
            depth[n] = d
            pred[n] = k
        level = list(nxt)
    return depth, pred


def follow(pred, start, goal):
    """(atoms, links) start .. goal along pred; None when the goal was not reached."""
    if goal != start and goal not in pred:
        return None
    atoms, links = [goal], []
    while atoms[-1] != start:
        a, l = pred[atoms[-1]]
        atoms.append(a)
        links.append(l)
    return atoms[::-1], links[::-1]
