"""TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Restatement of the reference's GraphClassics.dijkstra (core/src/java/org/hypergraphdb/algorithms/
GraphClassics.java:126-209) over oracle_ctypes.OracleGraph.generate, plus the helpers the shortest-path
tests share (rule R, a Bellman-Ford fixed point over pyref.reachable, path validation).
"""
from __future__ import annotations

import heapq

import numpy as np

import pyref
from oracle_ctypes import algen

# One (preceding, succeeding, reverse, source) tuple per generator mode of pyref.mode_of.
MODES = {
    pyref.MODE_SYM: (True, True, False, False),
    pyref.MODE_AFTER_FIRST: (False, True, False, False),
    pyref.MODE_BEFORE_FIRST: (True, False, False, False),
    pyref.MODE_BEFORE_LAST: (False, True, True, False),
    pyref.MODE_AFTER_LAST: (True, False, True, False),
}
assert all(pyref.mode_of(*m) == k for k, m in MODES.items())


def row_weights(g, w):
    """link atom -> weight for a per-link-row array (None: the reference's default Mapping, 1.0)."""
    if w is None:
        return lambda l: 1.0
    row = {int(l): r for r, l in enumerate(np.asarray(g["link_atom"]).tolist())}
    ww = [float(x) for x in w]
    return lambda l: ww[row[l]]


def dijkstra(orc, start, goal, opts=None, weight=None):
    """GraphClassics.java:126-209 line for line.  The TreeSet ordered by (dm, handle) is emulated by
    taking the minimum (dm, id) of the unsettled atoms (its remove + re-insert around a dm update are
    then free).  Returns (distance or None, dm, pred, settled order)."""
    weight = weight or (lambda l: 1.0)                       # :167-168
    dm = {start: 0.0}                                        # :135
    pred = {}
    settled = set()                                          # :170
    unsettled = {start}                                      # :171-172
    order = []
    while unsettled:                                         # :173
        a = min(unsettled, key=lambda h: (dm[h], h))         # :175 first() under the comparator :147-165
        unsettled.remove(a)                                  # :176
        if a == goal:                                        # :177
            return dm[goal], dm, pred, order                 # :178
        settled.add(a)                                       # :179
        order.append(a)
        weight_current = dm[a]                               # :181
        for l, n in orc.generate(a, opts):                   # :180,182-184
            if n in settled:                                 # :185
                continue
            weight_n = dm.get(n)                             # :187
            weight_an = weight(l)                            # :188
            if weight_n is None:                             # :189
                dm[n] = weight_current + weight_an           # :191
                unsettled.add(n)                             # :192
                pred[n] = a                                  # :193-194
            elif weight_n > weight_current + weight_an:      # :196
                dm[n] = weight_current + weight_an           # :199-201
                pred[n] = a                                  # :202-203
    return None, dm, pred, order                             # :208


def memo_generate(orc, opts=None):
    cache = {}

    def gen(a):
        r = cache.get(a)
        if r is None:
            r = cache[a] = orc.generate(a, opts)
        return r
    return gen


def dijkstra_heap(gen, start, goal, weight=None):
    """The same algorithm with a binary heap of (dm, id) and lazy deletion (larger graphs).  ``gen``:
    atom -> [(link, atom)].  Returns what ``dijkstra`` returns."""
    weight = weight or (lambda l: 1.0)
    dm = {start: 0.0}
    pred = {}
    settled = set()
    heap = [(0.0, start)]
    order = []
    while heap:
        d, a = heapq.heappop(heap)
        if a in settled or d != dm[a]:
            continue
        if a == goal:
            return dm[goal], dm, pred, order
        settled.add(a)
        order.append(a)
        for l, n in gen(a):
            if n in settled:
                continue
            nd = d + weight(l)
            wn = dm.get(n)
            if wn is None or wn > nd:
                dm[n] = nd
                pred[n] = a
                heapq.heappush(heap, (nd, n))
    return None, dm, pred, order


def rule_r(gen, weight, dm, start, sources):
    """Rule R: for every n != start that has a tight edge from an atom of ``sources`` (atoms whose dm is
    final), the predecessor minimising (dm[a], a) and a's lowest qualifying link: {n: (a, link)}."""
    weight = weight or (lambda l: 1.0)
    best = {}
    for a in sources:
        da = dm[a]
        for l, n in gen(a):
            if n == a or n == start or n not in dm:
                continue
            if bits(da + weight(l)) == bits(dm[n]):
                key = (da, a, l)
                if n not in best or key < best[n]:
                    best[n] = key
    return {n: (k[1], k[2]) for n, k in best.items()}


def bits(x) -> int:
    return int(np.float64(x).view(np.uint64))


def edges(g, mode, link_type=-1):
    """(src, dst, link row) of every generator edge of the mode, from pyref.reachable."""
    off, tg = np.asarray(g["tgt_off"]), np.asarray(g["tgt_idx"]).tolist()
    ty = g.get("link_type")
    out = []
    for r in range(len(g["link_atom"])):
        if link_type >= 0 and int(ty[r]) != link_type:
            continue
        T = tg[off[r]:off[r + 1]]
        for v in set(T):
            for t in set(T):
                if t != v and pyref.reachable(mode, T, v, t):
                    out.append((v, t, r))
    return np.array(out, np.int64).reshape(-1, 3)


def bellman_ford(num_atoms, e, w, start):
    """The least fixed point of d(n) = min(d(a) + w) by whole-graph sweeps (numpy): float64[num_atoms]."""
    d = np.full(num_atoms, np.inf)
    d[start] = 0.0
    if len(e) == 0:
        return d
    ww = np.ones(len(e)) if w is None else np.asarray(w, np.float64)[e[:, 2]]
    while True:
        nd = d.copy()
        np.minimum.at(nd, e[:, 1], d[e[:, 0]] + ww)
        if np.array_equal(nd.view(np.uint64), d.view(np.uint64)):
            return d
        d = nd


def check_path(gen, weight, start, goal, atoms, links, distance):
    """A reported path is valid: it runs start .. goal, every step is a pair the generator yields and
    the left-to-right weight sum is the distance, bit for bit."""
    weight = weight or (lambda l: 1.0)
    atoms, links = list(map(int, atoms)), list(map(int, links))
    assert atoms[0] == start and atoms[-1] == goal and len(links) == len(atoms) - 1, (atoms, links)
    d = 0.0
    for k, l in enumerate(links):
        assert (l, atoms[k + 1]) in gen(atoms[k]), (atoms, links, k)
        d = d + weight(l)
    assert bits(d) == bits(distance), (d, distance, atoms, links)


def opts_of(mode_tuple, link_type=-1):
    return algen(link_type, *mode_tuple)
