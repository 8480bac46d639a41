"""TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Reference for the sibling predicate tests (no GPU).  With a siblingPredicate the iterator of
DefaultALGenerator.generate(src) yields exactly the null-predicate adjacency list, in the same order, without
every target h for which siblingPredicate.satisfies(hg, h) is false -- the focus atom under returnSource included
(core/src/java/org/hypergraphdb/algorithms/DefaultALGenerator.java: filter() 120-150 and 207-237, its call sites
156-157, 188-189, 251-252, 272-273, the focus cases 131, 177, 193, 218, 243, 256).  So the predicate is an
element-wise filter on the adjacency list: ``filtered`` wraps any generator callable (oracle/pyref.py's generate,
sp_ref.memo_generate over the C oracle) and everything else -- per-depth sets, hop_ref.hop_rule,
sp_ref.dijkstra_heap / rule_r -- runs on the wrapped callable unchanged.  The start atom is never tested, an atom
that fails is never reached and so never expanded.

``holds`` evaluates a sibling tree on one atom's type by direct recursion over And / Or / Not; it knows nothing of
negation normal form, terms or the encoding, so it checks the lowering and the kernel independently."""
from __future__ import annotations

import numpy as np

import hop_ref
import sp_ref
from hypergraphdb_amd.algorithms import AtomTypeCondition
from hypergraphdb_amd.query import And, Not, Or, TypePlusCondition


def filtered(gen, keep):
    """``gen``: atom -> [(link, atom)]; ``keep``: a sequence of truth values per atom, or a callable atom -> bool.
    The same callable without the pairs whose atom fails ``keep`` (memoised)."""
    ok = keep if callable(keep) else (lambda a, k=keep: bool(k[a]))
    cache = {}

    def fgen(a):
        r = cache.get(a)
        if r is None:
            r = cache[a] = [(l, n) for l, n in gen(a) if ok(int(n))]
        return r
    return fgen


def levels(fgen, start, max_depth=None):
    """[V_0 = {start}, V_1, ...] as sorted lists, by a plain level BFS that never tests the start."""
    seen = {int(start)}
    out = [[int(start)]]
    d = 0
    while out[-1] and (max_depth is None or max_depth < 0 or d < max_depth):
        nxt = set()
        for a in out[-1]:
            for _, n in fgen(a):
                n = int(n)
                if n not in seen:
                    seen.add(n)
                    nxt.add(n)
        d += 1
        out.append(sorted(nxt))
    if not out[-1]:
        out.pop()
    return out


class ManyLevels:
    """``levels`` for many starts at once, for the batches of a thousand seeds: the same plain level BFS over the
    pairs of ``fgen`` with one bit per start (numpy).  ``rows[d]``: uint64[A, W], bit i of row n set iff atom n is
    in V_d of start i.  tests/test_sibling_ref.py checks it against ``levels`` start by start."""

    def __init__(self, fgen, num_atoms, seeds, max_depth=None):
        A, S = int(num_atoms), len(seeds)
        W = max(1, (S + 63) // 64)
        pairs = sorted({(int(n), a) for a in range(A) for _, n in fgen(a) if int(n) != a})
        dst = np.array([p[0] for p in pairs], np.int64)
        src = np.array([p[1] for p in pairs], np.int64)
        uniq, first = np.unique(dst, return_index=True) if len(dst) else (dst, dst)
        vis = np.zeros((A, W), np.uint64)
        for i, s in enumerate(seeds):
            vis[int(s), i >> 6] |= np.uint64(1) << np.uint64(i & 63)
        self.S, self.rows, self._bits = S, [vis.copy()], {}
        front, d = vis.copy(), 0
        while len(dst) and (max_depth is None or max_depth < 0 or d < max_depth):
            new = np.zeros_like(vis)
            new[uniq] = np.bitwise_or.reduceat(front[src], first, axis=0) & ~vis[uniq]
            if not new.any():
                break
            vis |= new
            self.rows.append(new)
            front, d = new, d + 1

    def bits(self, d):
        """bool[A, S]: membership of level d."""
        if d not in self._bits:
            self._bits[d] = np.unpackbits(self.rows[d].view(np.uint8), axis=1, bitorder="little")[:, :self.S].astype(bool)
        return self._bits[d]

    def counts(self):
        """int64[S, levels]"""
        return np.stack([self.bits(d).sum(0) for d in range(len(self.rows))], axis=1).astype(np.int64)

    def levels(self, i):
        return [np.nonzero(self.bits(d)[:, i])[0].tolist() for d in range(len(self.rows))]


def hop_rule(fgen, start, max_depth=None):
    return hop_ref.hop_rule(fgen, start, max_depth)


def dijkstra(fgen, start, goal, weight=None):
    return sp_ref.dijkstra_heap(fgen, start, goal, weight)


def rule_r(fgen, weight, dm, start, sources):
    return sp_ref.rule_r(fgen, weight, dm, start, sources)


def holds(tree, type_) -> bool:
    """A sibling tree over hg.type / hg.typePlus on an atom of this type key."""
    if isinstance(tree, And):
        return all(holds(c, type_) for c in tree)
    if isinstance(tree, Or):
        return any(holds(c, type_) for c in tree)
    if isinstance(tree, Not):
        return not holds(tree.negated, type_)
    if isinstance(tree, AtomTypeCondition):          # AtomTypeCondition.java:121-135
        return type_ == tree.type
    if isinstance(tree, TypePlusCondition):          # TypePlusCondition.java:63-71
        return type_ in tree.types
    raise TypeError(tree)


def flags(atom_types, tree) -> np.ndarray:
    """uint8[A]: 1 where the atom's type satisfies the tree."""
    return np.array([holds(tree, int(t)) for t in atom_types], np.uint8)


def atom_types(g, rng, n_types=3) -> np.ndarray:
    """One type key per atom: the link atoms keep their link types, the others get random ones."""
    t = rng.integers(0, n_types, g["num_atoms"]).astype(np.int32)
    lt = g.get("link_type")
    t[np.asarray(g["link_atom"])] = 0 if lt is None else np.asarray(lt, np.int32)
    return t
