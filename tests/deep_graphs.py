"""Deep test graphs: hundreds to thousands of BFS levels on a few thousand atoms.

Plain numpy builders in the dict form kat_graphs.random_graph returns (num_atoms, link_atom, tgt_off, tgt_idx,
link_type).  Atom ids are the nodes first, then one atom per link, ascending in link order.  Every builder also
returns ``pos``: pos[p] = the atom id of chain position p (the identity unless ``rng`` permutes the node ids),
and the closed-form depths below hold from pos[...]; tests/test_deep_graphs.py proves them against the oracle
without a GPU.

  path(n, arity)     link i = (i, .., i + arity - 1): from position 0 the deepest distance is
                     ceil((n - 1) / (arity - 1)) in the symmetric mode and in (False, True, False, False).
  band(n, hubs)      path(n, 3) plus ``hubs`` hub atoms at the ends of the band (hub 0 behind position n - 1, hub 1
                     behind position 0, ...), each with PENDANTS pendant atoms on arity-2 links: atoms above the heavy
                     threshold (512 incident links) that enter the frontier at a late level.  From position 0 the
                     deepest distance is ceil((n - 1) / 2), + 2 with a hub at the far end (hub, then pendants).
  ladder(levels, w)  levels + 1 layers of w atoms; an atom of layer l has a link (a, b) to every b of layer l + 1
                     whose column is within +-1 of its own.  (False, True, False, False) from a layer-0 atom walks
                     one layer a level: deepest distance ``levels``, about w pairs a level.
"""
from __future__ import annotations

import numpy as np

PENDANTS = 700          # pendant atoms of one hub: its degree is PENDANTS + 1 > 512, the heavy threshold
SYM = (True, True, False, False)
FWD = (False, True, False, False)      # succeeding targets only: the chain walked in link order
BACK = (True, False, True, False)      # reversed target order: what precedes the focus there, i.e. the later targets, last first


def _graph(n_nodes, rows, types, pos, **extra):
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    tgt = np.concatenate([np.asarray(r, np.int64) for r in rows]).astype(np.int32) if rows else np.zeros(0, np.int32)
    return dict(num_atoms=n_nodes + len(rows), link_atom=np.arange(n_nodes, n_nodes + len(rows), dtype=np.int32),
                tgt_off=off, tgt_idx=tgt, link_type=np.asarray(types, np.int32), n_nodes=n_nodes,
                pos=np.asarray(pos, np.int32), **extra)


def _ids(n_nodes, rng):
    return np.arange(n_nodes) if rng is None else rng.permutation(n_nodes)


def path(n, arity=2, rng=None, loop=False):
    """n chain atoms; link i = (pos[i], .., pos[i + arity - 1]) for i <= n - arity, all of type 0.  loop: one more
    link (pos[n - 1], pos[0]) -- in FWD the deepest atom then still has something to expand (it yields the seed
    again), and the depths from position 0 stay the same; not for the symmetric mode (a cycle)."""
    ids = _ids(n, rng)
    rows = [ids[i:i + arity].tolist() for i in range(n - arity + 1)]
    if loop:
        rows.append([int(ids[n - 1]), int(ids[0])])
    return _graph(n, rows, np.zeros(len(rows), np.int32), ids)


def band(n, hubs=0, rng=None):
    """path(n, 3) + hubs: hub h hangs behind chain position n - 1 (h even) or 0 (h odd) on the link (end, hub) and
    carries PENDANTS links (hub, pendant).  Types: 0 on the band and hub links, j % 3 on a hub's j-th pendant
    link, so a traversal of type 0 is as deep as the untyped one and still meets a heavy atom, and the
    traversals of types 1 and 2 are shallow.  Returns also ``hub`` (the hub atom ids) and ``pendants`` (each hub's
    pendant atom ids)."""
    n_nodes = n + hubs * (1 + PENDANTS)
    ids = _ids(n_nodes, rng)
    rows = [ids[i:i + 3].tolist() for i in range(n - 2)]
    types = [0] * len(rows)
    hub_ids, pend = [], []
    for h in range(hubs):
        hub = n + h * (1 + PENDANTS)
        end = n - 1 if h % 2 == 0 else 0
        rows.append([int(ids[end]), int(ids[hub])])
        types.append(0)
        for j in range(PENDANTS):
            rows.append([int(ids[hub]), int(ids[hub + 1 + j])])
            types.append(j % 3)
        hub_ids.append(int(ids[hub]))
        pend.append(ids[hub + 1:hub + 1 + PENDANTS].astype(np.int32))
    return _graph(n_nodes, rows, types, ids[:n], hub=np.asarray(hub_ids, np.int32), pendants=pend)


def ladder(levels, width, loop=False):
    """(levels + 1) * width atoms, atom = layer * width + column; links (a, b) from layer l to l + 1 for
    |column(a) - column(b)| <= 1, in ascending (a, b) order, all of type 0.  loop: every atom of the last layer
    also gets a link (a, 0) back to atom 0, so in FWD the deepest atoms still have something to expand (the
    seed again: nothing new, the depths and pairs from atom 0 stay the same)."""
    rows = []
    for l in range(levels):
        for c in range(width):
            for c2 in range(max(0, c - 1), min(width, c + 2)):
                rows.append([l * width + c, (l + 1) * width + c2])
    if loop:
        rows += [[levels * width + c, 0] for c in range(width)]
    n_nodes = (levels + 1) * width
    return _graph(n_nodes, rows, np.zeros(len(rows), np.int32), np.arange(n_nodes))


def disjoint(*graphs):
    """The disjoint union, again nodes first and then links: ``pos`` becomes the list of the parts' pos arrays."""
    n_nodes = sum(g["n_nodes"] for g in graphs)
    rows, types, pos, base = [], [], [], 0
    for g in graphs:
        off, tgt = g["tgt_off"], g["tgt_idx"]
        rows += [(tgt[off[r]:off[r + 1]] + base).tolist() for r in range(len(off) - 1)]
        types += g["link_type"].tolist()
        pos.append((g["pos"] + base).astype(np.int32))
        base += g["n_nodes"]
    out = _graph(n_nodes, rows, types, np.zeros(0, np.int32))
    out["pos"] = pos
    return out


def ladder_pairs(levels, width):
    """Pairs of (False, True, False, False) from atom 0 (layer 0, column 0): layer l holds min(width, l + 1)
    reached atoms."""
    return sum(min(width, l + 1) for l in range(1, levels + 1))
