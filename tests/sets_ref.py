"""TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Reference for the visited-sets readout (include/hgx_sets.h; no GPU).  Set i of hgx_bfs_result_sets is the set form
of a TraversalBasedQuery over the breadth-first traversal of one start, intersected with an atom condition
(core/src/java/org/hypergraphdb/query/cond2qry/ToQueryMap.java:282-370): the atoms v with
min_depth <= depth_i(v) <= max_depth that satisfy ``keep``, ascending.  The per-depth sets come from the frozen
oracle (``oracle_levels``: OracleGraph.bfs_levels, the reference's FIFO traversal); ``sets`` only selects, filters
and sorts them, by plain Python over lists -- it knows nothing of bit rows, tiles or offsets of blocks."""
from __future__ import annotations

import numpy as np


def oracle_levels(orc, seeds, max_depth=None, opts=None):
    """[[V_0 = [seed], V_1, ...] for every seed]: lists of sorted atom lists from the oracle's traversal."""
    md = -1 if max_depth is None else int(max_depth)
    return [[lv.tolist() for lv in orc.bfs_levels(int(s), md, opts)] for s in seeds]


def sets(levels_per_seed, min_depth=0, max_depth=None, keep=None, with_depths=False):
    """(offsets int64[n + 1], atoms int32[total], depths int32[total] or None) of the selection
    ``levels_per_seed`` (one list of per-depth atom lists per set, in set order).  ``max_depth`` None or negative:
    to the last level.  ``keep``: one truth value per atom, or None."""
    off, atoms, deps = [0], [], []
    for levels in levels_per_seed:
        ent = []
        for d, lv in enumerate(levels):
            if d < min_depth or (max_depth is not None and 0 <= max_depth < d):
                continue
            ent.extend((int(a), d) for a in lv if keep is None or bool(keep[int(a)]))
        ent.sort()
        atoms.extend(a for a, _ in ent)
        deps.extend(d for _, d in ent)
        off.append(len(atoms))
    return (np.array(off, np.int64), np.array(atoms, np.int32),
            np.array(deps, np.int32) if with_depths else None)
