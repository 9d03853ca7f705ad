"""BFS atom masking of the reference's datasets (Molecule3DDataset.subgraph, Geom3D/datasets/datasets_3D.py:24-67, and
MoleculeDataset3DRadius.subgraph, datasets_3D_Radius.py:43-87), host side.

The reference keeps ``int(n * (1 - mask_ratio)) + 1`` atoms of every molecule it fetches: a BFS over the bond graph
``data.edge_index`` from a random atom, one random frontier atom per step, a random unvisited atom when the frontier is
empty.  The kept count depends on n alone, so every index structure of a masked batch is known on the host before the
draw; which atoms are kept is decided per batch, either

* ``mask_rng="numpy"``: ``reference_bfs`` below, a restatement of the reference's loop that makes the same
  ``np.random`` calls in the same order on the same Python sets (bit-for-bit reproduction of a reference run, about as
  slow as the reference), or
* ``mask_rng="device"``: drawn on the GPU by ``geossl_gather_masked_molecules`` (csrc/gather.hip) from a counter-based
  stream - the rule is in include/geossl_hip.h and DESIGN 2.
"""
import numpy as np

MASK_RNGS = ("device", "numpy")
MASK_MAX_N = 2048   # the device BFS keeps its visited / frontier bitsets as one 32-bit word per lane of a wave


def check_ratio(ratio):
    r = float(ratio)
    if not (0.0 <= r < 1.0):
        raise ValueError("mask_ratio is in [0, 1), got %r" % (ratio,))
    return r


def kept_count(n, ratio):
    """int(n * (1 - ratio)) + 1 per molecule (datasets_3D.py:26,33: the BFS loop runs while len(idx_sub) <= sub_num),
    float64 and truncated as Python's int() does."""
    n = np.asarray(n, dtype=np.int64)
    return np.trunc(n * (1.0 - float(ratio))).astype(np.int64) + 1


def successors(n, bonds):
    """to_networkx(data).neighbors(a) of every atom a < n (a DiGraph built from edge_index in column order: successors
    in order of first appearance, repeats dropped); bonds: [2, E] local indices."""
    succ = [dict() for _ in range(n)]
    for u, v in zip(bonds[0].tolist(), bonds[1].tolist()):
        succ[u].setdefault(v, None)
    return [list(s) for s in succ]


def reference_bfs(n, succ, ratio):
    """The kept atoms of one molecule, ascending: datasets_3D.py:25-45 restated over the successor lists `succ` (the
    same np.random draws, the same Python set operations in the same order)."""
    sub_num = int(n * (1 - ratio))
    idx_sub = [np.random.randint(n, size=1)[0]]
    idx_neigh = set([v for v in succ[int(idx_sub[-1])]])
    while len(idx_sub) <= sub_num:
        if len(idx_neigh) == 0:
            idx_unsub = list(set([v for v in range(n)]).difference(set(idx_sub)))
            idx_neigh = set([np.random.choice(idx_unsub)])
        sample_node = np.random.choice(list(idx_neigh))
        idx_sub.append(sample_node)
        idx_neigh = idx_neigh.union(set([v for v in succ[int(idx_sub[-1])]])).difference(set(idx_sub))
    idx_sub.sort()
    return np.asarray(idx_sub, dtype=np.int64)


class MaskDraw:
    """How the kept atoms of one masked batch are chosen: `seed` (device draw) or `keep` (the host's kept lists,
    int32 local indices concatenated in batch order)."""

    def __init__(self, ratio, seed=None, keep=None):
        self.ratio, self.seed, self.keep = ratio, seed, keep
