"""Batch assembly behind the names of the reference's Geom3D/dataloaders/dataloaders_AtomTriple.py (:8-82): the loader
surface of angle prediction on atom triples (examples/pretrain_TorsionAnglePrediction.py).

``AtomTripleExtractor(ratio)(data)`` sets ``data.super_edge_index`` ((3, T) int64, local atom indices): every
``itertools.permutations(range(n), 3)`` in lexicographic order, ``(3, 0)`` for n < 3; for ``ratio < 1`` the columns
``np.random.choice(M, int(M * ratio), replace=False)`` of that list in the drawn order - same global numpy stream, same
call, same triples as the reference.  The n (n - 1) (n - 2) permutations are never listed for a sampled molecule: the
drawn ranks are unranked in closed form (``unrank_triples``; a 255-atom molecule has 16.4 million permutations, of which
the script's ratio 1e-3 keeps 16 386).  ``BatchAtomTriple.from_data_list`` and ``DataLoaderAtomTriple`` are the
reference's collation and loader; every key beside the three index keys is concatenated as it is, so a per-molecule
``super_edge_angle`` rides along.
"""
import numpy as np
import torch
from torch.utils.data import DataLoader

from .dataloaders_AtomTuple import _INDEX_KEYS, Data


def triple_count(n):
    """Ordered triples of distinct atoms of an n-atom molecule: n (n - 1) (n - 2), 0 below three atoms."""
    n = int(n)
    return n * (n - 1) * (n - 2) if n >= 3 else 0


def unrank_triples(n, ranks):
    """Columns `ranks` of ``np.array(list(itertools.permutations(np.arange(n), 3))).T`` -> int64 [3, len(ranks)], without
    the list: rank m = i (n-1)(n-2) + j' (n-2) + k' with j' / k' the positions of j / k among the atoms left."""
    m = np.asarray(ranks, dtype=np.int64).reshape(-1)
    n = int(n)
    if n < 3:
        if m.size:
            raise ValueError("a molecule below three atoms has no triple")
        return np.empty((3, 0), dtype=np.int64)
    i, r = np.divmod(m, (n - 1) * (n - 2))
    jp, k = np.divmod(r, n - 2)
    j = jp + (jp >= i)
    k = k + (k >= np.minimum(i, j))
    k = k + (k >= np.maximum(i, j))
    return np.stack([i, j, k]).astype(np.int64)


class AtomTripleExtractor:
    """``AtomTripleExtractor(ratio=1)`` (:8-31): the per-molecule transform that sets ``data.super_edge_index``."""

    def __init__(self, ratio=1):
        self.ratio = ratio
        return

    def triples(self, n):
        """The triples of an n-atom molecule as int64 numpy [3, T] (one ``np.random.choice`` call for ratio < 1, n >= 3)."""
        M = triple_count(n)
        if M == 0:
            return np.empty((3, 0), dtype=np.int64)
        if self.ratio < 1:
            sampled_M = int(M * self.ratio)
            ranks = np.random.choice(M, sampled_M, replace=False)
        else:
            ranks = np.arange(M, dtype=np.int64)
        return unrank_triples(n, ranks)

    def __call__(self, data):
        N = len(data.x)
        data.super_edge_index = torch.from_numpy(self.triples(N))
        return data


class BatchAtomTriple(Data):
    """A collated batch with the attributes the loop of pretrain_TorsionAnglePrediction.py:64-78 reads (:34-72): ``x``,
    ``positions``, ``batch``, ``super_edge_index`` [3, T], ``super_edge_angle`` [T] [, ``radius_edge_index``],
    ``num_graphs``."""

    def __init__(self, batch=None, **kwargs):
        super().__init__(**kwargs)
        self.batch = batch
        self._sizes = None       # atoms per molecule (host integers) when the collation knows them
        self._triples = False    # super_edge_index holds triples grouped by molecule in batch order (collation's output)
        self._canonical = None   # (sampled lists are not a function of the sizes: no size-keyed step graph)
        self._num_graphs = None

    @staticmethod
    def from_data_list(data_list):
        """:40-67 - concatenate per-molecule ``Data`` objects; the three index keys get the cumulative node offset,
        ``batch = full((n_i,), i)``."""
        keys = [set(data.keys) for data in data_list]
        keys = list(set.union(*keys))
        assert "batch" not in keys
        items = {key: [] for key in keys}
        bvec, sizes = [], []
        cumsum_node = 0
        for i, data in enumerate(data_list):
            num_nodes = data.x.size()[0]
            bvec.append(torch.full((num_nodes,), i, dtype=torch.long))
            for key in data.keys:
                item = data[key]
                if key in _INDEX_KEYS:
                    item = item + cumsum_node
                items[key].append(item)
            cumsum_node += num_nodes
            sizes.append(int(num_nodes))
        out = BatchAtomTriple()
        for key in keys:
            out[key] = torch.cat(items[key], dim=data_list[0].__cat_dim__(key, items[key][0]))
        out.batch = torch.cat(bvec, dim=-1)
        out._sizes = sizes
        out._num_graphs = len(sizes)
        sei = getattr(out, "super_edge_index", None)
        out._triples = sei is not None and sei.dim() == 2 and sei.size(0) == 3
        return out.contiguous()

    def to(self, device, **kw):
        super().to(device, **kw)
        sei = getattr(self, "super_edge_index", None)
        if self._triples and sei is not None and self.batch is not None:
            # collated AtomTripleExtractor output is grouped by molecule in batch order: the step needs no check
            sei._geossl_grouped = (self.batch._version, sei._version)
            if self._sizes is not None and self.batch.is_cuda:
                self.batch._geossl_sizes = ([int(n) for n in self._sizes], self.batch._version)
        return self

    @property
    def num_graphs(self):
        """:69-72"""
        if self._num_graphs is None:
            self._num_graphs = self.batch[-1].item() + 1
        return self._num_graphs


def _collate(data_list):
    return BatchAtomTriple.from_data_list(data_list)


class DataLoaderAtomTriple(DataLoader):
    """:75-82 - a ``torch.utils.data.DataLoader`` whose collate function is ``BatchAtomTriple.from_data_list``."""

    def __init__(self, dataset, batch_size=1, shuffle=True, **kwargs):
        super().__init__(dataset, batch_size, shuffle, collate_fn=_collate, **kwargs)
