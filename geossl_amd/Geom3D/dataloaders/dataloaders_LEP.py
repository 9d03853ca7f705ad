"""Batch assembly behind the names of the reference's Geom3D/dataloaders/dataloaders_LEP.py: a protein-ligand pair is one
item with its ACTIVE and its INACTIVE conformation side by side (``x_active``, ``positions_active``, ``x_inactive``,
``positions_inactive``, ``y`` and, for PaiNN, ``radius_edge_index_active`` / ``radius_edge_index_inactive``).

``BatchLEP.from_data_list(data_list)`` and ``DataLoaderLEP(dataset, batch_size, shuffle, **kw)`` collate as the
reference does (:11-53, :61-68), so the caller at finetune_lep.py:170-172 runs unchanged.  Beside the reference's
attributes a collated batch keeps the atom counts of both sides on the host (``_sizes_active`` / ``_sizes_inactive``):
the step (geossl_amd/finetune_lep.py) builds its index structures from them and never reads a size back from the device.
"""
import numpy as np
import torch
from torch.utils.data import DataLoader

from .dataloaders_AtomTuple import Data

# The two key lists of :35,37, as the reference spells them: its second list names 'full_edge_index_active' again, so that
# key is shifted by both running counts.  No dataset of the reference sets a full_edge_index_*; kept for the same batches.
_ACTIVE_INDEX_KEYS = ("radius_edge_index_active", "full_edge_index_active")
_INACTIVE_INDEX_KEYS = ("radius_edge_index_inactive", "full_edge_index_active")


class BatchLEP(Data):
    """A collated batch of B pairs with the attributes the loop of examples/finetune_lep.py:31-45 reads."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self._sizes_active = None     # atoms per active / inactive structure (int64 numpy, host)
        self._sizes_inactive = None
        self._num_graphs = None

    @staticmethod
    def from_data_list(data_list):
        """:11-53 - every key of the items concatenated (index keys along the last dimension, shifted by the running
        atom count of their own side), ``batch_active`` / ``batch_inactive`` = the pair index of every atom."""
        keys = [set(data.keys) for data in data_list]
        keys = list(set.union(*keys))
        items = {key: [] for key in keys}
        bvec_active, bvec_inactive = [], []
        cumsum_node_active, cumsum_node_inactive = 0, 0
        for i, data in enumerate(data_list):
            num_nodes_active = data.x_active.size()[0]
            num_nodes_inactive = data.x_inactive.size()[0]
            bvec_active.append(torch.full((num_nodes_active,), i, dtype=torch.long))
            bvec_inactive.append(torch.full((num_nodes_inactive,), i, dtype=torch.long))
            for key in data.keys:
                item = data[key]
                if key in _ACTIVE_INDEX_KEYS:
                    item = item + cumsum_node_active
                if key in _INACTIVE_INDEX_KEYS:
                    item = item + cumsum_node_inactive
                items[key].append(item)
            cumsum_node_active += num_nodes_active
            cumsum_node_inactive += num_nodes_inactive
        out = BatchLEP()
        for key in keys:
            out[key] = torch.cat(items[key], dim=data_list[0].__cat_dim__(key, items[key][0]))
        out.batch_active = torch.cat(bvec_active, dim=-1)
        out.batch_inactive = torch.cat(bvec_inactive, dim=-1)
        # the reference's two asserts (:49-52): a position row that sums to 0 marks a padded / missing atom
        assert (out.positions_active.sum(1) == 0).sum() == 0
        assert (out.positions_inactive.sum(1) == 0).sum() == 0
        out._sizes_active = np.asarray([int(v.numel()) for v in bvec_active], dtype=np.int64)
        out._sizes_inactive = np.asarray([int(v.numel()) for v in bvec_inactive], dtype=np.int64)
        out._num_graphs = len(data_list)
        return out.contiguous()

    def to(self, device, **kw):
        super().to(device, **kw)
        self.__dict__.pop("_geossl_fused", None)   # (the one-pass batch of the step is built from these tensors)
        return self

    @property
    def num_graphs(self):
        """The number of pairs.  (The reference's property, :55-58, reads ``self.batch``, an attribute its class never
        sets, so it cannot be evaluated there; the count below is what it is meant to be.)"""
        if self._num_graphs is None:
            self._num_graphs = self.batch_active[-1].item() + 1
        return self._num_graphs


def _collate(data_list):
    return BatchLEP.from_data_list(data_list)


class DataLoaderLEP(DataLoader):
    """:61-68 - a ``torch.utils.data.DataLoader`` whose collate function is ``BatchLEP.from_data_list``."""

    def __init__(self, dataset, batch_size=1, shuffle=True, **kwargs):
        super().__init__(dataset, batch_size, shuffle, collate_fn=_collate, **kwargs)
