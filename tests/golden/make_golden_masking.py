#!/usr/bin/env python3
"""Generate fixture G16 (atom masking) by running the UNMODIFIED reference on CPU.

Run in the build container only:  python tests/golden/make_golden_masking.py
Molecule3DDataset.subgraph (Geom3D/datasets/datasets_3D.py:24-67) and MoleculeDataset3DRadius.subgraph
(datasets_3D_Radius.py:43-87) are loaded from their files and called on instances made without __init__ (no dataset on
disk), with mask_ratio set; the masked records then go through the reference's AtomTupleExtractor and
BatchAtomTuple.from_data_list (Geom3D/dataloaders/dataloaders_AtomTuple.py).  The third-party names those files import
and the shims of make_golden.py lack - InMemoryDataset, torch_geometric.utils.{subgraph, to_networkx} and a Data with
``__contains__`` - are defined below (networkx builds the graph, as in torch_geometric).

For np.random.seed(s), r in {0.3, 0.5}: the molecules are masked in dataset order (what a loader without shuffling
fetches); stored: the kept local atoms, the collated masked batch (x, positions, batch, super_edge_index of both
options, radius_edge_index at 5 A) and the inputs (molecules, bond graph, unmasked radius edges).  Output: tests/golden/g16_masking.npz.
"""
import importlib.util
import os
import sys
import types

import networkx as nx
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path[:0] = [os.path.join(HERE, "ref_shims"), REF, REPO]

import torch_geometric.data as tg_data  # noqa: E402  (shim)
from torch_geometric.nn import radius_graph  # noqa: E402  (shim)

from geossl_amd.synthetic import add_bonds, make_molecules  # noqa: E402

SEEDS = (0, 7)
RATIOS = (0.3, 0.5)
RADIUS = 5.0


class Data(tg_data.Data):
    def __contains__(self, key):
        return getattr(self, key, None) is not None


class InMemoryDataset:
    pass


def to_networkx(data):
    G = nx.DiGraph()
    G.add_nodes_from(range(data.x.size(0)))
    for u, v in data.edge_index.t().tolist():
        G.add_edge(u, v)
    return G


def subgraph(subset, edge_index, edge_attr=None, relabel_nodes=False, num_nodes=None):
    subset = torch.as_tensor(np.asarray(subset, dtype=np.int64))
    mask = torch.zeros(num_nodes, dtype=torch.bool)
    mask[subset] = True
    keep = mask[edge_index[0]] & mask[edge_index[1]]
    edge_index = edge_index[:, keep]
    edge_attr = edge_attr[keep] if edge_attr is not None else None
    if relabel_nodes:
        idx = torch.full((num_nodes,), -1, dtype=torch.long)
        idx[subset] = torch.arange(subset.numel())
        edge_index = idx[edge_index]
    return edge_index, edge_attr


tg_data.InMemoryDataset = InMemoryDataset
tg_data.Data = Data
utils = types.ModuleType("torch_geometric.utils")
utils.subgraph, utils.to_networkx = subgraph, to_networkx
sys.modules["torch_geometric.utils"] = utils
sys.modules["torch_geometric"].utils = utils


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def molecules():
    """~40 molecules with bonds: one- and two-atom molecules, isolated atoms and several components among them."""
    sizes = [1, 2, 3, 1, 5, 9, 14, 18, 23, 2, 30, 41, 7, 12, 1, 26, 33, 19, 4, 6]
    sizes += np.clip(np.rint(np.random.default_rng(16).normal(26.0, 10.0, size=20)), 4, 72).astype(int).tolist()
    return add_bonds(make_molecules(0, seed=16, sizes=sizes), seed=16, cut=0.5)


def main():
    d3 = load("ref_datasets_3D", "Geom3D/datasets/datasets_3D.py")
    d3r = load("ref_datasets_3D_Radius", "Geom3D/datasets/datasets_3D_Radius.py")
    from Geom3D.dataloaders.dataloaders_AtomTuple import AtomTupleExtractor, BatchAtomTuple
    mols = molecules()
    sizes, boff = mols["sizes"], np.concatenate([[0], np.cumsum(mols["bond_counts"])])
    off = np.concatenate([[0], np.cumsum(sizes)])
    out = {k: mols[k] for k in ("x", "positions", "sizes", "bond_index", "bond_counts")}
    out["radius"] = np.float32(RADIUS)
    whole = [radius_graph(torch.from_numpy(mols["positions"][off[m]:off[m + 1]]), r=RADIUS, loop=False)
             for m in range(len(sizes))]
    out["rei_src"] = torch.cat(whole, dim=1).numpy()   # radius edges of the whole molecules, local indices
    out["rei_cnt"] = np.asarray([e.size(1) for e in whole], dtype=np.int64)

    def record(m):
        a, b = off[m], off[m + 1]
        x = torch.from_numpy(mols["x"][a:b]).clone()
        x = torch.cat([x, torch.arange(b - a, dtype=torch.long)[:, None]], dim=1)   # (a third column: the local atom id)
        pos = torch.from_numpy(mols["positions"][a:b]).clone()
        d = Data(x=x, positions=pos, edge_index=torch.from_numpy(mols["bond_index"][:, boff[m]:boff[m + 1]]).clone(),
                 edge_attr=None)
        d.radius_edge_index = radius_graph(pos, r=RADIUS, loop=False)
        return d

    for r in RATIOS:
        for s in SEEDS:
            tag = "r%g_s%d" % (r, s)
            plain, radius = d3.Molecule3DDataset.__new__(d3.Molecule3DDataset), \
                d3r.MoleculeDataset3DRadius.__new__(d3r.MoleculeDataset3DRadius)
            plain.mask_ratio = radius.mask_ratio = r
            np.random.seed(s)
            masked = [plain.subgraph(record(m)) for m in range(len(sizes))]
            np.random.seed(s)
            masked_r = [radius.subgraph(record(m)) for m in range(len(sizes))]
            keep = [d.x[:, 2].clone() for d in masked]
            for d, dr, kk in zip(masked, masked_r, keep):
                assert torch.equal(dr.x[:, 2], kk) and torch.equal(dr.positions, d.positions)
                d.radius_edge_index = dr.radius_edge_index
                d.x = d.x[:, :2].contiguous()
                del d.edge_index, d.edge_attr, d.__num_nodes__
            out["keep/" + tag] = torch.cat(keep).numpy().astype(np.int32)
            out["kept/" + tag] = np.asarray([k.numel() for k in keep], dtype=np.int64)
            for option in ("combination", "permutation"):
                ext = AtomTupleExtractor(ratio=1, option=option)
                bt = BatchAtomTuple.from_data_list([ext(Data(**{k: v for k, v in vars(d).items()})) for d in masked])
                key = "%s/%s" % (tag, option)
                out["sei/" + key] = bt.super_edge_index.numpy()
                if option == "combination":
                    out["x/" + tag], out["positions/" + tag] = bt.x.numpy(), bt.positions.numpy()
                    out["batch/" + tag], out["rei/" + tag] = bt.batch.numpy(), bt.radius_edge_index.numpy()
    path = os.path.join(HERE, "g16_masking.npz")
    np.savez_compressed(path, **out)
    print("wrote g16_masking.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
