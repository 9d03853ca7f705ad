#!/usr/bin/env python3
"""Molecules/s of the SchNet DDM step (DDMTrainer, bucket replay, device noise) fed by a DeviceLoader, unmasked and with
BFS atom masking (the reference's default --GeoSSL_atom_masking_ratio 0.3, device draw), at the same batch size.

    python tools/bench_masked_loader.py [--model schnet|painn] [--bs 128 1024] [--ratios 0 0.3] [--steps 60] [--warmup 10]

Set C molecules (Molecule3D with hydrogens, synthetic.molecule_sizes) with a bond graph (synthetic.add_bonds), SchNet
at the reference's 10 A cutoff.  One JSON line per (batch size, ratio).  The cost of the masked gather itself comes
from a kernel trace of the same run, e.g.  rocprofv3 --kernel-trace --stats -d <dir> -- python
tools/bench_masked_loader.py --bs 128 --ratios 0.3  (k_gather_masked in the stats file).

--model painn: the same loader over a dataset with radius edges (5 A) and PaiNN with 3 interactions, 20 radial functions,
cutoff 5 A; its lines carry "model": "painn".  A masked PaiNN handle takes the capacity bucket (four fill launches:
k_gather_masked twice, k_masked_edge_offsets, k_painn_edge_layout) unless GEOSSL_MASKED_PAINN_BUCKETS=0, which collates
it with a read-back of its edge counts - the A/B of DESIGN 3.2.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def run(bs, ratio, steps, warmup, dataset_mols, dev="cuda:0", model_3d="schnet"):
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    from geossl_amd.Geom3D.models import SchNet
    from geossl_amd.NCSN import NCSN_version_03
    from geossl_amd.synthetic import add_bonds, make_molecules
    torch.manual_seed(1234)
    np.random.seed(1234)
    mols = add_bonds(make_molecules(dataset_mols, seed=7, mode="C"), seed=7)
    if model_3d == "painn":
        from geossl_amd.Geom3D.models import PaiNN
        ds = DeviceDataset.from_numpy(mols, dev, radius=5.0)
        model = PaiNN(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add").to(dev)
    else:
        ds = DeviceDataset.from_numpy(mols, dev)
        model = SchNet(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0,
                       node_class=9, readout="mean").to(dev)
    n1 = NCSN_version_03(128, 10.0, 0.01, 50, "symmetry", 2).to(dev)
    n2 = NCSN_version_03(128, 10.0, 0.01, 50, "symmetry", 2).to(dev)
    tr = pg.DDMTrainer(model, n1, n2, lr=5e-4, mu=0.0, sigma=0.3, device_noise=True, model_3d=model_3d, use_graph=True)
    loader = DeviceLoader(ds, batch_size=bs, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(5),
                          mask_ratio=ratio)

    def batches():
        while True:
            yield from loader
    it = batches()
    for _ in range(warmup):
        tr.step(next(it))
    torch.cuda.synchronize()
    mol_count, atoms = 0, 0
    t0 = time.perf_counter()
    for _ in range(steps):
        hb = next(it)
        loss = tr.step(hb)
        mol_count += hb.num_graphs
        atoms += hb.n_atoms
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"bs": bs, "mask_ratio": ratio, "molecules_per_s": round(mol_count / dt, 1), "ms_per_step": round(1e3 * dt / steps, 4),
            "atoms_per_molecule": round(atoms / mol_count, 2), "steps": steps, "warmup": warmup,
            "captures": tr.step_graphs.captures, "final_loss": float(loss)}
    if model_3d != "schnet":
        out = dict({"model": model_3d}, **out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["schnet", "painn"], default="schnet")
    ap.add_argument("--bs", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--ratios", type=float, nargs="+", default=[0.0, 0.3])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dataset-mols", type=int, default=20000)
    a = ap.parse_args()
    from geossl_amd import _lib
    _lib.load()
    for bs in a.bs:
        for r in a.ratios:
            print(json.dumps(run(bs, r, a.steps, a.warmup, a.dataset_mols, model_3d=a.model)), flush=True)


if __name__ == "__main__":
    main()
