#!/usr/bin/env python3
"""Molecules/s of the contrastive steps (ContrastiveTrainer: InfoNCE, EBM-NCE) fed by a shuffled DeviceLoader, with and
without HIP-graph replay, next to the DDM step (DDMTrainer, graph replay) on the same molecules, batch size and masking.

    python tools/bench_contrastive.py [--options InfoNCE EBM_NCE] [--models schnet painn] [--bs 128 1024]
                                      [--ratios 0 0.3] [--steps 30] [--warmup 5]

Set C molecules (synthetic.molecule_sizes, with a bond graph for the masking), SchNet at the reference's 10 A cutoff,
PaiNN at its defaults (5 A, radius edges built once on the device).  One JSON line per configuration and mode:
"contrastive/graph" (use_graph=True: the ragged batches of the shuffled loader share capacity-bucket graphs, gathered on
the device), "contrastive/eager" and "ddm/graph" (the DDM twin, same buckets).  The warm-up makes the captures; a
capture that still falls into the timed window (a batch that outgrows its bucket) is reported in
"captures_in_timed_region".  --modes restricts the run to some of the three (one trace per mode).
The kernels behind a line come from a trace of the same run, e.g.  rocprofv3 --kernel-trace --stats -d <dir> -- python
tools/bench_contrastive.py --bs 128 --models schnet --ratios 0
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


def _model(kind, dev):
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    if kind == "schnet":
        return SchNet(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0,
                      node_class=9, readout="mean").to(dev)
    return PaiNN(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add").to(dev)


def run(mode, option, kind, bs, ratio, steps, warmup, ds, dev="cuda:0"):
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    from geossl_amd.NCSN import NCSN_version_03
    torch.manual_seed(1234)
    np.random.seed(1234)
    model = _model(kind, dev)
    if mode == "ddm/graph":
        n1 = NCSN_version_03(128, 10.0, 0.01, 50, "symmetry", 2).to(dev)
        n2 = NCSN_version_03(128, 10.0, 0.01, 50, "symmetry", 2).to(dev)
        tr = pg.DDMTrainer(model, n1, n2, lr=5e-4, mu=0.0, sigma=0.3, device_noise=True, model_3d=kind, use_graph=True)
    else:
        tr = pg.ContrastiveTrainer(model, option=option, lr=5e-4, mu=0.0, sigma=0.3, T=0.1, num_neg=1, model_3d=kind,
                                   device_noise=True, use_graph=mode == "contrastive/graph")
    loader = DeviceLoader(ds, batch_size=bs, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(5),
                          mask_ratio=ratio)

    def batches():
        while True:
            yield from loader
    it = batches()
    for _ in range(warmup):
        tr.step(next(it))
    torch.cuda.synchronize()
    caps0 = tr.step_graphs.captures
    mols = 0
    t0 = time.perf_counter()
    for _ in range(steps):
        hb = next(it)
        out = tr.step(hb)
        mols += hb.num_graphs
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    loss = out[0] if isinstance(out, tuple) else out
    return {"mode": mode, "option": option if mode != "ddm/graph" else "DDM", "model_3d": kind, "bs": bs,
            "mask_ratio": ratio, "molecules_per_s": round(mols / dt, 1), "ms_per_step": round(1e3 * dt / steps, 4),
            "steps": steps, "warmup": warmup, "captures": tr.step_graphs.captures,
            "captures_in_timed_region": tr.step_graphs.captures - caps0, "final_loss": float(loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--options", nargs="+", default=["InfoNCE", "EBM_NCE"])
    ap.add_argument("--models", nargs="+", default=["schnet", "painn"])
    ap.add_argument("--bs", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--ratios", type=float, nargs="+", default=[0.0, 0.3])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--modes", nargs="+", default=["contrastive/graph", "contrastive/eager", "ddm/graph"])
    ap.add_argument("--dataset-mols", type=int, default=12000)
    ap.add_argument("--no-ddm", action="store_true", help="skip the DDM twins")
    a = ap.parse_args()
    from geossl_amd import _lib
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    from geossl_amd.synthetic import add_bonds, make_molecules
    _lib.load()
    mols = add_bonds(make_molecules(a.dataset_mols, seed=7, mode="C"), seed=7)
    for kind in a.models:
        ds = DeviceDataset.from_numpy(mols, "cuda:0", **({"radius": 5.0} if kind == "painn" else {}))
        for bs in a.bs:
            for r in a.ratios:
                modes = [(m, o) for o in a.options for m in ("contrastive/graph", "contrastive/eager") if m in a.modes]
                if not a.no_ddm and "ddm/graph" in a.modes:
                    modes.append(("ddm/graph", None))
                for mode, option in modes:
                    print(json.dumps(run(mode, option, kind, bs, r, a.steps, a.warmup, ds)), flush=True)


if __name__ == "__main__":
    main()
