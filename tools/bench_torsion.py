#!/usr/bin/env python3
"""Molecules/s of the angle-prediction step (atom triples) next to the Distance Prediction step on the same molecules.

    python tools/bench_torsion.py [--models schnet painn] [--bs 128 1024] [--steps 100] [--reps 3] [--ratio 1e-3]

Set C molecules with hydrogens (synthetic.make_molecules), SchNet at the reference's 10 A cutoff, PaiNN at its defaults
(5 A); both trainers from DatasetBatch handles of a shuffled DeviceLoader: TorsionAnglePredictionTrainer(use_graph=True)
over a triple dataset sampled at `ratio` (the script's 1e-3), DistancePredictionTrainer(use_graph=True) over the
"permutation" super-edges of the same molecules.  One process: both trainers are warmed up first (every capture happens
there), then device-synchronised windows of `steps` steps alternate between the two lines, `reps` times; the medians are
compared.  The two steps share the one-view backbone; the acceptance line is torsion >= 0.95 x distance.
One JSON line per (model, batch size): both medians, every window, the ratio, the captures that fell into timed windows
(0 expected) and the C-ABI calls the host makes for one replayed torsion step (the refresh of the graph's inputs and
the fused Adam; the step itself is one graph launch on top).  The kernels behind a line come from a trace of its own:
rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_torsion.py --bs 128 --models schnet --reps 1
"""
import argparse
import json
import os
import statistics
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


def _forever(loader):
    while True:
        yield from loader


def run(kind, bs, steps, warmup, reps, ds_tor, ds_dist, dev="cuda:0"):
    from geossl_amd import _lib
    from geossl_amd import pretrain_DistancePrediction as pd
    from geossl_amd import pretrain_TorsionAnglePrediction as pt
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    torch.manual_seed(1234)
    lines = {}
    for name, ds, make in (("torsion", ds_tor, lambda m: pt.TorsionAnglePredictionTrainer(
                                m, pt.TorsionAnglePredictor(128).to(dev), lr=5e-4, model_3d=kind, use_graph=True)),
                           ("distance", ds_dist, lambda m: pd.DistancePredictionTrainer(
                               m, pd.DistancePredictor(128).to(dev), lr=5e-4, model_3d=kind, use_graph=True))):
        tr = make(_model(kind, dev))
        it = _forever(DeviceLoader(ds, batch_size=bs, shuffle=True, drop_last=True,
                                   generator=torch.Generator().manual_seed(5)))
        lines[name] = (tr, it)
    for tr, it in lines.values():   # warm-up of every shape: the captures (and any recapture at a larger capacity)
        for _ in range(warmup):
            tr.step(next(it))
    torch.cuda.synchronize()
    caps0 = {k: tr.step_graphs.captures for k, (tr, _) in lines.items()}
    windows = {k: [] for k in lines}
    for _ in range(reps):
        for name, (tr, it) in lines.items():   # alternating: drift of the machine lands on both lines
            torch.cuda.synchronize()
            mols = 0
            t0 = time.perf_counter()
            for _ in range(steps):
                b = next(it)
                loss = tr.step(b)
                mols += b.num_graphs
            torch.cuda.synchronize()
            windows[name].append(round(mols / (time.perf_counter() - t0), 1))
    tr, it = lines["torsion"]
    _lib.CALLS = 0
    tr.step(next(it))
    calls, _lib.CALLS = _lib.CALLS, None
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in windows.items()}
    (g,) = tr.step_graphs.graphs.values()
    return {"model_3d": kind, "bs": bs, "torsion_molecules_per_s": med["torsion"],
            "distance_molecules_per_s": med["distance"], "ratio": round(med["torsion"] / med["distance"], 4),
            "windows": windows, "steps_per_window": steps, "warmup": warmup,
            "captures_in_timed_region": {k: lines[k][0].step_graphs.captures - caps0[k] for k in lines},
            "abi_calls_per_replayed_torsion_step": calls, "graph_launches_per_step": 1,
            "bucket": {"T_cap": g["bucket"].T_cap, "N_cap": g["bucket"].N_cap},
            "triples_per_molecule": round(float(ds_tor.triple_cnt.mean()), 2), "final_loss": float(loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["schnet", "painn"])
    ap.add_argument("--bs", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=1e-3)
    ap.add_argument("--dataset-mols", type=int, default=12000)
    a = ap.parse_args()
    from geossl_amd import _lib
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    from geossl_amd.synthetic import make_molecules
    _lib.load()
    mols = make_molecules(a.dataset_mols, seed=7, mode="C")
    for kind in a.models:
        kw = {"radius": 5.0} if kind == "painn" else {}
        np.random.seed(1234)
        ds_tor = DeviceDataset.from_numpy(mols, "cuda:0", **kw).sample_triples(a.ratio)
        ds_dist = DeviceDataset.from_numpy(mols, "cuda:0", option="permutation", **kw)
        for bs in a.bs:
            print(json.dumps(run(kind, bs, a.steps, a.warmup, a.reps, ds_tor, ds_dist)), flush=True)


if __name__ == "__main__":
    main()
