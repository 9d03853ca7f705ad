#!/usr/bin/env python3
"""Molecules/s of the Supervised step (pretrain_Supervised.py / finetune_qm9.py train()) next to the DDM step on the
same molecules and batch size.

    python tools/bench_supervised.py [--models schnet painn] [--bs 128 1024] [--inputs loader ragged] [--steps 50]

Set C molecules (synthetic.make_molecules) with 12 targets each (task_id 6), SchNet at the reference's 10 A cutoff with
its "mean" readout and graph_pred_linear = Linear(128, 1), PaiNN at its defaults (5 A, "add" readout) with
create_output_layers(); L1 loss.  Inputs: "loader" = DatasetBatch handles of a shuffled DeviceLoader over a dataset that
carries y, "ragged" = collated ragged batches (the same molecules collated on the device first, cycled).
One JSON line per configuration and mode:
  "supervised/trainer"    SupervisedTrainer(use_graph=True)
  "supervised/ref_loop"   do_Supervised + loss.backward() + a stock torch.optim.Adam over the reference's two parameter
                          groups (the reference loop, graph replay)
  "supervised/aten_head"  the same loop with the backbone's readout and the reference's ATen head and loss (eager)
  "ddm/graph"             DDMTrainer(use_graph=True), the DDM step
The warm-up makes the captures; "captures_in_timed_region" counts any that fall into the timed window.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
MODES = ("supervised/trainer", "supervised/ref_loop", "supervised/aten_head", "ddm/graph")
TASK = 6


def _model(kind, dev):
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    if kind == "schnet":
        return SchNet(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0,
                      node_class=9, readout="mean").to(dev)
    return PaiNN(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add").to(dev)


def _head(kind, model):
    return torch.nn.Linear(128, 1) if kind == "schnet" else model.create_output_layers()


def run(mode, kind, bs, inputs, steps, warmup, ds, stats, dev="cuda:0"):
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd import pretrain_Supervised as ps
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    from geossl_amd.NCSN import NCSN_version_03
    torch.manual_seed(1234)
    np.random.seed(1234)
    model = _model(kind, dev)
    head = _head(kind, model).to(dev)
    args = types.SimpleNamespace(model_3d=kind, loss="mae")
    mean, std = stats
    if mode == "ddm/graph":
        n1 = NCSN_version_03(128, 10.0, 0.01, 50, "symmetry", 2).to(dev)
        n2 = NCSN_version_03(128, 10.0, 0.01, 50, "symmetry", 2).to(dev)
        tr = pg.DDMTrainer(model, n1, n2, lr=5e-4, mu=0.0, sigma=0.3, device_noise=True, model_3d=kind, use_graph=True)
        step = tr.step
    elif mode == "supervised/trainer":
        tr = ps.SupervisedTrainer(model, head, mean, std, task_id=TASK, loss="mae", lr=5e-4, model_3d=kind,
                                  use_graph=True)
        step = tr.step
    else:
        tr = None
        opt = torch.optim.Adam([{"params": model.parameters(), "lr": 5e-4}, {"params": head.parameters(), "lr": 5e-4}],
                               lr=5e-4)
        crit = torch.nn.L1Loss()

        def fused(b):
            return ps.do_Supervised(args, b, model, head, mean, std, task_id=TASK)

        def aten(b):   # the backbone's readout, then the reference's head and loss lines
            return ps.supervised_step_aten(args, b, model, head, mean, std, TASK, crit)
        fn = fused if mode == "supervised/ref_loop" else aten

        def step(b):
            loss = fn(b)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.detach()
    loader = DeviceLoader(ds, batch_size=bs, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(5))
    if inputs == "ragged":   # collated batches, cycled (a structure comes back every len(pool) steps)
        pool = []
        for _, hb in zip(range(8), loader):
            b = hb.materialize()
            b.y = hb.y   # (the reference's collation of the targets)
            pool.append(b)

        def batches():
            while True:
                yield from pool
    else:
        def batches():
            while True:
                yield from loader
    it = batches()
    for _ in range(warmup):
        step(next(it))
    torch.cuda.synchronize()
    caps = lambda: tr.step_graphs.captures if tr is not None else 0
    caps0 = caps()
    mols = 0
    t0 = time.perf_counter()
    for _ in range(steps):
        b = next(it)
        loss = step(b)
        mols += b.num_graphs
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"mode": mode, "model_3d": kind, "bs": bs, "inputs": inputs, "molecules_per_s": round(mols / dt, 1),
            "ms_per_step": round(1e3 * dt / steps, 4), "steps": steps, "warmup": warmup, "captures": caps(),
            "captures_in_timed_region": caps() - caps0, "final_loss": float(loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["schnet", "painn"])
    ap.add_argument("--bs", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--inputs", nargs="+", default=["ragged", "loader"])
    ap.add_argument("--modes", nargs="+", default=list(MODES))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dataset-mols", type=int, default=12000)
    a = ap.parse_args()
    from geossl_amd import _lib
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    from geossl_amd.synthetic import make_molecules
    _lib.load()
    mols = make_molecules(a.dataset_mols, seed=7, mode="C")
    y = np.random.default_rng(8).standard_normal((a.dataset_mols, 12)).astype(np.float32) * 2.0 - 1.0
    col = torch.from_numpy(y[:, TASK])
    stats = (col.mean().item(), col.std().item())
    for kind in a.models:
        ds = DeviceDataset.from_numpy(mols, "cuda:0", option="permutation", y=y,
                                      **({"radius": 5.0} if kind == "painn" else {}))
        for bs in a.bs:
            for inputs in a.inputs:
                for mode in a.modes:
                    print(json.dumps(run(mode, kind, bs, inputs, a.steps, a.warmup, ds, stats)), flush=True)


if __name__ == "__main__":
    main()
