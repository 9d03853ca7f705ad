#!/usr/bin/env python3
"""Molecules/s of the RR step (RRTrainer: two AutoEncoder heads on csrc/rr_head.hip) next to the InfoNCE step
(ContrastiveTrainer) on the same molecules: both replayed from capacity-bucket graphs, fed by a shuffled DeviceLoader, the
loader inside the timed region.

    python tools/bench_rr.py [--models schnet painn] [--bs 128 1024] [--runs 3] [--steps 200] [--warmup 20]
                             [--AE_loss l2] [--out profiles/rr_bench.json]

Set C molecules (synthetic.molecule_sizes), SchNet at the reference's 10 A cutoff, PaiNN at its defaults (5 A, radius edges
built once on the device).  Per configuration the two objectives run `--runs` times each, ALTERNATING (RR, InfoNCE, RR,
...), every run a fresh model and trainer; reported: the median ms per step with (min - max) and the ratio of the
medians.  One JSON line per configuration; --out also writes the list to a file.  The head is B x 128 work next to a
backbone over 2B molecules: the expectation is parity within the run-to-run spread.
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


def run(objective, kind, bs, steps, warmup, ds, ae_loss, dev="cuda:0"):
    """One run -> (ms per step, captures inside the timed region, final loss)."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    from geossl_amd.Geom3D.models import AutoEncoder
    torch.manual_seed(1234)
    np.random.seed(1234)
    model = _model(kind, dev)
    if objective == "RR":
        heads = [AutoEncoder(emb_dim=128, loss=ae_loss, detach_target=True, beta=1).to(dev) for _ in range(2)]
        tr = pg.RRTrainer(model, heads[0], heads[1], lr=5e-4, mu=0.0, sigma=0.3, model_3d=kind, device_noise=True,
                          use_graph=True)
    else:
        tr = pg.ContrastiveTrainer(model, option="InfoNCE", lr=5e-4, mu=0.0, sigma=0.3, T=0.1, model_3d=kind,
                                   device_noise=True, use_graph=True)
    loader = DeviceLoader(ds, batch_size=bs, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(5))

    def batches():
        while True:
            yield from loader
    it = batches()
    for _ in range(warmup):
        tr.step(next(it))
    torch.cuda.synchronize()
    caps0 = tr.step_graphs.captures
    t0 = time.perf_counter()
    for _ in range(steps):
        out = tr.step(next(it))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    loss = out[0] if isinstance(out, tuple) else out
    return 1e3 * dt / steps, tr.step_graphs.captures - caps0, float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["schnet", "painn"])
    ap.add_argument("--bs", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--AE_loss", type=str, default="l2", choices=["l1", "l2", "cosine"])
    ap.add_argument("--dataset-mols", type=int, default=12000)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    from geossl_amd import _lib
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    from geossl_amd.synthetic import add_bonds, make_molecules
    _lib.load()
    mols = add_bonds(make_molecules(a.dataset_mols, seed=7, mode="C"), seed=7)
    results = []
    for kind in a.models:
        ds = DeviceDataset.from_numpy(mols, "cuda:0", **({"radius": 5.0} if kind == "painn" else {}))
        for bs in a.bs:
            ms = {"RR": [], "InfoNCE": []}
            late = {"RR": 0, "InfoNCE": 0}
            for _ in range(a.runs):
                for objective in ("RR", "InfoNCE"):   # alternating: a drift of the clock meets both alike
                    t, caps, loss = run(objective, kind, bs, a.steps, a.warmup, ds, a.AE_loss)
                    assert np.isfinite(loss), (objective, loss)
                    ms[objective].append(t)
                    late[objective] += caps
            line = {"model_3d": kind, "bs": bs, "AE_loss": a.AE_loss, "runs": a.runs, "steps": a.steps, "warmup": a.warmup}
            for objective, v in ms.items():
                med = statistics.median(v)
                line[objective] = {"ms_per_step_median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4),
                                   "molecules_per_s": round(1e3 * bs / med, 1),
                                   "captures_in_timed_region": late[objective]}
            line["RR_over_InfoNCE"] = round(line["RR"]["ms_per_step_median"] / line["InfoNCE"]["ms_per_step_median"], 4)
            results.append(line)
            print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
