#!/usr/bin/env python3
"""Distance Prediction pretraining with geossl_amd.pretrain_DistancePrediction on a device-resident dataset: every step
gathers its molecules on the device and replays one capacity-bucket graph per batch size.

    python examples/pretrain_DistancePrediction.py [--model_3d schnet|painn] [--data FILE.npz] [--epochs 100]
                                                   [--distance_sample_ratio 1] ...

``--distance_sample_ratio r`` (the reference's flag, AtomTupleExtractor(ratio=r)): r < 1 keeps int(M * r) of every
molecule's M atom pairs, drawn on the device behind the gather (``DeviceLoader(tuple_ratio=r)``; ``--tuple_rng numpy``
makes the reference's own np.random.choice draws on the host instead).  ``--data``: a file with ``x [Ntot]`` or
``[Ntot, C]`` (atom types, molecule after molecule), ``positions [Ntot, 3]`` and ``sizes [M]``; without it the script runs
on synthetic molecules with hydrogens."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset, DeviceLoader  # noqa: E402
from geossl_amd.Geom3D.models import PaiNN, SchNet  # noqa: E402
from geossl_amd.pretrain_DistancePrediction import DistancePredictionTrainer, DistancePredictor  # noqa: E402


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--model_3d", type=str, default="schnet", choices=["schnet", "painn"])
    p.add_argument("--data", type=str, default="")
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--epochs", type=int, default=100)
    p.add_argument("--lr", type=float, default=5e-4)
    p.add_argument("--decay", type=float, default=0)
    p.add_argument("--distance_sample_ratio", type=float, default=1)
    p.add_argument("--tuple_rng", type=str, default="device", choices=["device", "numpy"])
    p.add_argument("--no_graph", action="store_true", help="eager launches for the step")
    p.add_argument("--emb_dim", type=int, default=128)
    p.add_argument("--num_interactions", type=int, default=6)
    p.add_argument("--num_gaussians", type=int, default=51)
    p.add_argument("--cutoff", type=float, default=10)
    p.add_argument("--readout", type=str, default="mean", choices=["mean", "add"])
    p.add_argument("--painn_radius_cutoff", type=float, default=5.0)
    p.add_argument("--painn_n_interactions", type=int, default=3)
    p.add_argument("--painn_n_rbf", type=int, default=20)
    p.add_argument("--molecules", type=int, default=4096, help="synthetic molecules")
    return p.parse_args()


def main():
    args = parse()
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    device = torch.device("cuda:%d" % args.device)
    if args.data:
        d = np.load(args.data)
        mols = {"x": d["x"], "positions": d["positions"].astype(np.float32), "sizes": d["sizes"].astype(np.int64)}
    else:
        from geossl_amd.synthetic import make_molecules
        mols = make_molecules(args.molecules, seed=args.seed, mode="C")
    painn = args.model_3d == "painn"
    ds = DeviceDataset.from_numpy(mols, device, option="permutation",
                                  radius=args.painn_radius_cutoff if painn else None)
    loader = DeviceLoader(ds, batch_size=args.batch_size, shuffle=True, drop_last=True,
                          tuple_ratio=args.distance_sample_ratio, tuple_rng=args.tuple_rng)
    if painn:
        model = PaiNN(n_atom_basis=args.emb_dim, n_interactions=args.painn_n_interactions, n_rbf=args.painn_n_rbf,
                      cutoff=args.painn_radius_cutoff, max_z=9, n_out=1, readout=args.readout)
    else:
        model = SchNet(hidden_channels=args.emb_dim, num_filters=args.emb_dim, num_interactions=args.num_interactions,
                       num_gaussians=args.num_gaussians, cutoff=args.cutoff, readout=args.readout, node_class=9)
    predictor = DistancePredictor(args.emb_dim)
    trainer = DistancePredictionTrainer(model.to(device), predictor.to(device), lr=args.lr, weight_decay=args.decay,
                                        model_3d=args.model_3d, use_graph=not args.no_graph)
    for epoch in range(1, args.epochs + 1):
        t0 = time.time()
        losses = [trainer.step(batch) for batch in loader]
        print("Epoch: {}\nLoss: {:.6f}\ttook {:.2f} s".format(epoch, float(torch.stack(losses).mean()), time.time() - t0))


if __name__ == "__main__":
    main()
