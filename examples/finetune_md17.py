#!/usr/bin/env python3
"""MD17 fine-tuning on energies and forces with geossl_amd.finetune_md17: the shape of the reference's
examples/finetune_md17.py (train on 1000 frames, validate on 1000, report the energy and force MAE per epoch, cosine
learning-rate schedule) on ``MD17Trainer`` and a device-resident dataset.

    python examples/finetune_md17.py [--model_3d schnet|painn] [--data FILE.npz] [--epochs 100] ...

``--data``: a trajectory file with the usual MD17 arrays ``z [n]``, ``R [M, n, 3]``, ``E [M]`` (or ``[M, 1]``) and
``F [M, n, 3]``.  Without it the script runs on synthetic frames of one 21-atom molecule with targets drawn from a frozen
copy of the model, so that there is something to fit.  The defaults are those of the reference's config.py."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geossl_amd.finetune_md17 import MD17Trainer  # noqa: E402
from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset, DeviceLoader  # noqa: E402
from geossl_amd.Geom3D.models import PaiNN, SchNet  # noqa: E402
from geossl_amd.optim import cosine_annealing_lr  # noqa: E402


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--model_3d", type=str, default="schnet", choices=["schnet", "painn"])
    p.add_argument("--data", type=str, default="")
    p.add_argument("--md17_energy_coeff", type=float, default=0.05)
    p.add_argument("--md17_force_coeff", type=float, default=0.95)
    p.add_argument("--MD17_train_batch_size", type=int, default=1)
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--epochs", type=int, default=100)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--decay", type=float, default=0)
    p.add_argument("--print_every_epoch", type=int, default=1)
    p.add_argument("--emb_dim", type=int, default=128)
    p.add_argument("--num_filters", type=int, default=128)
    p.add_argument("--num_interactions", type=int, default=6)
    p.add_argument("--num_gaussians", type=int, default=51)
    p.add_argument("--cutoff", type=float, default=10)
    p.add_argument("--readout", type=str, default="mean", choices=["mean", "add"])
    p.add_argument("--painn_radius_cutoff", type=float, default=5.0)
    p.add_argument("--painn_n_interactions", type=int, default=3)
    p.add_argument("--painn_n_rbf", type=int, default=20)
    p.add_argument("--painn_readout", type=str, default="add", choices=["mean", "add"])
    p.add_argument("--train_size", type=int, default=1000)
    p.add_argument("--valid_size", type=int, default=1000)
    return p.parse_args()


def modules(args, device):
    if args.model_3d == "schnet":
        model = SchNet(hidden_channels=args.emb_dim, num_filters=args.num_filters, num_interactions=args.num_interactions,
                       num_gaussians=args.num_gaussians, cutoff=args.cutoff, readout=args.readout, node_class=9)
        head = torch.nn.Linear(args.emb_dim, 1)
    else:
        model = PaiNN(n_atom_basis=args.emb_dim, n_interactions=args.painn_n_interactions, n_rbf=args.painn_n_rbf,
                      cutoff=args.painn_radius_cutoff, max_z=9, n_out=1, readout=args.painn_readout)
        head = model.create_output_layers()
    return model.to(device), head.to(device)


def synthetic_frames(args, device, frames):
    """One synthetic 21-atom molecule moved by 0.05 A of noise per frame; energies and forces of a frozen, differently
    seeded copy of the model."""
    from geossl_amd.finetune_md17 import predict_MD17
    from geossl_amd.synthetic import make_batch
    base = make_batch(0, seed=41, sizes=[21])
    rng = np.random.default_rng(args.seed)
    z = np.clip(base["x"][:, 0], 1, 8)
    R = (base["positions"][None] + 0.05 * rng.standard_normal((frames, 21, 3))).astype(np.float32)
    torch.manual_seed(args.seed + 1)
    teacher, teacher_head = modules(args, device)
    ds = DeviceDataset(np.tile(z, frames), R.reshape(-1, 3), [21] * frames, device,
                       radius=args.painn_radius_cutoff if args.model_3d == "painn" else None)
    E, F = [], []
    for handle in DeviceLoader(ds, batch_size=args.batch_size, shuffle=False):
        e, f = predict_MD17(args, handle, teacher, teacher_head)
        E.append(e.cpu().numpy())
        F.append(f.cpu().numpy().reshape(-1, 21, 3))
    return z, R, np.concatenate(E), np.concatenate(F)


def main():
    args = parse()
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    device = torch.device("cuda:%d" % args.device)
    frames = args.train_size + args.valid_size
    if args.data:
        d = np.load(args.data)
        z, R, E, F = d["z"].astype(np.int64), d["R"].astype(np.float32), d["E"].reshape(-1), d["F"].astype(np.float32)
        order = np.random.default_rng(args.seed).permutation(len(R))[:frames]
        R, E, F = R[order], E[order], F[order]
    else:
        z, R, E, F = synthetic_frames(args, device, frames)
    n = len(z)

    def dataset(lo, hi):
        return DeviceDataset(np.tile(z, hi - lo), R[lo:hi].reshape(-1, 3), [n] * (hi - lo), device, y=E[lo:hi],
                             force=F[lo:hi].reshape(-1, 3),
                             radius=args.painn_radius_cutoff if args.model_3d == "painn" else None)

    train_loader = DeviceLoader(dataset(0, args.train_size), batch_size=args.MD17_train_batch_size, shuffle=True)
    val_loader = DeviceLoader(dataset(args.train_size, frames), batch_size=args.batch_size, shuffle=False)
    torch.manual_seed(args.seed)
    model, head = modules(args, device)
    trainer = MD17Trainer(model, head, model_3d=args.model_3d, lr=args.lr, weight_decay=args.decay,
                          energy_coeff=args.md17_energy_coeff, force_coeff=args.md17_force_coeff)
    best = float("inf")
    for epoch in range(1, args.epochs + 1):
        t0 = time.time()
        model.train()
        head.train()
        losses = [trainer.step(batch) for batch in train_loader]
        loss_acc = float(torch.stack(losses).mean())          # (one read per epoch)
        trainer.set_lr(cosine_annealing_lr(args.lr, epoch, args.epochs))
        print("Epoch: {}\nLoss: {}".format(epoch, loss_acc))
        if epoch % args.print_every_epoch == 0:
            val_energy_mae, val_force_mae = trainer.evaluate(val_loader)
            best = min(best, val_force_mae)
            print("Energy\tval: {:.6f}".format(val_energy_mae))
            print("Force\tval: {:.6f}\tbest: {:.6f}".format(val_force_mae, best))
        print("Took\t{}\n".format(time.time() - t0))


if __name__ == "__main__":
    main()
