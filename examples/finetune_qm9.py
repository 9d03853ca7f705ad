#!/usr/bin/env python3
"""Property fine-tuning with geossl_amd.pretrain_Supervised: train on one target column, evaluate on the validation and
test splits after every epoch (and on the training split with ``--eval_train``), keep the test MAE of the epoch with the
best validation MAE - on ``SupervisedTrainer`` and a device-resident dataset, with the evaluation passes replayed from
forward-only graphs (``SupervisedTrainer.evaluate``).

    python examples/finetune_qm9.py [--model_3d schnet|painn] [--data FILE.npz] [--task_id 6] [--epochs 100] ...

``--data``: a file with ``x [Ntot]`` (atom types, molecule after molecule), ``positions [Ntot, 3]``, ``sizes [M]`` (atoms
per molecule) and ``y [M, T]`` (targets).  Without it the script runs on synthetic QM9-sized molecules whose targets are
the predictions of a frozen, differently seeded copy of the model, so that there is something to fit."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset, DeviceLoader  # noqa: E402
from geossl_amd.Geom3D.models import PaiNN, SchNet  # noqa: E402
from geossl_amd.optim import cosine_annealing_lr  # noqa: E402
from geossl_amd.pretrain_Supervised import SupervisedTrainer, predict_Supervised  # noqa: E402


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--model_3d", type=str, default="schnet", choices=["schnet", "painn"])
    p.add_argument("--data", type=str, default="")
    p.add_argument("--task_id", type=int, default=0)
    p.add_argument("--loss", type=str, default="mae", choices=["mae", "mse"])
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--epochs", type=int, default=100)
    p.add_argument("--lr", type=float, default=5e-4)
    p.add_argument("--decay", type=float, default=0)
    p.add_argument("--eval_train", action="store_true")
    p.add_argument("--no_graph", action="store_true", help="eager launches for the step and the evaluation")
    p.add_argument("--emb_dim", type=int, default=128)
    p.add_argument("--num_interactions", type=int, default=6)
    p.add_argument("--num_gaussians", type=int, default=51)
    p.add_argument("--cutoff", type=float, default=10)
    p.add_argument("--readout", type=str, default="mean", choices=["mean", "add"])
    p.add_argument("--painn_radius_cutoff", type=float, default=5.0)
    p.add_argument("--painn_n_interactions", type=int, default=3)
    p.add_argument("--painn_n_rbf", type=int, default=20)
    p.add_argument("--molecules", type=int, default=4096, help="synthetic molecules (80 / 10 / 10 split)")
    return p.parse_args()


def modules(args, device):
    if args.model_3d == "schnet":
        model = SchNet(hidden_channels=args.emb_dim, num_filters=args.emb_dim, num_interactions=args.num_interactions,
                       num_gaussians=args.num_gaussians, cutoff=args.cutoff, readout=args.readout, node_class=9)
        head = torch.nn.Linear(args.emb_dim, 1)
    else:
        model = PaiNN(n_atom_basis=args.emb_dim, n_interactions=args.painn_n_interactions, n_rbf=args.painn_n_rbf,
                      cutoff=args.painn_radius_cutoff, max_z=9, n_out=1, readout=args.readout)
        head = model.create_output_layers()
    return model.to(device), head.to(device)


def radius_of(args):
    return args.painn_radius_cutoff if args.model_3d == "painn" else None


def synthetic_records(args, device):
    """Ragged molecules of at most 33 atoms with one target column: what a frozen copy of the model predicts for them."""
    from geossl_amd.synthetic import make_molecules
    mols = make_molecules(args.molecules, seed=args.seed, mode="B")
    torch.manual_seed(args.seed + 1)
    teacher, teacher_head = modules(args, device)
    ds = DeviceDataset.from_numpy(mols, device, radius=radius_of(args))
    y = [predict_Supervised(args, handle, teacher, teacher_head, 0.0, 1.0).cpu().numpy()
         for handle in DeviceLoader(ds, batch_size=args.batch_size, shuffle=False)]
    return mols["x"], mols["positions"], mols["sizes"], np.concatenate(y)[:, None]


def main():
    args = parse()
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    device = torch.device("cuda:%d" % args.device)
    if args.data:
        d = np.load(args.data)
        x, positions, sizes, y = d["x"], d["positions"].astype(np.float32), d["sizes"].astype(np.int64), d["y"]
        y = y.reshape(len(sizes), -1).astype(np.float32)
    else:
        x, positions, sizes, y = synthetic_records(args, device)
        args.task_id = 0
    M = len(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    order = np.random.default_rng(args.seed).permutation(M)
    cut = (0, int(0.8 * M), int(0.9 * M), M)

    def split(k):
        ids = np.sort(order[cut[k]:cut[k + 1]])
        rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in ids])
        return DeviceDataset(x[rows], positions[rows], sizes[ids], device, y=y[ids], radius=radius_of(args))

    train, valid, test = split(0), split(1), split(2)
    column = y[np.sort(order[:cut[1]]), args.task_id]
    mean, std = float(column.mean()), float(column.std())
    train_loader = DeviceLoader(train, batch_size=args.batch_size, shuffle=True, drop_last=True)
    loaders = dict(train=DeviceLoader(train, batch_size=args.batch_size, shuffle=False),
                   valid=DeviceLoader(valid, batch_size=args.batch_size, shuffle=False),
                   test=DeviceLoader(test, batch_size=args.batch_size, shuffle=False))
    torch.manual_seed(args.seed)
    model, head = modules(args, device)
    trainer = SupervisedTrainer(model, head, mean, std, task_id=args.task_id, loss=args.loss, lr=args.lr,
                                weight_decay=args.decay, model_3d=args.model_3d, use_graph=not args.no_graph)
    use_graph = False if args.no_graph else None          # (None: replayed, the measured default)
    best_valid, best_test = float("inf"), float("inf")
    for epoch in range(1, args.epochs + 1):
        t0 = time.time()
        model.train()
        head.train()
        losses = [trainer.step(batch) for batch in train_loader]
        print("Epoch: {}\nLoss: {}".format(epoch, float(torch.stack(losses).mean())))     # (one read per epoch)
        trainer.set_lr(cosine_annealing_lr(args.lr, epoch, args.epochs))
        # the MAE alone, from the sums kept on the device; arrays=True returns (mae, y_true, y_scores) as well
        mae = {k: trainer.evaluate(loader, arrays=False, use_graph=use_graph)
               for k, loader in loaders.items() if k != "train" or args.eval_train}
        if mae["valid"] < best_valid:
            best_valid, best_test = mae["valid"], mae["test"]
        print("\t".join("{}: {:.6f}".format(k, v) for k, v in mae.items()))
        print("best valid: {:.6f}\ttest at it: {:.6f}\ttook {:.2f} s\n".format(best_valid, best_test, time.time() - t0))


if __name__ == "__main__":
    main()
