#!/usr/bin/env python3
"""Molecular dynamics on a fine-tuned MD17 force field with geossl_amd.md: thermalize, equilibrate under a Langevin
thermostat, then a production run at constant energy; prints the total-energy drift and writes the trajectory.

    python examples/simulate_md17.py [--model_3d schnet|painn] [--checkpoint FILE.pth] [--data FILE.npz]
                                     [--temperature 300] [--equilibrate 2000] [--steps 10000] [--out traj.npz]

``--checkpoint``: a file as the fine-tuning script of the reference saves it, ``{"model": state_dict, "graph_pred_linear":
state_dict}``; without it the weights are the seeded initialisation (a force field of no chemical meaning: the run shows
the machinery).  ``--data``: an MD17 file; the first frame of ``R`` and ``z`` give the start.  Its ``z`` are atomic
numbers: they go to the model as the atom types (as examples/finetune_md17.py trains on them), and the masses are
those of the elements (``file_masses``) - not the Simulator's default, which reads an atom type as the reference's index
Z - 1.  Without ``--data``: one synthetic 21-atom molecule whose atom types are such indices.  Units: kcal/mol, A, fs.
The model options are those of examples/finetune_md17.py."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset  # noqa: E402
from geossl_amd.Geom3D.models import PaiNN, SchNet  # noqa: E402
from geossl_amd.md import Simulator  # noqa: E402


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--model_3d", type=str, default="schnet", choices=["schnet", "painn"])
    p.add_argument("--checkpoint", type=str, default="")
    p.add_argument("--data", type=str, default="")
    p.add_argument("--out", type=str, default="trajectory.npz")
    p.add_argument("--dt", type=float, default=0.5)
    p.add_argument("--temperature", type=float, default=300.0)
    p.add_argument("--gamma", type=float, default=0.01)
    p.add_argument("--equilibrate", type=int, default=2000)
    p.add_argument("--steps", type=int, default=10000)
    p.add_argument("--record_every", type=int, default=10)
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
    if args.checkpoint:
        weights = torch.load(args.checkpoint, map_location="cpu")
        model.load_state_dict(weights["model"])
        if "graph_pred_linear" in weights:
            head.load_state_dict(weights["graph_pred_linear"])
    return model.to(device).eval(), head.to(device).eval()


def file_masses(z):
    """Masses in amu of the atomic numbers z of an MD17 file."""
    from geossl_amd.Geom3D.models._atomic_mass import atomic_masses
    table = torch.as_tensor(atomic_masses(), dtype=torch.float64)
    return table[torch.as_tensor(np.asarray(z), dtype=torch.long)]


def main():
    args = parse()
    torch.manual_seed(args.seed)
    device = torch.device("cuda:%d" % args.device)
    if args.data:
        d = np.load(args.data)
        z, R = d["z"].astype(np.int64), d["R"][0].astype(np.float32)
        masses = file_masses(z)
    else:
        masses = None   # (the synthetic atom types are indices Z - 1: the Simulator's default masses)
        from geossl_amd.synthetic import make_batch
        base = make_batch(0, seed=41, sizes=[21])
        z, R = np.clip(base["x"][:, 0], 1, 8), base["positions"]
    n = len(z)
    model, head = modules(args, device)
    ds = DeviceDataset(z, R, [n], device, radius=args.painn_radius_cutoff if args.model_3d == "painn" else None)
    sim = Simulator(model, head, ds.batch([0]), model_3d=args.model_3d, masses=masses, dt=args.dt, seed=args.seed,
                    thermostat=("langevin", args.temperature, args.gamma))
    sim.thermalize(args.temperature, generator=torch.Generator().manual_seed(args.seed))
    t0 = time.time()
    eq = sim.run(args.equilibrate, record_every=max(args.equilibrate, 1))
    print("equilibrated {} steps at {} K: temperature now {:.1f} K".format(args.equilibrate, args.temperature,
                                                                           float(eq.temperature[-1, 0])))
    sim.set_thermostat()                       # production at constant energy
    traj = sim.run(args.steps, record_every=args.record_every)
    total = (traj.potential.double() + traj.kinetic)[:, 0].cpu().numpy()
    took = time.time() - t0
    ps = args.steps * args.dt * 1e-3
    print("production {} steps ({:.2f} ps), {:.0f} steps/s with the equilibration".format(
        args.steps, ps, (args.equilibrate + args.steps) / took))
    print("mean temperature {:.1f} K".format(float(traj.temperature.mean())))
    print("total energy {:.6f} -> {:.6f} kcal/mol: drift {:.3e} kcal/mol per atom per ps (largest excursion {:.3e})".format(
        total[0], total[-1], (total[-1] - total[0]) / n / max(ps, 1e-30), np.abs(total - total[0]).max() / n))
    np.savez(args.out, z=z, R=traj.positions.cpu().numpy(), V=traj.velocities.cpu().numpy(),
             E=traj.potential[:, 0].cpu().numpy(), KE=traj.kinetic[:, 0].cpu().numpy(), step=traj.steps.cpu().numpy(),
             dt=args.dt)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
