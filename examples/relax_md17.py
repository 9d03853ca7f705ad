#!/usr/bin/env python3
"""Structure relaxation on a fine-tuned MD17 force field with geossl_amd.relax: bring a batch of structures to a minimum of
the model's own energy surface with FIRE; prints per structure the steps made, the final fmax and the energy drop, and
writes the relaxed structures.

    python examples/relax_md17.py [--model_3d schnet|painn] [--checkpoint FILE.pth] [--data FILE.npz] [--frames 8]
                                  [--fmax 0.05] [--max_steps 2000] [--out relaxed.npz] [--then_md]

The options of examples/simulate_md17.py apply (model, checkpoint, data, masses: see there).  ``--frames``: the first so
many frames of ``--data`` are relaxed as one batch of independent replicas (without ``--data``: copies of one synthetic
21-atom molecule, displaced at random by 0.05 A).  ``--then_md``: the relaxed positions start a ``Simulator`` - thermalize at
``--temperature``, ``--steps`` NVE steps - and the total-energy drift is printed.  Units: kcal/mol, A, fs."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]

from simulate_md17 import file_masses, modules  # noqa: E402
from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset  # noqa: E402
from geossl_amd.md import Simulator  # noqa: E402
from geossl_amd.relax import Minimizer  # noqa: E402


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--model_3d", type=str, default="schnet", choices=["schnet", "painn"])
    p.add_argument("--checkpoint", type=str, default="")
    p.add_argument("--data", type=str, default="")
    p.add_argument("--out", type=str, default="relaxed.npz")
    p.add_argument("--frames", type=int, default=8)
    p.add_argument("--fmax", type=float, default=0.05)
    p.add_argument("--max_steps", type=int, default=2000)
    p.add_argument("--max_step", type=float, default=0.1)
    p.add_argument("--record_every", type=int, default=0)
    p.add_argument("--then_md", action="store_true")
    p.add_argument("--dt", type=float, default=0.5)
    p.add_argument("--temperature", type=float, default=300.0)
    p.add_argument("--steps", type=int, default=10000)
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


def main():
    args = parse()
    torch.manual_seed(args.seed)
    device = torch.device("cuda:%d" % args.device)
    B = max(args.frames, 1)
    if args.data:
        d = np.load(args.data)
        z1 = d["z"].astype(np.int64)
        R = d["R"][:B].astype(np.float32)
        B = len(R)
        masses = file_masses(z1).repeat(B)
    else:
        masses = None   # (the synthetic atom types are indices Z - 1: the default masses)
        from geossl_amd.synthetic import make_batch
        base = make_batch(0, seed=41, sizes=[21])
        z1 = np.clip(base["x"][:, 0], 1, 8)
        rng = np.random.default_rng(args.seed)
        R = (base["positions"][None] + 0.05 * rng.standard_normal((B, 21, 3))).astype(np.float32)
    n = len(z1)
    model, head = modules(args, device)
    ds = DeviceDataset(np.tile(z1, B), R.reshape(B * n, 3), [n] * B, device,
                       radius=args.painn_radius_cutoff if args.model_3d == "painn" else None)
    batch = ds.batch(list(range(B)))
    mz = Minimizer(model, head, batch, model_3d=args.model_3d, masses=masses, fmax=args.fmax, max_step=args.max_step)
    start = mz.run(0)
    t0 = time.time()
    res = mz.run(args.max_steps, record_every=args.record_every)
    torch.cuda.synchronize()
    took = time.time() - t0
    steps = res.steps.cpu().numpy()
    print("relaxed {} structures of {} atoms ({} route): {} steps launched, {:.0f} steps/s".format(
        B, n, "fused" if mz.fused else "torch", int(steps.max()), steps.max() / max(took, 1e-9)))
    for b in range(B):
        print("  structure {}: {} steps, fmax {:.4f} -> {:.4f} kcal/mol/A, energy {:.5f} -> {:.5f} ({:+.5f}){}".format(
            b, int(steps[b]), float(start.fmax[b]), float(res.fmax[b]), float(start.energy[b]), float(res.energy[b]),
            float(res.energy[b] - start.energy[b]), "" if bool(res.converged[b]) else "  NOT converged"))
    out = dict(z=z1, R=res.positions.cpu().numpy().reshape(B, n, 3), R0=R, E=res.energy.cpu().numpy(),
               E0=start.energy.cpu().numpy(), fmax=res.fmax.cpu().numpy(), converged=res.converged.cpu().numpy(), steps=steps)
    if res.history is not None:
        out.update(history_R=res.history.positions.cpu().numpy(), history_E=res.history.energy.cpu().numpy(),
                   history_fmax=res.history.fmax.cpu().numpy(), history_step=res.history.steps.cpu().numpy())
    np.savez(args.out, **out)
    print("wrote", args.out)
    if args.then_md:
        sim = Simulator(model, head, batch, model_3d=args.model_3d, masses=masses, dt=args.dt, seed=args.seed)
        sim.set_positions(res.positions)
        sim.thermalize(args.temperature, generator=torch.Generator().manual_seed(args.seed))
        traj = sim.run(args.steps, record_every=max(args.steps // 100, 1))
        total = (traj.potential.double() + traj.kinetic).sum(1).cpu().numpy()
        ps = args.steps * args.dt * 1e-3
        print("NVE from the relaxed structures, {} steps ({:.2f} ps): total energy drift {:.3e} kcal/mol per atom per ps".format(
            args.steps, ps, (total[-1] - total[0]) / (B * n) / max(ps, 1e-30)))


if __name__ == "__main__":
    main()
