#!/usr/bin/env python3
"""Normal-mode analysis on a fine-tuned MD17 force field with geossl_amd.vibrations: the Hessian of the model's own energy
surface at every structure of a batch, harmonic frequencies and normal modes; prints per structure fmax, the number of
imaginary modes, the lowest and highest real frequency and the zero-point energy, and writes an ``.npz``.

    python examples/vibrations_md17.py [--model_3d schnet|painn] [--checkpoint FILE.pth] [--data FILE.npz] [--frames 4]
                                       [--relax_first] [--fmax 0.01] [--delta 0.00125] [--out modes.npz]

The options of examples/simulate_md17.py apply (model, checkpoint, data, masses: see there).  ``--frames``: the first so
many frames of ``--data`` are analysed as one batch (without ``--data``: copies of one synthetic 21-atom molecule, displaced
at random by 0.05 A).  ``--relax_first``: a ``Minimizer`` run to ``--fmax`` first, its positions handed over with
``set_positions`` - frequencies mean something at a stationary point only, and ``fmax`` in the output says how far from one
the analysis was made.  Units: kcal/mol, A, amu; frequencies in cm^-1, imaginary ones negative."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]

from simulate_md17 import file_masses, modules  # noqa: E402
from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset  # noqa: E402
from geossl_amd.relax import Minimizer  # noqa: E402
from geossl_amd.vibrations import DELTA_DEFAULT, NormalModeAnalysis, cartesian_modes, zero_point_energy  # noqa: E402


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--model_3d", type=str, default="schnet", choices=["schnet", "painn"])
    p.add_argument("--checkpoint", type=str, default="")
    p.add_argument("--data", type=str, default="")
    p.add_argument("--out", type=str, default="modes.npz")
    p.add_argument("--frames", type=int, default=4)
    p.add_argument("--relax_first", action="store_true")
    p.add_argument("--fmax", type=float, default=0.01)
    p.add_argument("--max_steps", type=int, default=2000)
    p.add_argument("--delta", type=float, default=DELTA_DEFAULT)
    p.add_argument("--coords_per_pass", type=int, default=0)
    p.add_argument("--project", type=str, default="tr", choices=["tr", "t", "none"])
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
    nm = NormalModeAnalysis(model, head, batch, model_3d=args.model_3d, masses=masses, delta=args.delta,
                            coords_per_pass=args.coords_per_pass or None,
                            project=None if args.project == "none" else args.project)
    if args.relax_first:
        mz = Minimizer(model, head, batch, model_3d=args.model_3d, masses=masses, fmax=args.fmax)
        rel = mz.run(args.max_steps)
        print("relaxed first: up to {} steps, {} of {} converged".format(int(rel.steps.max()), int(rel.converged.sum()), B))
        nm.set_positions(rel.positions)
    t0 = time.time()
    res = nm.run()
    torch.cuda.synchronize()
    took = time.time() - t0
    print("analysed {} structures of {} atoms ({} route, {} coordinates per pass, {} rounds) in {:.3f} s".format(
        B, n, "fused" if nm.fused else "torch", nm.coords_per_pass, nm.rounds, took))
    zpe = zero_point_energy(res).cpu().numpy()
    freq, nproj = res.frequencies.cpu().numpy(), res.n_projected.cpu().numpy()
    for b in range(B):
        f = freq[b, :3 * n]
        rest = np.delete(f, np.argsort(np.abs(f))[:nproj[b]])          # (without the projected ones: the smallest |f|)
        real = rest[rest > 0]
        print("  structure {}: fmax {:.4f} kcal/mol/A, {} imaginary modes, real modes {:.1f} .. {:.1f} cm^-1, zero-point "
              "energy {:.3f} kcal/mol{}".format(b, float(res.fmax[b]), int((rest < 0).sum()),
                                                 real.min() if len(real) else float("nan"),
                                                 real.max() if len(real) else float("nan"), zpe[b],
                                                 "" if bool(res.converged[b]) else "  (eigensolver NOT converged)"))
    m = nm.masses.numpy()
    np.savez(args.out, z=z1, R=nm.positions.cpu().numpy().reshape(B, n, 3), masses=m, hessian=res.hessian.cpu().numpy(),
             eigenvalues=res.eigenvalues.cpu().numpy(), frequencies=freq, modes=res.modes.cpu().numpy(),
             cartesian_modes=cartesian_modes(res, m).cpu().numpy(), n_projected=nproj, asymmetry=res.asymmetry.cpu().numpy(),
             energy=res.energy.cpu().numpy(), fmax=res.fmax.cpu().numpy(), zero_point_energy=zpe)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
