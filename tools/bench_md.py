#!/usr/bin/env python3
"""Molecular dynamics on a force field: steps per second of ``geossl_amd.md.Simulator`` next to the loop a user had
before it, and the NVE energy drift of the fp32 run next to the fp64 twin's.

    python tools/bench_md.py [--kinds schnet painn] [--replicas 1 64 1024] [--record-every 1 100] [--spr 1 4 16]
                             [--steps 200] [--runs 3] [--drift-steps 2000] [--out profiles/md_bench.json]

Workload: B replicas of ONE 21-atom molecule (a make_batch molecule) at the reference's MD17 configuration (SchNet 128 /
6 blocks / 51 gaussians / 10 A / mean with Linear(128, 1); PaiNN 128 / 3 blocks / 20 radial functions / 5 A / add with
its output layers), 300 K velocities, NVE at 0.5 fs.  Routes, per shape (kind, B, record_every):

* ``baseline``: the loop a user writes on ``predict_MD17(use_graph=True)`` - kick, drift, predict, kick in torch
  operations, a ``clone()`` of positions and velocities per recorded frame.  That code is unchanged by md.py, so its
  timing here is the parent commit's;
* ``eager``: ``Simulator(use_graph=False)``;
* ``replay@U``: ``Simulator(steps_per_replay=U)``.

A timed run is ``--steps`` MD steps between two device synchronises, after one untimed run of the same kind (captures
included there); every route of a shape is timed once per round, ``--runs`` rounds, so the routes alternate; reported
as steps per second, median (min - max).  Decision rules, evaluated per shape and printed: the default
``steps_per_replay`` is the smallest U whose median lies within the min - max spread of the best U; ``use_graph``
stays True only where the slowest replayed run beats the fastest baseline run.

Drift (reported, not asserted): ``--drift-steps`` NVE steps at 0.5 fs of one molecule from 300 K - the total energy's
change per atom per ps for the GPU run and for the fp64 twin (tests/md_twin.py on tests/force_twin.py) from the same
start.  Needs the GPU.  Prints one JSON document; --out also writes it."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

N_ATOMS, DEV, DT, T0 = 21, "cuda:0", 0.5, 300.0
SCHNET = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0, readout="mean",
              node_class=9)
PAINN = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")


def modules(kind):
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    torch.manual_seed(1234)
    if kind == "schnet":
        return SchNet(**SCHNET).to(DEV), torch.nn.Linear(128, 1).to(DEV)
    model = PaiNN(**PAINN).to(DEV)
    return model, model.create_output_layers().to(DEV)


def replicas(kind, B):
    """B copies of one molecule as the collated batch of the MD17 loaders (1-D x, host sizes; PaiNN with radius edges)."""
    from geossl_amd import ops, pretrain_GeoSSL as pg
    from geossl_amd.synthetic import make_batch
    base = make_batch(0, seed=41, sizes=[N_ATOMS])
    raw = make_batch(0, seed=41, sizes=[N_ATOMS] * B)   # (the index structures of B molecules; atoms and positions below)
    raw["x"] = np.tile(np.clip(base["x"][:, 0], 1, 8), B)
    raw["positions"] = np.tile(base["positions"], (B, 1))
    bt = pg.Batch.from_numpy(raw, DEV)
    if kind == "painn":
        bt.radius_edge_index = ops.radius_graph(bt.positions, PAINN["cutoff"], bt.batch)
    return bt, raw


def start_velocities(sim):
    sim.thermalize(T0, generator=torch.Generator().manual_seed(7))
    return sim.velocities.clone()


class Baseline:
    """Velocity Verlet around predict_MD17 in torch operations: what a user wrote before md.py."""

    def __init__(self, kind, model, head, bt, masses, v0):
        from geossl_amd.md import ACCEL
        self.args, self.model, self.head, self.bt = types.SimpleNamespace(model_3d=kind), model, head, bt
        self.cinv = (ACCEL / masses).float().to(DEV)[:, None]
        self.v = v0.clone()

    def run(self, steps, every):
        from geossl_amd.finetune_md17 import predict_MD17
        bt, v, cinv, hdt = self.bt, self.v, self.cinv, 0.5 * DT
        energy, force = predict_MD17(self.args, bt, self.model, self.head, use_graph=True)
        frames = [(bt.positions.clone(), v.clone(), energy)]
        for k in range(1, steps + 1):
            v.add_(force * cinv, alpha=hdt)
            bt.positions.add_(v, alpha=DT)
            energy, force = predict_MD17(self.args, bt, self.model, self.head, use_graph=True)
            v.add_(force * cinv, alpha=hdt)
            if k % every == 0:
                frames.append((bt.positions.clone(), v.clone(), energy))
        return frames


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def summary(rates):
    return dict(steps_per_s=[round(r, 1) for r in rates], median=round(statistics.median(rates), 1),
                min_max=[round(min(rates), 1), round(max(rates), 1)])


def throughput(a):
    from geossl_amd.md import Simulator
    lines, decisions = [], []
    for kind in a.kinds:
        for B in a.replicas:
            for every in a.record_every:
                model, head = modules(kind)
                routes = {}
                bt, _ = replicas(kind, B)
                sim = Simulator(model, head, bt, model_3d=kind, dt=DT, use_graph=False)
                v0 = start_velocities(sim)
                routes["eager"] = lambda s=sim: s.run(a.steps, every)
                base = Baseline(kind, model, head, replicas(kind, B)[0], sim.masses, v0)
                routes["baseline"] = lambda b=base: b.run(a.steps, every)
                sims = {"eager": sim}
                for U in a.spr:
                    s = sims["replay@%d" % U] = Simulator(model, head, bt, model_3d=kind, dt=DT, use_graph=True, steps_per_replay=U)
                    s.set_velocities(v0)
                    routes["replay@%d" % U] = lambda s=s: s.run(a.steps, every)
                rates = {name: [] for name in routes}
                for rnd in range(a.runs + 1):   # (round 0: untimed, captures included)
                    for name, fn in routes.items():
                        r = timed(fn, a.steps)
                        if rnd:
                            rates[name].append(r)
                for name in routes:
                    line = dict(case="throughput", kind=kind, replicas=B, record_every=every, route=name,
                                steps_per_run=a.steps, captures=sims[name].captures if name in sims else None,
                                **summary(rates[name]))
                    lines.append(line)
                    print(json.dumps(line), flush=True)
                rep = {U: rates["replay@%d" % U] for U in a.spr}
                best = max(a.spr, key=lambda U: statistics.median(rep[U]))
                default = min(U for U in a.spr if statistics.median(rep[U]) >= min(rep[best]))
                graph_wins = min(min(r) for r in rep.values()) > max(rates["baseline"])
                d = dict(case="decision", kind=kind, replicas=B, record_every=every, best_spr=best, default_spr=default,
                         slowest_replay_beats_fastest_baseline=bool(graph_wins),
                         speedup_default_over_baseline=round(statistics.median(rep[default])
                                                             / statistics.median(rates["baseline"]), 2))
                decisions.append(d)
                print(json.dumps(d), flush=True)
                del sims, routes, base, sim, model, head
    return lines, decisions


def drift(a):
    """Total energy per atom at the start and end of --drift-steps NVE steps: the GPU run and the fp64 twin."""
    import force_twin as tw
    import md_twin as mt
    from geossl_amd.md import Simulator
    from oracle.graph import radius_graph_np
    lines = []
    ps = a.drift_steps * DT * 1e-3
    for kind in a.kinds:
        cfg = SCHNET if kind == "schnet" else PAINN
        model, head = modules(kind)
        bt, raw = replicas(kind, 1)
        sim = Simulator(model, head, bt, model_3d=kind, dt=DT, use_graph=True)
        v0 = start_velocities(sim)
        traj = sim.run(a.drift_steps, record_every=10)
        total = traj.potential.double().sum(1) + traj.kinetic.sum(1)
        torch.cuda.synchronize()
        total = total.cpu().numpy()
        gpu = dict(drift_per_atom_per_ps=float(total[-1] - total[0]) / N_ATOMS / ps,
                   max_excursion_per_atom=float(np.abs(total - total[0]).max()) / N_ATOMS)
        # the twin, parameters uploaded once
        P, Bf = tw.module_tensors(model)
        H = tw.module_tensors(head)[0]
        dd = dict(dtype=torch.float64, device=DEV)
        Pd = {k: v.to(**dd) for k, v in list(P.items()) + list(Bf.items()) if v.is_floating_point()}
        Hd = {k: v.to(**dd) for k, v in H.items()}
        keys = (("num_interactions", "cutoff", "readout") if kind == "schnet"
                else ("n_atom_basis", "n_interactions", "cutoff", "readout"))
        tcfg = {k: cfg[k] for k in keys}
        z, bvec = torch.from_numpy(raw["x"]).to(DEV), torch.from_numpy(raw["batch"]).to(DEV)
        last = {}

        def force(x):
            p32 = x.astype(np.float32)
            ei = (tw.schnet_edges(p32, raw["batch"], cfg["cutoff"]) if kind == "schnet"
                  else torch.from_numpy(radius_graph_np(p32, cfg["cutoff"], raw["batch"])))
            xt = torch.from_numpy(x).to(**dd).requires_grad_(True)
            e = tw._energy(kind, tcfg, Pd, Hd, z, xt, bvec, ei.to(DEV))
            last["e"] = float(e.sum())
            return (-torch.autograd.grad(e.sum(), xt)[0]).cpu().numpy()
        masses = sim.masses.numpy()
        x, v = traj.positions[0].cpu().double().numpy(), v0.cpu().double().numpy()
        force(x)
        e0 = last["e"] + mt.kinetic(v, masses, raw["batch"]).sum()
        xs, vs = mt.integrate(x, v, force, masses, DT, a.drift_steps)
        force(xs[-1])
        e1 = last["e"] + mt.kinetic(vs[-1], masses, raw["batch"]).sum()
        line = dict(case="drift", kind=kind, steps=a.drift_steps, dt_fs=DT, temperature_K=T0, units="kcal/mol per atom",
                    gpu_fp32=gpu, twin_fp64=dict(drift_per_atom_per_ps=float(e1 - e0) / N_ATOMS / ps),
                    kinetic_per_atom_at_start=float(traj.kinetic[0].sum()) / N_ATOMS)
        lines.append(line)
        print(json.dumps(line), flush=True)
    return lines


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kinds", nargs="+", default=["schnet", "painn"])
    p.add_argument("--replicas", nargs="+", type=int, default=[1, 64, 1024])
    p.add_argument("--record-every", nargs="+", type=int, default=[1, 100])
    p.add_argument("--spr", nargs="+", type=int, default=[1, 4, 16])
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--drift-steps", type=int, default=2000)
    p.add_argument("--out", default="")
    a = p.parse_args()
    from geossl_amd import build
    lines, decisions = throughput(a)
    doc = dict(tool="bench_md", device=torch.cuda.get_device_name(0), source_hash=build.source_hash(),
               config=dict(atoms=N_ATOMS, dt_fs=DT, schnet=SCHNET, painn=PAINN, runs=a.runs, steps_per_run=a.steps),
               lines=lines, decisions=decisions, drift=drift(a) if a.drift_steps else [])
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
