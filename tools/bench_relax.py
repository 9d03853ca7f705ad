#!/usr/bin/env python3
"""Structure relaxation on a force field: steps per second of ``geossl_amd.relax.Minimizer`` next to the loop a user had
before it.

    python tools/bench_relax.py [--kinds schnet painn] [--replicas 1 64 1024] [--spr 4 16] [--steps 200] [--runs 3]
                                [--out profiles/relax_bench.json]

Workload: B replicas of ONE 21-atom molecule (a make_batch molecule) at the reference's MD17 configuration (SchNet 128 /
6 blocks / 51 gaussians / 10 A / mean with Linear(128, 1); PaiNN 128 / 3 blocks / 20 radial functions / 5 A / add with
its output layers), seeded weights, FIRE with the Minimizer's defaults and a tolerance no molecule reaches, so that every
run makes all of its ``--steps`` steps.  Routes, per shape (kind, B):

* ``baseline``: the loop a user writes on ``predict_MD17(use_graph=True)`` - the same FIRE, per molecule, in torch
  operations (``Baseline`` below), with the one read-back per step such a loop needs to decide whether to stop.  That code
  is unchanged by relax.py, so its timing here is the parent commit's;
* ``eager@U``: ``Minimizer(use_graph=False, steps_per_replay=U)`` - eager launches, one word read per U steps;
* ``replay@U``: ``Minimizer(use_graph=True, steps_per_replay=U)``.

A timed run is a reset to the start and ``--steps`` steps between two device synchronises, after one untimed run of the same
kind (captures included there); every route of a shape is timed once per round, ``--runs`` rounds, so the routes alternate;
reported as steps per second, median (min - max).  Decision rules, evaluated per shape and printed: the default
``steps_per_replay`` is the smallest U whose median lies within the min - max spread of the best U; ``use_graph`` stays True
only where the slowest replayed run beats the fastest eager run of the same U.  Needs the GPU.  Prints one JSON document;
--out also writes it."""
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
sys.path[:0] = [REPO]

N_ATOMS, DEV, FTOL = 21, "cuda:0", 1e-6
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
    return bt


class Baseline:
    """FIRE (the definition of geossl_amd/relax.py, its defaults) around predict_MD17 in torch operations: what a user
    wrote before relax.py."""

    def __init__(self, kind, model, head, bt, masses, B):
        from geossl_amd.relax import ACCEL
        self.args, self.model, self.head, self.bt, self.B = types.SimpleNamespace(model_3d=kind), model, head, bt, B
        self.cinv = (ACCEL / masses).float().to(DEV)[:, None]
        self.mol = bt.batch.long()
        self.x0 = bt.positions.clone()

    def _sum(self, t):
        return torch.zeros(self.B, device=DEV).index_add_(0, self.mol, t)

    def _max(self, t):
        return torch.zeros(self.B, device=DEV).scatter_reduce_(0, self.mol, t, "amax")

    def run(self, steps, ftol=FTOL, dt_max=5.0, dt_min=0.01, max_step=0.1, n_min=5, f_inc=1.1, f_dec=0.5, a0=0.1, f_a=0.99):
        from geossl_amd.finetune_md17 import predict_MD17
        bt, mol, B = self.bt, self.mol, self.B
        bt.positions.copy_(self.x0)
        v = torch.zeros_like(bt.positions)
        dt, alpha = torch.full((B,), 0.5, device=DEV), torch.full((B,), a0, device=DEV)
        npos, done = torch.zeros(B, dtype=torch.long, device=DEV), torch.zeros(B, dtype=torch.bool, device=DEV)
        for _ in range(steps):
            _, F = predict_MD17(self.args, bt, self.model, self.head, use_graph=True)
            done = done | (self._max((F * F).sum(1)).sqrt() < ftol)
            if bool(done.all()):   # (the read-back such a loop decides on)
                break
            P, vv, ff = self._sum((F * v).sum(1)), self._sum((v * v).sum(1)), self._sum((F * F).sum(1))
            down = (P > 0) | (vv == 0)
            c = alpha * torch.sqrt(vv / ff.clamp_min(1e-30))
            v1 = torch.where(down[mol, None], (1 - alpha)[mol, None] * v + c[mol, None] * F, torch.zeros_like(v))
            grow = down & (npos > n_min)
            dt_n = torch.where(down, torch.where(grow, (dt * f_inc).clamp(max=dt_max), dt), (dt * f_dec).clamp(min=dt_min))
            alpha_n = torch.where(down, torch.where(grow, alpha * f_a, alpha), torch.full_like(alpha, a0))
            v2 = v1 + dt_n[mol, None] * (F * self.cinv)
            dr = dt_n[mol, None] * v2
            dm = self._max((dr * dr).sum(1)).sqrt()
            s = torch.where(dm > max_step, max_step / dm.clamp_min(1e-30), torch.ones_like(dm))
            move = ~done
            am = move[mol, None]
            v = torch.where(am, v2, v)
            bt.positions.copy_(torch.where(am, bt.positions + s[mol, None] * dr, bt.positions))
            dt, alpha = torch.where(move, dt_n, dt), torch.where(move, alpha_n, alpha)
            npos = torch.where(move, torch.where(down, npos + 1, torch.zeros_like(npos)), npos)
        return bt.positions


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
    from geossl_amd.relax import Minimizer
    lines, decisions = [], []
    for kind in a.kinds:
        for B in a.replicas:
            model, head = modules(kind)
            bt = replicas(kind, B)
            x0 = bt.positions.clone()
            routes, mins = {}, {}

            def relax(mz):
                mz.reset()
                mz.set_positions(x0)
                res = mz.run(a.steps)
                assert int(res.steps.min()) == a.steps, "a molecule converged: the runs are not the same work"
            for U in a.spr:
                for name, graph in (("eager", False), ("replay", True)):
                    mz = mins["%s@%d" % (name, U)] = Minimizer(model, head, bt, model_3d=kind, fmax=FTOL, use_graph=graph,
                                                               steps_per_replay=U, max_frames=1)
                    assert mz.fused
                    routes["%s@%d" % (name, U)] = lambda mz=mz: relax(mz)
            base = Baseline(kind, model, head, replicas(kind, B), mz.masses, B)
            routes["baseline"] = lambda: base.run(a.steps)
            rates = {name: [] for name in routes}
            for rnd in range(a.runs + 1):   # (round 0: untimed, captures included)
                for name, fn in routes.items():
                    r = timed(fn, a.steps)
                    if rnd:
                        rates[name].append(r)
            same = float((mins["replay@%d" % a.spr[0]].positions - base.bt.positions).abs().max())
            for name in routes:
                line = dict(case="throughput", kind=kind, replicas=B, route=name, steps_per_run=a.steps,
                            captures=mins[name].captures if name in mins else None, **summary(rates[name]))
                lines.append(line)
                print(json.dumps(line), flush=True)
            rep = {U: rates["replay@%d" % U] for U in a.spr}
            best = max(a.spr, key=lambda U: statistics.median(rep[U]))
            default = min(U for U in a.spr if statistics.median(rep[U]) >= min(rep[best]))
            graph_wins = all(min(rep[U]) > max(rates["eager@%d" % U]) for U in a.spr)
            d = dict(case="decision", kind=kind, replicas=B, best_spr=best, default_spr=default,
                     slowest_replay_beats_fastest_eager=bool(graph_wins),
                     speedup_default_over_baseline=round(statistics.median(rep[default]) / statistics.median(rates["baseline"]), 2),
                     max_position_difference_to_baseline=same)
            decisions.append(d)
            print(json.dumps(d), flush=True)
            del mins, routes, base, model, head
    return lines, decisions


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kinds", nargs="+", default=["schnet", "painn"])
    p.add_argument("--replicas", nargs="+", type=int, default=[1, 64, 1024])
    p.add_argument("--spr", nargs="+", type=int, default=[4, 16])
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--out", default="")
    a = p.parse_args()
    from geossl_amd import build
    lines, decisions = throughput(a)
    doc = dict(tool="bench_relax", device=torch.cuda.get_device_name(0), source_hash=build.source_hash(),
               config=dict(atoms=N_ATOMS, ftol=FTOL, schnet=SCHNET, painn=PAINN, runs=a.runs, steps_per_run=a.steps),
               lines=lines, decisions=decisions)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
