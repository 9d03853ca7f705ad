#!/usr/bin/env python3
"""Normal-mode analysis on a force field: seconds per analysis of ``geossl_amd.vibrations.NormalModeAnalysis`` next to the
loop a user had before it.

    python tools/bench_vibrations.py [--kinds schnet painn] [--molecules 1 64] [--runs 3] [--out profiles/vibrations_bench.json]

Workload: B copies of ONE 21-atom molecule (a make_batch molecule, M = 63 coordinates) at the reference's MD17
configuration (tools/bench_relax.py's), seeded weights, the default delta.  Routes, per shape (kind, B):

* ``baseline``: the loop a user writes on ``predict_MD17(use_graph=True)`` - for each of the 63 coordinates the positions of
  the batch displaced by +delta and by -delta (one coordinate per molecule, all molecules at once), one call each, the row
  of every Hessian formed in torch operations, then (H + H^T) / 2, mass-weighting and ``torch.linalg.eigh`` on the device
  (no projection: less work than the analysis does).  That code is unchanged by vibrations.py: its timing is the parent's;
* ``eager@C`` / ``replay@C``: ``NormalModeAnalysis(use_graph=False / True, coords_per_pass=C).run()``.

A timed run is one whole analysis between two device synchronises, after one untimed run of the same kind (captures
included there); every route of a shape is timed once per round, ``--runs`` rounds, so the routes alternate; reported in
milliseconds, median (min - max).  Decision rules, printed per shape: the default C is the smallest C whose median lies
within the min - max spread of the best C; replay stays the default only where the slowest replayed run beats the fastest
eager run of the same C.  Needs the GPU.  Prints one JSON document; --out also writes it."""
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
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]

from bench_relax import DEV, N_ATOMS, PAINN, SCHNET, modules, replicas  # noqa: E402

COORDS = {1: [1, 8, 21, 63], 64: [1, 2, 4]}


def baseline(kind, model, head, bt, masses, delta):
    """6 n calls of predict_MD17 and the Hessians in torch operations -> eigenvalues [B, M]."""
    from geossl_amd.finetune_md17 import predict_MD17
    args = types.SimpleNamespace(model_3d=kind)
    B, M = len(bt._sizes), 3 * N_ATOMS
    x0 = bt.positions.clone()
    H = torch.zeros(B, M, M, dtype=torch.float64, device=DEV)
    flat = bt.positions.view(B, M)
    for k in range(M):
        g = []
        for s in (1.0, -1.0):
            bt.positions.copy_(x0)
            flat[:, k] += s * delta
            xk = flat[:, k].double().clone()
            _, F = predict_MD17(args, bt, model, head, use_graph=True)
            g.append((-F.double().view(B, M), xk))
        H[:, k, :] = (g[0][0] - g[1][0]) / (g[0][1] - g[1][1])[:, None]
    bt.positions.copy_(x0)
    H = 0.5 * (H + H.transpose(1, 2))
    w = masses.to(DEV).double().repeat_interleave(3).view(B, M)
    return torch.linalg.eigh(H / torch.sqrt(w[:, :, None] * w[:, None, :]))[0]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def summary(ms):
    return dict(ms=[round(t, 2) for t in ms], median=round(statistics.median(ms), 2), min_max=[round(min(ms), 2), round(max(ms), 2)])


def measure(a):
    from geossl_amd.vibrations import DELTA_DEFAULT, NormalModeAnalysis
    lines, decisions = [], []
    for kind in a.kinds:
        for B in a.molecules:
            model, head = modules(kind)
            bt = replicas(kind, B)
            coords = COORDS.get(B, [1])
            routes, nms = {}, {}
            for C in coords:
                for name, graph in (("eager", False), ("replay", True)):
                    nm = nms["%s@%d" % (name, C)] = NormalModeAnalysis(model, head, bt, model_3d=kind, use_graph=graph,
                                                                       coords_per_pass=C)
                    assert nm.fused
                    routes["%s@%d" % (name, C)] = nm.run
            bb = replicas(kind, B)
            routes["baseline"] = lambda: baseline(kind, model, head, bb, nm.masses, DELTA_DEFAULT)
            ms = {name: [] for name in routes}
            for rnd in range(a.runs + 1):   # (round 0: untimed, captures included)
                for name, fn in routes.items():
                    t = timed(fn)
                    if rnd:
                        ms[name].append(t)
            lam = nms["replay@%d" % coords[0]].run().eigenvalues
            top = float((lam[:, -1] - baseline(kind, model, head, bb, nm.masses, DELTA_DEFAULT)[:, -1]).abs().max()
                        / lam[:, -1].abs().max())
            for name in routes:
                line = dict(case="analysis", kind=kind, molecules=B, route=name,
                            captures=nms[name].captures if name in nms else None, **summary(ms[name]))
                lines.append(line)
                print(json.dumps(line), flush=True)
            rep = {C: ms["replay@%d" % C] for C in coords}
            best = min(coords, key=lambda C: statistics.median(rep[C]))
            default = min(C for C in coords if statistics.median(rep[C]) <= max(rep[best]))
            graph_wins = all(max(rep[C]) < min(ms["eager@%d" % C]) for C in coords)
            d = dict(case="decision", kind=kind, molecules=B, best_coords_per_pass=best, default_coords_per_pass=default,
                     image_atoms_at_default=2 * default * B * N_ATOMS, slowest_replay_beats_fastest_eager=bool(graph_wins),
                     speedup_default_over_baseline=round(statistics.median(ms["baseline"]) / statistics.median(rep[default]), 2),
                     largest_eigenvalue_relative_difference_to_baseline=top)
            decisions.append(d)
            print(json.dumps(d), flush=True)
            del nms, routes, model, head
    return lines, decisions


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kinds", nargs="+", default=["schnet", "painn"])
    p.add_argument("--molecules", nargs="+", type=int, default=[1, 64])
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--out", default="")
    a = p.parse_args()
    from geossl_amd import build
    from geossl_amd.vibrations import DELTA_DEFAULT
    lines, decisions = measure(a)
    doc = dict(tool="bench_vibrations", device=torch.cuda.get_device_name(0), source_hash=build.source_hash(),
               config=dict(atoms=N_ATOMS, delta=DELTA_DEFAULT, schnet=SCHNET, painn=PAINN, runs=a.runs, coords=COORDS),
               lines=lines, decisions=decisions)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
