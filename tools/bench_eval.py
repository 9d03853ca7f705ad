#!/usr/bin/env python3
"""Evaluation passes over a whole loader, eager against replayed: seconds per pass, ms per batch and graph captures.

    python tools/bench_eval.py [--workloads supervised lba lep] [--kinds schnet painn] [--passes 3]
                               [--out profiles/eval_bench.json]

Workloads, seeded and generated here, each from ``DeviceLoader`` handles (shuffle off, as an evaluation loader is):

* ``supervised``: 8192 ragged QM9-sized molecules (``synthetic`` set B, at most 33 atoms), batch sizes 128 and 1024.
  ``eager``: the loop a user writes today, the reference's eval() - ``predict_Supervised`` per batch, ``torch.cat`` and one
  copy to the host at the end (``eval_Supervised(use_graph=False)`` is these lines); ``graph``:
  ``eval_Supervised(use_graph=True)``.
* ``lba``: 512 pockets of 100 to 500 atoms, batch sizes 8 and 32; ``eval_LBA`` with use_graph False / True (the eager
  lines read each handle's gathered tensors with x as LBA's records hold it, 1-D: ``_Records``).
* ``lep``: 256 pairs of 100 to 400 atoms per side, batch sizes 8 and 32; ``eval_LEP`` with use_graph False / True.

Each with SchNet (128 / 6 blocks / 51 gaussians / 10 A / mean, Linear head) and PaiNN (128 / 3 blocks / 20 radial
functions / 5 A / add, its output layers; radius edges built with the dataset).  Per shape one untimed pass per route (the
graph route's captures), then ``--passes`` timed passes per route, the two routes ALTERNATING in one process; a pass is
timed with the host clock from its start to a device synchronise behind it.  Reported per route: seconds per pass (median,
min - max), ms per batch, captures in the untimed pass and in the timed ones.  ``replay_wins``: the slowest replayed pass
is faster than the fastest eager pass.  The default of the entry points that are new with geossl_amd/evaluate.py follows
from it (``defaults``): on for a head kind when the replay wins at both batch sizes for every measured backbone.
Needs the GPU.  Prints one JSON document; --out also writes it."""
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

DEV = "cuda:0"
SCHNET = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0, readout="mean",
              node_class=9)
PAINN = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")
SHAPES = {"supervised": (8192, (128, 1024)), "lba": (512, (8, 32)), "lep": (256, (8, 32))}
SPACING = 2.3   # A: a jittered cubic lattice at about the atom density of a pocket


def pockets(sizes, rng):
    """Positions of structures of `sizes` atoms: the sites of a cubic lattice nearest its centre, each moved by up to
    0.5 A per axis (no two atoms closer than 1.3 A), and atom types 1 .. 8."""
    pos = []
    for n in sizes:
        side = int(np.ceil(n ** (1.0 / 3.0))) + 1
        grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        keep = np.argsort(((grid - (side - 1) / 2.0) ** 2).sum(1), kind="stable")[:n]
        pos.append(grid[keep] * SPACING + rng.uniform(-0.5, 0.5, size=(n, 3)) + 1.0)
    pos = np.concatenate(pos).astype(np.float32)
    return pos, rng.integers(1, 9, size=pos.shape[0]).astype(np.int64)


def modules(kind, pair):
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    torch.manual_seed(1234)
    model = (SchNet(**SCHNET) if kind == "schnet" else PaiNN(**PAINN)).to(DEV)
    if pair:
        head = torch.nn.Linear(256, 1).to(DEV)
    else:
        head = torch.nn.Linear(128, 1).to(DEV) if kind == "schnet" else model.create_output_layers().to(DEV)
    return model, head


def dataset(workload, kind):
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset, PairedDeviceDataset
    from geossl_amd.synthetic import make_molecules
    rng = np.random.default_rng(7)
    radius = PAINN["cutoff"] if kind == "painn" else None
    M = SHAPES[workload][0]
    if workload == "supervised":
        mols = make_molecules(M, seed=7, mode="B")
        return DeviceDataset.from_numpy(mols, DEV, y=rng.standard_normal((M, 12)).astype(np.float32), radius=radius)
    if workload == "lba":
        sizes = rng.integers(100, 501, size=M)
        pos, x = pockets(sizes, rng)
        return DeviceDataset(x, pos, sizes, DEV, y=rng.standard_normal(M).astype(np.float32), radius=radius)
    sa, si = rng.integers(100, 401, size=M), rng.integers(100, 401, size=M)
    (pa, xa), (pi, xi) = pockets(sa, rng), pockets(si, rng)
    return PairedDeviceDataset(xa, pa, sa, xi, pi, si, rng.integers(0, 2, size=M), DEV, radius=radius)


class _Records:
    """A pocket handle as eval_LBA's eager lines read it: ``predict_LBA`` hands ``batch.x`` to the backbone as it is
    (DatasetLBA's 1-D atomic numbers), and a handle of such a dataset shows x as one column - its view, no copy."""

    def __init__(self, hb):
        self.hb, self.num_graphs, self._sizes = hb, hb.num_graphs, hb._sizes

    x = property(lambda self: self.hb.x[:, 0])
    positions = property(lambda self: self.hb.positions)
    batch = property(lambda self: self.hb.batch)
    radius_edge_index = property(lambda self: self.hb.radius_edge_index)
    y = property(lambda self: self.hb.y)

    def to(self, device):
        return self


def one_pass(workload, args, loader, model, head, use_graph):
    from geossl_amd.finetune_lba import eval_LBA
    from geossl_amd.finetune_lep import eval_LEP
    from geossl_amd.pretrain_Supervised import eval_Supervised
    if workload == "supervised":
        return float(eval_Supervised(args, loader, model, head, 0.25, 1.5, task_id=6, use_graph=use_graph)[0])
    if workload == "lba":
        return float(eval_LBA(args, loader if use_graph else (_Records(hb) for hb in loader), model, head,
                              use_graph=use_graph)[0])
    return float(eval_LEP(args, loader, model, head, use_graph=use_graph)[0])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(secs, n_batches):
    med = statistics.median(secs)
    return dict(s_per_pass=[round(s, 5) for s in secs], s_median=round(med, 5),
                s_min_max=[round(min(secs), 5), round(max(secs), 5)], ms_per_batch=round(med / n_batches * 1e3, 4))


def run(a):
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceLoader
    lines = []
    for workload in a.workloads:
        for kind in a.kinds:
            ds = dataset(workload, kind)
            args = types.SimpleNamespace(model_3d=kind, loss="mae")
            for bs in SHAPES[workload][1]:
                model, head = modules(kind, workload == "lep")
                loader = DeviceLoader(ds, batch_size=bs, shuffle=False)
                n_batches = len(loader)
                captures = lambda: getattr(model.__dict__.get("_geossl_evaluator"), "captures", 0)
                first = {}
                for route in ("eager", "graph"):                                   # the untimed pass of each route
                    first[route] = timed(lambda: one_pass(workload, args, loader, model, head, route == "graph"))
                cap_first = captures()
                secs = {"eager": [], "graph": []}
                for _ in range(a.passes):                                          # ... then the two alternate
                    for route in ("eager", "graph"):
                        secs[route].append(timed(lambda: one_pass(workload, args, loader, model, head,
                                                                  route == "graph"))[0])
                eager, graph = summary(secs["eager"], n_batches), summary(secs["graph"], n_batches)
                line = dict(workload=workload, kind=kind, bs=bs, batches=n_batches, rows=len(ds), eager=eager,
                            graph=graph, first_pass_s=dict(eager=round(first["eager"][0], 4),
                                                           graph=round(first["graph"][0], 4)),
                            captures_first_pass=cap_first, captures_timed_passes=captures() - cap_first,
                            figure=dict(eager=first["eager"][1], graph=first["graph"][1]),
                            speedup=round(eager["s_median"] / graph["s_median"], 3),
                            replay_wins=bool(graph["s_min_max"][1] < eager["s_min_max"][0]))
                lines.append(line)
                print(json.dumps(line), flush=True)
                del model, head, loader
                torch.cuda.empty_cache()
            del ds
            torch.cuda.empty_cache()
    return lines


def defaults(lines):
    """use_graph of the new entry points by head kind: on when the replay wins on every measured (backbone, batch size)
    of the workload that entry point serves (eval_Supervised: supervised; LEPTrainer.evaluate: lep)."""
    out = {}
    for key, workload in (("property", "supervised"), ("pair", "lep")):
        mine = [l for l in lines if l["workload"] == workload]
        out[key] = bool(mine) and all(l["replay_wins"] for l in mine)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="*", default=["supervised", "lba", "lep"], choices=sorted(SHAPES))
    ap.add_argument("--kinds", nargs="*", default=["schnet", "painn"], choices=["schnet", "painn"])
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on the GPU: none found")
    from geossl_amd import build
    lines = run(a)
    doc = dict(tool="bench_eval", label=a.label, device=torch.cuda.get_device_name(0), source_hash=build.source_hash(),
               config=dict(schnet=SCHNET, painn=PAINN, shapes={k: dict(rows=v[0], batch_sizes=list(v[1]))
                                                               for k, v in SHAPES.items()}, passes=a.passes),
               lines=lines, defaults=defaults(lines))
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
