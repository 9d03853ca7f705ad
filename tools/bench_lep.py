#!/usr/bin/env python3
"""One LEP training step (forward, backward, Adam) on the one-pass fused step against the reference's two-pass lines.

    python tools/bench_lep.py [--bs 8 32] [--steps 10] [--warmup 3] [--rounds 5] [--out profiles/NAME.json]

Synthetic pairs: every structure a pocket of tests/lba_structures.py (rejection sampling at 0.08 atoms per cubic
Angstrom, 1 A minimum separation), its size drawn uniformly in 100 ... 400 per side (`--LEP_maxnum 400` is the script's
default), one fixed batch per (backbone, batch size).  SchNet at the script's defaults (128 features, 6 blocks, 51
gaussians, 10 A, "mean") and PaiNN at its defaults (128 features, 3 blocks, 20 rbf, 5 A, "add"; the edge lists built per
side by ops.radius_graph).  Three ways through the same step, each on its own copy of the same weights:

  (a) trainer_eager   LEPTrainer.step, eager launches;
  (b) trainer_graph   LEPTrainer.step with use_graph=True on the repeating batch (one per-structure graph, replayed);
  (c) aten_two_pass   the reference's lines :33-49 in ATen on our backbone - two backbone calls, torch.cat, the Linear,
                      BCEWithLogitsLoss - with a stock torch.optim.Adam: what runs without geossl_amd.finetune_lep.

A step ends in the optimizer's launches; the time is a host clock around `steps` steps that end in a device
synchronise, after `warmup` steps of the same shape.  The three alternate round by round in one process; per line the
median and the min / max over the rounds, and the ratio (a) / (c) with the ratios of the extremes.  Needs the GPU: there
is no fallback.  Prints one JSON document; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden")]

CONFIGS = {
    "schnet": dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0,
                   readout="mean", node_class=9),
    "painn": dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add"),
}


def make_batch(kind, bs, dev, seed):
    """A BatchLEP of bs pairs on the device, sizes uniform in 100 ... 400 per side."""
    import lba_structures as ls
    from geossl_amd import ops
    from geossl_amd.Geom3D.dataloaders import BatchLEP
    rng = np.random.default_rng(seed)
    out = BatchLEP(y=torch.from_numpy(rng.integers(0, 2, size=bs)).to(dev))
    for s, side in enumerate(("active", "inactive")):
        sizes = rng.integers(100, 401, size=bs).astype(np.int64)
        d = ls.structures(sizes, seed + 1 + s)
        pos, bvec = torch.from_numpy(d["positions"]).to(dev), torch.from_numpy(d["batch"]).to(dev)
        out["x_" + side], out["positions_" + side], out["batch_" + side] = torch.from_numpy(d["x"]).to(dev), pos, bvec
        setattr(out, "_sizes_" + side, sizes)
        if kind == "painn":
            out["radius_edge_index_" + side] = ops.radius_graph(pos, CONFIGS["painn"]["cutoff"], bvec)
    out._num_graphs = bs
    return out


def modules(kind, dev):
    from filler import fill_module_
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    model = fill_module_((SchNet if kind == "schnet" else PaiNN)(**CONFIGS[kind])).to(dev)
    head = fill_module_(torch.nn.Linear(256, 1)).to(dev)
    with torch.no_grad():
        head.weight.mul_(0.05)   # (logits of order one with the filler's weights)
    return model, head


def aten_step(kind, batch, model, head, criterion, opt):
    if kind == "schnet":
        active = model(batch.x_active, batch.positions_active, batch.batch_active)
        inactive = model(batch.x_inactive, batch.positions_inactive, batch.batch_inactive)
    else:
        active = model(batch.x_active, batch.positions_active, batch.radius_edge_index_active, batch.batch_active)
        inactive = model(batch.x_inactive, batch.positions_inactive, batch.radius_edge_index_inactive,
                         batch.batch_inactive)
    pred = head(torch.cat((active, inactive), dim=1)).squeeze()
    loss = criterion(pred, batch.y.float())
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--kinds", nargs="*", default=["schnet", "painn"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lep.py measures on the GPU: none found")
    from geossl_amd import build
    from geossl_amd.finetune_lep import LEPTrainer
    dev = "cuda:0"
    lines = []
    for kind in a.kinds:
        for bs in a.bs:
            batch = make_batch(kind, bs, dev, seed=400 + bs)
            steps, first = {}, {}
            for name, use_graph in (("trainer_eager", False), ("trainer_graph", True)):
                model, head = modules(kind, dev)
                tr = LEPTrainer(model, head, lr=a.lr, model_3d=kind, use_graph=use_graph, graph_mode="structure")
                steps[name] = (lambda tr=tr: tr.step(batch))
            model, head = modules(kind, dev)
            opt = torch.optim.Adam(list(model.parameters()) + list(head.parameters()), lr=a.lr)
            criterion = torch.nn.BCEWithLogitsLoss()
            steps["aten_two_pass"] = (lambda m=model, h=head, o=opt: aten_step(kind, batch, m, h, criterion, o))

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / a.steps * 1e3

            for name, fn in steps.items():              # warm-up of every variant; the first loss for the agreement check
                first[name] = float(fn())
                for _ in range(a.warmup - 1):
                    fn()
            ms = {name: [] for name in steps}
            for _ in range(a.rounds):                   # the variants alternate
                for name, fn in steps.items():
                    ms[name].append(timed(fn))
            line = dict(kind=kind, bs=bs, atoms=int(batch.batch_active.numel() + batch.batch_inactive.numel()),
                        max_atoms=int(max(batch._sizes_active.max(), batch._sizes_inactive.max())), steps=a.steps,
                        rounds=a.rounds)
            for name in steps:
                line[name + "_ms"] = round(statistics.median(ms[name]), 4)
                line[name + "_ms_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
            e, c = ms["trainer_eager"], ms["aten_two_pass"]
            line["eager_over_aten"] = round(statistics.median(e) / statistics.median(c), 4)
            line["eager_over_aten_min_max"] = [round(min(e) / max(c), 4), round(max(e) / min(c), 4)]
            line["graph_over_aten"] = round(statistics.median(ms["trainer_graph"]) / statistics.median(c), 4)
            line["first_loss_rel_diff"] = max(abs(first[n] - first["aten_two_pass"]) for n in first) / abs(first["aten_two_pass"])
            lines.append(line)
            print(json.dumps(line), flush=True)
            del steps, batch
            torch.cuda.empty_cache()
    doc = dict(tool="bench_lep", device=torch.cuda.get_device_name(0), source_hash=build.source_hash(),
               configs=CONFIGS, lines=lines)
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
