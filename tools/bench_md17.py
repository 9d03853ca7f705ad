#!/usr/bin/env python3
"""MD17 fine-tuning on a shuffled trajectory, loader included: ms per step and graph captures, before and after
geossl_amd/finetune_md17.py.

    python tools/bench_md17.py [--train-bs 1 32] [--eval-bs 128] [--runs 3] [--warmup-runs 1] [--steps 200]
                               [--kinds painn schnet] [--out profiles/md17_bench.json]

Workload: 1000 synthetic frames of ONE 21-atom molecule (a make_batch molecule moved by 0.05 A of noise per frame, the
atom types fixed), random energy and force targets, at the reference's MD17 configuration (SchNet 128 / 6 blocks / 51
gaussians / 10 A / mean with Linear(128, 1); PaiNN 128 / 3 blocks / 20 radial functions / 5 A / add with its output
layers; L1, 0.05 / 0.95).  Every epoch visits the frames in a new shuffled order; the loader's work is inside the timed
region.  Routes:

* training, ``before``: ``graphed.ForceTrainer`` (unchanged by this module, so its timing here is the parent commit's)
  on batches the host collates per step from per-frame records - PaiNN with each frame's own radius list, as
  ``DatasetMD17Radius`` builds it - and uploads;
* training, ``after_collated`` / ``after_handles``: ``MD17Trainer`` on the same collated batches, and on ``DeviceLoader``
  handles of a ``DeviceDataset(..., y=, force=)``.  ``after_collated@0``: GEOSSL_MD17_COMPLETE_EDGES=0;
* evaluation, ``before``: the reference's eval() lines (per-batch autograd force, ``torch.cat`` on the device) on this
  library's modules over collated batches; ``after``: ``eval_MD17`` on handles, replayed.

A timed run is ``--steps`` training steps (whole shuffled epochs are chained) or one evaluation of all frames, between
two device synchronises, after ``--warmup-runs`` runs of the same kind; ms per step (per batch for the evaluation) per
run, median and min - max over ``--runs`` runs, with the capture count of the route.  The PaiNN default follows from the
rule: at a batch size the complete list is the default only if ``after_collated`` is faster than ``before`` by more than
the larger min - max spread of the two.  Needs the GPU.  Prints one JSON document; --out also writes it."""
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

N_FRAMES, N_ATOMS, DEV = 1000, 21, "cuda:0"
SWITCH = "GEOSSL_MD17_COMPLETE_EDGES"
SCHNET = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0, readout="mean",
              node_class=9)
PAINN = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")


def trajectory(seed=0):
    """x [21] (one molecule), positions [1000, 21, 3], y [1000], force [1000, 21, 3], per-frame 5 A radius lists."""
    from geossl_amd.synthetic import make_batch
    from oracle.graph import radius_graph_np
    base = make_batch(0, seed=41, sizes=[N_ATOMS])
    rng = np.random.default_rng(seed)
    pos = (base["positions"][None] + 0.05 * rng.standard_normal((N_FRAMES, N_ATOMS, 3))).astype(np.float32)
    x = np.clip(base["x"][:, 0], 1, 8)
    y = rng.standard_normal(N_FRAMES).astype(np.float32)
    force = rng.standard_normal((N_FRAMES, N_ATOMS, 3)).astype(np.float32)
    edges = [radius_graph_np(p, PAINN["cutoff"]) for p in pos]
    return dict(x=x, pos=pos, y=y, force=force, edges=edges)


def collated(data, kind, ids):
    """One batch as the host collates it from per-frame records (edges with their node offsets) and uploads it."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.layout import prepare_batch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, non_blocking=True)
    B = len(ids)
    bv = up(np.repeat(np.arange(B, dtype=np.int64), N_ATOMS))
    rei = None
    if kind == "painn":
        rei = up(np.concatenate([data["edges"][i] + k * N_ATOMS for k, i in enumerate(ids)], axis=1))
    b = pg.Batch(up(np.tile(data["x"], B)), up(data["pos"][ids].reshape(-1, 3)), bv, None, rei, B, [N_ATOMS] * B)
    prepare_batch(bv, None, b._sizes, lazy=True)
    b.y, b.force = up(data["y"][ids]), up(data["force"][ids].reshape(-1, 3))
    return b


def modules(kind):
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    torch.manual_seed(1234)
    if kind == "schnet":
        return SchNet(**SCHNET).to(DEV), torch.nn.Linear(128, 1).to(DEV)
    model = PaiNN(**PAINN).to(DEV)
    return model, model.create_output_layers().to(DEV)


def dataset(data, kind):
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset
    return DeviceDataset(np.tile(data["x"], N_FRAMES), data["pos"].reshape(-1, 3), [N_ATOMS] * N_FRAMES, DEV,
                         y=data["y"], force=data["force"].reshape(-1, 3),
                         radius=PAINN["cutoff"] if kind == "painn" else None)


def batches_for_ever(data, kind, bs, handles, gen):
    """Shuffled epochs chained: collated batches, or the handles of a DeviceLoader."""
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceLoader
    if handles:
        loader = DeviceLoader(dataset(data, kind), batch_size=bs, shuffle=True, drop_last=True, generator=gen)
        while True:
            yield from loader
    while True:
        order = torch.randperm(N_FRAMES, generator=gen).numpy()
        for k in range(N_FRAMES // bs):
            yield collated(data, kind, order[k * bs:(k + 1) * bs])


def summary(ms):
    return dict(ms_per_step=ms, ms_median=round(statistics.median(ms), 4), ms_min_max=[min(ms), max(ms)])


def run_training(a, data):
    from geossl_amd.finetune_md17 import MD17Trainer
    from geossl_amd.graphed import ForceTrainer
    lines = []
    for kind in a.kinds:
        routes = (["before", "after_collated", "after_collated@0", "after_handles"] if kind == "painn"
                  else ["before", "after_handles"])
        for bs in a.train_bs:
            for route in routes:
                name, _, sw = route.partition("@")
                os.environ.pop(SWITCH, None)
                if sw:
                    os.environ[SWITCH] = sw
                model, head = modules(kind)
                tr = (ForceTrainer if name == "before" else MD17Trainer)(model, head, model_3d=kind, lr=1e-5)
                it = batches_for_ever(data, kind, bs, name == "after_handles", torch.Generator().manual_seed(1))
                ms, last = [], None
                for run in range(a.warmup_runs + a.runs):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        b = next(it)
                        last = tr.step(b, b.y, b.force) if name == "before" else tr.step(b)
                    torch.cuda.synchronize()
                    if run >= a.warmup_runs:
                        ms.append(round((time.perf_counter() - t0) / a.steps * 1e3, 4))
                line = dict(case="training", kind=kind, bs=bs, route=name, switch=sw or None, steps_per_run=a.steps,
                            captures=tr.captures, last_loss=float(last), **summary(ms))
                lines.append(line)
                print(json.dumps(line), flush=True)
                del tr, model, head, it
                torch.cuda.empty_cache()
    os.environ.pop(SWITCH, None)
    return lines


def reference_eval(kind, model, head, loader):
    """eval() of the reference's script on this library's modules: the route a user has before eval_MD17."""
    pred_energy_list, actual_energy_list = [], []
    pred_force_list, actual_force_list = torch.Tensor([]).to(DEV), torch.Tensor([]).to(DEV)
    for b in loader:
        positions = b.positions
        positions.requires_grad_()
        rep = model(b.x, positions, b.batch) if kind == "schnet" else model(b.x, positions, b.radius_edge_index, b.batch)
        pred_energy = head(rep).squeeze(1)
        force = -torch.autograd.grad(pred_energy, positions, torch.ones_like(pred_energy), create_graph=True,
                                     retain_graph=True)[0].detach_()
        actual = b.force
        if torch.sum(torch.isnan(force)) != 0:
            mask = torch.isnan(force)
            force, actual = force[~mask].reshape((-1, 3)), actual[~mask].reshape((-1, 3))
        pred_energy_list.append(pred_energy.cpu().detach())
        actual_energy_list.append(b.y.cpu())
        pred_force_list = torch.cat([pred_force_list, force], dim=0)
        actual_force_list = torch.cat([actual_force_list, actual], dim=0)
    pe, ae = torch.cat(pred_energy_list, dim=0), torch.cat(actual_energy_list, dim=0)
    return (torch.mean(torch.abs(pe - ae)).cpu().item(),
            torch.mean(torch.abs(pred_force_list - actual_force_list)).cpu().item())


def run_evaluation(a, data):
    import types
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceLoader
    from geossl_amd.finetune_md17 import _predictor, eval_MD17
    lines = []
    for kind in a.kinds:
        for bs in a.eval_bs:
            n_batches = -(-N_FRAMES // bs)
            model, head = modules(kind)
            ds = dataset(data, kind)
            args = types.SimpleNamespace(model_3d=kind)
            results = {}
            for route in ("before", "after"):
                ms = []
                for run in range(a.warmup_runs + a.runs):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if route == "before":
                        order = np.arange(N_FRAMES)
                        got = reference_eval(kind, model, head, (collated(data, kind, order[k * bs:(k + 1) * bs])
                                                                 for k in range(n_batches)))
                    else:
                        got = eval_MD17(args, DeviceLoader(ds, batch_size=bs, shuffle=False), model, head)
                    torch.cuda.synchronize()
                    if run >= a.warmup_runs:
                        ms.append(round((time.perf_counter() - t0) / n_batches * 1e3, 4))
                results[route] = got
                line = dict(case="evaluation", kind=kind, bs=bs, route=route, batches_per_run=n_batches,
                            captures=_predictor(model, head, kind).captures if route == "after" else 0,
                            energy_mae=got[0], force_mae=got[1], **summary(ms))
                lines.append(line)
                print(json.dumps(line), flush=True)
            del model, head, ds
            torch.cuda.empty_cache()
    return lines


def decisions(lines):
    """The rule of the module docstring, per PaiNN training batch size."""
    out = []
    pick = lambda bs, route, sw: next((l for l in lines if l["case"] == "training" and l["kind"] == "painn"
                                       and l["bs"] == bs and l["route"] == route and l["switch"] == sw), None)
    for bs in sorted({l["bs"] for l in lines if l["case"] == "training" and l["kind"] == "painn"}):
        before, after = pick(bs, "before", None), pick(bs, "after_collated", None)
        if before is None or after is None:
            continue
        spread = max(before["ms_min_max"][1] - before["ms_min_max"][0], after["ms_min_max"][1] - after["ms_min_max"][0])
        gain = before["ms_median"] - after["ms_median"]
        out.append(dict(bs=bs, before_ms=before["ms_median"], after_ms=after["ms_median"], spread_ms=round(spread, 4),
                        complete_list_default=bool(gain > spread)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-bs", type=int, nargs="*", default=[1, 32])
    ap.add_argument("--eval-bs", type=int, nargs="*", default=[128])
    ap.add_argument("--kinds", nargs="*", default=["painn", "schnet"], choices=["painn", "schnet"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup-runs", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="training steps per timed run")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_md17.py measures on the GPU: none found")
    from geossl_amd import build
    data = trajectory()
    live = [int(e.shape[1]) for e in data["edges"]]
    lines = run_training(a, data) + run_evaluation(a, data)
    doc = dict(tool="bench_md17", label=a.label, device=torch.cuda.get_device_name(0), source_hash=build.source_hash(),
               config=dict(frames=N_FRAMES, atoms=N_ATOMS, schnet=SCHNET, painn=PAINN, runs=a.runs,
                           warmup_runs=a.warmup_runs, steps_per_run=a.steps,
                           live_pairs_of_420=[min(live), int(statistics.median(live)), max(live)]),
               lines=lines, painn_default=decisions(lines))
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
