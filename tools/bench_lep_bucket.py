#!/usr/bin/env python3
"""LEP training steps on shuffled pairs, loader included: ms per step and graph captures per epoch.

    python tools/bench_lep_bucket.py [--bs 8 32] [--routes ...] [--epochs 3] [--warmup-epochs 2] [--label NAME] [--out FILE.json]
    python tools/bench_lep_bucket.py --merge RUN.json [RUN.json ...] --out profiles/lep_bucket_bench.json

``LEPTrainer(model, head, model_3d="schnet")`` - the trainer of finetune_lep.py - at 128 features, 6 blocks, 51
gaussians, cutoff 10 A, "mean", on 256 synthetic pairs of 100 to 400 atoms per side (the generator of
tools/bench_lep.py: the pockets of tests/lba_structures.py).  Every epoch visits the pairs in a new shuffled order, so no
two batches share both size sequences.  The routes, per batch size:

* "collated_graph":  ``DataLoaderLEP(items, batch_size, shuffle=True)`` - the reference's Python collation - ``.to(device)``,
  ``LEPTrainer(use_graph=True).step``.  With GEOSSL_SPARSE_BUCKETS=1 on a commit that has the route, the batches replay
  one sparse bucket graph; otherwise a per-structure graph is never replayed and every step is eager launches.
* "collated_eager":  the same loader with ``use_graph=False``.
* "handles":         ``DeviceLoader(PairedDeviceDataset)`` pair handles, ``use_graph=True`` (skipped, and recorded as
  absent, on a commit without ``PairedDeviceDataset``).

The timed region is a whole epoch - the loader's work and ``trainer.step`` of every batch - between two device
synchronises, after ``--warmup-epochs`` epochs of the same kind; the result is milliseconds per step per epoch.  The
graphs captured in every epoch (warm-up included) are reported beside it.  Only public API is used: the file runs
unchanged on the parent commit.  Needs the GPU.  Prints one JSON document; --out also writes it to a file.

--merge: the runs of one session (labels ``parent_*`` and ``new_*``, alternating) into one document with, per batch
size and route, the median and min - max of the per-epoch times of each side, and the rule of DESIGN section 5: pair
handles take the bucket by default only if their median is below the faster parent route's median by more than the
parent's own run-to-run spread (max - min of that route) at both batch sizes."""
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

N_PAIRS, N_LO, N_HI, CUTOFF = 256, 100, 400, 10.0
ROUTES = ("collated_graph", "collated_eager", "handles")


def items(seed=0):
    """The pairs as the reference's LEP records: 1-D atom types, float32 positions, an integer label."""
    import lba_structures as ls
    from geossl_amd.Geom3D.dataloaders import Data
    rng = np.random.default_rng(seed)
    sizes = rng.integers(N_LO, N_HI + 1, size=(2, N_PAIRS))
    y = rng.integers(0, 2, size=N_PAIRS)
    out = []
    for m in range(N_PAIRS):
        d = {}
        for s, side in enumerate(("active", "inactive")):
            n = int(sizes[s, m])
            d["x_" + side] = torch.from_numpy(((np.arange(n, dtype=np.int64) * 7 + m) % 8) + 1)
            d["positions_" + side] = torch.from_numpy(ls.molecule(n, 90 + s, m))
        out.append(Data(y=torch.tensor([int(y[m])]), **d))
    return out, sizes


def modules(dev):
    from filler import fill_module_
    from geossl_amd.Geom3D.models import SchNet
    model = fill_module_(SchNet(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51,
                                cutoff=CUTOFF, node_class=9, readout="mean")).to(dev)
    head = fill_module_(torch.nn.Linear(256, 1)).to(dev)
    with torch.no_grad():
        head.weight.mul_(0.05)   # (logits of order one with the filler's weights)
    return model, head


def run(a):
    if not torch.cuda.is_available():
        raise SystemExit("bench_lep_bucket.py measures on the GPU: none found")
    from geossl_amd import build
    from geossl_amd.finetune_lep import LEPTrainer
    from geossl_amd.Geom3D import dataloaders as dl
    dev = "cuda:0"
    data, sizes = items()
    paired = getattr(dl, "PairedDeviceDataset", None)
    ds = paired.from_data_list(data, dev) if paired is not None else None
    lines = []
    for bs in a.bs:
        for route in a.routes:
            if route == "handles" and ds is None:
                continue
            torch.manual_seed(0)
            model, head = modules(dev)
            tr = LEPTrainer(model, head, lr=1e-5, model_3d="schnet", use_graph=route != "collated_eager")
            gen = torch.Generator().manual_seed(1)
            if route == "handles":
                loader = dl.DeviceLoader(ds, batch_size=bs, shuffle=True, drop_last=True, generator=gen)
            else:
                loader = dl.DataLoaderLEP(data, batch_size=bs, shuffle=True, drop_last=True, generator=gen)
            ms, caps, last, steps = [], [], None, 0
            for epoch in range(a.warmup_epochs + a.epochs):
                before = tr.step_graphs.captures
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps = 0
                for b in loader:
                    last = tr.step(b.to(dev))
                    steps += 1
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / steps * 1e3
                caps.append(tr.step_graphs.captures - before)
                if epoch >= a.warmup_epochs:
                    ms.append(round(dt, 4))
            kinds = sorted({str(k[0]) for k in tr.step_graphs.graphs})
            line = dict(bs=bs, route=route, steps_per_epoch=steps, ms_per_step=ms, ms_min_max=[min(ms), max(ms)],
                        captures_per_epoch=caps, graphs=len(tr.step_graphs), graph_kinds=kinds, last_loss=float(last))
            lines.append(line)
            print(json.dumps(line), flush=True)
            del tr, model, head, loader
            torch.cuda.empty_cache()
    return dict(tool="bench_lep_bucket", label=a.label, device=torch.cuda.get_device_name(0),
                GEOSSL_SPARSE_BUCKETS=os.environ.get("GEOSSL_SPARSE_BUCKETS"), source_hash=build.source_hash(),
                has_paired_dataset=ds is not None,
                config=dict(F=128, L=6, G=51, cutoff=CUTOFF, pairs=N_PAIRS, atoms_per_side=[N_LO, N_HI],
                            epochs=a.epochs, warmup_epochs=a.warmup_epochs), lines=lines)


def merge(paths):
    runs = [json.load(open(p)) for p in paths]
    side = lambda r: "parent" if r["label"].startswith("parent") else "new"
    cell = {}   # (bs, side, route name) -> {"ms": [...], "captures": [[...] per run], "kinds": set}
    for r in runs:
        for ln in r["lines"]:
            route = ln["route"]
            if side(r) == "new" and route == "collated_graph" and r["GEOSSL_SPARSE_BUCKETS"] == "1":
                route = "collated_bucket"
            c = cell.setdefault((ln["bs"], side(r), route), dict(ms=[], captures=[], kinds=set()))
            c["ms"] += ln["ms_per_step"]
            c["captures"].append(ln["captures_per_epoch"])
            c["kinds"] |= set(ln["graph_kinds"])
    summary, verdict = [], []
    for bs in sorted({k[0] for k in cell}):
        parent = {k[2]: v for k, v in cell.items() if k[0] == bs and k[1] == "parent"}
        fastest = min(parent, key=lambda n: statistics.median(parent[n]["ms"]))
        ref = parent[fastest]["ms"]
        spread = max(ref) - min(ref)
        for (b_, sd, route), v in sorted(cell.items()):
            if b_ != bs:
                continue
            summary.append(dict(bs=bs, side=sd, route=route, median_ms=round(statistics.median(v["ms"]), 4),
                                ms_min_max=[min(v["ms"]), max(v["ms"])], epochs=len(v["ms"]),
                                captures_per_epoch=v["captures"], graph_kinds=sorted(v["kinds"])))
        h = cell.get((bs, "new", "handles"))
        gain = None if h is None else statistics.median(ref) - statistics.median(h["ms"])
        verdict.append(dict(bs=bs, fastest_parent_route=fastest, fastest_parent_median_ms=round(statistics.median(ref), 4),
                            parent_spread_ms=round(spread, 4),
                            handles_median_ms=None if h is None else round(statistics.median(h["ms"]), 4),
                            handles_gain_ms=None if gain is None else round(gain, 4),
                            handles_beat_parent_by_more_than_its_spread=bool(gain is not None and gain > spread)))
    return dict(tool="bench_lep_bucket",
                what="runs on the parent commit (label parent_*) and on this one (label new_*: GEOSSL_SPARSE_BUCKETS unset "
                     "- pair handles through the bucket, collated batches as on the parent - and = 1 - collated batches "
                     "through the bucket too: route collated_bucket), alternating in one session on one MI355X; ms per "
                     "step per timed epoch, loader inside the timed region; captures_per_epoch includes the warm-up epochs",
                rule="pair handles take the bucket by default only if their median is below the faster parent route's "
                     "median by more than that route's own max - min, at both batch sizes",
                handles_default_on=all(v["handles_beat_parent_by_more_than_its_spread"] for v in verdict),
                verdict=verdict, summary=summary, runs=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--routes", nargs="*", default=list(ROUTES), choices=ROUTES)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--warmup-epochs", type=int, default=2)
    ap.add_argument("--label", default="")
    ap.add_argument("--merge", nargs="*", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = merge(a.merge) if a.merge else run(a)
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text if not a.merge else json.dumps(dict(handles_default_on=doc["handles_default_on"], verdict=doc["verdict"]),
                                               indent=1))


if __name__ == "__main__":
    main()
