#!/usr/bin/env python3
"""Supervised (LBA) training steps on shuffled pockets, loader included: ms per step and graph captures per epoch.

    python tools/bench_sparse_bucket.py [--bs 8 32] [--epochs 3] [--warmup-epochs 2] [--label NAME] [--out FILE.json]

``SupervisedTrainer(model, head, 0.0, 1.0, task_id=0, loss="mse", use_graph=True)`` - the trainer of finetune_lba.py - at
128 features, 6 blocks, 51 gaussians, cutoff 10 A, on a synthetic pocket dataset of 512 structures with 100 to 500 atoms
(the generator of tools/bench_sparse_pairs.py: rejection sampling at 0.08 atoms per cubic Angstrom, 1 A minimum
separation).  Every epoch visits the structures in a new shuffled order, so no two batches share a size sequence.  Two
loaders per batch size:

* "collated": the host concatenates the batch's structures (numpy), uploads them and attaches the host sizes - what a
  ``DataLoader`` with a collate function does;
* "device": ``DeviceLoader`` handles of a ``DeviceDataset`` that holds the structures and their targets in HBM.

The timed region is a whole epoch - the loader's work and ``trainer.step`` of every batch - between two device
synchronises, after ``--warmup-epochs`` epochs of the same kind; the result is milliseconds per step per epoch.  The
number of graphs captured in every epoch (warm-up included) is reported beside it.  Only public API is used: the file
runs unchanged on a commit without the sparse bucket, where such batches run as eager launches.  Which batches take the
bucket is the library's choice (GEOSSL_SPARSE_BUCKETS, recorded in the document: unset serves DeviceLoader handles, 1
collated batches too, 0 neither).  Needs the GPU.  Prints one JSON document; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "golden"),
                os.path.dirname(os.path.abspath(__file__))]

N_STRUCT, N_LO, N_HI, CUTOFF = 512, 100, 500, 10.0


def dataset(seed=0):
    from bench_sparse_pairs import pocket
    rng = np.random.default_rng(seed)
    sizes = rng.integers(N_LO, N_HI + 1, size=N_STRUCT)
    pos = [pocket(int(n), 7000 + k) for k, n in enumerate(sizes)]
    x = [((np.arange(int(n), dtype=np.int64) * 7 + k) % 8) + 1 for k, n in enumerate(sizes)]
    y = rng.standard_normal(N_STRUCT).astype(np.float32)
    return sizes, pos, x, y


def collated_epoch(data, bs, order, dev):
    """Batches of one epoch, collated on the host step by step."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.layout import prepare_batch
    sizes, pos, x, y = data
    for k in range(len(order) // bs):
        ids = order[k * bs:(k + 1) * bs]
        n = sizes[ids]
        bv = torch.from_numpy(np.repeat(np.arange(bs, dtype=np.int64), n)).to(dev, non_blocking=True)
        b = pg.Batch(torch.from_numpy(np.concatenate([x[i] for i in ids])).to(dev, non_blocking=True),
                     torch.from_numpy(np.concatenate([pos[i] for i in ids])).to(dev, non_blocking=True),
                     bv, None, num_graphs=bs, sizes=[int(v) for v in n])
        b.y = torch.from_numpy(y[ids]).to(dev, non_blocking=True)
        prepare_batch(bv, None, b._sizes, lazy=True)
        yield b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--warmup-epochs", type=int, default=2)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_bucket.py measures on the GPU: none found")
    from filler import fill_module_
    from geossl_amd import build
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    from geossl_amd.Geom3D.models import SchNet
    from geossl_amd.pretrain_Supervised import SupervisedTrainer
    dev = "cuda:0"
    data = dataset()
    sizes, pos, x, y = data
    ds = DeviceDataset(np.concatenate(x)[:, None], np.concatenate(pos), sizes, dev, y=y)
    lines = []
    for bs in a.bs:
        for loader in ("collated", "device"):
            torch.manual_seed(0)
            model = fill_module_(SchNet(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51,
                                        cutoff=CUTOFF, node_class=9, readout="mean")).to(dev)
            head = fill_module_(torch.nn.Linear(128, 1)).to(dev)
            tr = SupervisedTrainer(model, head, 0.0, 1.0, task_id=0, loss="mse", lr=1e-5, use_graph=True)
            gen = torch.Generator().manual_seed(1)
            dl = DeviceLoader(ds, batch_size=bs, shuffle=True, drop_last=True, generator=gen)
            ms, caps, last = [], [], None
            for epoch in range(a.warmup_epochs + a.epochs):
                before = tr.step_graphs.captures
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps = 0
                if loader == "collated":
                    order = torch.randperm(N_STRUCT, generator=gen).numpy()
                    batches = collated_epoch(data, bs, order, dev)
                else:
                    batches = iter(dl)
                for b in batches:
                    last = tr.step(b)
                    steps += 1
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / steps * 1e3
                caps.append(tr.step_graphs.captures - before)
                if epoch >= a.warmup_epochs:
                    ms.append(round(dt, 4))
            keys = sorted({str(k[0]) for k in tr.step_graphs.graphs})
            line = dict(bs=bs, loader=loader, steps_per_epoch=steps, ms_per_step=ms, ms_min_max=[min(ms), max(ms)],
                        captures_per_epoch=caps, graphs=len(tr.step_graphs), graph_kinds=keys,
                        last_loss=float(last))
            lines.append(line)
            print(json.dumps(line), flush=True)
            del tr, model, head
            torch.cuda.empty_cache()
    doc = dict(tool="bench_sparse_bucket", label=a.label, device=torch.cuda.get_device_name(0),
               GEOSSL_SPARSE_BUCKETS=os.environ.get("GEOSSL_SPARSE_BUCKETS"),
               source_hash=build.source_hash(), config=dict(F=128, L=6, G=51, cutoff=CUTOFF, structures=N_STRUCT,
                                                            atoms=[N_LO, N_HI], epochs=a.epochs,
                                                            warmup_epochs=a.warmup_epochs),
               lines=lines)
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
