#!/usr/bin/env python3
"""PaiNN training steps on shuffled pockets, loader included: ms per step and graph captures per epoch; and the cost of
the edge structures of such a batch.

    python tools/bench_painn_bucket.py [--bs 8 32] [--objectives supervised lep] [--routes ...] [--runs 3]
                                       [--warmup-runs 1] [--epochs 4] [--layout] [--label NAME] [--out FILE.json]

``SupervisedTrainer`` (512 pockets) and ``LEPTrainer`` (256 pairs) on PaiNN at the reference's defaults (128 features, 3
blocks, 20 radial functions, 5 A) over synthetic pockets of 100 to 500 atoms (tests/lba_structures.py: rejection sampling
at 0.08 atoms per cubic Angstrom, 1 A minimum separation), every structure's radius graph built once up front - on the
host records for the collated routes, in the device dataset for the handles.  Every epoch visits the structures in a
new shuffled order.  A route is ``<loader>_<mode>``:

* ``collated_eager`` / ``collated_graph``: the host concatenates the batch's structures and their edges and uploads
  them (what the reference's loaders do); the trainer with ``use_graph`` False / True;
* ``handles_graph``: ``DeviceLoader`` handles of a ``DeviceDataset`` / ``PairedDeviceDataset`` built with ``radius=``.

A suffix ``@1`` / ``@0`` runs the route with GEOSSL_PAINN_SPARSE_BUCKETS set to that value (no suffix: unset).  The
timed region is a run of ``--epochs`` whole epochs - the loader's work and ``trainer.step`` of every batch - between two
device synchronises, after ``--warmup-runs`` runs of the same kind: milliseconds per step per run, median and min - max
over the ``--runs`` timed runs.  Graph captures are counted per epoch (warm-up included); a route whose graphs are capacity buckets must capture
ONCE, in its first epoch: the tool exits with an error after writing its document when one did not.  Only public API is
used, so the file runs unchanged on the commit before the sparse PaiNN bucket (where the switch does nothing and a
paired dataset takes no ``radius=``: such routes are skipped and named).

``--layout``: HIP-event times of the edge structures of one batch of 8 and of 32 pockets - the launches of
``layout.EdgeLayout`` (its three entry points timed one by one, and the whole constructor with its cumsums and its
read-back) and, where the library has it, the one launch of ``ops.painn_incidence_layout``.
Needs the GPU.  Prints one JSON document; --out also writes it to a file."""
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

N_STRUCT, N_LO, N_HI, CUTOFF = 512, 100, 500, 5.0
SWITCH = "GEOSSL_PAINN_SPARSE_BUCKETS"
DEV = "cuda:0"


def structures(seed=0):
    """sizes [512], positions, atom types and - per structure, on the host - the radius graph at 5 A (local indices)."""
    import lba_structures as ls
    from geossl_amd import ops
    rng = np.random.default_rng(seed)
    sizes = rng.integers(N_LO, N_HI + 1, size=N_STRUCT)
    pos = [ls.molecule(int(n), 70, k) for k, n in enumerate(sizes)]
    x = [((np.arange(int(n), dtype=np.int64) * 7 + k) % 8) + 1 for k, n in enumerate(sizes)]
    edges = [ops.radius_graph(torch.from_numpy(p).to(DEV), CUTOFF).cpu().numpy() for p in pos]
    y = rng.standard_normal(N_STRUCT).astype(np.float32)
    return sizes, pos, x, edges, y


def collated_supervised(data, bs, order):
    """Batches of one epoch, collated on the host step by step (edges with their node offsets)."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.layout import prepare_batch
    sizes, pos, x, edges, y = data
    up = lambda a: torch.from_numpy(a).to(DEV, non_blocking=True)
    for k in range(len(order) // bs):
        ids = order[k * bs:(k + 1) * bs]
        n = sizes[ids]
        off = np.concatenate([[0], np.cumsum(n)[:-1]])
        bv = up(np.repeat(np.arange(bs, dtype=np.int64), n))
        b = pg.Batch(up(np.concatenate([x[i] for i in ids])[:, None]), up(np.concatenate([pos[i] for i in ids])), bv, None,
                     radius_edge_index=up(np.concatenate([edges[i] + o for i, o in zip(ids, off)], axis=1)),
                     num_graphs=bs, sizes=[int(v) for v in n])
        b.y = up(y[ids])
        prepare_batch(bv, None, b._sizes, lazy=True)
        yield b


def lep_items(data):
    """256 pairs of the structures (m, 256 + m) as the reference's LEP records, with their radius edges."""
    from geossl_amd.Geom3D.dataloaders import Data
    sizes, pos, x, edges, y = data
    M = N_STRUCT // 2
    f = torch.from_numpy
    return [Data(x_active=f(x[m]), positions_active=f(pos[m]), radius_edge_index_active=f(edges[m]),
                 x_inactive=f(x[M + m]), positions_inactive=f(pos[M + m]), radius_edge_index_inactive=f(edges[M + m]),
                 y=torch.tensor([int(y[m] > 0)])) for m in range(M)]


def modules(objective):
    from filler import fill_module_
    from geossl_amd.Geom3D.models import PaiNN
    model = fill_module_(PaiNN(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=CUTOFF, max_z=9, n_out=1,
                               readout="add")).to(DEV)
    if objective == "supervised":
        return model, fill_module_(model.create_output_layers()).to(DEV)
    head = fill_module_(torch.nn.Linear(256, 1)).to(DEV)
    with torch.no_grad():
        head.weight.mul_(0.05)   # (logits of order one with the filler's weights)
    return model, head


def epochs_of(objective, loader, bs, data, items, sets, gen):
    """A function that yields one epoch's batches of this route's loader."""
    from geossl_amd.Geom3D import dataloaders as dl
    if loader == "handles":
        dloader = dl.DeviceLoader(sets[objective], batch_size=bs, shuffle=True, drop_last=True, generator=gen)
        return lambda: iter(dloader)
    if objective == "supervised":
        return lambda: collated_supervised(data, bs, torch.randperm(N_STRUCT, generator=gen).numpy())
    lloader = dl.DataLoaderLEP(items, batch_size=bs, shuffle=True, drop_last=True, generator=gen)
    return lambda: (b.to(DEV) for b in lloader)


def device_sets(data, items):
    """The device-resident datasets of the handle routes; a name maps to None where this commit cannot build it."""
    from geossl_amd.Geom3D import dataloaders as dl
    sizes, pos, x, edges, y = data
    sets = {"supervised": dl.DeviceDataset(np.stack([np.concatenate(x), np.zeros(int(sizes.sum()), np.int64)], axis=1),
                                           np.concatenate(pos), sizes, DEV, radius=CUTOFF, y=y), "lep": None}
    paired = getattr(dl, "PairedDeviceDataset", None)
    try:
        sets["lep"] = paired.from_data_list(items, DEV, radius=CUTOFF)
    except TypeError:   # (a paired dataset without radius edges: the commit before the sparse PaiNN bucket)
        pass
    return sets


def run_routes(a, data):
    from geossl_amd.finetune_lep import LEPTrainer
    from geossl_amd.pretrain_Supervised import SupervisedTrainer
    items = lep_items(data)
    sets = device_sets(data, items)
    lines, skipped, broken = [], [], []
    for objective in a.objectives:
        for bs in a.bs:
            for route in a.routes:
                name, _, sw = route.partition("@")
                loader, mode = name.split("_")
                if loader == "handles" and sets[objective] is None:
                    skipped.append("%s %s: no radius edges in this commit's paired dataset" % (objective, route))
                    continue
                os.environ.pop(SWITCH, None)
                if sw:
                    os.environ[SWITCH] = sw
                torch.manual_seed(0)
                model, head = modules(objective)
                if objective == "supervised":
                    tr = SupervisedTrainer(model, head, 0.0, 1.0, task_id=0, loss="mse", lr=1e-5, model_3d="painn",
                                           use_graph=mode == "graph")
                else:
                    tr = LEPTrainer(model, head, lr=1e-5, model_3d="painn", use_graph=mode == "graph")
                epoch_batches = epochs_of(objective, loader, bs, data, items, sets, torch.Generator().manual_seed(1))
                ms, caps, last, steps = [], [], None, 0
                for run in range(a.warmup_runs + a.runs):   # a run: `--epochs` shuffled epochs between two synchronises
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    steps = 0
                    for _ in range(a.epochs):
                        before = tr.step_graphs.captures
                        for b in epoch_batches():
                            last = tr.step(b)
                            steps += 1
                        caps.append(tr.step_graphs.captures - before)
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) / steps * 1e3
                    if run >= a.warmup_runs:
                        ms.append(round(dt, 4))
                kinds = sorted({str(k[0]) for k in tr.step_graphs.graphs})
                line = dict(objective=objective, bs=bs, route=name, switch=sw or None, steps_per_run=steps,
                            ms_per_step=ms, ms_median=statistics.median(ms), ms_min_max=[min(ms), max(ms)],
                            captures_per_epoch=caps, graphs=len(tr.step_graphs), graph_kinds=kinds, last_loss=float(last))
                if kinds == ["bucket"] and (caps[0] != 1 or sum(caps[1:]) != 0):
                    broken.append("%s bs %d %s: captures per epoch %s" % (objective, bs, route, caps))
                lines.append(line)
                print(json.dumps(line), flush=True)
                del tr, model, head
                torch.cuda.empty_cache()
    os.environ.pop(SWITCH, None)
    return lines, skipped, broken


def event_ms(fn, reps=30, warm=5):
    """Median and min - max of HIP-event times around fn() (warm launches first; one sync per sample)."""
    out = []
    for k in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= warm:
            out.append(e0.elapsed_time(e1))
    return dict(median_ms=round(statistics.median(out), 5), min_max_ms=[round(min(out), 5), round(max(out), 5)])


def run_layout(data):
    """The edge structures of one batch of 8 and of 32 pockets: EdgeLayout's launches against the one-launch entry."""
    from geossl_amd import _lib, layout, ops
    out = []
    rng = np.random.default_rng(5)
    for bs in (8, 32):
        b = next(collated_supervised(data, bs, rng.permutation(N_STRUCT)))
        ei, bv, sizes = b.radius_edge_index, b.batch, b._sizes
        lay = layout.MolLayout(bv, sizes=sizes)
        line = dict(bs=bs, atoms=int(bv.numel()), edges=int(ei.size(1)), max_n=max(sizes))
        line["edge_layout_constructor"] = event_ms(lambda: layout.EdgeLayout(bv, ei, bs))
        names = ("geossl_super_edge_ptr", "geossl_incidence_count", "geossl_incidence_fill")
        sums = []
        for k in range(35):   # per entry point (bench.py's timers): 1 + 2 + 2 launches, without the two cumsums
            _lib.TIMERS = {n: [] for n in names}
            layout.EdgeLayout(bv, ei, bs)
            torch.cuda.synchronize()
            if k >= 5:
                sums.append(sum(e0.elapsed_time(e1) for evs in _lib.TIMERS.values() for e0, e1 in evs))
            _lib.TIMERS = None
        line["edge_layout_launches"] = dict(median_ms=round(statistics.median(sums), 5),
                                            min_max_ms=[round(min(sums), 5), round(max(sums), 5)])
        if hasattr(ops, "painn_incidence_layout"):
            N, E = int(bv.numel()), int(ei.size(1))
            bufs = (torch.empty(N + 1, dtype=torch.int64, device=DEV), torch.empty(E, dtype=torch.int32, device=DEV),
                    torch.empty(N + 1, dtype=torch.int64, device=DEV), torch.empty(E, dtype=torch.int32, device=DEV))
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            line["incidence_layout"] = event_ms(lambda: ops.painn_incidence_layout(ei, lay.mol_ptr, N, bs, max(sizes),
                                                                                   out=bufs, status=status))
            # (a bucket launches it at its capacities: the grid of the 512-atom class)
            line["incidence_layout_grid_512"] = event_ms(lambda: ops.painn_incidence_layout(ei, lay.mol_ptr, N, bs, 512,
                                                                                            out=bufs, status=status))
            assert int(status.item()) == 0
        out.append(line)
        print(json.dumps(line), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--objectives", nargs="*", default=["supervised", "lep"], choices=["supervised", "lep"])
    ap.add_argument("--routes", nargs="*", default=["collated_eager", "collated_graph", "handles_graph",
                                                    "collated_graph@1", "handles_graph@0"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup-runs", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=4, help="shuffled epochs per run")
    ap.add_argument("--layout", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_painn_bucket.py measures on the GPU: none found")
    from geossl_amd import build
    data = structures()
    lines, skipped, broken = run_routes(a, data) if a.routes else ([], [], [])
    doc = dict(tool="bench_painn_bucket", label=a.label, device=torch.cuda.get_device_name(0),
               source_hash=build.source_hash(),
               config=dict(F=128, L=3, R=20, cutoff=CUTOFF, structures=N_STRUCT, atoms=[N_LO, N_HI], runs=a.runs,
                           warmup_runs=a.warmup_runs, epochs_per_run=a.epochs),
               lines=lines, skipped=skipped, capture_rule_broken=broken)
    if a.layout:
        doc["layout"] = run_layout(data)
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)
    if broken:
        raise SystemExit("a bucket route did not capture once, in its first epoch: %s" % "; ".join(broken))


if __name__ == "__main__":
    main()
