#!/usr/bin/env python3
"""ms per step and molecules/s of the DDM step (DDMTrainer, graphs on, device noise) on SAMPLED atom tuples
(the reference's --distance_sample_ratio: AtomTupleExtractor(ratio), pretrain_GeoSSL.py:295), loader inside the timed
region, on shuffled epochs of set C molecules (Molecule3D with hydrogens, synthetic.molecule_sizes).

    python tools/bench_sampled_tuples.py [--models schnet painn] [--bs 128 1024] [--ratios 1 0.3 0.1]
                                         [--routes handles collated] [--steps 30] [--warmup 8] [--root TREE] [--tag NAME]
    python tools/bench_sampled_tuples.py --aggregate RUN.jsonl [RUN.jsonl ...] --out profiles/sampled_tuples_bench.json
    python tools/bench_sampled_tuples.py --kernel

Routes:
  handles   DeviceLoader(tuple_ratio=ratio): tuples drawn on the device, one sampled capacity-bucket graph
  collated  DataLoaderAtomTuple over host molecules with AtomTupleExtractor(ratio) as the per-molecule transform, then
            ``batch.to(device)`` - the reference's loader.  Which graph serves such a batch is the library's routing
            (GEOSSL_SAMPLED_BUCKETS; the line records the switch and whether a bucket graph served the run).
--root: the tree whose ``geossl_amd`` is measured (a checkout of the parent commit with its library built: only the
collated route exists there).  One JSON line per (model, batch size, ratio, route); run the tool once per run and tree,
alternating, and --aggregate the files: median (min - max) over the runs per configuration, the ratio-0.1 step against the
ratio-1 step of the same build and against the parent's step at the same ratio.
--kernel: microseconds of geossl_sampled_tuples alone (HIP events around the launch inside Bucket.fill, median of 20 fills)
for 1024 set C molecules and for ONE 255-atom molecule, whose incidence fill walks all its tuples with one thread per atom.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _HostMolecules(torch.utils.data.Dataset):
    """Per-molecule records with the extractor as the transform of every fetch (Molecule3DDataset.__getitem__)."""

    def __init__(self, mols, transform, edges=None):
        from geossl_amd.Geom3D.dataloaders.dataloaders_AtomTuple import Data
        self.Data, self.transform = Data, transform
        off = np.concatenate([[0], np.cumsum(mols["sizes"])])
        x, pos = torch.from_numpy(mols["x"]), torch.from_numpy(mols["positions"])
        self.items = [(x[off[i]:off[i + 1]], pos[off[i]:off[i + 1]], None if edges is None else edges[i])
                      for i in range(len(mols["sizes"]))]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        x, pos, rei = self.items[i]
        d = self.Data(x=x, positions=pos)
        if rei is not None:
            d.radius_edge_index = rei
        return self.transform(d)


def _local_edges(ds):
    """The device dataset's radius edges per molecule, local atom indices, on the host."""
    e, off = ds.edges.cpu(), ds.off
    return [e[:, ds.edge_off[i]:ds.edge_off[i + 1]] - int(off[i]) for i in range(len(ds))]


def run(model_3d, bs, ratio, route, steps, warmup, mols, dev="cuda:0"):
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    from geossl_amd.Geom3D.dataloaders.dataloaders_AtomTuple import AtomTupleExtractor, DataLoaderAtomTuple
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    from geossl_amd.NCSN import NCSN_version_03
    torch.manual_seed(1234)
    np.random.seed(1234)
    if model_3d == "painn":
        model = PaiNN(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add").to(dev)
    else:
        model = SchNet(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0,
                       node_class=9, readout="mean").to(dev)
    n1 = NCSN_version_03(128, 10.0, 0.01, 50, "symmetry", 2).to(dev)
    n2 = NCSN_version_03(128, 10.0, 0.01, 50, "symmetry", 2).to(dev)
    tr = pg.DDMTrainer(model, n1, n2, lr=5e-4, mu=0.0, sigma=0.3, device_noise=True, model_3d=model_3d, use_graph=True)
    ds = DeviceDataset.from_numpy(mols, dev, **({"radius": 5.0} if model_3d == "painn" else {}))
    gen = torch.Generator().manual_seed(5)
    if route == "handles":
        kw = {"tuple_ratio": ratio} if ratio < 1 else {}
        loader = DeviceLoader(ds, batch_size=bs, shuffle=True, drop_last=True, generator=gen, **kw)
    else:
        host = _HostMolecules(mols, AtomTupleExtractor(ratio, "combination"),
                              _local_edges(ds) if model_3d == "painn" else None)
        loader = DataLoaderAtomTuple(host, batch_size=bs, shuffle=True, drop_last=True, generator=gen)

    def batches():
        while True:
            for b in loader:
                yield b.to(dev)
    it = batches()
    for _ in range(warmup):
        tr.step(next(it))
    torch.cuda.synchronize()
    mol_count, tuples = 0, 0
    t0 = time.perf_counter()
    for _ in range(steps):
        b = next(it)
        loss = tr.step(b)
        mol_count += b.num_graphs
        tuples += b.n_super if route == "handles" else b.super_edge_index.size(1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    keys = list(tr.step_graphs.graphs)
    return {"model": model_3d, "bs": bs, "ratio": ratio, "route": route, "ms_per_step": round(1e3 * dt / steps, 4),
            "molecules_per_s": round(mol_count / dt, 1), "tuples_per_molecule": round(tuples / mol_count, 1),
            "steps": steps, "warmup": warmup, "captures": tr.step_graphs.captures,
            "bucket_graph": bool(keys) and all(isinstance(k, tuple) and k and k[0] == "bucket" for k in keys),
            "GEOSSL_SAMPLED_BUCKETS": os.environ.get("GEOSSL_SAMPLED_BUCKETS"), "final_loss": float(loss)}


def kernel_times(dev="cuda:0"):
    from geossl_amd import _lib, bucket as bk
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    from geossl_amd.synthetic import make_molecules
    cases = [("1024 set C molecules", make_molecules(1024, seed=7, mode="C"), "combination", r) for r in (0.3, 0.1)]
    big = make_molecules(0, seed=7, sizes=[255])
    cases += [("one 255-atom molecule", big, o, r) for o, r in (("combination", 0.5), ("permutation", 0.1),
                                                                ("permutation", 0.5))]
    for what, mols, option, ratio in cases:
        ds = DeviceDataset.from_numpy(mols, dev, option=option)
        np.random.seed(1)
        (hb,) = list(DeviceLoader(ds, batch_size=len(ds), shuffle=False, tuple_ratio=ratio))
        bkt = bk.Bucket.for_batch(hb, bk.option_of(hb), "schnet", 1)
        bkt.fill(hb)
        _lib.TIMERS = {"geossl_sampled_tuples": []}
        for _ in range(20):
            bkt.fill(hb)
        torch.cuda.synchronize()
        us = sorted(1e3 * a.elapsed_time(b) for a, b in _lib.TIMERS["geossl_sampled_tuples"])
        _lib.TIMERS = None
        print(json.dumps({"kernel": "geossl_sampled_tuples", "case": what, "option": option, "ratio": ratio,
                          "tuples": hb.n_super, "us_median": round(float(np.median(us)), 1), "us_min": round(us[0], 1),
                          "us_max": round(us[-1], 1)}), flush=True)


def aggregate(files, out):
    rows = {}
    for path in files:
        with open(path) as fh:
            for line in fh:
                if line.startswith("{"):
                    r = json.loads(line)
                    key = (r["tag"], r["model"], r["bs"], r["ratio"], r["route"], r["GEOSSL_SAMPLED_BUCKETS"])
                    rows.setdefault(key, []).append(r)
    table = []
    for key, rs in sorted(rows.items(), key=lambda kv: tuple(str(v) for v in kv[0])):
        ms, mps = sorted(r["ms_per_step"] for r in rs), sorted(r["molecules_per_s"] for r in rs)
        table.append(dict(zip(("tag", "model", "bs", "ratio", "route", "GEOSSL_SAMPLED_BUCKETS"), key),
                          runs=len(rs), ms_per_step_median=float(np.median(ms)), ms_per_step_min=ms[0], ms_per_step_max=ms[-1],
                          molecules_per_s_median=float(np.median(mps)), bucket_graph=all(r["bucket_graph"] for r in rs),
                          tuples_per_molecule=rs[0]["tuples_per_molecule"], steps=rs[0]["steps"]))
    doc = {"what": "DDM step on sampled atom tuples: tools/bench_sampled_tuples.py, loader inside the timed region, "
                   "set C molecules, median (min - max) over the runs of one configuration",
           "rows": table}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    for r in table:
        print("%-7s %-6s bs %4d ratio %.1f %-8s switch %-4s  %8.3f (%.3f - %.3f) ms  %9.0f mol/s  bucket %s"
              % (r["tag"], r["model"], r["bs"], r["ratio"], r["route"], r["GEOSSL_SAMPLED_BUCKETS"], r["ms_per_step_median"],
                 r["ms_per_step_min"], r["ms_per_step_max"], r["molecules_per_s_median"], r["bucket_graph"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["schnet", "painn"])
    ap.add_argument("--bs", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--ratios", type=float, nargs="+", default=[1.0, 0.3, 0.1])
    ap.add_argument("--routes", nargs="+", default=["handles", "collated"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--dataset-mols", type=int, default=8192)
    ap.add_argument("--root", default=REPO)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--aggregate", nargs="+")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sampled_tuples_bench.json"))
    a = ap.parse_args()
    if a.aggregate:
        return aggregate(a.aggregate, a.out)
    sys.path.insert(0, os.path.abspath(a.root))
    from geossl_amd import _lib
    from geossl_amd.synthetic import make_molecules
    _lib.load()
    if a.kernel:
        return kernel_times()
    mols = make_molecules(a.dataset_mols, seed=7, mode="C")
    for model_3d in a.models:
        for bs in a.bs:
            for ratio in a.ratios:
                for route in a.routes:
                    # (a collated step is bound by the host's per-molecule enumeration: fewer of them tell as much)
                    steps = a.steps if route == "handles" else max(16, a.steps * 128 // bs)
                    warm = a.warmup if route == "handles" else max(3, a.warmup // 2)
                    r = run(model_3d, bs, ratio, route, steps, warm, mols)
                    print(json.dumps(dict({"tag": a.tag}, **r)), flush=True)


if __name__ == "__main__":
    main()
