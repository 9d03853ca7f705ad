#!/usr/bin/env python3
"""PaiNN on pocket-sized structures: today's interaction kernels against the atom-tile kernels (csrc/painn_tile.hip).

    python tools/bench_painn_tile.py --part launches [--out FILE]
    python tools/bench_painn_tile.py --part steps [--settings 0 1] [--tree CHECKOUT --label parent] [--out FILE]
    python tools/bench_painn_tile.py --part occupancy [--out FILE]                       (no GPU: compiles the file)
    python tools/bench_painn_tile.py --merge FILE ... --out profiles/painn_tile_bench.json

Workload: the synthetic pockets of tools/bench_lep.py (tests/lba_structures.py: 0.08 atoms per cubic Angstrom), 100 ... 500
atoms, 8 and 32 structures (LEP: pairs, 100 ... 400 atoms per side as in bench_lep), PaiNN at 128 features, 20 radial
functions, three blocks, 5 A.

  launches   one eager forward + backward of the backbone per pass; device events around every geossl_painn_interaction_*
             call, after warm-up: microseconds per call, per setting of GEOSSL_PAINN_TILE.
  steps      SupervisedTrainer (LBA) and LEPTrainer steps (forward, backward, Adam), eager and as a replayed per-structure
             graph, one fixed batch per (trainer, batch size).  The settings of GEOSSL_PAINN_TILE alternate run by run in
             one process (a trainer per setting, same weights); per line the median and min - max of `--runs` runs of
             `--steps` steps, host clock around steps that end in a device synchronise.  --tree: import geossl_amd from
             another built checkout (the parent commit, which has no switch: --settings with one empty entry).
  occupancy  registers, LDS and waves per SIMD of the R = 20 instantiations from -Rpass-analysis=kernel-resource-usage.
  --merge    one document from the parts, with the rule for the default applied: the unset switch takes the tile kernels
             above 255 atoms only if the `1` step's range lies below the parent's range at both batch sizes for at least
             one (trainer, mode), and above the parent's at none.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PAINN = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")


def _set(setting):
    if setting == "":
        os.environ.pop("GEOSSL_PAINN_TILE", None)
    else:
        os.environ["GEOSSL_PAINN_TILE"] = setting


def lba_batch(bs, dev, seed):
    import numpy as np
    import torch
    import lba_structures as ls
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    rng = np.random.default_rng(seed)
    sizes = rng.integers(100, 501, size=bs).astype(np.int64)
    d = ls.structures(sizes, seed + 1)
    pos, bvec = torch.from_numpy(d["positions"]).to(dev), torch.from_numpy(d["batch"]).to(dev)
    b = pg.Batch(torch.from_numpy(d["x"]).to(dev)[:, None].contiguous(), pos, bvec, None,
                 radius_edge_index=ops.radius_graph(pos, PAINN["cutoff"], bvec), num_graphs=bs,
                 sizes=tuple(int(n) for n in sizes))
    b.y = torch.from_numpy(rng.normal(size=bs).astype(np.float32)).to(dev)
    return b, sizes


def painn(dev):
    from filler import fill_module_
    from geossl_amd.Geom3D.models import PaiNN
    return fill_module_(PaiNN(**PAINN)).to(dev)


def part_launches(a):
    import torch
    import geossl_amd.Geom3D.models.painn as pm
    dev, lines, real = "cuda:0", [], pm.call
    for bs in a.bs:
        batch, sizes = lba_batch(bs, dev, 700 + bs)
        model = painn(dev)
        for setting in a.settings:
            _set(setting)
            events = []

            def timed_call(name, *args):
                if not name.startswith("geossl_painn_interaction_"):
                    return real(name, *args)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = real(name, *args)
                e1.record()
                events.append((name, e0, e1))
                return r

            def one_pass():
                model.zero_grad(set_to_none=True)
                out = model(batch.x, batch.positions, batch.radius_edge_index, batch.batch)
                (out ** 2).sum().backward()

            for _ in range(a.warmup):
                one_pass()
            pm.call = timed_call
            try:
                for _ in range(a.steps):
                    one_pass()
            finally:
                pm.call = real
            torch.cuda.synchronize()
            per = {}
            for name, e0, e1 in events:
                per.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
            fwd = sum(sum(v) for k, v in per.items() if "_fwd" in k) / (a.steps * PAINN["n_interactions"])
            bwd = sum(sum(v) for k, v in per.items() if "_bwd" in k) / (a.steps * PAINN["n_interactions"])
            line = dict(part="launches", bs=bs, atoms=int(sizes.sum()), max_atoms=int(sizes.max()), setting=setting,
                        passes=a.steps, forward_us_per_block=round(fwd, 2), backward_us_per_block=round(bwd, 2),
                        calls={k: dict(n_per_pass=len(v) // a.steps, median_us=round(statistics.median(v), 2),
                                       min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in sorted(per.items())})
            lines.append(line)
            print(json.dumps(line), flush=True)
    return lines


def part_steps(a):
    import torch
    import bench_lep
    if a.tree:   # (bench_lep puts its own checkout in front when imported: the tree under test goes before it)
        sys.path[:0] = [a.tree, os.path.join(a.tree, "tests"), os.path.join(a.tree, "tests", "golden")]
    from filler import fill_module_
    from geossl_amd.finetune_lep import LEPTrainer
    from geossl_amd.pretrain_Supervised import SupervisedTrainer
    dev, lines = "cuda:0", []
    for trainer in ("lba", "lep"):
        for bs in a.bs:
            if trainer == "lba":
                batch, sizes = lba_batch(bs, dev, 700 + bs)
                atoms, max_atoms = int(sizes.sum()), int(sizes.max())
            else:
                batch = bench_lep.make_batch("painn", bs, dev, seed=400 + bs)
                atoms = int(batch.batch_active.numel() + batch.batch_inactive.numel())
                max_atoms = int(max(batch._sizes_active.max(), batch._sizes_inactive.max()))
            fns = {}
            for mode, use_graph in (("eager", False), ("graph", True)):
                for setting in a.settings:
                    _set(setting)
                    model = painn(dev)
                    if trainer == "lba":
                        head = fill_module_(model.create_output_layers()).to(dev)
                        tr = SupervisedTrainer(model, head, 0.1, 1.3, task_id=0, loss="mse", lr=a.lr, model_3d="painn",
                                               use_graph=use_graph, graph_mode="structure")
                    else:
                        head = fill_module_(torch.nn.Linear(256, 1)).to(dev)
                        with torch.no_grad():
                            head.weight.mul_(0.05)
                        tr = LEPTrainer(model, head, lr=a.lr, model_3d="painn", use_graph=use_graph, graph_mode="structure")
                    fns[(mode, setting)] = (lambda tr=tr: tr.step(batch))
                    first = None
                    for _ in range(a.warmup):     # (a graph is captured here, under this setting)
                        loss = fns[(mode, setting)]()
                        first = float(loss) if first is None else first
                    fns[(mode, setting, "loss")] = first
            for mode in ("eager", "graph"):
                ms = {s: [] for s in a.settings}
                for _ in range(a.runs):           # the settings alternate
                    for s in a.settings:
                        _set(s)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(a.steps):
                            fns[(mode, s)]()
                        torch.cuda.synchronize()
                        ms[s].append((time.perf_counter() - t0) / a.steps * 1e3)
                for s in a.settings:
                    line = dict(part="steps", label=a.label, trainer=trainer, mode=mode, bs=bs, atoms=atoms,
                                max_atoms=max_atoms, setting=s, steps=a.steps, runs=a.runs,
                                ms=round(statistics.median(ms[s]), 4), ms_min_max=[round(min(ms[s]), 4), round(max(ms[s]), 4)],
                                first_loss=fns[(mode, s, "loss")])
                    lines.append(line)
                    print(json.dumps(line), flush=True)
            del fns, batch
            torch.cuda.empty_cache()
    return lines


def part_occupancy(a):
    src = os.path.join(REPO, "geossl_amd", "csrc", "painn_tile.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I",
           os.path.join(REPO, "include"), "-I", os.path.dirname(src), "-Wno-pass-failed", "-fno-slp-vectorize",
           "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    lines, cur = [], None
    for ln in text.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            k = re.search(r"(k_painn_(?:fwd|bwd)_tile)ILi(\d+)ELb([01])E", m.group(1))
            cur = dict(part="occupancy", kernel="%s<%s, %s>" % (k.group(1), k.group(2), "true" if k.group(3) == "1" else "false")) \
                if k and k.group(2) == "20" else None
            if cur:
                lines.append(cur)
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch_bytes", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, ln)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    assert len(lines) == 4 and all(l["scratch_bytes"] == 0 for l in lines), lines
    for l in lines:
        print(json.dumps(l))
    return lines


def decide(lines):
    """The rule for the unset default, on the step lines: label 'parent' against setting '1' of label 'this'."""
    by = {(l["label"], l["setting"], l["trainer"], l["mode"], l["bs"]): l["ms_min_max"] for l in lines if l["part"] == "steps"}
    groups = sorted({(k[2], k[3]) for k in by})
    sizes = sorted({k[4] for k in by})
    below, above = [], []
    for tr, mode in groups:
        cmp_ = [(by.get(("parent", "", tr, mode, bs)), by.get(("this", "1", tr, mode, bs))) for bs in sizes]
        if any(p is None or t is None for p, t in cmp_):
            return dict(default_on=False, reason="incomplete: parent or tile lines missing")
        if all(t[1] < p[0] for p, t in cmp_):
            below.append([tr, mode])
        above += [[tr, mode, bs] for bs, (p, t) in zip(sizes, cmp_) if t[0] > p[1]]
    return dict(default_on=bool(below) and not above, tile_range_below_parent_at_every_size=below,
                tile_range_above_parent=above)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["launches", "steps", "occupancy"])
    ap.add_argument("--merge", nargs="*")
    ap.add_argument("--bs", type=int, nargs="*", default=[8, 32])
    ap.add_argument("--settings", nargs="*", default=["0", "1"])
    ap.add_argument("--tree", default=None)
    ap.add_argument("--label", default="this")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.tree = os.path.abspath(a.tree) if a.tree else None
    if a.merge is not None:
        lines = []
        for path in a.merge:
            with open(path) as fh:
                lines += json.load(fh)["lines"]
        doc = dict(tool="bench_painn_tile", config=PAINN, rule=decide(lines), lines=lines)
    else:
        if a.part == "occupancy":
            lines = part_occupancy(a)
            doc = dict(lines=lines)
        else:
            tree = a.tree or REPO
            sys.path[:0] = [HERE, tree, os.path.join(tree, "tests"), os.path.join(tree, "tests", "golden")]
            import torch
            if not torch.cuda.is_available():
                raise SystemExit("bench_painn_tile.py measures on the GPU: none found")
            from geossl_amd import build
            lines = part_launches(a) if a.part == "launches" else part_steps(a)
            doc = dict(device=torch.cuda.get_device_name(0), source_hash=build.source_hash(), lines=lines)
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
