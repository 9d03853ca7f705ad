#!/usr/bin/env python3
"""SchNet forward + backward per step on the sparse pair list against the dense pair-slot form.

    python tools/bench_sparse_pairs.py [--bs 128] [--steps 20] [--warmup 5] [--rounds 3] [--out profiles/NAME.json]

Batches of `bs` structures of 64, 128, 192 and 255 atoms (both branches, same batch, one process, the two branches
alternating round by round) and of 500 atoms (sparse alone: the dense form stops at 255), at cutoffs 5 A and 10 A, full
configuration (128 features, 6 blocks, 51 gaussians).  Structures: rejection sampling at pocket density (0.08 atoms per
cubic Angstrom, 1 A minimum separation), eight distinct pockets per size repeated over the batch, each copy shifted by
3 A times its index - the graphs, and so the work, are those of pockets of this density.

A step = forward, backward to the parameters, and a device synchronise; the time is a host clock around `steps` steps
that end in the synchronise, after `warmup` steps of the same shape.  Per line: milliseconds per step of either branch
(median and spread over the rounds), their ratio, the real number of pairs against the slots.  Needs the GPU: there is
no fallback.  Prints one JSON document; --out also writes it to a file."""
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

DENSITY, MIN_SEP = 0.08, 1.0


def pocket(n, seed):
    rng = np.random.default_rng(seed)
    side = (n / DENSITY) ** (1.0 / 3.0)
    pts = np.empty((n, 3))
    have = 0
    while have < n:
        p = rng.uniform(0.0, side, size=3)
        if have == 0 or np.min(np.sum((pts[:have] - p) ** 2, axis=1)) >= MIN_SEP ** 2:
            pts[have] = p
            have += 1
    return pts.astype(np.float32)


def make_batch(n, bs, dev):
    mols = [pocket(n, 1000 * n + k % 8) + np.float32(3.0 * k) for k in range(bs)]   # eight distinct pockets, shifted
    pos = torch.from_numpy(np.concatenate(mols)).to(dev)
    batch = torch.repeat_interleave(torch.arange(bs), n).to(dev)
    z = ((torch.arange(n * bs) * 7) % 8 + 1).to(dev)
    return z, pos, batch


def layout_of(batch, sizes, sparse):
    from geossl_amd.layout import MolLayout
    os.environ["GEOSSL_SPARSE_PAIRS"] = "1" if sparse else "0"
    try:
        return MolLayout(batch, len(sizes), sizes=sizes)
    finally:
        del os.environ["GEOSSL_SPARSE_PAIRS"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 128, 192, 255, 500])
    ap.add_argument("--cutoffs", type=float, nargs="*", default=[5.0, 10.0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_pairs.py measures on the GPU: none found")
    from filler import fill_module_
    from geossl_amd import build, ops
    from geossl_amd.Geom3D.models import SchNet
    dev = "cuda:0"
    lines = []
    for cutoff in a.cutoffs:
        model = fill_module_(SchNet(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51,
                                    cutoff=cutoff, node_class=9, readout="mean")).to(dev)
        for n in a.sizes:
            z, pos, batch = make_batch(n, a.bs, dev)
            sizes = [n] * a.bs
            branches = {"sparse": layout_of(batch, sizes, True)}
            if n <= 255:
                branches["dense"] = layout_of(batch, sizes, False)

            def step(lay):
                model.zero_grad(set_to_none=True)
                model(z, pos, batch, layout=lay).sum().backward()

            def timed(lay):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step(lay)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / a.steps * 1e3

            outs = {}
            for name, lay in branches.items():          # warm-up of every shape; the outputs for the agreement check
                for _ in range(a.warmup):
                    step(lay)
                with torch.no_grad():
                    outs[name] = model(z, pos, batch, layout=lay).double()
            ms = {name: [] for name in branches}
            for _ in range(a.rounds):                   # the branches alternate
                for name, lay in branches.items():
                    ms[name].append(timed(lay))
            n_pairs = int(ops.sparse_pair_geometry(pos, branches["sparse"], cutoff).n_pairs.item())
            line = dict(atoms=n, bs=a.bs, cutoff=cutoff, pairs=n_pairs, capacity=branches["sparse"].P,
                        slots=a.bs * n * (n - 1) // 2, steps=a.steps, rounds=a.rounds)
            for name in branches:
                line[name + "_ms"] = round(statistics.median(ms[name]), 4)
                line[name + "_ms_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
            if "dense" in branches:
                line["sparse_over_dense"] = round(line["sparse_ms"] / line["dense_ms"], 4)
                line["max_abs_diff_over_max"] = float((outs["sparse"] - outs["dense"]).abs().max()
                                                      / outs["dense"].abs().max())
            lines.append(line)
            print(json.dumps(line), flush=True)
            del branches, outs
            torch.cuda.empty_cache()
    doc = dict(tool="bench_sparse_pairs", device=torch.cuda.get_device_name(0), source_hash=build.source_hash(),
               config=dict(F=128, L=6, G=51), lines=lines)
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
