#!/usr/bin/env python3
"""Share of the dense pair slots that carry an edge (n_live / P of geossl_live_pairs_build) for the molecules bench.py
times: `python tools/live_share.py [mols=1024] [set=A] [cutoff=5.0]` - the clean view, the perturbed view (sigma = 0.3)
and the two-view batch the filter launches of a DDM step run on.  The perturbed view is drawn here (numpy, N(0, 0.3)
per coordinate), not by the trainer's device generator: the same distribution as a step's second view, not its draws."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    from geossl_amd import _lib, ops
    from geossl_amd.layout import MolLayout
    from geossl_amd.synthetic import make_molecules
    mols = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    molset = sys.argv[2] if len(sys.argv) > 2 else "A"
    cutoff = float(sys.argv[3]) if len(sys.argv) > 3 else 5.0
    _lib.load()
    dev = "cuda:0"
    m = make_molecules(mols, seed=1000, mode=molset)
    sizes = [int(n) for n in m["sizes"]]
    batch = torch.arange(len(sizes), device=dev).repeat_interleave(torch.tensor(sizes, device=dev))
    lay = MolLayout(batch, len(sizes), sizes=sizes)
    clean = torch.from_numpy(m["positions"]).to(dev)
    noise = torch.from_numpy(np.random.default_rng(1).normal(0.0, 0.3, size=m["positions"].shape).astype(np.float32)).to(dev)
    tot = [0, 0]
    for name, pos in (("clean view", clean), ("perturbed view (sigma 0.3)", clean + noise)):
        mol_live = torch.empty(lay.B, dtype=torch.int32, device=dev)
        d, c, fl = ops.pair_geometry(pos, lay, cutoff, mol_live=mol_live)
        lp = ops.live_pairs(d, c, fl, lay, mol_live, cutoff)
        n = int(lp.n_live)
        assert n == int((fl != 0).sum())
        tot[0] += n
        tot[1] += lay.P
        print("set %s, %d molecules, %.1f A, %-28s n_live / P = %d / %d = %.4f  (per molecule %d .. %d)"
              % (molset, mols, cutoff, name, n, lay.P, n / lay.P, int(mol_live.min()), int(mol_live.max())))
    print("two-view batch: n_live / P = %d / %d = %.4f, dead share %.4f" % (tot[0], tot[1], tot[0] / tot[1], 1 - tot[0] / tot[1]))


if __name__ == "__main__":
    main()
