"""The end-to-end cases tests/test_gpu_vibrations.py runs against the twin, and what makes their starts comparable:
tests/test_vibrations_cpu.py checks on the CPU that every displaced image of every case keeps force_twin's cutoff margin
(a property of the inputs alone).  Backbones, modules and batches are those of tests/md_cases.py."""
import numpy as np
import torch

import force_twin as tw
import md_cases as mc
import vibrations_twin as vt

# name -> (backbone, sizes, start seed): the first seed from SEARCH_FROM on whose start (md_cases._raw) every image of
# every round at the default delta (0.00125 A) keeps tw.CUTOFF_MARGIN - `first_start`.
CASES = {"schnet_9": ("schnet", [9], 901), "schnet_ragged": ("schnet", [1, 2, 9, mc.N_ATOMS], 911),
         "painn_9x2": ("painn", [9, 9], 921)}
SEARCH_FROM = {"schnet_9": 901, "schnet_ragged": 911, "painn_9x2": 921}


def raw_of(name, seed=None):
    kind, sizes, s = CASES[name]
    return mc._raw(sizes, s if seed is None else seed, mc._cfg(kind)["cutoff"])


def images_margin(name, delta, seed=None):
    """The smallest cutoff margin over the 6 n_max displaced images of a case (C = 1: one coordinate per image pair)."""
    kind, sizes, _ = CASES[name]
    raw = raw_of(name, seed)
    cutoff = mc._cfg(kind)["cutoff"]
    best = np.inf
    for r in range(vt.rounds(sizes, 1)):
        for im in vt.images(raw["positions"], sizes, delta, 1, r):
            best = min(best, tw.cutoff_margin(im, raw["batch"], cutoff))
    return best


def first_start(name, delta):
    for seed in range(SEARCH_FROM[name], SEARCH_FROM[name] + 50):
        if images_margin(name, delta, seed) >= tw.CUTOFF_MARGIN:
            return seed
    raise AssertionError("no start whose images keep the cutoff margin")


class Twin:
    """The fp64 twin of a case: modules, start, masses, gradient(pos) -> dE/dpos [N, 3] in fp64 and the analytic Hessian."""

    def __init__(self, name, snapshot=None, device="cpu"):
        from geossl_amd.md import default_masses
        from oracle.graph import radius_graph_np
        self.kind, self.sizes, self.seed = CASES[name]
        self.cfg = mc._cfg(self.kind)
        self.raw = raw_of(name)
        if snapshot is None:
            snapshot = mc.module_snapshot(*mc.cpu_modules(self.kind, self.cfg))
        self.snapshot, self.device = snapshot, device
        self.z, self.mol = self.raw["x"][:, 0].copy(), self.raw["batch"]
        self.masses = default_masses(torch.from_numpy(self.z)).numpy()
        self._radius = radius_graph_np

    def edges(self, x):
        p32 = np.asarray(x, dtype=np.float32)
        return (tw.schnet_edges(p32, self.mol, self.cfg["cutoff"]) if self.kind == "schnet"
                else torch.from_numpy(self._radius(p32, self.cfg["cutoff"], self.mol)))

    def gradient(self, x):
        _, f = tw.predict(self.kind, mc._twin_cfg(self.kind, self.cfg), *self.snapshot, self.z, x, self.mol, self.edges(x),
                          device=self.device)
        return -f.numpy()

    def analytic_hessian(self):
        """torch.autograd.functional.hessian of the twin's summed energy at the start -> [B, M, M] blocks."""
        params, buffers, head = self.snapshot
        dd = dict(dtype=torch.float64, device=self.device)
        P = {k: v.detach().to(**dd) for k, v in list(params.items()) + list(buffers.items()) if v.is_floating_point()}
        Hd = {k: v.detach().to(**dd) for k, v in head.items()}
        x0 = torch.as_tensor(self.raw["positions"], dtype=torch.float32).to(**dd)
        z, mol = torch.as_tensor(self.z).to(self.device), torch.as_tensor(self.mol).to(self.device)
        ei = self.edges(self.raw["positions"]).to(self.device)
        cfg = mc._twin_cfg(self.kind, self.cfg)
        full = torch.autograd.functional.hessian(lambda x: tw._energy(self.kind, cfg, P, Hd, z, x, mol, ei).sum(), x0)
        N = x0.size(0)
        full = full.reshape(3 * N, 3 * N).cpu().numpy()
        M, ptr = 3 * max(self.sizes), vt.mol_ptr(self.sizes)
        out = np.zeros((len(self.sizes), M, M))
        for b, n in enumerate(self.sizes):
            out[b, :3 * n, :3 * n] = full[3 * ptr[b]:3 * ptr[b + 1], 3 * ptr[b]:3 * ptr[b + 1]]
        return out
