"""The relaxation cases tests/test_gpu_relax.py runs against the twin, their starts and what the twin's own fp64 runs on the
CPU say about them; tests/test_relax_cpu.py checks every recorded figure here against such a run.  Backbones, modules and
batches are those of tests/md_cases.py.

A case is run twice on the device.  TRAJECTORY: from v = 0 with the tolerance TRAJ_FTOL (so low that every molecule of more
than one atom keeps moving), STEPS_A recorded steps, PRE_STEPS - STEPS_A unrecorded ones - by then the twin's dt has been
at dt_max for a few steps (n_min + 1 + 25 growths of 1.1 from 0.5 fs: step 32) - and STEPS_B recorded ones.  CONVERGENCE:
from v = 0 with the tolerance FRACTION x (the largest start fmax of the case's molecules) until the twin reports every
molecule converged; CONVERGE records that tolerance's step count, the device gets twice as many."""
import numpy as np
import torch

import force_twin as tw
import md_cases as mc
import md_twin as mt
import relax_twin as rt

STEPS_A, PRE_STEPS, STEPS_B = 24, 36, 12
TRAJ_FTOL = 1e-3
FRACTION = 0.6
SEARCH_MARGIN = mc.SEARCH_MARGIN
# name -> (backbone, sizes, start seed): the first seed from SEARCH_FROM (md_cases') on whose start the twin's trajectory
# keeps SEARCH_MARGIN on every checked frame (the STEPS_A + 1 and STEPS_B + 1 recorded ones, and the converged positions),
# stays below the head condition number at which an fp32 head can meet BOUNDS[kind]["energy"] (md_twin.head_condition_limit)
# and within the skip cap of relax_twin.check_history - `first_start`.  All properties of the fp64 twin alone.
CASES = {"schnet_B1": ("schnet", [mc.N_ATOMS], 801), "schnet_B4": ("schnet", [mc.N_ATOMS] * 4, 811),
         "schnet_ragged": ("schnet", [1, 2, 9, mc.N_ATOMS], 821),
         "painn_B1": ("painn", [mc.N_ATOMS], 832), "painn_B4": ("painn", [mc.N_ATOMS] * 4, 841)}
SEARCH_FROM = mc.SEARCH_FROM
# name -> the steps the twin needs until every molecule is converged at FRACTION of the start's largest fmax (`converge`)
CONVERGE = {"schnet_B1": 100, "schnet_B4": 106, "schnet_ragged": 111, "painn_B1": 62, "painn_B4": 59}


class Twin:
    """The fp64 twin of a case from `seed`: modules, start, masses and force(x) -> (E [B], F [N, 3])."""

    def __init__(self, name, seed=None, snapshot=None, device="cpu"):
        from geossl_amd.md import default_masses
        from oracle.graph import radius_graph_np
        self.kind, self.sizes, s = CASES[name]
        self.seed = s if seed is None else seed
        self.cfg = mc._cfg(self.kind)
        self.raw = mc._raw(self.sizes, self.seed, self.cfg["cutoff"])
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

    def force(self, x):
        e, f = tw.predict(self.kind, mc._twin_cfg(self.kind, self.cfg), *self.snapshot, self.z, x, self.mol, self.edges(x),
                          device=self.device)
        return e.numpy(), f.numpy()

    def margin(self, x):
        return tw.cutoff_margin(np.asarray(x, dtype=np.float32), self.mol, self.cfg["cutoff"])

    def condition(self, x):
        return mt.head_condition(self.kind, mc._twin_cfg(self.kind, self.cfg), *self.snapshot, self.z, x, self.mol,
                                 self.edges(x))

    def converge_ftol(self):
        return FRACTION * float(rt.minimize(self.raw["positions"], self.force, self.masses, self.mol, rt.params(), 0)[0]
                                ["fmax"].max())


def trajectory(twin):
    """The twin's own TRAJECTORY run -> (frames of stage A, frames of stage B): lists of relax_twin.minimize's dicts."""
    fr = rt.minimize(twin.raw["positions"], twin.force, twin.masses, twin.mol, rt.params(ftol=TRAJ_FTOL),
                     PRE_STEPS + STEPS_B)
    return fr[:STEPS_A + 1], fr[PRE_STEPS:]


def converge(twin, limit=400):
    """The twin's own CONVERGENCE run -> (tolerance, steps until every molecule is converged, its frames)."""
    ftol = twin.converge_ftol()
    fr = rt.minimize(twin.raw["positions"], twin.force, twin.masses, twin.mol, rt.params(ftol=ftol), limit,
                     until_converged=True)
    assert fr[-1]["done"].all(), "the twin does not converge within %d steps" % limit
    return ftol, len(fr) - 1, fr


def start_report(name, seed=None, with_convergence=True):
    """dict(margin, condition, checked, skipped, bad, dt_max_reached[, converge_steps, converge_margin, freeze_steps]) of
    the twin's own runs of a case from `seed`: what `start_ok` judges."""
    twin = Twin(name, seed)
    a, b = trajectory(twin)
    p = rt.params(ftol=TRAJ_FTOL)
    eps = tw.BOUNDS[twin.kind]["force"]
    checked = skipped = 0
    bad = []
    for frames in (a, b):
        c, s, bd = rt.check_history(frames, np.stack([f["F"] for f in frames]), twin.masses, twin.mol, p, eps,
                                    latched=frames[0]["done"] & (frames[0]["fmax"] >= p["ftol"]), exact_words=False)
        checked, skipped, bad = checked + c, skipped + s, bad + bd
    out = dict(margin=min(twin.margin(f["x"]) for f in a + b), condition=max(twin.condition(f["x"]) for f in a + b),
               checked=checked, skipped=skipped, bad=bad,
               dt_max_reached=bool((b[0]["dt"][np.asarray(twin.sizes) > 1] == p["dt_max"]).all()))
    if with_convergence:
        ftol, steps, fr = converge(twin)
        freeze = [next(k for k, f in enumerate(fr) if f["done"][m]) for m in range(len(twin.sizes))]
        out.update(converge_steps=steps, converge_margin=twin.margin(fr[-1]["x"]), freeze_steps=freeze,
                   energy_drop=(fr[0]["energy"] - fr[-1]["energy"]).tolist())
    return out


def start_ok(name, report):
    kind = CASES[name][0]
    limit = mt.head_condition_limit(kind, tw.BOUNDS[kind]["energy"])
    ok = (report["margin"] >= SEARCH_MARGIN and report["condition"] <= limit and report["bad"] == []
          and report["skipped"] * 10 <= report["checked"] and report["dt_max_reached"])
    if "converge_margin" in report:
        ok = ok and report["converge_margin"] >= SEARCH_MARGIN
    return ok


def first_start(name):
    for seed in range(SEARCH_FROM[name], SEARCH_FROM[name] + 50):
        if start_ok(name, start_report(name, seed)):
            return seed
    raise AssertionError("no start the twin can be compared on")
