"""The trajectory cases tests/test_gpu_md.py runs against the twin, their starts and the helpers both MD test files
share: tests/test_md_cpu.py checks on the CPU that the twin's own fp64 trajectory of every case keeps the cutoff margin
on every frame.  The configurations are the MD17 ones of tests/test_gpu_md17.py, restated so that no test module
imports another."""
import math

import torch

import force_twin as tw
import md_twin as mt

N_ATOMS = 21
SCHNET_MD17 = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0,
                   readout="mean", node_class=9)
PAINN_MD17 = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")
NORMALS_SEED = 20240611   # the seed of the device stream's statistics (test_gpu_md.py) and of their numpy restatement


def _cfg(kind):
    return dict(SCHNET_MD17 if kind == "schnet" else PAINN_MD17)


def _twin_cfg(kind, cfg):
    keys = (("num_interactions", "cutoff", "readout") if kind == "schnet"
            else ("n_atom_basis", "n_interactions", "cutoff", "readout"))
    return {k: cfg[k] for k in keys}


def _raw(sizes, seed, cutoff):
    """make_batch over `sizes`: the first seed from `seed` on whose pairs all keep the twin's cutoff margin."""
    from geossl_amd.synthetic import make_batch
    for s in range(seed, seed + 50):
        r = make_batch(0, seed=s, sizes=sizes)
        if tw.cutoff_margin(r["positions"], r["batch"], cutoff) >= tw.CUTOFF_MARGIN:
            return r
    raise AssertionError("no seed with a cutoff margin")


def device_modules(kind, cfg, device):
    model, head = cpu_modules(kind, cfg)
    return model.to(device), head.to(device)


def device_batch(kind, cfg, raw, device):
    """The collated batch of the reference's MD17 loaders: 1-D x, host sizes, PaiNN with the frame's own radius list."""
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    bt = pg.Batch.from_numpy(dict(raw, x=raw["x"][:, 0].copy()), device)
    if kind == "painn":
        bt.radius_edge_index = ops.radius_graph(bt.positions, cfg["cutoff"], bt.batch)
    return bt


def module_snapshot(model, head):
    p, b = tw.module_tensors(model)
    return p, b, tw.module_tensors(head)[0]

DT, STEPS, T0, THERMOSTAT_SEED = 0.5, 12, 300.0, 99
LANGEVIN = ("langevin", 300.0, 0.01)
SEARCH_MARGIN = 2 * tw.CUTOFF_MARGIN   # of the twin's frames: the fp32 run's frames lie within 1e-5 A of them
# name -> (backbone, sizes, start seed): the first seed from SEARCH_FROM on whose start (_raw) and whose twin
# trajectories, NVE and Langevin, keep SEARCH_MARGIN and stay below the head condition number at which an fp32 energy
# head can meet BOUNDS[kind]["energy"] at all (md_twin.head_condition_limit) - `first_start`.  Both are properties of
# the fp64 twin alone.  Why the second: the energy bound is relative to max |E|, and a molecule whose energy is a near
# cancellation of the head's terms (seed 831: E = -2.8 from terms of 44, kappa 16 against a limit of 4.2) asks of the
# fp32 head more than fp32 arithmetic holds - measured there, the recorded energies were off by up to 2.4e-6 of the 2e-6
# allowed, the head's own rounding 8e-7 ... 2.2e-6 of it and the backbone's latent under 4e-7, where the case BOUNDS was measured on (kappa 5.8) gives 1e-7 ... 4e-7.
CASES = {"schnet_B1": ("schnet", [N_ATOMS], 801), "schnet_B4": ("schnet", [N_ATOMS] * 4, 811),
         "schnet_ragged": ("schnet", [1, 2, 9, N_ATOMS], 821),
         "painn_B1": ("painn", [N_ATOMS], 832), "painn_B4": ("painn", [N_ATOMS] * 4, 880)}
SEARCH_FROM = {"schnet_B1": 801, "schnet_B4": 811, "schnet_ragged": 821, "painn_B1": 831, "painn_B4": 841}


def cpu_modules(kind, cfg):
    """Backbone and head with torch's own initialisation under a fixed seed, on the CPU."""
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    torch.manual_seed(1234)
    model = SchNet(**cfg) if kind == "schnet" else PaiNN(**cfg)
    head = torch.nn.Linear(cfg["hidden_channels"], 1) if kind == "schnet" else model.create_output_layers()
    return model, head


def start_velocities(raw, seed):
    """Simulator.thermalize's draws for the case (fp32, as the device run starts from) and the default masses."""
    import types
    from geossl_amd.md import Simulator
    batch = types.SimpleNamespace(x=torch.from_numpy(raw["x"][:, 0].copy()), positions=torch.from_numpy(raw["positions"]),
                                  batch=torch.from_numpy(raw["batch"]), _sizes=[int(n) for n in raw["sizes"]])
    sim = Simulator(None, None, batch, energy_and_gradient=lambda pos: (None, None))
    sim.thermalize(T0, generator=torch.Generator().manual_seed(seed))
    return sim.velocities.double().numpy(), sim.masses.numpy()


def langevin_coefficients():
    c1 = math.exp(-LANGEVIN[2] * DT)
    return c1, math.sqrt(1 - c1 * c1) * math.sqrt(mt.KB * LANGEVIN[1] * mt.ACCEL)


def twin_margins(name, seed, snapshot=None):
    """[(smallest cutoff margin, largest head condition number) of the twin trajectory under NVE, under Langevin] of a
    case started from `seed`."""
    kind, sizes, _ = CASES[name]
    cfg = _cfg(kind)
    raw = _raw(sizes, seed, cfg["cutoff"])
    if snapshot is None:
        model, head = cpu_modules(kind, cfg)
        p, b = tw.module_tensors(model)
        snapshot = (p, b, tw.module_tensors(head)[0])
    v0, masses = start_velocities(raw, seed)
    out = []
    for lv in (None, langevin_coefficients()):
        out.append(mt.twin_trajectory_margin(kind, cfg, _twin_cfg(kind, cfg), *snapshot, raw, v0, masses, DT, STEPS, lv,
                                             THERMOSTAT_SEED))
    return out


def start_ok(name, margins):
    kind = CASES[name][0]
    limit = mt.head_condition_limit(kind, tw.BOUNDS[kind]["energy"])
    return all(m >= SEARCH_MARGIN and c <= limit for m, c in margins)


def first_start(name):
    for seed in range(SEARCH_FROM[name], SEARCH_FROM[name] + 50):
        if start_ok(name, twin_margins(name, seed)):
            return seed
    raise AssertionError("no start with a cutoff margin on every frame")
