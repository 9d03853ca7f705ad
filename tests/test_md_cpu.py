"""CPU tests of molecular dynamics (geossl_amd/md.py): the fp64 twin (tests/md_twin.py) and the Simulator's torch route
against closed forms, the teeth of the one-step check, the torch route on the oracle's reduced backbones against the
twin, recording, velocities and units, the refusals, the C ABI of the three kernels, and the numpy restatement of the
thermostat's stream at the limits the GPU test applies to the device's."""
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import force_twin as tw
import md_twin as mt
from conftest import load_golden
from md_cases import NORMALS_SEED
from oracle.graph import radius_graph_np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MD_SYMBOLS = ("geossl_md_advance", "geossl_md_finish", "geossl_md_normals")


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _tethered(sizes, k=80.0, dtype=torch.float64):
    """Every atom on a spring to the origin: E_b = sum k |x|^2 / 2 -> (batch namespace, hook, numpy force)."""
    N = sum(sizes)
    mol = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    g = torch.Generator().manual_seed(N)
    batch = _ns(x=torch.zeros(N, dtype=torch.long), positions=torch.randn(N, 3, generator=g, dtype=torch.float64).to(dtype),
                batch=mol, _sizes=list(sizes))

    def hook(pos):
        e = torch.zeros(len(sizes), dtype=pos.dtype).index_add_(0, mol, 0.5 * k * (pos * pos).sum(1))
        return e, k * pos
    return batch, hook, (lambda x: -k * x)


# ------------------------------------------------------------------------------------------------- closed forms
def _verlet_closed_form(x0, v0, w2, dt, ks):
    theta = 2.0 * math.asin(math.sqrt(w2) * dt / 2.0)   # (cos theta = 1 - (omega dt)^2 / 2, without acos near 1)
    return x0 * np.cos(ks * theta)[:, None, None] + dt * v0 / math.sin(theta) * np.sin(ks * theta)[:, None, None]


def test_velocity_verlet_is_the_closed_form_of_the_harmonic_oscillator():
    """x_k = A cos(k theta + phi), cos theta = 1 - (omega dt)^2 / 2, over 1000 steps to 1e-12 (of the amplitude): the
    twin, and the Simulator's torch route on fp64 positions through the energy_and_gradient hook."""
    from geossl_amd.md import ACCEL, Simulator
    k, mass, dt, steps = 80.0, 12.011, 0.5, 1000
    batch, hook, force = _tethered([1, 2], k)
    masses = np.full(3, mass)
    x0 = batch.positions.numpy().copy()
    v0 = 0.01 * np.random.default_rng(1).standard_normal((3, 3))
    ref = _verlet_closed_form(x0, v0, ACCEL * k / mass, dt, np.arange(steps + 1))
    scale = np.abs(ref).max()
    xs, _ = mt.integrate(x0, v0, force, masses, dt, steps)
    assert np.abs(xs - ref).max() <= 1e-12 * scale
    sim = Simulator(None, None, batch, masses=masses, dt=dt, energy_and_gradient=hook)
    assert not sim.fused
    sim.set_velocities(torch.from_numpy(v0))
    traj = sim.run(steps)
    assert traj.positions.dtype == torch.float64 and tuple(traj.positions.shape) == (steps + 1, 3, 3)
    assert np.abs(traj.positions.numpy() - ref).max() <= 1e-12 * scale
    assert sim.step_count == steps and traj.steps.tolist() == list(range(steps + 1))
    # the energies it records: potential from the hook, kinetic m v^2 / (2 ACCEL) per molecule
    mol = batch.batch.numpy()
    assert np.allclose(traj.kinetic[-1].numpy(), mt.kinetic(traj.velocities[-1].numpy(), masses, mol), rtol=1e-13)
    assert np.allclose(traj.potential[0].numpy(), np.bincount(mol, weights=0.5 * k * (x0 ** 2).sum(1)), rtol=1e-6)


def test_baoab_at_zero_temperature_is_its_closed_form_damping():
    """T = 0: the step is a linear map M of (x, v) with det M = c1, so the state is M^k (x0, v0) and its envelope decays as
    c1^(k/2) = exp(-gamma dt k / 2): the twin and the torch route against the eigen-decomposition of M, 1000 steps."""
    from geossl_amd.md import ACCEL, Simulator
    k, mass, dt, gamma, steps = 80.0, 12.011, 0.5, 0.01, 1000
    w2, h, c1 = ACCEL * k / mass, 0.25, math.exp(-0.01 * 0.5)
    Bk = np.array([[1.0, 0.0], [-h * w2, 1.0]])
    A = np.array([[1.0, h], [0.0, 1.0]])
    O = np.array([[1.0, 0.0], [0.0, c1]])
    M = Bk @ A @ O @ A @ Bk
    lam, V = np.linalg.eig(M)
    assert abs(np.linalg.det(M) - c1) < 1e-15 and np.allclose(np.abs(lam) ** 2, c1, rtol=1e-13)
    batch, hook, force = _tethered([1, 2], k)
    masses = np.full(3, mass)
    x0 = batch.positions.numpy().copy()
    v0 = 0.01 * np.random.default_rng(2).standard_normal((3, 3))
    coef = np.linalg.solve(V, np.stack([x0.reshape(-1), v0.reshape(-1)]))          # [2, 9]
    ks = np.arange(steps + 1)
    ref = np.real(np.einsum("ij,kj,jn->kin", V, lam[None, :] ** ks[:, None], coef))   # [steps + 1, 2, 9]
    scale = np.abs(ref[:, 0]).max()
    xs, vs = mt.integrate(x0, v0, force, masses, dt, steps, langevin=(c1, 0.0), xi=lambda k_: np.zeros((3, 3)))
    assert np.abs(xs.reshape(steps + 1, -1) - ref[:, 0]).max() <= 1e-12 * scale
    sim = Simulator(None, None, batch, masses=masses, dt=dt, thermostat=("langevin", 0.0, gamma), energy_and_gradient=hook)
    sim.set_velocities(torch.from_numpy(v0))
    traj = sim.run(steps)
    assert np.abs(traj.positions.numpy().reshape(steps + 1, -1) - ref[:, 0]).max() <= 1e-12 * scale
    assert np.abs(traj.velocities.numpy().reshape(steps + 1, -1) - ref[:, 1]).max() <= 1e-12 * np.abs(ref[:, 1]).max()


# ------------------------------------------------------------------------------------------------------- teeth
def _anharmonic(x):
    return -60.0 * x - 25.0 * x ** 3


def test_one_step_check_has_teeth():
    """A twin trajectory rounded to fp32 passes at the SchNet force bound; a stale force in the second kick, dt off by
    1 %, a dropped atom and a frame written one slot late are each flagged."""
    eps = tw.BOUNDS["schnet"]["force"]
    g = np.random.default_rng(5)
    n, dt, steps = 5, 0.5, 12
    masses = np.array([12.011, 1.008, 15.999, 1.008, 14.007])
    x0, v0 = g.standard_normal((n, 3)), 0.02 * g.standard_normal((n, 3))

    def check(xs, vs):
        # (an fp32 frame is within u of the fp64 state; the recorded states of a real run ARE fp32: integrate from them)
        F = np.stack([_anharmonic(x.astype(np.float64)) for x in xs])
        return mt.check_trajectory(xs, vs, F, masses, dt, eps)

    def run32(dt_run=dt, stale=False):
        """A trajectory whose every step starts from the fp32 state recorded before it, as a device run's does."""
        xs, vs = [x0.astype(np.float32)], [v0.astype(np.float32)]
        for _ in range(steps):
            x, v = mt.verlet_step(xs[-1].astype(np.float64), vs[-1].astype(np.float64), _anharmonic, masses, dt_run, stale)
            xs.append(x.astype(np.float32))
            vs.append(v.astype(np.float32))
        return np.stack(xs), np.stack(vs)

    xs, vs = run32()
    checked, skipped, bad = check(xs, vs)
    assert (checked, skipped, bad) == (steps, 0, [])
    assert len(check(*run32(stale=True))[2]) == steps
    assert len(check(*run32(dt_run=1.01 * dt))[2]) == steps
    dx, dv = xs.copy(), vs.copy()
    dx[1:, 3], dv[1:, 3] = xs[0, 3], vs[0, 3]                          # atom 3 never moves
    assert len(check(dx, dv)[2]) == steps
    late = np.concatenate([xs[:1], xs[:-1]]), np.concatenate([vs[:1], vs[:-1]])   # slot k holds frame k - 1
    assert [b[0] for b in check(*late)[2]][:1] == [0]
    # and the Langevin form: with the step's own draws it holds, with another step's it does not
    c1, sigma = math.exp(-0.01 * dt), math.sqrt(1 - math.exp(-0.02 * dt)) * math.sqrt(mt.KB * 300.0 * mt.ACCEL)
    xi = [mt.normals(7, k, n) for k in range(steps + 1)]
    lx, lv = [x0.astype(np.float32)], [v0.astype(np.float32)]
    for k in range(steps):
        x, v = mt.baoab_step(lx[-1].astype(np.float64), lv[-1].astype(np.float64), _anharmonic, masses, dt, c1, sigma, xi[k])
        lx.append(x.astype(np.float32))
        lv.append(v.astype(np.float32))
    F = np.stack([_anharmonic(x.astype(np.float64)) for x in lx])
    assert mt.check_trajectory(lx, lv, F, masses, dt, eps, langevin=(c1, sigma), xis=xi)[2] == []
    assert len(mt.check_trajectory(lx, lv, F, masses, dt, eps, langevin=(c1, sigma), xis=xi[1:])[2]) == steps


# ---------------------------------------------------------------------------- the torch route against the twin
@pytest.mark.parametrize("case", ["schnet_B1", "painn_B4"])
def test_cpu_route_on_the_oracle_backbones_meets_the_twin(case):
    """10 NVE steps of the torch route (fp32) on the reduced backbones of tests/test_md17_cpu.py from 300 K velocities:
    every step within the one-step bounds with eF = TOL max|F| (that file's fp32-against-fp64 tolerance)."""
    from test_md17_cpu import TOL, _OracleBackbone, _cpu_head
    from geossl_amd.md import Simulator, default_masses
    g = load_golden("g22_md17_" + case)
    cfg, meta = json.loads(str(g["cfg"])), json.loads(str(g["meta"]))
    kind = meta["kind"]
    model = _OracleBackbone(kind, cfg)
    head, named = _cpu_head(kind, model)
    x, bvec = torch.from_numpy(g["x"]), torch.from_numpy(g["batch"])
    z = x if x.dim() == 1 else x[:, 0]
    sizes = torch.bincount(bvec).tolist()
    batch = _ns(x=x, positions=torch.from_numpy(g["positions"]).clone(), batch=bvec, _sizes=sizes)
    P, Bf = tw.module_tensors(model.net)
    H = {k: p.detach().clone() for k, p in named.items()}
    keys = ("num_interactions", "cutoff", "readout") if kind == "schnet" else ("n_atom_basis", "n_interactions", "cutoff",
                                                                               "readout")
    tcfg = {k: cfg[k] for k in keys}
    masses = default_masses(z).numpy()

    def twin_force(pos):
        pos = np.asarray(pos, dtype=np.float32)
        ei = (tw.schnet_edges(pos, bvec.numpy(), cfg["cutoff"]) if kind == "schnet"
              else torch.from_numpy(radius_graph_np(pos, cfg["cutoff"], bvec.numpy())))
        return tw.predict(kind, tcfg, P, Bf, H, z, pos, bvec, ei)[1].numpy()

    steps, dt = 10, 0.5
    for seed in range(20):   # (a start whose frames all keep the twin's cutoff margin)
        sim = Simulator(model, head, batch, model_3d=kind, dt=dt)
        assert not sim.fused
        sim.thermalize(300.0, generator=torch.Generator().manual_seed(seed))
        traj = sim.run(steps)
        pos, vel = traj.positions.numpy(), traj.velocities.numpy()
        usable = [tw.cutoff_margin(p, bvec.numpy(), cfg["cutoff"]) >= tw.CUTOFF_MARGIN for p in pos]
        if all(usable):
            break
    else:
        raise AssertionError("no start with a cutoff margin on every frame")
    assert traj.positions.dtype == torch.float32 and traj.kinetic.dtype == torch.float64
    F = np.stack([twin_force(p) for p in pos])
    checked, skipped, bad = mt.check_trajectory(pos, vel, F, masses, dt, TOL)
    print(case, "seed", seed, "checked", checked, "max |F|", np.abs(F).max())
    assert checked == steps and skipped == 0 and bad == []
    assert np.abs(pos[-1] - pos[0]).max() > 1e-3        # (it moved)


# ---------------------------------------------------------------------------------------------------- recording
@pytest.mark.parametrize("thermostat", [None, ("langevin", 300.0, 0.01)])
def test_record_every_three_keeps_frames_0_3_6_9(thermostat):
    from geossl_amd.md import Simulator
    batch, hook, _ = _tethered([2, 3])
    out = []
    for every in (1, 3):
        sim = Simulator(None, None, batch, masses=np.full(5, 12.0), thermostat=thermostat, seed=3, energy_and_gradient=hook)
        sim.thermalize(300.0, generator=torch.Generator().manual_seed(1))
        out.append(sim.run(10, record_every=every))
    full, thin = out
    assert full.positions.size(0) == 11 and thin.positions.size(0) == 4 and thin.steps.tolist() == [0, 3, 6, 9]
    for a, b in zip(full, thin):
        assert torch.equal(a[[0, 3, 6, 9]], b)
    # a second run goes on where the first ended
    again = sim.run(2)
    assert again.steps.tolist() == [10, 11, 12] and sim.step_count == 12


# ------------------------------------------------------------------------------------------- velocities and units
def test_units_and_default_masses():
    from geossl_amd import md
    from geossl_amd.Geom3D.models._atomic_mass import atomic_masses
    assert md.ACCEL == 4.184e-4 and md.KB == 8.31446261815324 / 4184
    assert (md.ACCEL, md.KB) == (mt.ACCEL, mt.KB)
    # 1 kcal/mol/A/amu = 4184 J/mol / (1e-10 m) / (1e-3 kg/mol) = 4.184e16 m/s^2 = 4.184e-4 A/fs^2
    assert abs(4184.0 / 1e-10 / 1e-3 * 1e10 / 1e30 - md.ACCEL) <= 1e-18
    x = torch.tensor([0, 5, 6, 7, 0])
    table = torch.as_tensor(atomic_masses(), dtype=torch.float64)
    assert torch.equal(md.default_masses(x), table[x + 1])
    assert abs(float(md.default_masses(x)[0]) - 1.008) < 1e-12 and abs(float(md.default_masses(x)[1]) - 12.011) < 1e-12
    assert torch.equal(md.default_masses(x[:, None].repeat(1, 2)), table[x + 1])
    batch, hook, _ = _tethered([5])
    batch.x = x
    assert torch.equal(md.Simulator(None, None, batch, energy_and_gradient=hook).masses, table[x + 1])


def test_thermalize_removes_the_centre_of_mass_velocity_and_has_the_right_mean_kinetic_energy():
    from geossl_amd.md import KB, Simulator
    sizes = [1, 2, 9, 21]
    batch, hook, _ = _tethered(sizes)
    masses = np.random.default_rng(0).uniform(1.0, 16.0, sum(sizes))
    sim = Simulator(None, None, batch, masses=masses, energy_and_gradient=hook)
    sim.thermalize(300.0, generator=torch.Generator().manual_seed(4))
    v, mol = sim.velocities.numpy(), batch.batch.numpy()
    for b, n in enumerate(sizes):
        p = (masses[mol == b, None] * v[mol == b]).sum(0)
        if n > 1:
            assert np.abs(p).max() <= 1e-12 * np.abs(masses[mol == b, None] * v[mol == b]).max()
        else:
            assert np.abs(p).max() > 0
    # 4096 one-atom molecules: KE = (3/2) KB T each in the mean; the variance of one is (3/2) (KB T)^2
    M, T = 4096, 300.0
    batch, hook, _ = _tethered([1] * M)
    masses = np.random.default_rng(1).uniform(1.0, 16.0, M)
    sim = Simulator(None, None, batch, masses=masses, energy_and_gradient=hook)
    sim.thermalize(T, generator=torch.Generator().manual_seed(5))
    traj = sim.run(0)
    ke = traj.kinetic[0].numpy()
    assert ke.shape == (M,)
    assert abs(ke.mean() - 1.5 * KB * T) <= 5 * math.sqrt(1.5 / M) * KB * T
    assert abs(traj.temperature[0].numpy().mean() - T) <= 5 * math.sqrt(2.0 / (3 * M)) * T


# ----------------------------------------------------------------------------------------------------- refusals
def test_refusals_say_why():
    from geossl_amd.md import Simulator
    ragged, hook, _ = _tethered([21, 20])
    with pytest.raises(ValueError, match="rebuilt every step"):
        Simulator(None, None, ragged, model_3d="painn")
    big, _, _ = _tethered([34])
    with pytest.raises(ValueError, match="complete pair list"):
        Simulator(None, None, big, model_3d="painn")
    huge, _, _ = _tethered([256])
    with pytest.raises(ValueError, match="at most 255 atoms"):
        Simulator(None, None, huge, model_3d="schnet")
    with pytest.raises(ValueError, match="masses has 40 entries, the batch 41 atoms"):
        Simulator(None, None, ragged, masses=np.ones(40), energy_and_gradient=hook)
    with pytest.raises(ValueError, match="langevin"):
        Simulator(None, None, ragged, masses=np.ones(41), thermostat=("nose", 300.0, 0.1), energy_and_gradient=hook)
    with pytest.raises(Exception, match="not included"):
        Simulator(None, None, ragged, model_3d="egnn")


# ------------------------------------------------------------------------------------------------------ surface
def test_md_surface_and_abi():
    import inspect
    import geossl_amd
    from geossl_amd import _lib, build, md, ops
    assert "md" in geossl_amd.__doc__
    sig = inspect.signature(md.Simulator).parameters
    assert list(sig)[:4] == ["model", "graph_pred_linear", "batch", "model_3d"]
    want = dict(model_3d="schnet", masses=None, dt=0.5, thermostat=None, seed=None, use_graph=md.USE_GRAPH_DEFAULT,
                steps_per_replay=md.STEPS_PER_REPLAY_DEFAULT, max_frames=1024, energy_and_gradient=None)
    assert {k: sig[k].default for k in want} == want
    for name in ("thermalize", "set_velocities", "run", "set_thermostat", "set_dt"):
        assert callable(getattr(md.Simulator, name))
    assert md.Trajectory._fields == ("positions", "velocities", "potential", "kinetic", "temperature", "steps")
    assert "different stream" in md.__doc__.lower().replace("\n", " ")
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in MD_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    for name in MD_SYMBOLS:
        assert getattr(lib, name) is not None
    assert "md_integrate.hip" in build._sources() and build.SOURCE_FLAGS.get("md_integrate.hip") == ["-fno-slp-vectorize"]
    for name in ("md_advance", "md_finish", "md_normals"):
        assert callable(getattr(ops, name))
    src = open(os.path.join(REPO, "geossl_amd", "csrc", "graph.hip")).read()
    assert '#include "philox.h"' in src and "uint4 philox4x32_10(" not in src       # (one definition, shared)


# ------------------------------------------------------------------------------------ the reference stream itself
def test_the_restated_stream_keeps_the_limits_of_the_gpu_test():
    """Philox-4x32-10 with Box-Muller restated in numpy, at the seed, steps and size of test_gpu_md.py's statistics: the
    stream itself lies within the 5-standard-error limits applied to the device's there."""
    n = 65536
    steps = [0, 1, 2, 2 ** 32 + 1, 2 ** 32 + 2]
    d = [mt.normals(NORMALS_SEED, s, n) for s in steps]
    st = mt.stream_statistics(d[:3])
    st2 = mt.stream_statistics(d[3:])
    lim = st["limits"]
    print({k: ["%.2e" % v for v in st[k] + st2[k]] for k in ("mean", "var", "lag")}, lim)
    for k in ("mean", "var", "lag"):
        assert max(st[k] + st2[k]) <= lim[k], k
    assert not np.array_equal(d[0], d[1]) and not np.array_equal(d[1], d[3])
    # the generator against Random123's known-answer vector for Philox-4x32-10 (counter and key all ones' complement)
    kat = mt.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    assert [int(w) for w in kat] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


# ------------------------------------------------------------------------------ the starts of the GPU trajectory cases
@pytest.mark.parametrize("name", ["schnet_B1", "schnet_B4", "schnet_ragged", "painn_B1", "painn_B4"])
def test_the_twin_trajectory_of_every_gpu_case_keeps_the_cutoff_margin(name):
    """The twin's own fp64 trajectory (NVE, and Langevin with the device's draws restated) from the start of each case of
    tests/md_cases.py keeps twice force_twin's cutoff margin on all 13 frames, and its energies stay below the head
    condition number beyond which no fp32 head can meet BOUNDS[kind]["energy"] (md_twin.head_condition_limit)."""
    import md_cases as mc
    assert set(mc.CASES) == {"schnet_B1", "schnet_B4", "schnet_ragged", "painn_B1", "painn_B4"}
    kind = mc.CASES[name][0]
    limit = mt.head_condition_limit(kind, tw.BOUNDS[kind]["energy"])
    assert abs(limit - tw.BOUNDS[kind]["energy"] / ((9 if kind == "schnet" else 8) * 2.0 ** -24)) < 1e-9
    margins = mc.twin_margins(name, mc.CASES[name][2])
    print(name, [("%.2e" % m, "%.2f" % c) for m, c in margins], "limit %.2f" % limit)
    assert all(m >= mc.SEARCH_MARGIN and c <= limit for m, c in margins) and mc.start_ok(name, margins)
    # the start the search left behind: its energy is a near cancellation of the head's terms
    if name == "painn_B1":
        assert not mc.start_ok(name, mc.twin_margins(name, mc.SEARCH_FROM[name]))


# ------------------------------------------------------------------------------------------------- the example's masses
def test_the_example_gives_a_file_s_atomic_numbers_their_own_masses():
    """examples/simulate_md17.py on a data file: z are atomic numbers, so H, C, O weigh 1.008, 12.011, 15.999 - where the
    Simulator's default, which reads an atom type as the index Z - 1, would give the next element's."""
    import importlib.util
    from geossl_amd.md import default_masses
    spec = importlib.util.spec_from_file_location("simulate_md17", os.path.join(REPO, "examples", "simulate_md17.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    z = np.array([1, 6, 8])
    assert ex.file_masses(z).tolist() == [1.008, 12.011, 15.999]
    assert default_masses(torch.from_numpy(z) - 1).tolist() == [1.008, 12.011, 15.999]
    src = open(os.path.join(REPO, "examples", "simulate_md17.py")).read()
    assert "masses = file_masses(z)" in src and "masses=masses" in src


def test_a_seed_beyond_the_state_word_is_refused():
    from geossl_amd.md import Simulator
    batch, hook, _ = _tethered([2])
    for seed in (2 ** 63, -1):
        with pytest.raises(ValueError, match="seed is an integer in"):
            Simulator(None, None, batch, masses=np.ones(2), seed=seed, energy_and_gradient=hook)
    assert Simulator(None, None, batch, masses=np.ones(2), seed=2 ** 63 - 1, energy_and_gradient=hook).seed == 2 ** 63 - 1
