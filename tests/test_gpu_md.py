"""Molecular dynamics on the GPU (geossl_amd/md.py, csrc/md_integrate.hip): the integrator kernels alone per element
against fp64 numpy, the thermostat's stream, replayed and eager trajectories of SchNet and PaiNN force fields against the
fp64 twin by the one-step check of tests/md_twin.py, the replay protocol, and live parameters."""
import math

import numpy as np
import pytest
import torch

import force_twin as tw
import md_twin as mt
from md_cases import (CASES, DT, LANGEVIN, N_ATOMS, NORMALS_SEED, STEPS, T0, THERMOSTAT_SEED, _cfg, _raw, _twin_cfg,
                      device_batch, device_modules, module_snapshot as _snapshot)
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _modules(kind, cfg):
    return device_modules(kind, cfg, DEV)


def _batch(kind, cfg, raw):
    return device_batch(kind, cfg, raw, DEV)


# ------------------------------------------------------------------------------------------------ kernels alone
KERNEL_SIZES = [1, 2, 33, 34, 64, 65, 255]


def _kernel_state(thermostat, step0, every, first, seed=11):
    from geossl_amd import ops
    g = torch.Generator().manual_seed(3)
    N, B = sum(KERNEL_SIZES), len(KERNEL_SIZES)
    masses = 1.0 + 15.0 * torch.rand(N, generator=g, dtype=torch.float64)
    dt, gamma, T = 0.5, 0.01, 300.0
    c1 = math.exp(-gamma * dt) if thermostat else 1.0
    sigma = math.sqrt(1 - c1 * c1) * math.sqrt(mt.KB * T * mt.ACCEL) if thermostat else 0.0
    st = dict(
        pos=torch.randn(N, 3, generator=g).to(DEV), vel=(0.01 * torch.randn(N, 3, generator=g)).to(DEV),
        grad=(20.0 * torch.randn(N, 3, generator=g)).to(DEV), energy=torch.randn(B, generator=g).to(DEV),
        cinv=(mt.ACCEL / masses).float().to(DEV), rsqrt=masses.rsqrt().float().to(DEV),
        ke_coef=(masses / (2 * mt.ACCEL)).to(DEV),
        mol_ptr=torch.tensor(np.concatenate([[0], np.cumsum(KERNEL_SIZES)]), dtype=torch.int32, device=DEV),
        params=torch.tensor([dt, c1, sigma, 0.0], dtype=torch.float32, device=DEV),
        state=torch.tensor([step0, 0, seed, every, first, 1 if thermostat else 0, 0, 0], dtype=torch.int64, device=DEV))
    assert ops.MD_STATE_WORDS == 8 and st["mol_ptr"][-1] == N
    return st, g, N, B


@pytest.mark.parametrize("thermostat", [False, True], ids=["nve", "langevin"])
def test_integrator_kernels_vs_fp64(thermostat):
    """Molecules of 1, 2, 33, 34, 64, 65 and 255 atoms, four steps with a random gradient per step, from a step counter
    whose high word changes on the way: positions and velocities per element at the rounding terms of the one-step check
    (no force error: the gradient is given), kinetic energies at 1e-12, the step words, and which slots are written."""
    from geossl_amd import ops
    step0, every, frames, SENT = 2 ** 32 - 2, 2, 3, -7.0
    st, g, N, B = _kernel_state(thermostat, step0, every, step0 + 1)
    # the trajectory buffers sit inside larger ones: a write outside slots [0, frames) would show
    big = [torch.full((frames + 2, N, 3), SENT, device=DEV), torch.full((frames + 2, N, 3), SENT, device=DEV),
           torch.full((frames + 2, B), SENT, device=DEV), torch.full((frames + 2, B), SENT, dtype=torch.float64, device=DEV)]
    traj = tuple(t[1:1 + frames] for t in big)
    dt, c1, sigma = (float(v) for v in st["params"].cpu()[:3])
    m_eff = mt.ACCEL / st["cinv"].cpu().double().numpy()             # (so that ACCEL / m IS the fp32 factor the kernel uses)
    mol = np.repeat(np.arange(B), KERNEL_SIZES)
    cpu = lambda t: t.detach().cpu().double().numpy()
    recorded = {}
    for k in range(1, 5):
        x_t, v_t, G_t = cpu(st["pos"]), cpu(st["vel"]), cpu(st["grad"])
        step = step0 + k - 1
        xi = cpu(ops.md_normals(11, step, N, DEV)) if thermostat else None
        ops.md_advance(st["pos"], st["vel"], st["grad"], st["cinv"], st["rsqrt"], st["params"], st["state"])
        assert st["state"].cpu()[:2].tolist() == [step, step + 1]
        G_new, E_new = (20.0 * torch.randn(N, 3, generator=g)).to(DEV), torch.randn(B, generator=g).to(DEV)
        ops.md_finish(st["pos"], st["vel"], G_new, E_new, st["grad"], st["energy"], st["cinv"], st["ke_coef"], st["mol_ptr"],
                      st["params"], st["state"], traj)
        torch.cuda.synchronize()
        assert st["state"].cpu()[:2].tolist() == [step + 1, step + 1]
        assert torch.equal(st["grad"], G_new) and torch.equal(st["energy"], E_new)
        x_n, v_n = cpu(st["pos"]), cpu(st["vel"])
        # a stand-in for sigma_T / sqrt(m) with the kernel's own fp32 factors
        lv = None
        if thermostat:
            lv = (c1, 1.0)
            xi = xi * (sigma * cpu(st["rsqrt"]) * np.sqrt(m_eff))[:, None]
        rv, rx = mt.one_step(x_t, v_t, x_n, v_n, -G_t, -cpu(G_new), m_eff, dt, 0.0, 0.0, lv, xi)
        assert rv <= 1.0 and rx <= 1.0, (k, rv, rx)
        assert np.abs(x_n - x_t).max() > 1e-4
        ke = np.bincount(mol, weights=cpu(st["ke_coef"]) * (v_n ** 2).sum(1))
        d = step + 1 - (step0 + 1)
        if d % every == 0:
            slot = d // every
            recorded[slot] = k
            assert torch.equal(traj[0][slot], st["pos"]) and torch.equal(traj[1][slot], st["vel"])
            assert torch.equal(traj[2][slot], E_new)
            assert np.abs(cpu(traj[3][slot]) - ke).max() <= 1e-12 * ke.max()
    assert recorded == {0: 1, 1: 3}
    assert all(bool((t[2] == SENT).all()) for t in traj)                     # the slot no step reached
    assert all(bool((t[0] == SENT).all()) and bool((t[-1] == SENT).all()) for t in big)

    # steps before `first` (d < 0, a multiple of record_every included) and beyond the last slot write nothing
    st["state"][3], st["state"][4] = 1, step0 + 4 + 3
    one = tuple(t[1:2] for t in big)
    for t in big:
        t.fill_(SENT)
    for k in range(4):
        ops.md_advance(st["pos"], st["vel"], st["grad"], st["cinv"], st["rsqrt"], st["params"], st["state"])
        ops.md_finish(st["pos"], st["vel"], st["grad"], st["energy"], st["grad"], st["energy"], st["cinv"], st["ke_coef"],
                      st["mol_ptr"], st["params"], st["state"], one)
        torch.cuda.synchronize()
        written = not bool((one[0] == SENT).all())
        assert written == (k >= 2), k                                        # slot 0 at the third step, nothing before
        if k == 2:
            assert torch.equal(one[0][0], st["pos"])
            keep = st["pos"].clone()
    assert torch.equal(one[0][0], keep)                                      # the fourth step's slot 1 does not exist
    assert all(bool((t[0] == SENT).all()) and bool((t[2:] == SENT).all()) for t in big)
    # record only: slot 0, no kick, no step word
    words, v_before = st["state"].clone(), st["vel"].clone()
    ops.md_finish(st["pos"], st["vel"], st["grad"], st["energy"], st["grad"], st["energy"], st["cinv"], st["ke_coef"],
                  st["mol_ptr"], st["params"], st["state"], traj, record_only=True)
    torch.cuda.synchronize()
    assert torch.equal(st["state"], words) and torch.equal(st["vel"], v_before)
    assert torch.equal(traj[0][0], st["pos"]) and torch.equal(traj[1][0], v_before) and torch.equal(traj[2][0], st["energy"])
    ke = np.bincount(mol, weights=cpu(st["ke_coef"]) * (cpu(v_before) ** 2).sum(1))
    assert np.abs(cpu(traj[3][0]) - ke).max() <= 1e-12 * ke.max()


# --------------------------------------------------------------------------------------------- the thermostat's stream
def test_md_normals_stream():
    """65 536 atoms x 3 at steps 0, 1, 2 and 2^32 + 1, 2^32 + 2: mean, variance and the lag correlation of consecutive
    steps within 5 standard errors (test_md_cpu.py shows the stream itself keeps them at this seed), no two steps equal,
    equal (seed, step) equal bits, another seed other bits - and the values against the numpy restatement: fp32 logf,
    sqrtf and sincosf at a few ulp on a radius below 5.8 and an angle rounded to 2 pi 2^-24 give well below 2e-5."""
    from geossl_amd import ops
    n = 65536
    steps = [0, 1, 2, 2 ** 32 + 1, 2 ** 32 + 2]
    d = [ops.md_normals(NORMALS_SEED, s, n, DEV) for s in steps]
    again = ops.md_normals(NORMALS_SEED, steps[3], n, DEV)
    other = ops.md_normals(NORMALS_SEED + 1, steps[3], n, DEV)
    torch.cuda.synchronize()
    assert torch.equal(again, d[3]) and not torch.equal(other, d[3])
    for i in range(len(d)):
        for j in range(i):
            assert not torch.equal(d[i], d[j])
    h = [t.cpu().double().numpy() for t in d]
    assert all(np.isfinite(t).all() for t in h)
    for group in (h[:3], h[3:]):
        st = mt.stream_statistics(group)
        for k in ("mean", "var", "lag"):
            assert max(st[k]) <= st["limits"][k], (k, st[k])
    for s, t in zip(steps, h):
        assert np.abs(t - mt.normals(NORMALS_SEED, s, n)).max() <= 2e-5, s


# ------------------------------------------------------------------------------------- trajectories against the twin
def _twin_frames(kind, cfg, snap, raw, positions):
    """The twin's (energies [R, B], forces [R, N, 3]) at recorded positions, and which frames keep its cutoff margin."""
    from geossl_amd import ops
    p, b, h = snap
    z, bvec = raw["x"][:, 0].copy(), raw["batch"]
    es, fs, usable = [], [], []
    for pos in positions:
        pos = pos.detach().cpu().numpy()
        usable.append(tw.cutoff_margin(pos, bvec, cfg["cutoff"]) >= tw.CUTOFF_MARGIN)
        if kind == "schnet":
            ei = tw.schnet_edges(pos, bvec, cfg["cutoff"])
        else:
            ei = ops.radius_graph(torch.from_numpy(pos).to(DEV), cfg["cutoff"], torch.from_numpy(bvec).to(DEV)).cpu()
        e, f = tw.predict(kind, _twin_cfg(kind, cfg), p, b, h, z, pos, bvec, ei, device=DEV)
        es.append(e.numpy())
        fs.append(f.numpy())
    return np.stack(es), np.stack(fs), np.array(usable)


def _steps_against_twin(kind, cfg, snap, raw, sim, traj, tag):
    """The one-step check on every recorded step -> (twin energies, usable frames) for the potentials' check."""
    from geossl_amd import ops
    E, F, usable = _twin_frames(kind, cfg, snap, raw, traj.positions)
    pos, vel = traj.positions.cpu().numpy(), traj.velocities.cpu().numpy()
    lv = xis = None
    if sim._thermostat is not None:
        _, c1, sigma = (float(v) for v in sim._params.cpu()[:3])
        lv = (c1, sigma)
        xis = [ops.md_normals(sim.seed, int(s), sim.N, DEV).cpu().numpy() for s in traj.steps.tolist()[:-1]]
    checked, skipped, bad = mt.check_trajectory(pos, vel, F, sim.masses.numpy(), DT, tw.BOUNDS[kind]["force"], usable, lv, xis)
    print(tag, "checked", checked, "skipped", skipped, "max|F| %.3g" % np.abs(F).max())
    assert bad == [], (tag, bad)
    assert checked >= 1 and skipped * 10 <= checked, (tag, checked, skipped)
    assert np.abs(pos[-1] - pos[0]).max() > 1e-3
    ke = np.stack([mt.kinetic(v, sim.masses.numpy(), raw["batch"]) for v in vel])
    assert np.abs(traj.kinetic.cpu().numpy() - ke).max() <= 1e-12 * ke.max()     # (m / (2 ACCEL) is fp64 on both sides)
    return E, usable


def _potentials_against_twin(kind, traj, E, usable, tag):
    pot = traj.potential.cpu().numpy()
    e_err = {int(k): tw.max_err(pot[k], E[k]) for k in np.flatnonzero(usable)}
    print(tag, "energy errors per frame", ["%.2e" % v for v in e_err.values()], "max|E| %.3g" % np.abs(E).max())
    assert max(e_err.values()) <= tw.BOUNDS[kind]["energy"], (tag, e_err)


_RUNS = {}   # (case, thermostat) -> the run and the twin's frames: computed once, shared by the two tests below


def _case_run(name, thermostat):
    from geossl_amd.md import Simulator
    key = (name, thermostat)
    if key not in _RUNS:
        kind, sizes, seed = CASES[name]
        cfg = _cfg(kind)
        raw = _raw(sizes, seed, cfg["cutoff"])
        model, head = _modules(kind, cfg)
        sim = Simulator(model, head, _batch(kind, cfg, raw), model_3d=kind, dt=DT, thermostat=thermostat,
                        seed=THERMOSTAT_SEED)
        assert sim.fused
        sim.thermalize(T0, generator=torch.Generator().manual_seed(seed))
        traj = sim.run(STEPS)
        torch.cuda.synchronize()
        assert sim.captures == 1 and sim.step_count == STEPS and traj.steps.tolist() == list(range(STEPS + 1))
        assert traj.kinetic.dtype == torch.float64 and traj.potential.dtype == torch.float32
        _RUNS[key] = [kind, traj, None, None]
        E, usable = _steps_against_twin(kind, cfg, _snapshot(model, head), raw, sim, traj, name)
        _RUNS[key][2:] = [E, usable]
    return _RUNS[key]


@pytest.mark.parametrize("thermostat", [None, LANGEVIN], ids=["nve", "langevin"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_trajectory_meets_the_twin_step_by_step(name, thermostat):
    """12 replayed steps of 0.5 fs from 300 K velocities (the starts of tests/md_cases.py, whose twin trajectories keep
    the cutoff margin): every recorded step within the one-step bounds of md_twin with eF = BOUNDS[kind]["force"] max|F|,
    no step skipped beyond 1 in 10, the kinetic energies those of the recorded velocities."""
    _case_run(name, thermostat)


@pytest.mark.parametrize("thermostat", [None, LANGEVIN], ids=["nve", "langevin"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_recorded_potentials_meet_the_twin(name, thermostat):
    """The recorded potentials of the same runs within BOUNDS[kind]["energy"] of the twin's energies at the recorded
    positions, frame by frame (force_twin.max_err: against the largest |E| of the frame's molecules).  The starts of
    tests/md_cases.py are those on which an fp32 head can meet that bound at all (md_twin.head_condition_limit)."""
    run = _case_run(name, thermostat)
    assert run[2] is not None, "the run's step check failed"
    _potentials_against_twin(run[0], run[1], run[2], run[3], name)


# -------------------------------------------------------------------------------------------------------- replay
def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("thermostat", [None, LANGEVIN], ids=["nve", "langevin"])
@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_replayed_runs_are_the_eager_runs_bit_for_bit(kind, thermostat):
    from geossl_amd.md import Simulator
    cfg = _cfg(kind)
    raw = _raw([N_ATOMS] * 2, 861, cfg["cutoff"])
    model, head = _modules(kind, cfg)
    bt = _batch(kind, cfg, raw)

    def make(**kw):
        kw.setdefault("seed", 5)
        sim = Simulator(model, head, bt, model_3d=kind, dt=DT, thermostat=thermostat, **kw)
        sim.thermalize(T0, generator=torch.Generator().manual_seed(1))
        return sim
    eager = make(use_graph=False)
    ref = eager.run(10)
    ref2 = eager.run(7, record_every=3)
    assert eager.captures == 0
    for U in (1, 4):
        sim = make(steps_per_replay=U)
        got = sim.run(10)                         # (U = 4: two replays and two eager steps)
        assert sim.captures == 1 and _equal(got, ref), U
        got2 = sim.run(7, record_every=3)
        assert sim.captures == 1 and _equal(got2, ref2) and got2.steps.tolist() == [10, 13, 16]
    # dt and the thermostat are device data: no capture, and the eager run of the same settings agrees
    for s in (eager, sim):
        s.set_dt(0.25)
        s.set_thermostat(T=250.0, gamma=0.02)
    assert _equal(sim.run(9), eager.run(9)) and sim.captures == 1
    # a run longer than the frame buffer is the run with room
    small = make(steps_per_replay=4, max_frames=4)
    assert _equal(small.run(10), ref) and _equal(small.run(7, record_every=3), ref2) and small.captures == 1
    # one seed, one trajectory; another seed, another (where the seed is used)
    assert _equal(make(seed=5).run(10), ref)
    other = make(seed=6).run(10)
    assert _equal(other, ref) == (thermostat is None)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- live parameters
@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_a_replayed_run_reads_the_live_parameters(kind):
    """After an in-place update of every weight the next replayed run meets the twin built from the NEW weights, without
    a capture - and differs from the run the old weights give."""
    from geossl_amd.md import Simulator
    cfg = _cfg(kind)
    raw = _raw([N_ATOMS], 871, cfg["cutoff"])
    model, head = _modules(kind, cfg)
    sim = Simulator(model, head, _batch(kind, cfg, raw), model_3d=kind, dt=DT)
    sim.thermalize(T0, generator=torch.Generator().manual_seed(2))
    x0, v0 = sim.positions.clone(), sim.velocities.clone()
    before = sim.run(STEPS)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for p in list(model.parameters()) + list(head.parameters()):
            p.mul_(1.0 + 0.05 * torch.randn(p.shape, generator=g).to(DEV))
    sim.set_positions(x0)
    sim.set_velocities(v0)
    traj = sim.run(STEPS)
    torch.cuda.synchronize()
    assert sim.captures == 1 and traj.steps.tolist() == list(range(STEPS, 2 * STEPS + 1))
    assert torch.equal(traj.positions[0], before.positions[0]) and not torch.equal(traj.positions[-1], before.positions[-1])
    E, usable = _steps_against_twin(kind, cfg, _snapshot(model, head), raw, sim, traj, kind + " after the update")
    _potentials_against_twin(kind, traj, E, usable, kind + " after the update")
