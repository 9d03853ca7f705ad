"""Structure relaxation on the GPU (geossl_amd/relax.py, csrc/relax.hip): the FIRE kernel alone over every branch against
the fp64 twin with exact decisions and words, replayed trajectories of SchNet and PaiNN force fields against the twin by the
one-step check of tests/relax_twin.py, convergence within twice the twin's step count, the replay protocol, and live
parameters."""
import numpy as np
import pytest
import torch

import force_twin as tw
import relax_cases as rc
import relax_twin as rt
from md_cases import N_ATOMS, _cfg, _raw, device_batch, device_modules, module_snapshot as _snapshot
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ the kernel alone
KERNEL_SIZES = [1, 2, 33, 34, 64, 65, 255]
KERNEL_PARAMS = rt.params(dt_max=1.0, dt_min=0.2, n_min=2)
SENT = -7
# the gradient of step k is SIGN[k] * scale_b * (a fixed direction + a little of a fresh one): 14 downhill steps (dt grows
# from the fourth on and reaches the cap), four alternating signs (each uphill: 1 -> 0.5 -> 0.25 -> the floor 0.2 -> 0.2), then
# downhill again.  Molecule 1's gradient is far below the tolerance at steps 6 and 7 and back afterwards: it stays latched.
SIGN = [1.0] * 14 + [-1.0, 1.0, -1.0, 1.0] + [1.0] * 3
SCALE = [1.0, 3.0, 10.0, 100.0, 1000.0, 3000.0, 30.0]
QUIET = {6: 1e-4, 7: 1e-4}


def _frame(bufs, slot):
    pos, vel, e, fm, dt, al, npos, done = (_np(t[slot]) for t in bufs)
    return dict(x=pos, v=vel, energy=e, fmax=fm, dt=dt, alpha=al, npos=npos, done=done != 0)


def test_fire_kernels_vs_fp64_over_every_branch():
    """Molecules of 1, 2, 33, 34, 64, 65 and 255 atoms, 21 steps with given gradients that reach every branch.  The twin,
    fed the device's recorded state, asserts that no decision lies within 1e-9 (relative) of its threshold; then `done`,
    dt, alpha, npos are exact and x, v lie within the rounding terms of the one-step check (eF = 0).  Frames are checked
    inside larger sentinel-filled buffers, the counters and the active count at every step, and evaluate_only changes
    nothing but its frame."""
    from geossl_amd import ops
    g = torch.Generator().manual_seed(3)
    N, B, K = sum(KERNEL_SIZES), len(KERNEL_SIZES), len(SIGN)
    mol = np.repeat(np.arange(B), KERNEL_SIZES)
    p = rt.params32(KERNEL_PARAMS)
    masses = 1.0 + 15.0 * torch.rand(N, generator=g, dtype=torch.float64)
    cinv = (rt.ACCEL / masses).float().to(DEV)
    m_eff = rt.ACCEL / _np(cinv).astype(np.float64)                # (so that ACCEL / m IS the fp32 factor the kernel uses)
    pos, vel = torch.randn(N, 3, generator=g).to(DEV), torch.zeros(N, 3, device=DEV)
    grad, energy = torch.zeros(N, 3, device=DEV), torch.zeros(B, device=DEV)
    mol_ptr = torch.tensor(np.concatenate([[0], np.cumsum(KERNEL_SIZES)]), dtype=torch.int32, device=DEV)
    params = torch.tensor([p[k] for k in ("ftol", "dt_max", "dt_min", "max_step", "f_inc", "f_dec", "alpha_start", "f_alpha")],
                          dtype=torch.float32, device=DEV)
    iparams = torch.tensor([p["n_min"], 1, 0, 0], dtype=torch.int64, device=DEV)
    mol_dt, mol_alpha = torch.full((B,), p["dt"], device=DEV), torch.full((B,), p["alpha_start"], device=DEV)
    mol_state = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
    active = torch.full((3,), SENT, dtype=torch.int32, device=DEV)
    big = ops.fire_frames(K + 2, N, B, DEV, fill=SENT)               # a write outside slots [0, K) would show
    traj = tuple(t[1:1 + K] for t in big)
    big1 = ops.fire_frames(3, N, B, DEV, fill=SENT)
    one = tuple(t[1:2] for t in big1)
    state = lambda: (mol_dt, mol_alpha, mol_state, pos, vel, grad, energy)
    args = lambda G, E: (pos, vel, G, E, grad, energy, cinv, mol_ptr, params, iparams, mol_dt, mol_alpha, mol_state)
    base = torch.randn(N, 3, generator=g)
    scale = torch.tensor(np.repeat(SCALE, KERNEL_SIZES), dtype=torch.float32)[:, None]
    grads, seen, latched, nsteps = [], dict(down=0, up=0, grow=0, cap=0, floor=0, clamp=0, free=0, frozen=0), np.zeros(B, bool), np.zeros(B, int)
    for k in range(K):
        G = SIGN[k] * scale * (base + 0.05 * torch.randn(N, 3, generator=g))
        if k in QUIET:
            G[torch.from_numpy(mol == 1)] *= QUIET[k]
        G, E = G.to(DEV), torch.randn(B, generator=g).to(DEV)
        grads.append(_np(G).astype(np.float64))
        x_t, v_t = _np(pos).astype(np.float64), _np(vel).astype(np.float64)
        st = dict(dt=_np(mol_dt).astype(np.float64), alpha=_np(mol_alpha).astype(np.float64),
                  npos=_np(mol_state[:, 0]).astype(np.int64), done=latched.copy(), nsteps=nsteps.copy())
        _, _, st_n, info = rt.fire_step(x_t, v_t, -grads[k], m_eff, mol, st, p)
        assert min(info["margins"]) >= rt.DECISION_MARGIN, (k, min(info["margins"]))
        ops.fire_step(*args(G, E), frames=traj)
        ops.fire_active(mol_state, active[1:2])
        torch.cuda.synchronize()
        fr = _frame(traj, k)
        moving = ~info["converged"]
        assert np.array_equal(fr["done"], info["converged"]) and np.array_equal(_np(mol_state[:, 1]) != 0, info["converged"])
        assert np.array_equal(fr["x"], x_t.astype(np.float32)) and np.array_equal(fr["v"], v_t.astype(np.float32))
        assert np.array_equal(fr["dt"], st["dt"].astype(np.float32)) and np.array_equal(fr["npos"], st["npos"])
        assert np.array_equal(fr["energy"], _np(E)) and np.abs(fr["fmax"] - info["fmax"]).max() <= 4 * rt.U * info["fmax"].max()
        assert torch.equal(grad, G) and torch.equal(energy, E)
        assert _np(mol_state[:, 3]).tolist() == [k + 1] * B and np.array_equal(_np(mol_state[:, 2]), st_n["nsteps"])
        assert active.tolist() == [SENT, int(moving.sum()), SENT]
        for b in np.flatnonzero(moving):
            want = rt.state_words(st["dt"][b], st["alpha"][b], st["npos"][b], info["downhill"][b], p)
            got = (_np(mol_dt)[b], _np(mol_alpha)[b], int(mol_state[b, 0]))
            assert got == want, (k, b, got, want)
            seen["cap"] += info["grow"][b] and want[0] == np.float32(p["dt_max"]) and st["dt"][b] < p["dt_max"]
            seen["floor"] += (not info["downhill"][b]) and want[0] == np.float32(p["dt_min"])
        seen["down"] += int((moving & info["downhill"]).sum())
        seen["up"] += int((moving & ~info["downhill"]).sum())
        seen["grow"] += int(info["grow"].sum())
        seen["clamp"] += int(info["clamped"].sum())
        seen["free"] += int((moving & ~info["clamped"]).sum())
        seen["frozen"] += int((latched & (info["fmax"] >= p["ftol"])).sum())
        latched, nsteps = st_n["done"], st_n["nsteps"]
        if k == 0:
            assert not (v_t != 0).any() and info["downhill"].all()            # vv == 0 at the start: downhill
    print("branches", seen)
    assert all(v > 0 for v in seen.values()), seen
    assert latched.tolist() == [False, True] + [False] * 5
    # the last state through evaluate_only: nothing but the frame changes
    before = [t.clone() for t in state()]
    G, E = torch.randn(N, 3, generator=g).to(DEV), torch.randn(B, generator=g).to(DEV)
    ops.fire_step(*args(G, E), frames=one, evaluate_only=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, state()))
    last = _frame(one, 0)
    assert np.array_equal(last["x"], _np(pos)) and np.array_equal(last["v"], _np(vel)) and np.array_equal(last["energy"], _np(E))
    assert np.array_equal(last["dt"], _np(mol_dt)) and np.array_equal(last["alpha"], _np(mol_alpha))
    assert np.array_equal(last["npos"], _np(mol_state[:, 0])) and last["done"].tolist() == [False, True] + [False] * 5
    assert all(bool((t[0] == SENT).all()) and bool((t[2] == SENT).all()) for t in big1)
    assert all(bool((t[0] == SENT).all()) and bool((t[-1] == SENT).all()) for t in big)
    # every recorded step within the rounding bounds of the one-step check, eF = 0
    frames = [_frame(traj, k) for k in range(K)] + [last]
    checked, skipped, bad = rt.check_history(frames, -np.stack(grads + [grads[-1]]), m_eff, mol, p, 0.0)
    assert (checked, skipped, bad) == (K, 0, []), bad
    assert np.abs(frames[-1]["x"] - frames[0]["x"]).max() > 1e-2
    # calls before `first`, off the stride and beyond the last slot write nothing
    for t in big1:
        t.fill_(SENT)
    iparams[1], iparams[2] = 2, K + 1
    for k in range(4):   # d = -1, 0, 1, 2: slot 0 at the second call; slot 1 (the fourth call) does not exist
        ops.fire_step(*args(grad, energy), frames=one)
        torch.cuda.synchronize()
        assert (not bool((one[0] == SENT).all())) == (k >= 1), k
        if k == 1:
            keep = [t.clone() for t in one]
    assert all(torch.equal(a, b) for a, b in zip(keep, one))
    assert all(bool((t[0] == SENT).all()) and bool((t[2] == SENT).all()) for t in big1)


# ------------------------------------------------------------------------------------- trajectories against the twin
def _twin_at(twin, positions):
    """The twin's (energies [R, B], forces [R, N, 3]) at recorded positions, and which frames keep its cutoff margin."""
    es, fs, usable = [], [], []
    for pos in positions:
        pos = _np(pos)
        usable.append(twin.margin(pos) >= tw.CUTOFF_MARGIN)
        e, f = twin.force(pos)
        es.append(e)
        fs.append(f)
    return np.stack(es), np.stack(fs), np.array(usable)


def _history_against_twin(twin, mz, res, ftol, latched, tag):
    """The one-step check on every recorded step and the recorded energies frame by frame."""
    h = res.history
    E, F, usable = _twin_at(twin, h.positions)
    p = rt.params32(rt.params(ftol=ftol))
    frames = rt.history_frames(h)
    checked, skipped, bad = rt.check_history(frames, F, mz.masses.numpy(), twin.mol, p, tw.BOUNDS[twin.kind]["force"], usable,
                                             latched)
    e_err = {int(k): tw.max_err(_np(h.energy[k]), E[k]) for k in np.flatnonzero(usable)}
    print(tag, "checked", checked, "skipped", skipped, "max|F| %.3g" % np.abs(F).max(), "energy errors",
          ["%.2e" % v for v in e_err.values()])
    assert bad == [], (tag, bad)
    assert checked >= 1 and skipped * 10 <= checked, (tag, checked, skipped)
    assert max(e_err.values()) <= tw.BOUNDS[twin.kind]["energy"], (tag, e_err)
    return F


def _setup(name):
    from geossl_amd.relax import Minimizer
    kind, sizes, seed = rc.CASES[name]
    cfg = _cfg(kind)
    model, head = device_modules(kind, cfg, DEV)
    twin = rc.Twin(name, snapshot=_snapshot(model, head), device=DEV)
    make = lambda **kw: Minimizer(model, head, device_batch(kind, cfg, twin.raw, DEV), model_3d=kind, **kw)
    return twin, make


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_trajectory_meets_the_twin_step_by_step(name):
    """24 recorded steps from v = 0, 12 unrecorded ones, and 12 recorded ones with dt at dt_max (the starts of
    tests/relax_cases.py): every step within the one-step bounds of relax_twin with eF = BOUNDS[kind]["force"] max|F|, the
    words exact, no more than 1 step in 10 skipped, the recorded energies within BOUNDS[kind]["energy"]."""
    twin, make = _setup(name)
    mz = make(fmax=rc.TRAJ_FTOL)
    assert mz.fused
    a = mz.run(rc.STEPS_A, record_every=1)
    mid = mz.run(rc.PRE_STEPS - rc.STEPS_A)
    b = mz.run(rc.STEPS_B, record_every=1)
    torch.cuda.synchronize()
    assert mz.captures == 1 and mid.history is None
    assert a.history.steps.tolist() == list(range(rc.STEPS_A + 1))
    assert b.history.steps.tolist() == list(range(rc.PRE_STEPS, rc.PRE_STEPS + rc.STEPS_B + 1))
    many = np.asarray(twin.sizes) > 1
    assert (_np(a.steps)[many] == rc.STEPS_A).all() and (_np(b.steps)[many] == rc.PRE_STEPS + rc.STEPS_B).all()
    assert (_np(b.steps)[~many] == 0).all()                                  # (an atom alone feels no force)
    _history_against_twin(twin, mz, a, rc.TRAJ_FTOL, None, name + " from rest")
    _history_against_twin(twin, mz, b, rc.TRAJ_FTOL, _np(mid.converged), name + " at dt_max")
    assert (_np(b.history.dt[0])[many] == 5.0).all()
    assert np.abs(_np(b.positions) - twin.raw["positions"]).max() > 1e-3
    assert torch.equal(b.positions, b.history.positions[-1]) and torch.equal(b.energy, b.history.energy[-1])


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_relaxation_converges_within_twice_the_twin_s_steps(name):
    """The tolerance FRACTION x (the start's largest fmax), which the twin's own fp64 run reaches in CONVERGE[name] steps
    (tests/relax_cases.py): with twice that budget the device reports every molecule converged, the twin's fmax at the
    device's final positions is below the tolerance + eF, its energy there lower than at the start for every molecule that
    moved, and in the ragged case molecules freeze at different steps."""
    twin, make = _setup(name)
    ftol, budget = twin.converge_ftol(), 2 * rc.CONVERGE[name]
    mz = make(fmax=ftol)
    res = mz.run(budget, record_every=1)
    torch.cuda.synchronize()
    steps = _np(res.steps)
    freeze = [int(np.argmax(_np(res.history.converged)[:, b])) for b in range(mz.B)]
    print(name, "ftol %.4g" % ftol, "steps", steps.tolist(), "freeze", freeze, "twin", rc.CONVERGE[name])
    assert bool(res.converged.all()) and steps.max() <= budget and res.history.positions.size(0) - 1 <= budget
    assert twin.margin(_np(res.positions)) >= tw.CUTOFF_MARGIN
    E0, _ = twin.force(twin.raw["positions"])
    E1, F1 = twin.force(_np(res.positions))
    fmax = np.array([np.sqrt((F1[twin.mol == b] ** 2).sum(1).max()) for b in range(mz.B)])
    assert (fmax < float(np.float32(ftol)) + tw.BOUNDS[twin.kind]["force"] * np.abs(F1).max()).all(), fmax
    assert (E1[steps > 0] < E0[steps > 0]).all() and np.allclose(E1[steps == 0], E0[steps == 0], rtol=1e-12, atol=0)
    assert (steps > 0).any() and np.array_equal(np.array(freeze) > 0, steps > 0)
    if name == "schnet_ragged":
        assert len(set(freeze)) >= 2


# -------------------------------------------------------------------------------------------------------- replay
def _flat(res):
    return [t for t in res[:5]] + ([] if res.history is None else list(res.history))


def _equal(a, b):
    fa, fb = _flat(a), _flat(b)
    return len(fa) == len(fb) and all(torch.equal(x, y) for x, y in zip(fa, fb))


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_replayed_runs_are_the_eager_runs_bit_for_bit(kind):
    from geossl_amd.relax import Minimizer
    cfg = _cfg(kind)
    raw = _raw([N_ATOMS] * 2, 861, cfg["cutoff"])
    model, head = device_modules(kind, cfg, DEV)
    bt = device_batch(kind, cfg, raw, DEV)
    make = lambda **kw: Minimizer(model, head, bt, model_3d=kind, fmax=rc.TRAJ_FTOL, **kw)
    eager = make(use_graph=False, steps_per_replay=4)
    ref = eager.run(10, record_every=1)
    ref2 = eager.run(7, record_every=3)
    assert eager.captures == 0 and ref.history.positions.size(0) == 11 and not bool(ref.converged.any())
    for U in (1, 4):
        mz = make(steps_per_replay=U)
        got = mz.run(10, record_every=1)                  # (U = 4: two replays and a group of two eager steps)
        assert mz.captures == 1 and _equal(got, ref), U
        got2 = mz.run(7, record_every=3)
        assert mz.captures == 1 and _equal(got2, ref2) and got2.history.steps.tolist() == [10, 13, 16]
    # a run longer than the frame buffer is the run with room
    small = make(steps_per_replay=4, max_frames=4)
    assert _equal(small.run(10, record_every=1), ref) and _equal(small.run(7, record_every=3), ref2) and small.captures == 1
    # the limits and the tolerance are device data: no capture, and the eager run of the same settings agrees
    for s in (eager, mz):
        s.set_limits(dt_max=0.7, max_step=0.001, n_min=1, f_alpha=0.9)
    r1, r2 = mz.run(9, record_every=1), eager.run(9, record_every=1)
    assert _equal(r1, r2) and mz.captures == 1 and float(r1.history.dt[-1].max()) == float(np.float32(0.7))
    for s in (eager, mz):
        s.set_tolerance(1e6)
    r1, r2 = mz.run(12, record_every=1), eager.run(12, record_every=1)   # everything converges: one group, then the stop
    assert _equal(r1, r2) and mz.captures == 1 and bool(r1.converged.all()) and r1.history.positions.size(0) == 5
    assert torch.equal(r1.history.positions[0], r1.positions)
    # reset and the start again: the first run again, still without a capture
    for s in (eager, mz):
        s.set_tolerance(rc.TRAJ_FTOL)
        s.set_limits(dt_max=5.0, max_step=0.1, n_min=5, f_alpha=0.99)
        s.reset()
        s.set_positions(bt.positions)
    assert _equal(mz.run(10, record_every=1), ref) and _equal(eager.run(10, record_every=1), ref) and mz.captures == 1
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- live parameters
@pytest.mark.parametrize("name", ["schnet_B1", "painn_B1"])
def test_a_replayed_run_reads_the_live_parameters(name):
    """After an in-place update of every weight the next replayed run meets the twin built from the NEW weights, without
    a capture - and differs from the run the old weights give."""
    from geossl_amd.relax import Minimizer
    kind, sizes, seed = rc.CASES[name]
    cfg = _cfg(kind)
    model, head = device_modules(kind, cfg, DEV)
    raw = _raw(sizes, seed, cfg["cutoff"])
    mz = Minimizer(model, head, device_batch(kind, cfg, raw, DEV), model_3d=kind, fmax=rc.TRAJ_FTOL, steps_per_replay=4)
    x0 = mz.positions.clone()
    before = mz.run(12, record_every=1)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for p in list(model.parameters()) + list(head.parameters()):
            p.mul_(1.0 + 0.05 * torch.randn(p.shape, generator=g).to(DEV))
    mz.reset()
    mz.set_positions(x0)
    after = mz.run(12, record_every=1)
    torch.cuda.synchronize()
    assert mz.captures == 1 and after.history.steps.tolist() == list(range(13))
    assert torch.equal(after.history.positions[0], before.history.positions[0])
    assert not torch.equal(after.positions, before.positions)
    twin = rc.Twin(name, snapshot=_snapshot(model, head), device=DEV)
    _history_against_twin(twin, mz, after, rc.TRAJ_FTOL, None, name + " after the update")
