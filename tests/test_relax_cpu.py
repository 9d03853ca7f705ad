"""CPU tests of structure relaxation (geossl_amd/relax.py): the Minimizer's torch route against the fp64 twin
(tests/relax_twin.py) on a tether potential, the teeth of the one-step check, the surface and the C ABI of the two kernels,
the refusals, and what tests/relax_cases.py records about the GPU cases, against the twin's own runs."""
import os
import re
import types

import numpy as np
import pytest
import torch

import relax_twin as rt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRE_SYMBOLS = ("geossl_fire_step", "geossl_fire_active")


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


# ------------------------------------------------------------------------------------------------- closed form
def test_the_torch_route_is_the_twin_on_the_tether_potential_and_converges():
    """E = k |x|^2 / 2 (F = -k x in closed form): the fallback route in fp64 through the energy_and_gradient hook equals the
    twin to 1e-12 on every frame and word, reaches fmax < ftol on every molecule, and the molecule that starts below the
    tolerance keeps its positions bit for bit while the others move.  A second run continues the first."""
    from geossl_amd.relax import Minimizer
    k, sizes = 80.0, [1, 2, 5]
    batch, hook, force = _tethered(sizes, k)
    batch.positions[0] *= 1e-4                                  # |F| = 80e-4 |x| < 0.05: frozen from the first test on
    masses = np.array([12.011, 1.008, 15.999, 1.008, 14.007, 12.011, 1.008, 1.008])
    mol, x0 = batch.batch.numpy(), batch.positions.numpy().copy()
    mz = Minimizer(None, None, batch, masses=masses, steps_per_replay=4, energy_and_gradient=hook)
    assert not mz.fused and mz.captures == 0
    res = mz.run(400, record_every=1)
    h = res.history
    R = h.positions.size(0)
    assert res.positions.dtype == torch.float64 and bool(res.converged.all()) and bool((res.fmax < 0.05).all())
    assert R - 1 < 400 and (R - 1) % 4 == 0                       # stopped after a whole group of 4
    assert h.steps.tolist() == list(range(R)) and res.steps.tolist()[0] == 0 and res.steps.max() < R - 1
    fr = rt.minimize(x0, force, masses, mol, rt.params(), R - 1)
    scale = np.abs(x0).max()
    for key, got in (("x", h.positions), ("v", h.velocities), ("fmax", h.fmax), ("dt", h.dt), ("alpha", h.alpha)):
        ref = np.stack([f[key] for f in fr])
        assert np.abs(got.numpy() - ref).max() <= 1e-12 * max(scale, np.abs(ref).max()), key
    assert np.array_equal(h.npos.numpy(), np.stack([f["npos"] for f in fr]))
    assert np.array_equal(h.converged.numpy(), np.stack([f["done"] for f in fr]))
    assert np.array_equal(res.steps.numpy(), fr[-1]["nsteps"])
    assert np.abs(res.energy.numpy() - np.bincount(mol, weights=0.5 * k * (fr[-1]["x"] ** 2).sum(1))).max() <= 1e-12
    assert torch.equal(h.positions[:, 0], h.positions[:1, 0].expand(R, 3)) and np.array_equal(res.positions[0].numpy(), x0[0])
    assert np.sqrt(((res.positions.numpy() - x0) ** 2).sum(1))[1:].min() > 1e-3
    assert len({int(np.argmax(h.converged.numpy()[:, b])) for b in range(3)}) == 3     # three different freezing steps
    # every branch was taken on the way: growth to the cap, uphill resets, the clamp active and inactive
    dts = h.dt.numpy()
    assert dts.max() == 5.0 and (np.diff(dts[:, 2]) < 0).any() and (h.npos.numpy()[1:, 2] == 0).any()
    step = np.sqrt((np.diff(h.positions.numpy(), axis=0) ** 2).sum(2)).max(1)
    assert step.max() <= 0.1 * (1 + 1e-12) and (np.abs(step - 0.1) < 1e-12).any() and (step[step > 0] < 0.099).any()
    # a second run continues: nothing moves any more, the counter goes on; reset starts over
    again = mz.run(3, record_every=1)
    assert again.history.steps.tolist()[0] == R - 1 and torch.equal(again.positions, res.positions)
    mz.reset()
    mz.set_positions(torch.from_numpy(x0))
    assert torch.equal(mz.run(R - 1).positions, res.positions) and mz.run(0, record_every=1).history.positions.size(0) == 1


# ------------------------------------------------------------------------------------------------------- teeth
def _anharmonic(x):
    return -60.0 * x - 25.0 * x ** 3


def _run32(x0, masses, mol, p, steps, stale=False, **wrong):
    """A trajectory as a device run records it: every step starts from the fp32 frame recorded before it, its words follow
    the fp32 restatement, positions and velocities are the fp64 step rounded to fp32."""
    B = int(mol.max()) + 1
    x, v = x0.astype(np.float32), np.zeros_like(x0, dtype=np.float32)
    dt, alpha = np.full(B, p["dt"], np.float32), np.full(B, p["alpha_start"], np.float32)
    npos, done = np.zeros(B, np.int64), np.zeros(B, bool)
    frames, x_prev = [], x
    for _ in range(steps + 1):
        F = _anharmonic((x_prev if stale else x).astype(np.float64))
        st = dict(dt=dt.astype(np.float64), alpha=alpha.astype(np.float64), npos=npos, done=done, nsteps=np.zeros(B, np.int64))
        xn, vn, sn, info = rt.fire_step(x, v, F, masses, mol, st, p, **wrong)
        frames.append(dict(x=x, v=v, dt=dt.copy(), alpha=alpha.copy(), npos=npos.copy(), done=info["converged"].copy(),
                           clamped=info["clamped"], downhill=info["downhill"]))
        x_prev = x
        for b in np.flatnonzero(~info["converged"]):
            dt[b], alpha[b], npos[b] = rt.state_words(dt[b], alpha[b], npos[b], info["downhill"][b], p)
            if wrong.get("keep_alpha") and not info["downhill"][b]:
                alpha[b] = np.float32(sn["alpha"][b])
        x, v, done = xn.astype(np.float32), vn.astype(np.float32), sn["done"]
    return frames


def test_one_step_check_has_teeth():
    """An fp32-recorded twin trajectory over every branch passes at the SchNet force bound with nothing skipped; a stale
    force, alpha not reset after an uphill step, a skipped clamp, a moved frozen molecule and a dropped atom are flagged."""
    import force_twin as tw
    eps = tw.BOUNDS["schnet"]["force"]
    g = np.random.default_rng(5)
    mol = np.repeat(np.arange(3), [1, 2, 5])
    masses = np.array([12.011, 1.008, 15.999, 1.008, 14.007, 12.011, 1.008, 1.008])
    x0 = g.standard_normal((8, 3))
    x0[0] *= 1e-4
    p, steps = rt.params32(rt.params(max_step=0.05)), 80

    def check(frames):
        F = np.stack([_anharmonic(f["x"].astype(np.float64)) for f in frames])
        return rt.check_history(frames, F, masses, mol, p, eps)
    good = _run32(x0, masses, mol, p, steps)
    assert check(good) == (steps, 0, [])
    moving = [f for f in good if not f["done"][2]]
    assert len(moving) > 40 and any(f["clamped"][2] for f in moving) and not all(f["clamped"][2] for f in moving)
    uphill = [(k, b) for k, f in enumerate(good) for b in range(3) if not f["done"][b] and not f["downhill"][b]]
    assert uphill and max(f["dt"].max() for f in good) == np.float32(5.0) and good[-1]["done"][0] and good[0]["done"][0]
    # a stale force: the step at frame k uses the force of frame k - 1
    assert len({k for k, _, _ in check(_run32(x0, masses, mol, p, steps, stale=True))[2]}) >= len(moving) // 2
    # alpha kept after an uphill step: the words of the step behind it
    bad = check(_run32(x0, masses, mol, p, steps, keep_alpha=True))[2]
    assert bad and bad[0][:2] in uphill and "state words" in bad[0][2]
    # the clamp skipped
    bad = check(_run32(x0, masses, mol, p, steps, skip_clamp=True))[2]
    assert bad and good[bad[0][0]]["clamped"][bad[0][1]]
    # the frozen molecule moved by one ulp
    moved = [dict(f) for f in good]
    moved[7] = dict(moved[7], x=moved[7]["x"].copy())
    moved[7]["x"][0, 1] = np.nextafter(moved[7]["x"][0, 1], np.float32(1))
    assert {(k, b) for k, b, _ in check(moved)[2]} == {(6, 0), (7, 0)}
    # an atom that never moves
    dropped = [dict(f, x=f["x"].copy(), v=f["v"].copy()) for f in good]
    for f in dropped[1:]:
        f["x"][5], f["v"][5] = good[0]["x"][5], good[0]["v"][5]
    assert len({k for k, b, _ in check(dropped)[2] if b == 2}) >= len(moving) // 2
    # and an undecidable step is skipped, not judged: a tolerance within eF of fmax at frame 0
    F0 = _anharmonic(good[0]["x"].astype(np.float64))
    near = dict(p, ftol=float(np.sqrt((F0[3:] ** 2).sum(1).max())))
    assert rt.one_step(good[0], good[1], F0, masses, mol, near, eps * np.abs(F0).max())[0][2] == "skip"


# ------------------------------------------------------------------------------------------------------ surface
def test_relax_surface_and_abi():
    import inspect
    import geossl_amd
    from geossl_amd import _lib, build, md, ops, relax, replicas
    assert "relax" in geossl_amd.__doc__ and "Minimizer" in geossl_amd.__doc__
    sig = inspect.signature(relax.Minimizer).parameters
    assert list(sig)[:4] == ["model", "graph_pred_linear", "batch", "model_3d"]
    want = dict(model_3d="schnet", masses=None, fmax=0.05, dt=0.5, dt_max=5.0, dt_min=0.01, max_step=0.1, n_min=5, f_inc=1.1,
                f_dec=0.5, alpha=0.1, f_alpha=0.99, use_graph=relax.USE_GRAPH_DEFAULT,
                steps_per_replay=relax.STEPS_PER_REPLAY_DEFAULT, max_frames=1024, energy_and_gradient=None)
    assert {k: sig[k].default for k in want} == want
    assert relax.STEPS_PER_REPLAY_DEFAULT == 4 and relax.USE_GRAPH_DEFAULT is None
    assert relax.GRAPH_DEFAULT_MAX_ATOMS == md.GRAPH_DEFAULT_MAX_ATOMS
    d = rt.DEFAULTS
    assert (d["ftol"], d["alpha_start"]) == (want["fmax"], want["alpha"]) and all(d[k] == want[k] for k in d if k in want)
    for name in ("run", "reset", "set_positions", "set_tolerance", "set_limits"):
        assert callable(getattr(relax.Minimizer, name))
    for name in ("positions", "captures"):
        assert isinstance(getattr(relax.Minimizer, name), property)
    assert relax.Relaxation._fields == ("positions", "energy", "fmax", "converged", "steps", "history")
    assert relax.History._fields == ("positions", "velocities", "energy", "fmax", "dt", "alpha", "npos", "converged", "steps")
    assert (relax.ACCEL, rt.ACCEL) == (md.ACCEL, md.ACCEL)
    doc = relax.__doc__.replace("\n", " ")
    assert "ASE" in doc and "mass-weighted" in doc and "Not built" in doc and "constraints" in doc
    # one set-up for both classes
    assert issubclass(relax.Minimizer, replicas.Replicas) and issubclass(md.Simulator, replicas.Replicas)
    for name in ("_init_fused", "_init_fallback", "_setup", "_route", "_capture", "_graph", "_force"):
        assert name not in vars(relax.Minimizer) and name not in vars(md.Simulator), name
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in FIRE_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES["geossl_fire_step"][1]) == 26 and len(_lib.PROTOTYPES["geossl_fire_active"][1]) == 4
    lib = _lib.load()
    for name in FIRE_SYMBOLS:
        assert getattr(lib, name) is not None
    assert "relax.hip" in build._sources() and build.SOURCE_FLAGS.get("relax.hip") == ["-fno-slp-vectorize"]
    for name in ("fire_step", "fire_active", "fire_frames"):
        assert callable(getattr(ops, name))
    assert (ops.FIRE_PARAM_WORDS, ops.FIRE_IPARAM_WORDS, ops.FIRE_MOL_WORDS) == (8, 4, 4)
    src = open(os.path.join(REPO, "geossl_amd", "csrc", "relax.hip")).read()
    assert "atomic" not in src[src.index("#include"):]                                    # (the code below the header comment)
    assert "GEOSSL_CHECK_LAUNCH" in src and "hipMalloc" not in src and "Synchronize" not in src
    with pytest.raises(ValueError, match="contiguous CUDA"):
        ops.fire_active(torch.zeros(3, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))


# ----------------------------------------------------------------------------------------------------- refusals
def test_refusals_say_why():
    from geossl_amd.relax import Minimizer
    ragged, hook, _ = _tethered([21, 20])
    with pytest.raises(ValueError, match="Minimizer: PaiNN runs on the interned complete pair list only.*rebuilt every step"):
        Minimizer(None, None, ragged, model_3d="painn")
    big, _, _ = _tethered([34])
    with pytest.raises(ValueError, match="complete pair list"):
        Minimizer(None, None, big, model_3d="painn")
    huge, _, _ = _tethered([256])
    with pytest.raises(ValueError, match="Minimizer: structures of at most 255 atoms"):
        Minimizer(None, None, huge, model_3d="schnet")
    with pytest.raises(ValueError, match="masses has 40 entries, the batch 41 atoms"):
        Minimizer(None, None, ragged, masses=np.ones(40), energy_and_gradient=hook)
    with pytest.raises(Exception, match="not included"):
        Minimizer(None, None, ragged, model_3d="egnn")
    with pytest.raises(ValueError, match="steps_per_replay and max_frames are at least 1"):
        Minimizer(None, None, ragged, masses=np.ones(41), steps_per_replay=0, energy_and_gradient=hook)
    with pytest.raises(ValueError, match="0 < dt_min <= dt_max"):
        Minimizer(None, None, ragged, masses=np.ones(41), dt_min=6.0, energy_and_gradient=hook)
    mz = Minimizer(None, None, ragged, masses=np.ones(41), energy_and_gradient=hook)
    with pytest.raises(ValueError, match="0 < f_dec < 1"):
        mz.set_limits(f_dec=1.5)
    assert mz._limits["f_dec"] == 0.5                              # (a refused setting changes nothing)
    with pytest.raises(ValueError, match="max_steps >= 0"):
        mz.run(-1)
    # and the Simulator still says its own name
    from geossl_amd.md import Simulator
    with pytest.raises(ValueError, match="Simulator: structures of at most 255 atoms"):
        Simulator(None, None, huge, model_3d="schnet")


def test_tolerance_and_limits_apply_to_the_following_steps():
    from geossl_amd.relax import Minimizer
    batch, hook, force = _tethered([3, 4])
    masses = np.full(7, 12.0)
    mz = Minimizer(None, None, batch, masses=masses, fmax=1e-9, steps_per_replay=1, energy_and_gradient=hook)
    first = mz.run(10, record_every=1)
    assert not bool(first.converged.any()) and first.steps.tolist() == [10, 10]
    mz.set_tolerance(1e6)
    mz.set_limits(dt_max=0.6, max_step=0.01, n_min=0)
    nxt = mz.run(5, record_every=1)
    assert bool(nxt.converged.all()) and nxt.history.positions.size(0) == 2 and torch.equal(nxt.positions, first.positions)
    mz.set_tolerance(1e-9)
    mz.reset()
    mz.set_positions(batch.positions)
    p = rt.params(ftol=1e-9, dt_max=0.6, max_step=0.01, n_min=0)
    fr = rt.minimize(batch.positions.numpy(), force, masses, batch.batch.numpy(), p, 10)
    got = mz.run(10, record_every=1).history
    assert np.abs(got.positions.numpy() - np.stack([f["x"] for f in fr])).max() <= 1e-12
    assert got.dt.max() == 0.6


# ------------------------------------------------------------------------------ the starts of the GPU trajectory cases
@pytest.mark.parametrize("name", ["schnet_B1", "schnet_B4", "schnet_ragged", "painn_B1", "painn_B4"])
def test_the_twin_runs_of_every_gpu_case_can_be_compared_on(name):
    """The twin's own fp64 runs from the start of each case of tests/relax_cases.py: the checked frames keep twice
    force_twin's cutoff margin and the head condition limit, its own steps pass the one-step check within the skip cap, dt
    has reached dt_max when the second recording starts, and the convergence run needs exactly the recorded step count,
    lowers every moving molecule's energy and - in the ragged case - freezes molecules at different steps."""
    import force_twin as tw
    import md_twin as mt
    import relax_cases as rc
    assert set(rc.CASES) == {"schnet_B1", "schnet_B4", "schnet_ragged", "painn_B1", "painn_B4"} == set(rc.CONVERGE)
    kind = rc.CASES[name][0]
    rep = rc.start_report(name)
    print(name, {k: v for k, v in rep.items()}, "limit %.2f" % mt.head_condition_limit(kind, tw.BOUNDS[kind]["energy"]))
    assert rc.start_ok(name, rep)
    assert rep["checked"] == rc.STEPS_A + rc.STEPS_B and rep["skipped"] == 0
    assert rep["margin"] >= rc.SEARCH_MARGIN >= 2 * tw.CUTOFF_MARGIN
    assert rep["converge_steps"] == rc.CONVERGE[name] and 0 < rc.CONVERGE[name] <= 200
    assert all(d > 0 for d, s in zip(rep["energy_drop"], rep["freeze_steps"]) if s > 0)
    if name == "schnet_ragged":
        assert len(set(rep["freeze_steps"])) >= 3 and rep["freeze_steps"][0] == 0
