"""CPU tests of normal-mode analysis (geossl_amd/vibrations.py): the torch route in fp64 through the energy_and_gradient hook
on closed-form surfaces, the twin's Jacobi (tests/vibrations_twin.py) against numpy.linalg.eigh with the figures the GPU
bounds are taken from, the finishing pass's reordering sensitivity, the surface and the C ABI of the four kernels, the
refusals, the choice of delta, and what tests/vibrations_cases.py records about the GPU cases."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import vibrations_twin as vt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("geossl_hessian_displace", "geossl_hessian_collect", "geossl_hessian_finish", "geossl_sym_eig_jacobi")
K = vt.K_WAVENUMBER


# ------------------------------------------------------------------------------------------------ closed forms
def _springs(sizes, springs, x):
    """Harmonic pair springs (i, j, k, r0) on global atom indices: (batch namespace, hook, numpy gradient)."""
    N = sum(sizes)
    mol = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    batch = types.SimpleNamespace(x=torch.zeros(N, dtype=torch.long), positions=torch.as_tensor(x, dtype=torch.float64).clone(),
                                  batch=mol, _sizes=list(sizes))

    def hook(pos):
        e, g = torch.zeros(len(sizes), dtype=pos.dtype), torch.zeros_like(pos)
        for i, j, k, r0 in springs:
            d = pos[j] - pos[i]
            r = d.norm()
            e[mol[i]] += 0.5 * k * (r - r0) ** 2
            f = k * (r - r0) * d / r
            g[j] += f
            g[i] -= f
        return e, g

    def gradient(p):
        return hook(torch.as_tensor(np.asarray(p, dtype=np.float64)))[1].numpy()
    return batch, hook, gradient


AXIS = np.array([0.6, -0.48, 0.64])                                   # a unit vector off every coordinate axis
DIATOMIC = dict(sizes=[2], x=np.array([0.1, 0.2, 0.3]) + np.outer([0.0, 1.1], AXIS), masses=[12.0, 15.995],
                springs=[(0, 1, 300.0, 1.1)])
LINEAR = dict(sizes=[3], x=np.array([-0.2, 0.1, 0.4]) + np.outer([-1.16, 0.0, 1.16], AXIS), masses=[15.995, 12.0, 15.995],
              springs=[(0, 1, 900.0, 1.16), (1, 2, 900.0, 1.16)])
BENT = dict(sizes=[3], x=np.array([[0.0, 0.0, 0.1], [0.76, 0.59, 0.1], [-0.76, 0.59, 0.1]]), masses=[15.995, 1.008, 1.008],
            springs=[(0, 1, 500.0, math.hypot(0.76, 0.59)), (0, 2, 500.0, math.hypot(0.76, 0.59)), (1, 2, 80.0, 1.52)])
ATOM = dict(sizes=[1], x=np.array([[0.3, -0.2, 0.9]]), masses=[4.0], springs=[])


def _run(case, **kw):
    from geossl_amd.vibrations import NormalModeAnalysis
    batch, hook, _ = _springs(case["sizes"], case["springs"], case["x"])
    nm = NormalModeAnalysis(None, None, batch, masses=np.array(case["masses"]), energy_and_gradient=hook, **kw)
    assert not nm.fused and nm.captures == 0
    return nm.run()


# central differences of these surfaces at the default step: the truncation is delta^2 / r0^2 <= 2e-6 of the Hessian
CLOSED_FORM_RTOL = 1e-5


def test_harmonic_diatomic():
    res = _run(DIATOMIC)
    mu = 12.0 * 15.995 / (12.0 + 15.995)
    f = res.frequencies[0]
    assert res.n_projected.tolist() == [5] and res.dims.tolist() == [6] and bool(res.converged.all())
    assert abs(float(f[5]) - K * math.sqrt(300.0 / mu)) <= CLOSED_FORM_RTOL * K * math.sqrt(300.0 / mu)
    assert float(f[:5].abs().max()) <= 1e-3 * float(f[5])              # (sqrt of eigenvalues at rounding level)
    assert float(res.fmax[0]) <= 1e-9 and float(res.energy[0]) <= 1e-18 and float(res.asymmetry[0]) <= 1e-4 * 300.0
    from geossl_amd.vibrations import CM1_TO_KCAL, zero_point_energy
    assert abs(float(zero_point_energy(res)[0]) - 0.5 * CM1_TO_KCAL * float(f[5])) <= 1e-12
    assert abs(CM1_TO_KCAL - 2.8591e-3) < 1e-7 and abs(K - 108.59) < 0.01


def test_linear_symmetric_triatomic():
    res = _run(LINEAR)
    mo, mc, k = 15.995, 12.0, 900.0
    want = sorted([K * math.sqrt(k / mo), K * math.sqrt(k * (mc + 2 * mo) / (mo * mc))])
    f = res.frequencies[0]
    assert res.n_projected.tolist() == [5]
    assert np.allclose(f[7:].numpy(), want, rtol=CLOSED_FORM_RTOL, atol=0)
    assert float(f[:7].abs().max()) <= 1e-2 * want[0]                  # five projected, two bends without a restoring force


def test_bent_triatomic_and_single_atom():
    res = _run(BENT)
    f = res.frequencies[0]
    assert res.n_projected.tolist() == [6] and bool((f[6:] > 50.0).all()) and float(f[:6].abs().max()) <= 1e-3 * float(f[6])
    modes = res.modes[0]
    assert float((modes.t() @ modes - torch.eye(9, dtype=torch.float64)).abs().max()) <= vt.JACOBI_ORTH * 9 * vt.U64
    one = _run(ATOM)
    assert one.n_projected.tolist() == [3] and one.eigenvalues.tolist() == [[0.0, 0.0, 0.0]] and one.sweeps.tolist() == [0]
    none = _run(BENT, project=None)
    assert none.n_projected.tolist() == [0] and np.allclose(none.frequencies[0, 6:], f[6:], rtol=1e-6, atol=0)


def _ragged():
    cases = [ATOM, DIATOMIC, LINEAR, BENT]
    sizes, x, masses, springs, off = [], [], [], [], 0
    for c in cases:
        sizes += c["sizes"]
        x.append(np.asarray(c["x"], dtype=np.float64))
        masses += c["masses"]
        springs += [(i + off, j + off, k, r0) for i, j, k, r0 in c["springs"]]
        off += c["sizes"][0]
    return cases, dict(sizes=sizes, x=np.concatenate(x), masses=masses, springs=springs)


def test_ragged_batch_of_all_four_and_every_coords_per_pass():
    cases, rag = _ragged()
    res = _run(rag)
    assert res.n_projected.tolist() == [3, 5, 5, 6] and res.dims.tolist() == [3, 6, 9, 9] and res.hessian.shape == (4, 9, 9)
    for b, c in enumerate(cases):
        one = _run(c)
        m = 3 * c["sizes"][0]
        assert torch.equal(res.hessian[b, :m, :m], one.hessian[0]) and bool((res.hessian[b, m:] == 0).all())
        scale = float(one.eigenvalues[0].abs().max())
        assert float((res.eigenvalues[b, :m] - one.eigenvalues[0]).abs().max()) <= vt.jacobi_bound(m) * 3 * scale
        assert bool(torch.isnan(res.eigenvalues[b, m:]).all())
    for C in (1, 4, 9, 40):
        assert torch.equal(_run(rag, coords_per_pass=C).hessian, res.hessian), C
    # and the torch route is the twin
    _, _, gradient = _springs(rag["sizes"], rag["springs"], rag["x"])
    from geossl_amd.vibrations import DELTA_DEFAULT
    x32 = np.asarray(rag["x"], dtype=np.float32)
    batch, hook, _ = _springs(rag["sizes"], rag["springs"], x32)
    batch.positions = batch.positions.float()
    from geossl_amd.vibrations import NormalModeAnalysis
    got = NormalModeAnalysis(None, None, batch, masses=np.array(rag["masses"]), coords_per_pass=4,
                             energy_and_gradient=lambda p: hook(p.double())).run()
    tw_ = vt.analyse(gradient, x32, rag["sizes"], rag["masses"], DELTA_DEFAULT, 4)
    assert np.abs(got.hessian.numpy() - tw_["hessian"]).max() <= 1e-12 * np.abs(tw_["hessian"]).max()
    assert got.n_projected.tolist() == tw_["n_projected"].tolist()
    for b, n in enumerate(rag["sizes"]):
        assert np.abs(got.eigenvalues[b, :3 * n].numpy() - tw_["eigenvalues"][b]).max() <= 1e-11 * np.abs(tw_["D"]).max()


# ------------------------------------------------------------------------------------------------------ Jacobi
def test_twin_jacobi_vs_lapack_and_the_sweep_cap():
    """The figures the GPU bounds and MAX_SWEEPS_DEFAULT are taken from: over the matrices of the GPU test the twin needs at
    most JACOBI_WORST_SWEEPS sweeps (0 for a diagonal and a zero matrix), deviates from numpy.linalg.eigh by at most
    JACOBI_WORST_EIG |A|_F and from orthogonality by JACOBI_WORST_ORTH m 2^-52.  The module's torch Jacobi makes the same
    sweeps."""
    from geossl_amd.vibrations import MAX_SWEEPS_DEFAULT, jacobi_eigh
    mats = vt.jacobi_matrices()
    assert sorted(m.shape[0] for m in mats.values()) == [1, 2, 3, 5, 7, 7, 63, 63, 99]
    worst = dict(sweeps=0, eig=0.0, orth=0.0)
    for name, A in mats.items():
        lam, V, sweeps, conv = vt.jacobi(A, 64)
        e = vt.eig_errors(A, lam, V)
        m = A.shape[0]
        print(name, sweeps, "eig %.2e res %.2e orth %.2f m u" % (e[0], e[1], e[2] / (m * vt.U64)))
        assert conv and e[1] <= vt.jacobi_bound(m)
        worst = dict(sweeps=max(worst["sweeps"], sweeps), eig=max(worst["eig"], e[0]), orth=max(worst["orth"], e[2] / (m * vt.U64)))
        if name in ("diagonal7", "zero5", "random1"):
            assert sweeps == 0
        if m <= 7 or name == "degenerate63":
            lt, Vt, st, ct = jacobi_eigh(A, MAX_SWEEPS_DEFAULT)
            assert (st, ct) == (sweeps, True) and np.abs(lt.numpy() - lam).max() <= vt.jacobi_bound(m) * max(np.linalg.norm(A), 1e-300)
    assert worst["sweeps"] == vt.JACOBI_WORST_SWEEPS and MAX_SWEEPS_DEFAULT == 2 * worst["sweeps"]
    assert worst["eig"] <= vt.JACOBI_WORST_EIG and worst["orth"] <= vt.JACOBI_WORST_ORTH
    assert vt.jacobi(mats["degenerate63"], 1)[2:] == (1, False)        # the cap ends the loop


def test_finish_reordering_sensitivity():
    """Forward against reversed sums in the twin's finishing pass on the GPU test's inputs: at most FINISH_C / 8 of m 2^-52
    max|D| (max|D| before projection), the same survivors; the module's torch pass lies within FINISH_C of the twin."""
    from geossl_amd import vibrations as vb
    sizes, x0, masses, H = vt.finish_inputs()
    for project in ("tr", "t", None):
        a, b = vt.finish(H, x0, masses, sizes, project, "forward"), vt.finish(H, x0, masses, sizes, project, "reverse")
        D0 = vt.finish(H, x0, masses, sizes, None)[1]
        assert a[3].tolist() == b[3].tolist() == {"tr": [3, 5, 6, 6, 5], "t": [3] * 5, None: [0] * 5}[project]
        Hm = np.where(H == -7.0, 0.0, H)
        got = vb.finish(torch.from_numpy(Hm), torch.from_numpy(x0), torch.from_numpy(masses), sizes, project)
        assert np.array_equal(got[0].numpy(), a[0]) and got[3].tolist() == a[3].tolist() and np.array_equal(got[2].numpy(), a[2])
        for i, n in enumerate(sizes):
            unit = 3 * n * vt.U64 * np.abs(D0[i]).max()
            s = np.abs(a[1][i] - b[1][i]).max() / unit
            print(project, n, "sensitivity %.3f" % s)
            assert s <= vt.FINISH_C / 8
            assert np.abs(got[1][i].numpy() - a[1][i]).max() <= vt.FINISH_C * unit


# ------------------------------------------------------------------------------------------------------ surface
def test_vibrations_surface_and_abi():
    import inspect
    from geossl_amd import _lib, build, ops, replicas, vibrations as vb
    sig = inspect.signature(vb.NormalModeAnalysis).parameters
    assert list(sig)[:4] == ["model", "graph_pred_linear", "batch", "model_3d"]
    want = dict(model_3d="schnet", masses=None, delta=vb.DELTA_DEFAULT, coords_per_pass=None, project="tr", use_graph=None,
                max_sweeps=vb.MAX_SWEEPS_DEFAULT, energy_and_gradient=None)
    assert {k: sig[k].default for k in want} == want
    assert issubclass(vb.NormalModeAnalysis, replicas.Replicas)
    for name in ("_setup", "_route", "_init_fused", "_init_fallback", "_capture", "_graph", "set_positions"):
        assert name not in vars(vb.NormalModeAnalysis), name
    for name in ("run", "set_positions", "set_delta"):
        assert callable(getattr(vb.NormalModeAnalysis, name))
    assert isinstance(vb.NormalModeAnalysis.captures, property)
    assert vb.NormalModes._fields == ("hessian", "dims", "eigenvalues", "frequencies", "modes", "n_projected", "asymmetry",
                                      "energy", "fmax", "sweeps", "converged")
    assert (vb.K_WAVENUMBER, vb.DROP_TOL) == (vt.K_WAVENUMBER, vt.DROP_TOL)
    doc = vb.__doc__.replace("\n", " ")
    assert "project's own definition" in doc and "Not built" in doc and "torch.linalg.eigh" in doc
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS + ("geossl_hessian_finish_workspace",):
        assert re.search(r"\b(int|int64_t) %s\(" % name, h), name
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    assert [len(_lib.PROTOTYPES[s][1]) for s in SYMBOLS] == [9, 14, 13, 10]
    assert "vibrations.hip" in build._sources() and build.SOURCE_FLAGS.get("vibrations.hip") == ["-fno-slp-vectorize"]
    for name in ("hessian_displace", "hessian_collect", "hessian_finish", "sym_eig_jacobi"):
        assert callable(getattr(ops, name))
    assert (ops.JACOBI_MAX_DIM, ops.HESSIAN_STATE_WORDS) == (99, 4)
    src = open(os.path.join(REPO, "geossl_amd", "csrc", "vibrations.hip")).read()
    code = src[src.index("#include"):]
    assert "atomic" not in code and "while" not in code                  # no atomics; every loop is a counted `for`
    assert "GEOSSL_CHECK_LAUNCH" in src and "hipMalloc" not in src and "Synchronize" not in src
    assert "Skip rule" in src and "Stop rule" in src and "Rotation of a pair" in src
    with pytest.raises(ValueError, match="contiguous CUDA"):
        ops.sym_eig_jacobi(torch.zeros(1, 3, 3, dtype=torch.float64), torch.zeros(1, dtype=torch.int32), 4)


def test_refusals_say_why():
    from geossl_amd.vibrations import NormalModeAnalysis
    mk = lambda sizes: _springs(sizes, [], np.zeros((sum(sizes), 3)))
    ragged, hook, _ = mk([21, 20])
    with pytest.raises(ValueError, match="NormalModeAnalysis: PaiNN runs on the interned complete pair list only"):
        NormalModeAnalysis(None, None, ragged, model_3d="painn")
    with pytest.raises(ValueError, match="complete pair list"):
        NormalModeAnalysis(None, None, mk([34])[0], model_3d="painn")
    with pytest.raises(ValueError, match="NormalModeAnalysis: structures of at most 255 atoms"):
        NormalModeAnalysis(None, None, mk([256])[0], model_3d="schnet")
    with pytest.raises(ValueError, match="masses has 40 entries, the batch 41 atoms"):
        NormalModeAnalysis(None, None, ragged, masses=np.ones(40), energy_and_gradient=hook)
    with pytest.raises(Exception, match="not included"):
        NormalModeAnalysis(None, None, ragged, model_3d="egnn")
    with pytest.raises(ValueError, match="project is 'tr', 't' or None"):
        NormalModeAnalysis(None, None, ragged, masses=np.ones(41), project="r", energy_and_gradient=hook)
    with pytest.raises(ValueError, match="coords_per_pass is at least 1"):
        NormalModeAnalysis(None, None, ragged, masses=np.ones(41), coords_per_pass=0, energy_and_gradient=hook)
    nm = NormalModeAnalysis(None, None, ragged, masses=np.ones(41), energy_and_gradient=hook)
    with pytest.raises(ValueError, match="delta is positive"):
        nm.set_delta(0.0)
    assert nm.delta == vt_delta()


def vt_delta():
    from geossl_amd.vibrations import DELTA_DEFAULT
    return DELTA_DEFAULT


# -------------------------------------------------------------------------------------------- the GPU cases
@pytest.mark.parametrize("name", ["schnet_9", "schnet_ragged", "painn_9x2"])
def test_every_displaced_image_of_a_gpu_case_keeps_the_cutoff_margin(name):
    """A property of the inputs alone: the recorded seed is the first from SEARCH_FROM on which every image of every round
    at the default delta keeps force_twin.CUTOFF_MARGIN."""
    import force_twin as tw
    import vibrations_cases as vc
    assert set(vc.CASES) == {"schnet_9", "schnet_ragged", "painn_9x2"}
    assert [vc.CASES[k][1] for k in ("schnet_9", "schnet_ragged", "painn_9x2")] == [[9], [1, 2, 9, 21], [9, 9]]
    margin = vc.images_margin(name, vt_delta())
    print(name, "margin %.4g" % margin)
    assert margin >= tw.CUTOFF_MARGIN and vc.first_start(name, vt_delta()) == vc.CASES[name][2]


def test_delta_default_minimises_truncation_plus_force_noise_and_a_short_run_is_seen():
    """Over the three end-to-end cases, on the twin: the measured truncation against torch.autograd.functional.hessian of
    the twin plus BOUNDS max|F| / delta (both relative to max|H|), summed, is least at DELTA_DEFAULT among delta / 2, delta,
    2 delta (DESIGN 4 has the whole table).  And the tooth: the twin's own Hessian passes the element check of the GPU
    test with room, the same Hessian one round short does not."""
    import force_twin as tw
    import vibrations_cases as vc
    d0 = vt_delta()
    total = {d: 0.0 for d in (0.5 * d0, d0, 2 * d0)}
    for name in vc.CASES:
        twin = vc.Twin(name)
        Ha = twin.analytic_hessian()
        scale = np.abs(Ha).max()
        F = np.abs(twin.gradient(twin.raw["positions"])).max()
        for d in total:
            H, imgs, grads = vt.hessian(twin.gradient, twin.raw["positions"], twin.sizes, d, 1)
            trunc, noise = np.abs(H - Ha).max() / scale, tw.BOUNDS[twin.kind]["force"] * F / d / scale
            print(name, "delta %.6f truncation %.3e noise %.3e" % (d, trunc, noise))
            total[d] += trunc + noise
            if d == d0 and name == "schnet_ragged":
                eps = tw.BOUNDS[twin.kind]["force"]
                g32 = [g.astype(np.float32).astype(np.float64) for g in grads]          # a pass that rounds to fp32
                H32 = np.zeros_like(H)
                for r, (im, g) in enumerate(zip(imgs, g32)):
                    vt.collect(H32, im, g, twin.sizes, 1, r)
                assert vt.element_check(twin.sizes, eps, H32, H, imgs, grads) <= 0.1
                short = vt.hessian(twin.gradient, twin.raw["positions"], twin.sizes, d, 4, n_rounds=vt.rounds(twin.sizes, 4) - 1)[0]
                assert vt.element_check(twin.sizes, eps, short, H, imgs, grads) > 1.0
    print({k: "%.3e" % v for k, v in total.items()})
    assert total[d0] == min(total.values())
