"""Normal-mode analysis on the GPU (geossl_amd/vibrations.py, csrc/vibrations.hip): the displacement and collect kernels
alone with made-up gradients against the twin (tests/vibrations_twin.py), the finishing pass alone, the batched Jacobi alone
against LAPACK, and the replayed analysis of SchNet and PaiNN force fields end to end against the twin's finite-difference
Hessian on the same rounded images."""
import numpy as np
import pytest
import torch

import force_twin as tw
import vibrations_cases as vc
import vibrations_twin as vt
from md_cases import _cfg, device_batch, device_modules, module_snapshot as _snapshot
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7.0
KERNEL_SIZES = vt.KERNEL_SIZES
FINISH_C, JACOBI_ORTH, jacobi_bound = vt.FINISH_C, vt.JACOBI_ORTH, vt.jacobi_bound   # (derived in vibrations_twin.py)


def _np(t):
    return t.detach().cpu().numpy()


def _mol_ptr(sizes):
    return torch.tensor(vt.mol_ptr(sizes), dtype=torch.int32, device=DEV)


# --------------------------------------------------------------------------------- displace and collect alone
@pytest.mark.parametrize("C", [1, 4, 64])
def test_displace_and_collect_vs_twin(C):
    """Sizes [1, 2, 9, 21] (M = 63), C = 1, 4 (divides neither 63 nor 3, 6, 27) and 64 (a single round), random fp32
    gradients: every round's images equal the twin's bit for bit (undisplaced images equal x0), the collected rows equal
    the twin's to the rounding of one subtraction and one division, rows and columns past 3 n_b keep the sentinel, the
    round words advance, and round R writes energy and fmax of image 0 and no row."""
    from geossl_amd import ops
    sizes, delta = KERNEL_SIZES, 0.005
    g = torch.Generator().manual_seed(11 + C)
    N, B, M = sum(sizes), len(sizes), 3 * max(sizes)
    R = vt.rounds(sizes, C)
    assert R == -(-M // C) and (C != 64 or R == 1)
    x0 = (1.5 * torch.randn(N, 3, generator=g)).to(DEV)
    ptr = _mol_ptr(sizes)
    dl = torch.tensor([delta], dtype=torch.float32, device=DEV)
    state = torch.zeros(4, dtype=torch.int64, device=DEV)
    img = torch.full((2 * C, N, 3), SENT, device=DEV)
    H = torch.full((B, M, M), SENT, dtype=torch.float64, device=DEV)
    energy = torch.full((B,), SENT, dtype=torch.float64, device=DEV)
    fmax = torch.full((B,), SENT, dtype=torch.float64, device=DEV)
    Ht = np.full((B, M, M), SENT)
    x0n = _np(x0)
    for r in range(R + 1):
        grad = (10.0 * torch.randn(2 * C * N, 3, generator=g)).to(DEV)
        e_img = torch.randn(2 * C * B, generator=g).to(DEV)
        ops.hessian_displace(x0, ptr, dl, state, C, img)
        torch.cuda.synchronize()
        want = vt.images(x0n, sizes, delta, C, r)
        assert np.array_equal(_np(img), want), r
        assert state.tolist() == [r, r, 0, 0]
        if r == R:
            assert np.array_equal(want, np.repeat(x0n[None], 2 * C, axis=0))
            before = H.clone()
            assert bool((energy == SENT).all()) and bool((fmax == SENT).all())
        ops.hessian_collect(x0, img, grad, e_img, ptr, state, C, R, H, energy, fmax)
        torch.cuda.synchronize()
        assert state.tolist() == [r + 1, r, 0, 0]
        if r < R:
            vt.collect(Ht, want, _np(grad).reshape(2 * C, N, 3), sizes, C, r)
        else:
            assert torch.equal(H, before)
            e_ref, f_ref = vt.reference_point(_np(grad)[:N], _np(e_img)[:B], sizes)
            assert np.array_equal(_np(energy), e_ref)
            assert np.abs(_np(fmax) - f_ref).max() <= 4 * vt.U64 * f_ref.max()
    got = _np(H)
    for b, n in enumerate(sizes):
        m = 3 * n
        blk, ref = got[b, :m, :m], Ht[b, :m, :m]
        assert (ref != SENT).all() and np.abs(blk - ref).max() <= 2 * vt.U64 * np.abs(ref).max()
        assert (np.abs(blk - ref) <= 2 * vt.U64 * np.abs(ref)).all()
        assert (got[b, m:, :] == SENT).all() and (got[b, :, m:] == SENT).all()
    # displaced coordinates really moved, by the rounded step
    first = vt.images(x0n, sizes, delta, C, 0)
    assert np.abs(first[0] - x0n).max() > 0.004 and np.abs(first[1] - x0n).max() > 0.004
    # a round word beyond R displaces nothing and collects nothing
    ops.hessian_displace(x0, ptr, dl, state, C, img)
    ops.hessian_collect(x0, img, grad, e_img, ptr, state, C, R, H, energy, fmax)
    torch.cuda.synchronize()
    assert np.array_equal(_np(img), np.repeat(x0n[None], 2 * C, axis=0)) and np.array_equal(_np(H), got)
    assert state.tolist() == [R + 2, R + 1, 0, 0]


# ----------------------------------------------------------------------------------------------- finish alone
@pytest.mark.parametrize("project", ["tr", "t", None])
def test_finish_vs_twin(project):
    """Sizes [1, 2, 9, 21] and a collinear 3-atom molecule, random non-symmetric H with a sentinel outside the blocks:
    asymmetry and the symmetrised H equal the twin's exactly, n_projected is [3, 5, 6, 6, 5] / 3 / 0, D lies within
    FINISH_C m 2^-52 max|D| of the twin's, D is exactly symmetric and both are zero outside the blocks."""
    from geossl_amd import ops
    sizes, x0, masses, H = vt.finish_inputs()
    B, M = H.shape[0], H.shape[1]
    Hd = torch.from_numpy(H).to(DEV)
    D = torch.full((B, M, M), SENT, dtype=torch.float64, device=DEV)
    asym = torch.full((B,), SENT, dtype=torch.float64, device=DEV)
    nproj = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    ops.hessian_finish(Hd, torch.from_numpy(x0).to(DEV), torch.from_numpy(masses).to(DEV), _mol_ptr(sizes), project, D,
                       asym, nproj)
    torch.cuda.synchronize()
    Hs, Dt, at, nt = vt.finish(H, x0, masses, sizes, project)
    _, D0, _, _ = vt.finish(H, x0, masses, sizes, None)
    assert np.array_equal(_np(asym), at) and np.array_equal(_np(Hd), Hs)
    want = {"tr": [3, 5, 6, 6, 5], "t": [3] * 5, None: [0] * 5}[project]
    assert _np(nproj).tolist() == want == nt.tolist()
    got = _np(D)
    assert np.array_equal(got, np.swapaxes(got, 1, 2))
    for b, n in enumerate(sizes):
        m = 3 * n
        err = np.abs(got[b] - Dt[b]).max() / (m * vt.U64 * np.abs(D0[b]).max())
        print(project, n, "D error %.3f of m u max|D|" % err)
        assert err <= FINISH_C, (b, err)
        assert (got[b, m:, :] == 0).all() and (got[b, :, m:] == 0).all()
    if project is None:
        assert np.array_equal(got, Dt)


# ----------------------------------------------------------------------------------------------- Jacobi alone
def _jacobi_batch(names=None):
    mats = vt.jacobi_matrices()
    names = sorted(mats) if names is None else names
    M = max(mats[k].shape[0] for k in names)
    A = np.full((len(names), M, M), np.nan)
    dims = np.array([mats[k].shape[0] for k in names], dtype=np.int32)
    for b, k in enumerate(names):
        A[b, :dims[b], :dims[b]] = mats[k]
    return names, mats, A, dims


def test_jacobi_vs_lapack():
    """The CPU test's matrices as one ragged batch (NaN outside every block: nothing there is read): eigenvalues within
    jacobi_bound(m) |A|_F of numpy.linalg.eigh, |A V - V L|_max likewise, |V^T V - I|_max <= JACOBI_ORTH m 2^-52, sweeps
    within the cap, converged set, zero sweeps for the diagonal and the zero matrix, NaN / zeros past dims."""
    from geossl_amd import ops
    from geossl_amd.vibrations import MAX_SWEEPS_DEFAULT
    names, mats, A, dims = _jacobi_batch()
    lam, V, sweeps, conv = ops.sym_eig_jacobi(torch.from_numpy(A).to(DEV), torch.from_numpy(dims).to(DEV),
                                               MAX_SWEEPS_DEFAULT)
    torch.cuda.synchronize()
    lam, V, sweeps, conv = _np(lam), _np(V), _np(sweeps), _np(conv)
    for b, k in enumerate(names):
        m = int(dims[b])
        e = vt.eig_errors(mats[k], lam[b, :m], V[b, :m, :m])
        print(k, "sweeps", sweeps[b], "eig %.2e res %.2e orth %.2f m u" % (e[0], e[1], e[2] / (m * vt.U64)))
        assert conv[b] == 1 and 0 <= sweeps[b] <= MAX_SWEEPS_DEFAULT, k
        assert e[0] <= jacobi_bound(m) and e[1] <= jacobi_bound(m) and e[2] <= JACOBI_ORTH * m * vt.U64, (k, e)
        assert (np.diff(lam[b, :m]) >= 0).all() and np.isnan(lam[b, m:]).all()
        assert (V[b, m:, :] == 0).all() and (V[b, :, m:] == 0).all()
        if k in ("diagonal7", "zero5", "random1"):
            assert sweeps[b] == 0
    assert sweeps.max() >= 8


def test_jacobi_sweep_cap_ends_the_loop():
    from geossl_amd import ops
    names, mats, A, dims = _jacobi_batch(["degenerate63", "diagonal7"])
    lam, V, sweeps, conv = ops.sym_eig_jacobi(torch.from_numpy(A).to(DEV), torch.from_numpy(dims).to(DEV), 1)
    torch.cuda.synchronize()
    assert sweeps.tolist() == [1, 0] and conv.tolist() == [0, 1]
    with pytest.raises(ValueError, match="device eigensolver"):
        ops.sym_eig_jacobi(torch.zeros(1, 100, 100, dtype=torch.float64, device=DEV),
                           torch.tensor([100], dtype=torch.int32, device=DEV), 4)


# ------------------------------------------------------------------------------------------------- end to end
def _same(a, b):
    """Bit-identical results (NaN past dims equal to NaN)."""
    return all(torch.equal(torch.nan_to_num(x, nan=-1e300), torch.nan_to_num(y, nan=-1e300)) if x.is_floating_point()
               else torch.equal(x, y) for x, y in zip(a, b))


def _element_check(twin, hessian, Ht, imgs, grads):
    return vt.element_check(twin.sizes, tw.BOUNDS[twin.kind]["force"], hessian, Ht, imgs, grads)


@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_analysis_meets_the_twin(name):
    """The MD17 configurations of tests/md_cases.py at the default delta: every Hessian element within the force bound's
    share of the twin's finite-difference Hessian on the same rounded images, every eigenvalue within m max|dD| (Weyl) plus
    the eigensolver's bound of the twin's, replayed and eager runs bit-identical, one capture and none after
    set_positions / set_delta, and a run one round short is seen by the element check."""
    from geossl_amd.vibrations import DELTA_DEFAULT, NormalModeAnalysis
    kind, sizes, seed = vc.CASES[name]
    cfg = _cfg(kind)
    model, head = device_modules(kind, cfg, DEV)
    twin = vc.Twin(name, snapshot=_snapshot(model, head), device=DEV)
    bt = device_batch(kind, cfg, twin.raw, DEV)
    C = 40 if name == "schnet_ragged" else None                      # (two rounds, the second one partly empty)
    nm = NormalModeAnalysis(model, head, bt, model_3d=kind, coords_per_pass=C)
    assert nm.fused and nm.delta == DELTA_DEFAULT and nm.rounds == (2 if C else 1)
    res = nm.run()
    eager = NormalModeAnalysis(model, head, bt, model_3d=kind, use_graph=False, coords_per_pass=C)
    ref = eager.run()
    torch.cuda.synchronize()
    assert nm.captures == 1 and eager.captures == 0 and _same(res, ref)
    # the twin: C = 1 (a row depends on its own image pair alone)
    Hraw, imgs, grads = vt.hessian(twin.gradient, twin.raw["positions"], sizes, DELTA_DEFAULT, 1)
    Ht, Dt, _, nt = vt.finish(Hraw, twin.raw["positions"], twin.masses, sizes, "tr")
    H = _np(res.hessian)
    worst = _element_check(twin, H, Ht, imgs, grads)
    print(name, "C", nm.coords_per_pass, "rounds", nm.rounds, "worst element %.3f of its tolerance" % worst,
          "max|H| %.4g" % np.abs(Ht).max(), "asymmetry", _np(res.asymmetry), "sweeps", _np(res.sweeps))
    assert worst <= 1.0
    assert _np(res.n_projected).tolist() == nt.tolist() and _np(res.dims).tolist() == [3 * n for n in sizes]
    assert bool(res.converged.all())
    _, Dd, _, _ = vt.finish(H, twin.raw["positions"], twin.masses, sizes, "tr")
    _, D0, _, _ = vt.finish(H, twin.raw["positions"], twin.masses, sizes, None)
    lam = _np(res.eigenvalues)
    for b, n in enumerate(sizes):
        m = 3 * n
        want = np.linalg.eigvalsh(Dt[b, :m, :m])
        # Weyl on the Hessian's error, on the finishing pass's own tolerance (the device's D against Dd), and the solver
        tol = (m * np.abs(Dd[b] - Dt[b]).max() + m * FINISH_C * m * vt.U64 * np.abs(D0[b]).max()
               + jacobi_bound(m) * np.linalg.norm(Dd[b]))
        assert np.abs(lam[b, :m] - want).max() <= tol, (b, np.abs(lam[b, :m] - want).max(), tol)
        assert np.isnan(lam[b, m:]).all()
    e0, f0 = vt.reference_point(twin.gradient(twin.raw["positions"]), np.zeros(len(sizes)), sizes)
    gmax = np.abs(grads[0]).max()
    assert np.abs(_np(res.fmax) - f0).max() <= 2 * tw.BOUNDS[kind]["force"] * gmax
    # a new geometry and a new step are data: no capture; the old ones again give the first result again
    nm.set_positions(bt.positions + 0.01)
    nm.set_delta(0.01)
    moved = nm.run()
    assert nm.captures == 1 and not torch.equal(moved.hessian, res.hessian)
    nm.set_positions(bt.positions)
    nm.set_delta(DELTA_DEFAULT)
    assert _same(nm.run(), res) and nm.captures == 1
    # the tooth: a run one round short leaves rows the element check sees
    short = _np(nm._run_fused(nm.rounds - 1)[0])
    torch.cuda.synchronize()
    assert _element_check(twin, short, Ht, imgs, grads) > 1.0


def test_above_the_device_eigensolver_eigh_on_the_cpu():
    """SchNet with 34 atoms (M = 102 > 99): the eigenvalues are torch.linalg.eigh's of the run's own D, sweeps 0."""
    from geossl_amd.vibrations import NormalModeAnalysis
    from md_cases import _raw
    cfg = _cfg("schnet")
    model, head = device_modules("schnet", cfg, DEV)
    raw = _raw([34], 941, cfg["cutoff"])
    nm = NormalModeAnalysis(model, head, device_batch("schnet", cfg, raw, DEV), coords_per_pass=51)
    res = nm.run()
    torch.cuda.synchronize()
    assert nm.fused and nm.rounds == 2 and res.sweeps.tolist() == [0] and bool(res.converged.all())
    _, D, _, nproj = vt.finish(_np(res.hessian), raw["positions"], nm.masses.numpy(), [34], "tr")
    want = np.linalg.eigvalsh(D[0])
    assert nproj.tolist() == [6] == res.n_projected.tolist()
    D0 = vt.finish(_np(res.hessian), raw["positions"], nm.masses.numpy(), [34], None)[1]
    # Weyl on the finishing pass's tolerance, plus LAPACK against LAPACK (1e-14 |D|_F)
    assert np.abs(_np(res.eigenvalues)[0] - want).max() <= (102 * FINISH_C * 102 * vt.U64 * np.abs(D0).max()
                                                            + 1e-14 * np.linalg.norm(D[0]))
