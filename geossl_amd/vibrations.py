"""Normal-mode analysis on a fine-tuned MD17 force field: the Hessian of the model's own energy surface at the geometry of
every molecule of a batch, by central differences of the replayed force pass, then harmonic frequencies and normal modes
from a batched eigensolver that stays on the device.

``NormalModeAnalysis(model, graph_pred_linear, batch, model_3d)`` takes the same batches as ``md.Simulator`` and
``relax.Minimizer`` (a collated batch with host sizes or a ``DeviceLoader`` handle; ragged sizes allowed).  ``run()`` returns
a ``NormalModes``; ``set_positions`` takes a new geometry (a ``Minimizer``'s relaxed positions:
``examples/vibrations_md17.py --relax_first``) and ``set_delta`` a new step, both without a new capture.

The algorithm is this project's own definition.  With C = ``coords_per_pass``, the force pass runs on an IMAGE BATCH of
2 C copies of the user's batch.  In round r, for every molecule b and c < C, with k = r C + c: image (c, +) holds coordinate k
of molecule b at fl32(x0_k + delta), image (c, -) at fl32(x0_k - delta), everything else at x0; an image with k >= 3 n_b is
left undisplaced and never read.  Row k of H_b is (g+ - g-) / (x+_k - x-_k), formed in fp64 from the fp32 gradients and the
fp32 positions actually written (the denominator is the real difference of the two rounded coordinates, not 2 delta).
R = ceil(3 n_max / C) rounds fill H; one more replay, with the round word at R, displaces nothing and takes ``energy`` and
``fmax`` from image 0.  Finishing, all in fp64 and in a fixed order:

  1. asymmetry = max |H - H^T|                          2. H <- (H + H^T) / 2
  3. D_ij = H_ij / sqrt(m_i m_j)
  4. the three translations sqrt(m_i) e_a and the three rotations sqrt(m_i) e_a x (x_i - com) about the centre of mass
  5. orthonormalised by modified Gram-Schmidt in the order Tx Ty Tz Rx Ry Rz
  6. a vector is dropped unless its remaining norm is above DROP_TOL = 1e-5 of its own norm (a linear molecule loses one
     rotation, a single atom all three)
  7. n_projected = the survivors                          8. D <- P D P,  P = I - sum v v^T

and D is eigen-decomposed: eigenvalues ascending, frequencies sign(lambda) sqrt(|lambda|) K in cm^-1 (imaginary modes are
reported negative), K = sqrt(4.184e26) / (2 pi 2.99792458e10).

On the fused route - exactly what ``Simulator.fused`` serves: SchNet up to 255 atoms with ragged sizes, PaiNN on the interned
complete pair list (one size n <= 33; the image batch lands on ``complete_edges(2 C B, n)``), the heads the energy-head
kernel takes - one round is ``geossl_hessian_displace`` -> the force pass of ``finetune_md17._energy_and_gradient`` on the
image batch -> ``geossl_hessian_collect`` (csrc/vibrations.hip), captured once as ONE graph.  ``run()`` resets the round word,
replays the graph R + 1 times, then launches ``geossl_hessian_finish`` and ``geossl_sym_eig_jacobi`` (cyclic Jacobi in
round-robin order, one block per matrix, stop at max off-diagonal <= 2^-50 |A|_F or after ``max_sweeps`` sweeps).  The host
reads nothing before the result.  delta and the round word are device data; the graph reads the live parameter values of the
modules (it is rebuilt when their addresses move).  For 3 n_max > 99 (SchNet above 33 atoms) the eigensolver is
``torch.linalg.eigh`` on a CPU copy of D in fp64: ``sweeps`` is 0 and ``converged`` True there.

The fallback route - CPU tensors, a head or width the kernels do not serve, or an ``energy_and_gradient=callable(positions)
-> (E [B], dE/dpos [N, 3])`` hook - is the same algorithm in torch operations in the dtype of the positions (fp64 allowed), one
force call per image, with the same Jacobi in torch.

Not built: an analytic Hessian through the tape, higher-order stencils, IR intensities, thermochemistry beyond the zero-point
energy, structures above 255 atoms, PaiNN off the complete pair list (both refused with the Simulator's sentences), and the
device eigensolver above dimension 99."""
import math
from collections import namedtuple

import torch

from . import _lib, ops
from .batch import Batch
from .finetune_md17 import _collated
from .replicas import Replicas, _host_sizes, default_masses

__all__ = ["NormalModeAnalysis", "NormalModes", "cartesian_modes", "zero_point_energy", "DELTA_DEFAULT",
           "MAX_SWEEPS_DEFAULT", "IMAGE_ATOMS_DEFAULT", "USE_GRAPH_DEFAULT", "DROP_TOL", "K_WAVENUMBER", "CM1_TO_KCAL"]

# delta: the minimum of (measured truncation against the twin's analytic Hessian) + (BOUNDS max|F| / delta) over the three
# end-to-end cases of tests/test_gpu_vibrations.py, on the CPU from the fp64 twin (DESIGN 4 has both curves).
DELTA_DEFAULT = 0.00125
# twice the worst sweep count (11, the degenerate spectrum) of the twin's Jacobi over the matrices of
# tests/test_vibrations_cpu.py.
MAX_SWEEPS_DEFAULT = 22
# Measured defaults (tools/bench_vibrations.py, profiles/vibrations_bench.json).  coords_per_pass None: the
# largest C <= 3 n_max whose image batch has at most IMAGE_ATOMS_DEFAULT atoms (at least 1).  Every measured shape got faster
# with every larger C: one 21-atom molecule is fastest at C = 63 = 3 n (2646 image atoms; SchNet 22.1 / 6.0 / 4.4 / 3.9 ms
# at C = 1 / 8 / 21 / 63), 64 molecules at the largest C measured, 4 (10752 image atoms; SchNet 32.1 / 25.9 / 19.8 ms at
# C = 1 / 2 / 4) - so the cap is the largest image batch that was measured.  use_graph None: replay - the slowest replayed
# run beat the fastest eager run of the same C on every shape but PaiNN at 64 molecules, where the two lie within 0.5 %.
IMAGE_ATOMS_DEFAULT = 2 * 4 * 64 * 21
USE_GRAPH_DEFAULT = None
DROP_TOL = 1e-5
K_WAVENUMBER = math.sqrt(4.184e26) / (2.0 * math.pi * 2.99792458e10)   # sqrt(kcal/mol/A^2/amu) -> cm^-1: 108.59
CM1_TO_KCAL = 6.62607015e-34 * 2.99792458e10 * 6.02214076e23 / 4184.0  # h c N_A: cm^-1 -> kcal/mol

NormalModes = namedtuple("NormalModes", "hessian dims eigenvalues frequencies modes n_projected asymmetry energy fmax "
                                        "sweeps converged")
NormalModes.__doc__ = """``NormalModeAnalysis.run``'s result, M = 3 n_max: hessian [B, M, M] fp64, the symmetrised Cartesian
Hessian in kcal/mol/A^2 (zero outside each molecule's 3 n_b block); dims [B] = 3 n_b; eigenvalues [B, M] fp64 of the
mass-weighted projected Hessian, ascending, NaN past dims; frequencies [B, M] in cm^-1, imaginary ones negative; modes
[B, M, M], mass-weighted eigenvectors in columns; n_projected [B], the translation / rotation vectors removed; asymmetry [B],
max |H - H^T| before symmetrising; energy [B] and fmax [B] at the reference geometry; sweeps [B] and converged [B] of the
eigensolver."""


# ------------------------------------------------------------------------------------------- the torch restatement
def round_pairs(n2, t):
    """The n2 / 2 disjoint pairs (p < q) of round t of the round-robin order over n2 (even) players: slot 0 is
    (n2 - 1, t), slot k is ((t + k) mod (n2 - 1), (t - k) mod (n2 - 1))."""
    w = n2 - 1
    k = torch.arange(1, n2 // 2)
    a = torch.cat([torch.tensor([w]), (t + k) % w])
    c = torch.cat([torch.tensor([t]), (t - k) % w])
    return torch.minimum(a, c), torch.maximum(a, c)


def jacobi_eigh(A, max_sweeps=MAX_SWEEPS_DEFAULT):
    """csrc/vibrations.hip's Jacobi on one symmetric fp64 matrix in torch operations -> (eigenvalues ascending, vectors
    in columns, sweeps, converged)."""
    A = torch.as_tensor(A, dtype=torch.float64).cpu()
    m = A.size(0)
    n2 = m + (m & 1)
    S = torch.zeros(n2, n2, dtype=torch.float64)
    S[:m, :m] = torch.triu(A) + torch.triu(A, 1).t()
    V = torch.eye(n2, dtype=torch.float64)
    thr = 2.0 ** -50 * float(S.norm())
    sweeps, conv = 0, False
    for it in range(int(max_sweeps) + 1):
        off = float(torch.triu(S, 1).abs().max()) if m > 1 else 0.0
        if off <= thr:
            conv = True
            break
        if it == max_sweeps:
            break
        for t in range(n2 - 1):
            p, q = round_pairs(n2, t)
            apq = S[p, q]
            act = (q < m) & (apq.abs() > 0.25 * thr)
            theta = (S[q, q] - S[p, p]) / (2.0 * torch.where(act, apq, torch.ones_like(apq)))
            sgn = torch.where(theta >= 0, torch.ones_like(theta), -torch.ones_like(theta))
            tt = torch.where(act, sgn / (theta.abs() + torch.sqrt(theta * theta + 1.0)), torch.zeros_like(theta))
            c = 1.0 / torch.sqrt(tt * tt + 1.0)
            s = tt * c
            app, aqq = S[p, p] - tt * apq, S[q, q] + tt * apq
            Sp, Sq = S[:, p].clone(), S[:, q].clone()
            S[:, p], S[:, q] = c * Sp - s * Sq, s * Sp + c * Sq
            Sp, Sq = S[p, :].clone(), S[q, :].clone()
            S[p, :], S[q, :] = c[:, None] * Sp - s[:, None] * Sq, s[:, None] * Sp + c[:, None] * Sq
            S[p, p], S[q, q] = app, aqq
            S[p, q] = torch.where(act, torch.zeros_like(apq), apq)
            S = torch.triu(S) + torch.triu(S, 1).t()
            Vp, Vq = V[:, p].clone(), V[:, q].clone()
            V[:, p], V[:, q] = c * Vp - s * Vq, s * Vp + c * Vq
        sweeps += 1
    lam = torch.diagonal(S)[:m]
    order = torch.sort(lam, stable=True).indices
    return lam[order].clone(), V[:m, :m][:, order].clone(), sweeps, conv


def projection_vectors(x, masses, project):
    """Steps 4 - 7 for one molecule: x [n, 3], masses [n] fp64 -> the kept orthonormal vectors [p, 3 n]."""
    n = x.size(0)
    if project is None or n == 0:
        return torch.zeros(0, 3 * n, dtype=torch.float64)
    w = masses.sqrt()
    raw = []
    for a in range(3):
        v = torch.zeros(n, 3, dtype=torch.float64)
        v[:, a] = w
        raw.append(v.reshape(-1))
    if project == "tr":
        r = x - (masses[:, None] * x).sum(0) / masses.sum()
        for a in range(3):
            e = torch.zeros(3, dtype=torch.float64)
            e[a] = 1.0
            raw.append((w[:, None] * torch.linalg.cross(e.expand(n, 3), r)).reshape(-1))
    kept = []
    for v in raw:
        n0 = float(v.norm())
        for u in kept:
            v = v - (u @ v) * u
        n1 = float(v.norm())
        if n1 > DROP_TOL * n0:
            kept.append(v / n1)
    return torch.stack(kept) if kept else torch.zeros(0, 3 * n, dtype=torch.float64)


def finish(H, x0, masses, sizes, project):
    """The finishing pass in torch: H [B, M, M] fp64 raw rows, x0 [N, 3], masses [N] -> (H symmetrised, D, asymmetry [B],
    n_projected [B]); everything outside the 3 n_b blocks zero."""
    B, M = H.size(0), H.size(1)
    Hs, D = torch.zeros_like(H), torch.zeros_like(H)
    asym, nproj = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.int64)
    a0 = 0
    for b, n in enumerate(sizes):
        m = 3 * n
        h = H[b, :m, :m]
        asym[b] = (h - h.t()).abs().max() if m else 0.0
        h = 0.5 * (h + h.t())
        mw = masses[a0:a0 + n].double().repeat_interleave(3)
        d = h / torch.sqrt(mw[:, None] * mw[None, :])
        V = projection_vectors(x0[a0:a0 + n].double(), masses[a0:a0 + n].double(), project)
        nproj[b] = V.size(0)
        if V.size(0):
            W = V @ d                                  # [p, m]: W_a = D v_a
            S = V @ W.t()
            d = d - (W.t() @ V + V.t() @ W) + V.t() @ (S @ V)
            d = torch.triu(d) + torch.triu(d, 1).t()
        Hs[b, :m, :m], D[b, :m, :m] = h, d
        a0 += n
    return Hs, D, asym, nproj


def frequencies_of(eigenvalues):
    return torch.sign(eigenvalues) * torch.sqrt(eigenvalues.abs()) * K_WAVENUMBER


def cartesian_modes(result, masses):
    """The Cartesian displacement patterns of the modes: modes[b, 3 i + a, :] / sqrt(m_i), columns not renormalised -> [B, M,
    M], zero outside each block.  masses: [N] in amu, the batch's atoms in order."""
    m = torch.as_tensor(masses, dtype=torch.float64).reshape(-1).to(result.modes.device)
    B, M = result.modes.size(0), result.modes.size(1)
    w = torch.ones(B, M, dtype=torch.float64, device=m.device)
    a0 = 0
    for b, d in enumerate(result.dims.tolist()):
        w[b, :d] = m[a0:a0 + d // 3].repeat_interleave(3)
        a0 += d // 3
    return result.modes / w.sqrt()[:, :, None]


def zero_point_energy(result):
    """1/2 sum h c nu over the real modes behind the projected ones, in kcal/mol -> [B]."""
    f = result.frequencies
    idx = torch.arange(f.size(1), device=f.device)[None, :]
    real = (idx >= result.n_projected.to(f.device)[:, None]) & (f > 0)
    return 0.5 * CM1_TO_KCAL * torch.where(real, f, torch.zeros_like(f)).sum(1)


# ----------------------------------------------------------------------------------------------------- the class
def _image_batch(b, sizes, copies):
    """`copies` copies of a collated batch as one batch: image j holds the atoms [j N, (j + 1) N)."""
    B = len(sizes)
    x = b.x.repeat(copies, *([1] * (b.x.dim() - 1)))
    bvec = (torch.arange(copies, device=b.batch.device)[:, None] * B + b.batch.long()[None, :]).reshape(-1)
    return Batch(x, b.positions.detach().repeat(copies, 1), bvec, None, None, copies * B, list(sizes) * copies)


class NormalModeAnalysis(Replicas):
    """See the module docstring.  masses: [N] in amu (None: ``default_masses(batch.x)``); delta: the central-difference
    step in A; coords_per_pass: C, the displaced coordinates per force pass (None: the largest whose image batch has at
    most IMAGE_ATOMS_DEFAULT atoms); project: "tr", "t" or None; use_graph: replay the captured round (None: yes);
    max_sweeps: the cap of the Jacobi sweeps."""

    _img = None

    def __init__(self, model, graph_pred_linear, batch, model_3d="schnet", masses=None, delta=DELTA_DEFAULT,
                 coords_per_pass=None, project="tr", use_graph=USE_GRAPH_DEFAULT, max_sweeps=MAX_SWEEPS_DEFAULT,
                 energy_and_gradient=None):
        if project not in (None, "t", "tr"):
            raise ValueError("NormalModeAnalysis: project is 'tr', 't' or None, got %r" % (project,))
        if not 0 <= int(max_sweeps) <= 4096:
            raise ValueError("NormalModeAnalysis: 0 <= max_sweeps <= 4096, got %r" % (max_sweeps,))
        b0 = _collated(batch)
        sizes = _host_sizes(b0)
        N0 = int(b0.positions.size(0))
        m0 = default_masses(b0.x) if masses is None else torch.as_tensor(masses).detach().cpu().double().reshape(-1)
        if m0.numel() != N0:
            raise ValueError("NormalModeAnalysis: masses has %d entries, the batch %d atoms" % (m0.numel(), N0))
        M = 3 * max(sizes) if sizes else 0
        if coords_per_pass is None:
            coords_per_pass = max(1, min(M, IMAGE_ATOMS_DEFAULT // max(2 * N0, 1)))
        C = int(coords_per_pass)
        if C < 1:
            raise ValueError("NormalModeAnalysis: coords_per_pass is at least 1, got %r" % (coords_per_pass,))
        self.coords_per_pass = C = min(C, max(M, 1))
        self.M, self.rounds = M, -(-M // C)
        self.project, self.max_sweeps = project, int(max_sweeps)
        self._user = (len(sizes), N0, sizes, m0)
        self.set_delta(delta)
        replay = True if use_graph is None else use_graph
        self.fused = False
        pos = b0.positions
        if energy_and_gradient is None and torch.is_tensor(pos) and pos.is_cuda and pos.dtype == torch.float32:
            img = _image_batch(b0, sizes, 2 * C)
            b = self._setup(model, graph_pred_linear, img, model_3d, m0.repeat(2 * C), replay, 1, 1, None)
            self._route(b)
        if not self.fused:
            b = self._setup(model, graph_pred_linear, b0, model_3d, m0, False, 1, 1, energy_and_gradient)
            self._init_fallback(b)
        self.B, self.N, self.sizes, self.masses = self._user

    # ---- state
    def _alloc_fused(self, dev):
        B, N, sizes, m0 = self._user
        C, M = self.coords_per_pass, self.M
        f64 = dict(dtype=torch.float64, device=dev)
        self._img = self._pos.view(2 * C, N, 3)
        self._pos = self._img[0].clone()                  # x0: what set_positions writes and `positions` shows
        self._mol_ptr0 = self._mol_ptr[:B + 1].clone()
        self._masses_dev = m0.to(**f64)
        self._delta = torch.full((1,), self._delta_host, dtype=torch.float32, device=dev)
        self._state = torch.zeros(ops.HESSIAN_STATE_WORDS, dtype=torch.int64, device=dev)
        self._hessian = torch.zeros(B, M, M, **f64)
        self._D = torch.zeros(B, M, M, **f64)
        self._energy0, self._fmax0, self._asym = (torch.zeros(B, **f64) for _ in range(3))
        self._nproj = torch.zeros(B, dtype=torch.int32, device=dev)
        self._dims = torch.tensor([3 * n for n in sizes], dtype=torch.int32, device=dev)
        self._work = torch.empty(int(_lib.load().geossl_hessian_finish_workspace(B, M)), **f64)

    def set_delta(self, delta):
        """The step of the following runs, in A (device data: no new capture)."""
        d = float(delta)
        if not (d > 0 and math.isfinite(d)):
            raise ValueError("NormalModeAnalysis: delta is positive, got %r" % (delta,))
        self._delta_host = d
        if self._img is not None:
            self._delta.fill_(d)

    @property
    def delta(self):
        return self._delta_host

    # ---- the fused route
    def _force(self):
        from .finetune_md17 import _energy_and_gradient
        pos = self._pos if self._img is None else self._img.view(-1, 3)
        return _energy_and_gradient(self.model_3d, self.model, self._ps, self._x, pos, self._bvec, self._rei)

    def _round(self):
        C = self.coords_per_pass
        ops.hessian_displace(self._pos, self._mol_ptr0, self._delta, self._state, C, self._img)
        energy, grad = self._force()
        ops.hessian_collect(self._pos, self._img, grad, energy, self._mol_ptr0, self._state, C, self.rounds, self._hessian,
                            self._energy0, self._fmax0)

    def _capture_round(self):
        C = self.coords_per_pass

        def dry_run():   # (the two kernels on copies)
            st, img = self._state.clone(), self._img.clone()
            ops.hessian_displace(self._pos, self._mol_ptr0, self._delta, st, C, img)
            ops.hessian_collect(self._pos, img, torch.zeros_like(img).view(-1, 3),
                                torch.zeros(2 * C * self.B, dtype=torch.float32, device=img.device), self._mol_ptr0, st, C,
                                self.rounds, self._hessian.clone(), self._energy0.clone(), self._fmax0.clone())
        return self._capture("the Hessian round", dry_run, self._round)

    def _run_fused(self, rounds):
        self._state.zero_()
        self._hessian.zero_()
        graph = self._graph(("round", self.coords_per_pass), self._capture_round)
        for _ in range(rounds):
            if graph is not None:
                graph.replay()
            else:
                self._round()
        ops.hessian_finish(self._hessian, self._pos, self._masses_dev, self._mol_ptr0, self.project, self._D, self._asym,
                           self._nproj, self._work)
        _lib.poll_status(self.model)
        if self.M <= ops.JACOBI_MAX_DIM:
            lam, modes, sweeps, conv = ops.sym_eig_jacobi(self._D, self._dims, self.max_sweeps)
            conv = conv != 0
        else:
            lam, modes, sweeps, conv = self._eigh_cpu(self._D)
        return (self._hessian.clone(), lam, modes, self._nproj.long(), self._asym.clone(), self._energy0.clone(),
                self._fmax0.clone(), sweeps.long(), conv)

    def _eigh_cpu(self, D):
        """torch.linalg.eigh on a CPU copy of D, block by block -> the eigensolver's four results on D's device."""
        B, M = D.size(0), D.size(1)
        Dc = D.detach().cpu()
        lam = torch.full((B, M), float("nan"), dtype=torch.float64)
        modes = torch.zeros(B, M, M, dtype=torch.float64)
        for b, n in enumerate(self._user[2]):
            m = 3 * n
            if m:
                lam[b, :m], modes[b, :m, :m] = torch.linalg.eigh(Dc[b, :m, :m])
        dev = D.device
        return lam.to(dev), modes.to(dev), torch.zeros(B, dtype=torch.int64, device=dev), torch.ones(B, dtype=torch.bool,
                                                                                                      device=dev)

    # ---- the fallback route
    def _run_fallback(self, rounds):
        B, N, sizes, m0 = self._user
        C, M = self.coords_per_pass, self.M
        dev, dt = self._pos.device, self._pos.dtype
        x0 = self._pos.detach().clone()
        first = torch.tensor([0] + sizes[:-1], dtype=torch.long).cumsum(0)
        H = torch.zeros(B, M, M, dtype=torch.float64)
        delta = torch.tensor(self._delta_host, dtype=dt, device=dev)
        energy = fmax = None
        with torch.no_grad():
            for r in range(rounds):
                if r >= self.rounds:   # the round behind the last: nothing displaced, energy and fmax
                    e, g = self._force_fallback()
                    energy = e.detach().double().cpu().reshape(-1)
                    g2 = (g.detach().double().cpu() ** 2).sum(1)
                    fmax = torch.stack([g2[a:a + n].max() if n else g2.new_zeros(()) for a, n in zip(first.tolist(), sizes)]
                                       ).sqrt()
                    continue
                for c in range(C):
                    k = r * C + c
                    live = [b for b, n in enumerate(sizes) if k < 3 * n]
                    if not live:
                        continue
                    flat = torch.tensor([3 * int(first[b]) + k for b in live], dtype=torch.long, device=dev)
                    grads, coords = [], []
                    for sign in (1.0, -1.0):
                        xi = x0.clone()
                        xi.view(-1)[flat] = x0.view(-1)[flat] + sign * delta
                        self._pos.copy_(xi)
                        grads.append(self._force_fallback()[1].detach().double().cpu())
                        coords.append(xi.view(-1)[flat].double().cpu())
                    den = coords[0] - coords[1]
                    for i, b in enumerate(live):
                        a, n = int(first[b]), sizes[b]
                        H[b, k, :3 * n] = (grads[0][a:a + n] - grads[1][a:a + n]).reshape(-1) / den[i]
                self._pos.copy_(x0)
        Hs, D, asym, nproj = finish(H, x0.detach().cpu(), m0, sizes, self.project)
        lam = torch.full((B, M), float("nan"), dtype=torch.float64)
        modes = torch.zeros(B, M, M, dtype=torch.float64)
        sweeps, conv = torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.bool)
        for b, n in enumerate(sizes):
            m = 3 * n
            if m and M <= ops.JACOBI_MAX_DIM:
                lam[b, :m], modes[b, :m, :m], s, ok = jacobi_eigh(D[b, :m, :m], self.max_sweeps)
                sweeps[b], conv[b] = s, ok
            elif m:
                lam[b, :m], modes[b, :m, :m] = torch.linalg.eigh(D[b, :m, :m])
        nan = torch.full((B,), float("nan"), dtype=torch.float64)
        return (Hs, lam, modes, nproj, asym, nan if energy is None else energy, nan.clone() if fmax is None else fmax,
                sweeps, conv)

    # ---- run
    def run(self):
        """The analysis at the current positions -> NormalModes.  R + 1 replays of the captured round, the finishing pass,
        the eigensolver: on the device for 3 n_max <= 99, else ``torch.linalg.eigh`` on a CPU copy of D in fp64."""
        rounds = self.rounds + 1
        H, lam, modes, nproj, asym, energy, fmax, sweeps, conv = (self._run_fused if self.fused
                                                                  else self._run_fallback)(rounds)
        dims = torch.tensor([3 * n for n in self._user[2]], dtype=torch.int64, device=H.device)
        return NormalModes(H, dims, lam, frequencies_of(lam), modes, nproj, asym, energy, fmax, sweeps, conv)
