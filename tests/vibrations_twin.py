"""fp64 numpy restatement of normal-mode analysis (geossl_amd/vibrations.py, csrc/vibrations.hip), written from the
definition in the module docstring: the image positions of a round, the rows a round collects, the finishing pass
(symmetrise, mass-weight, project translations and rotations by modified Gram-Schmidt) and the cyclic Jacobi in the same
round-robin rotation order.  `order` reverses the summation order of the finishing pass's sums: the difference between the
two orders is the reordering sensitivity the GPU test's tolerance is taken from."""
import math

import numpy as np

DROP_TOL = 1e-5
STOP = 2.0 ** -50
K_WAVENUMBER = math.sqrt(4.184e26) / (2.0 * math.pi * 2.99792458e10)
U64 = 2.0 ** -52


def mol_ptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def rounds(sizes, C):
    return -(-3 * max(sizes) // C)


# ------------------------------------------------------------------------------------------------- the Hessian rounds
def images(x0, sizes, delta, C, r):
    """The image batch of round r -> fp32 [2 C, N, 3]: image 2 c is (c, +), image 2 c + 1 is (c, -)."""
    x0 = np.asarray(x0, dtype=np.float32)
    d = np.float32(delta)
    ptr = mol_ptr(sizes)
    img = np.repeat(x0[None], 2 * C, axis=0).copy()
    flat = img.reshape(2 * C, -1)
    for c in range(C):
        k = r * C + c
        for b, n in enumerate(sizes):
            if k < 3 * n:
                i = 3 * ptr[b] + k
                flat[2 * c, i] = np.float32(x0.reshape(-1)[i] + d)
                flat[2 * c + 1, i] = np.float32(x0.reshape(-1)[i] - d)
    return img


def collect(H, img, grad, sizes, C, r):
    """Row k = r C + c of every molecule with k < 3 n_b, in place on H [B, M, M] fp64: (g+ - g-) / (x+_k - x-_k)."""
    ptr = mol_ptr(sizes)
    g = np.asarray(grad, dtype=np.float64).reshape(2 * C, -1)
    x = np.asarray(img, dtype=np.float32).reshape(2 * C, -1).astype(np.float64)
    for c in range(C):
        k = r * C + c
        for b, n in enumerate(sizes):
            if k < 3 * n:
                lo, hi = 3 * ptr[b], 3 * ptr[b + 1]
                H[b, k, :3 * n] = (g[2 * c, lo:hi] - g[2 * c + 1, lo:hi]) / (x[2 * c, lo + k] - x[2 * c + 1, lo + k])
    return H


def reference_point(grad0, energy0, sizes):
    """energy [B] and fmax [B] from image 0 of the round behind the last."""
    ptr = mol_ptr(sizes)
    g2 = (np.asarray(grad0, dtype=np.float32).astype(np.float64) ** 2).sum(1)
    fmax = np.array([math.sqrt(g2[ptr[b]:ptr[b + 1]].max()) if n else 0.0 for b, n in enumerate(sizes)])
    return np.asarray(energy0, dtype=np.float32).astype(np.float64), fmax


def hessian(gradient, x0, sizes, delta, C, n_rounds=None):
    """All rounds -> (H [B, M, M], the images of every round, their gradients).  gradient(pos fp32 [N, 3]) -> dE/dpos
    [N, 3] of the user's batch, used as it comes (fp64: the twin's own Hessian; fp32: what a device pass hands over)."""
    M, R = 3 * max(sizes), rounds(sizes, C)
    H = np.zeros((len(sizes), M, M))
    imgs, grads = [], []
    for r in range(R if n_rounds is None else n_rounds):
        img = images(x0, sizes, delta, C, r)
        g = np.stack([np.asarray(gradient(im), dtype=np.float64) for im in img])
        collect(H, img, g, sizes, C, r)
        imgs.append(img)
        grads.append(g)
    return H, imgs, grads


# ------------------------------------------------------------------------------------------------ the finishing pass
def _sum(v, order):
    acc = 0.0
    for t in (v if order == "forward" else v[::-1]):
        acc += float(t)
    return acc


def _dot(a, b, order):
    return _sum(a * b, order)


def projection_vectors(x, masses, project, order="forward"):
    n = len(x)
    if project is None or n == 0:
        return np.zeros((0, 3 * n))
    w = np.sqrt(masses)
    raw = []
    for a in range(3):
        v = np.zeros((n, 3))
        v[:, a] = w
        raw.append(v.reshape(-1))
    if project == "tr":
        tot = _sum(masses, order)
        com = np.array([_sum(masses * x[:, a], order) / tot for a in range(3)])
        r = x - com
        for a in range(3):
            e = np.zeros(3)
            e[a] = 1.0
            raw.append((w[:, None] * np.cross(e[None, :], r)).reshape(-1))
    kept = []
    for v in raw:
        n0 = math.sqrt(_dot(v, v, order))
        for u in kept:
            v = v - _dot(u, v, order) * u
        n1 = math.sqrt(_dot(v, v, order))
        if n1 > DROP_TOL * n0:
            kept.append(v / n1)
    return np.stack(kept) if kept else np.zeros((0, 3 * n))


def finish(H, x0, masses, sizes, project, order="forward"):
    """-> (H symmetrised, D, asymmetry [B], n_projected [B]); zero outside every 3 n_b block."""
    B, M = H.shape[0], H.shape[1]
    ptr = mol_ptr(sizes)
    x0 = np.asarray(x0, dtype=np.float32).astype(np.float64)
    Hs, D = np.zeros_like(H), np.zeros_like(H)
    asym, nproj = np.zeros(B), np.zeros(B, dtype=np.int64)
    for b, n in enumerate(sizes):
        m = 3 * n
        h = H[b, :m, :m]
        asym[b] = np.abs(h - h.T).max() if m else 0.0
        h = 0.5 * (h + h.T)
        mw = np.repeat(masses[ptr[b]:ptr[b + 1]], 3)
        d = h / np.sqrt(mw[:, None] * mw[None, :])
        V = projection_vectors(x0[ptr[b]:ptr[b + 1]], masses[ptr[b]:ptr[b + 1]], project, order)
        nproj[b] = len(V)
        if len(V):
            if order == "forward":
                W = V @ d
                S = V @ W.T
                d = d - (W.T @ V + V.T @ W) + V.T @ (S @ V)
            else:
                W = (V[:, ::-1] @ d[::-1, :])
                S = V[:, ::-1] @ W.T[::-1, :]
                d = d - (V.T @ W + W.T @ V) + (V.T @ S) @ V
            d = np.triu(d) + np.triu(d, 1).T
        Hs[b, :m, :m], D[b, :m, :m] = h, d
    return Hs, D, asym, nproj


# ----------------------------------------------------------------------------------------------------- the Jacobi
def round_pairs(n2, t):
    w = n2 - 1
    k = np.arange(1, n2 // 2)
    a = np.concatenate([[w], (t + k) % w])
    c = np.concatenate([[t], (t - k) % w])
    return np.minimum(a, c), np.maximum(a, c)


def jacobi(A, max_sweeps):
    """Cyclic Jacobi in round-robin order -> (eigenvalues ascending, vectors in columns, sweeps, converged)."""
    A = np.asarray(A, dtype=np.float64)
    m = A.shape[0]
    n2 = m + (m & 1)
    S = np.zeros((n2, n2))
    S[:m, :m] = np.triu(A) + np.triu(A, 1).T
    V = np.eye(n2)
    thr = STOP * math.sqrt(float((S * S).sum()))
    sweeps, conv = 0, False
    for it in range(max_sweeps + 1):
        off = float(np.abs(np.triu(S, 1)).max()) if m > 1 else 0.0
        if off <= thr:
            conv = True
            break
        if it == max_sweeps:
            break
        for t in range(n2 - 1):
            p, q = round_pairs(n2, t)
            apq = S[p, q]
            act = (q < m) & (np.abs(apq) > 0.25 * thr)
            with np.errstate(over="ignore", invalid="ignore"):
                theta = (S[q, q] - S[p, p]) / (2.0 * np.where(act, apq, 1.0))
                tt = np.where(act, np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0)), 0.0)
            c = 1.0 / np.sqrt(tt * tt + 1.0)
            s = tt * c
            app, aqq = S[p, p] - tt * apq, S[q, q] + tt * apq
            Sp, Sq = S[:, p].copy(), S[:, q].copy()
            S[:, p], S[:, q] = c * Sp - s * Sq, s * Sp + c * Sq
            Sp, Sq = S[p, :].copy(), S[q, :].copy()
            S[p, :], S[q, :] = c[:, None] * Sp - s[:, None] * Sq, s[:, None] * Sp + c[:, None] * Sq
            S[p, p], S[q, q] = app, aqq
            S[p, q] = np.where(act, 0.0, apq)
            S = np.triu(S) + np.triu(S, 1).T
            Vp, Vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c * Vp - s * Vq, s * Vp + c * Vq
        sweeps += 1
    lam = np.diagonal(S)[:m]
    order = np.argsort(lam, kind="stable")
    return lam[order].copy(), V[:m, :m][:, order].copy(), sweeps, conv


def frequencies(lam):
    return np.sign(lam) * np.sqrt(np.abs(lam)) * K_WAVENUMBER


def analyse(gradient, x0, sizes, masses, delta, C, project="tr", max_sweeps=64):
    """The whole pipeline -> dict(H raw, hessian, D, asymmetry, n_projected, eigenvalues [list per molecule], sweeps)."""
    H, imgs, grads = hessian(gradient, x0, sizes, delta, C)
    Hs, D, asym, nproj = finish(H, x0, np.asarray(masses, dtype=np.float64), sizes, project)
    eig = [jacobi(D[b, :3 * n, :3 * n], max_sweeps) for b, n in enumerate(sizes)]
    return dict(raw=H, hessian=Hs, D=D, asymmetry=asym, n_projected=nproj, eigenvalues=[e[0] for e in eig],
                modes=[e[1] for e in eig], sweeps=[e[2] for e in eig], converged=[e[3] for e in eig], images=imgs,
                gradients=grads)


# -------------------------------------------------------------------------------- the matrices of the Jacobi tests
def jacobi_matrices():
    """name -> symmetric fp64 matrix: random ones of dimension 1, 2, 3, 7, 63, 99, a diagonal and a zero matrix, and a
    63 x 63 spectrum with six zeros and three 10-fold clusters under a random orthogonal basis."""
    g = np.random.default_rng(20250)
    out = {}
    for m in (1, 2, 3, 7, 63, 99):
        a = g.standard_normal((m, m))
        out["random%d" % m] = a + a.T
    out["diagonal7"] = np.diag(g.standard_normal(7))
    out["zero5"] = np.zeros((5, 5))
    spec = np.concatenate([np.zeros(6), np.full(10, 1.0), np.full(10, 2.5), np.full(10, -0.75), g.standard_normal(27)])
    q, _ = np.linalg.qr(g.standard_normal((63, 63)))
    a = (q * spec) @ q.T
    out["degenerate63"] = 0.5 * (a + a.T)
    return out


def eig_errors(A, lam, V):
    """(max eigenvalue error against LAPACK, |A V - V L|_max, |V^T V - I|_max), the first two in units of |A|_F."""
    m = A.shape[0]
    fro = max(np.linalg.norm(A), 1e-300)
    ref = np.linalg.eigvalsh(A)
    return (float(np.abs(lam - ref).max()) / fro, float(np.abs(A @ V - V * lam).max()) / fro,
            float(np.abs(V.T @ V - np.eye(m)).max()))


# ------------------------------------------------------------------------------- what the CPU and the GPU tests share
KERNEL_SIZES = [1, 2, 9, 21]
# The finishing pass against the twin: FINISH_C m 2^-52 max|D|, max|D| of the mass-weighted Hessian before projection.
# FINISH_C = 8 x the twin's own sensitivity to the order of its sums (forward against reversed, at most 1.0 of m 2^-52
# max|D| on `finish_inputs`: measured 0.6, tests/test_vibrations_cpu.py::test_finish_reordering_sensitivity); the
# kernel's tree sums and fused multiply-adds are one more such reordering.
FINISH_C = 8.0
# The Jacobi against LAPACK, in units of |A|_F: the stop threshold's m 2^-50 plus 8 x the twin's worst measured deviation
# from numpy.linalg.eigh over `jacobi_matrices` (9.8e-16).  |V^T V - I|_max: 8 x the twin's worst measured 1.51 m 2^-52.
JACOBI_WORST_EIG, JACOBI_WORST_ORTH, JACOBI_WORST_SWEEPS = 1.0e-15, 1.51, 11
JACOBI_ROUNDING = 8 * JACOBI_WORST_EIG
JACOBI_ORTH = 8 * JACOBI_WORST_ORTH


def jacobi_bound(m):
    return m * STOP + JACOBI_ROUNDING


def finish_inputs():
    """Sizes [1, 2, 9, 21] and a collinear 3-atom molecule: (sizes, x0 fp32, masses, random non-symmetric H with the
    sentinel -7 outside the blocks)."""
    g = np.random.default_rng(5)
    sizes = KERNEL_SIZES + [3]
    N, M = sum(sizes), 3 * max(sizes)
    x0 = (1.5 * g.standard_normal((N, 3))).astype(np.float32)
    x0[-3:] = (np.array([[0.0], [1.0], [2.5]]) * np.array([[0.7, -0.4, 0.59]]) + 0.3).astype(np.float32)
    masses = 1.0 + 15.0 * g.random(N)
    H = np.full((len(sizes), M, M), -7.0)
    for b, n in enumerate(sizes):
        H[b, :3 * n, :3 * n] = g.standard_normal((3 * n, 3 * n))
    return sizes, x0, masses, H


def element_check(sizes, eps, hessian_got, hessian_ref, imgs, grads):
    """max over the elements of |H - H_ref| / tolerance; the tolerance of row k is eps max|g over the images| 2 / (x+_k -
    x-_k), and an element of the symmetrised Hessian gets the mean of its two rows'.  imgs, grads: the C = 1 rounds."""
    gmax = max(np.abs(g).max() for g in grads)
    worst, ptr = 0.0, mol_ptr(sizes)
    for b, n in enumerate(sizes):
        m = 3 * n
        if m == 0:
            continue
        den = np.array([float(imgs[k][0].reshape(-1)[3 * ptr[b] + k]) - float(imgs[k][1].reshape(-1)[3 * ptr[b] + k])
                        for k in range(m)])
        row = eps * gmax * 2.0 / den
        tol = 0.5 * (row[:, None] + row[None, :])
        worst = max(worst, float((np.abs(hessian_got[b, :m, :m] - hessian_ref[b, :m, :m]) / tol).max()))
    return worst
