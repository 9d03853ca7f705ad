"""fp64 restatement of ONE PaiNN interaction block as the atom-tile kernels compute it (csrc/painn_tile.hip; the block is
Geom3D/models/painn.py:54-64 with the filter of :241-245), forward and backward, for element-wise checks: for every
output element the reference value, the magnitude sum S, and the individual terms.

    W_c(e, f)   = (sum_k phi'_e[k] Wf'[c F + f][k]) fcut_e,        phi' = [phi, 1],  Wf' = [Wf | b]
    q_out[i, f] = q[i, f] + sum_{e -> i} W_0 x_0[j_e, f]
    mu_out[i, d, f] = mu[i, d, f] + sum_{e -> i} (W_1 x_1[j_e, f] dir_e[d] + W_2 x_2[j_e, f] mu[j_e, d, f])
and with the upstream gradients gq = dq_out[i_e], gm = dmu_out[i_e] of an edge e that leaves j:
    g_0 = gq,  g_1 = sum_d gm[d] dir_e[d],  g_2 = sum_d gm[d] mu[j, d]
    dxc[j, c F + f]  = sum_e g_c W_c
    dmu_in[j, d, f]  = dmu_out[j, d, f] + sum_e gm[d] W_2 x_2[j, f]
    t_c(e, f)        = g_c x_c[j, f] fcut_e,    dWf[c F + f, k] = sum_e t_c phi_e[k],    dbf[c F + f] = sum_e t_c

S is the sum of the absolute values of the products that enter an element, with |W_e| replaced by
Wabs = sum_k |phi'_k| |Wf'_k| |fcut| (the filter is itself a rounded sum) and the dot products g_1, g_2 by the sums of
their terms' magnitudes.

The bound |got - ref| <= c u S, u = 2^-22 (two-piece operands; one fp32 rounding is u / 4).  Rounding counts of the
kernels, all relative to the magnitude sums above.  Assumption on the hardware: a 32x32x16 MFMA adds its 16 products to
the accumulator in at most four fp32-rounded steps (u each).
  W:        each product phi'_k Wf'_k from two fp16 pieces per operand - 2 u for the two operands (22 significant bits;
            phi in [0, 1] random and weights of one scale keep the fp16 subnormal floor, 2^-39 of the row's largest
            product, far below u Wabs) + u for the dropped low x low product = 3 u; six chained MFMAs = 24 rounded steps
            = 6 u.  W: 9 u.
  forward:  W kk fcut x: kk fcut rounded once, three multiplications, the product with dir / mu_j = 5 roundings -> 1.25 u
            (1 u for q_out); a lane's chain takes an atom's rows of its half, 16 per tile, two rounded additions per row
            for mu_out, + the halves + the residual: (2 * 16 tiles + 2) / 4 u.
            C_FWD(D) = 9 + 1.25 + (32 ceil(D / 32) + 2) / 4               (D: largest in-degree; 70 -> 34.75)
  backward: dxc: W (9 u) + kk fcut and W kf (0.5 u) + the three-term dot g (0.75 u) + one fused addition per row + the
            halves: (16 tiles + 1) / 4 u.  dmu_in: W + 0.5 u + W_2 x_2 (0.25 u) + (16 tiles + 2) / 4 u: the larger.
            C_BWD(D) = 9 + 0.75 + 0.75 + (16 ceil(D / 32) + 2) / 4          (D: largest out-degree; 70 -> 23)
  dWf/dbf:  t = g x fcut: 0.75 u + two multiplications 0.5 u; both operands of the second GEMM split EXACTLY into three
            bf16 pieces, the three dropped piece products <= 3 * 2^-24 = 0.75 u; 12 MFMAs per tile = 48 rounded steps;
            the compensated sum over the blocks' partials and its four slice sums: at most 6 more.
            C_WGRAD(T) = 2 + (48 T + 6) / 4      (T: most tiles any one block accumulates; one 70-edge atom -> 39.5)
These come from the counts above, not from what the kernels return.

The same forward is computed by two more kernels, and `forward` serves them with constants of their own (again counted
in the sources, csrc/painn_mma.hip and csrc/painn.hip, never fitted to results; tests/test_gpu_painn_mma.py and
tests/test_gpu_painn_atom.py print the worst measured ratio next to each):
  k_painn_fwd_mma<R, MZ> (molecule-staged, groups of four rows per target atom, a tile = eight groups), u = 2^-22:
            W: the same six chained 32x32x16 MFMAs on two fp16 pieces per operand as the tile kernels: 9 u.
            kk fcut: kk = 2^(eW - 28) is a power of two: exact, no rounding.
            (acc kf) xv: two rounded products; x1 d + x2 mu_j: at most three roundings (two products and their sum, one
            less where the compiler contracts) = 5 roundings -> 1.25 u (q_out: 2, covered).
            additions: a row is added to its group's sum (one rounded addition per edge: D), a group's sum to the
            atom's running sum across groups and tiles (ceil(D / 4)), the residual (1); the exchange of the halves
            moves values and rounds nothing.  Each is u / 4 of a partial sum of magnitudes <= S.
            c_fwd_mma(D) = 9 + 1.25 + (D + ceil(D / 4) + 1) / 4        (D: largest in-degree; 17 -> 16, 43 -> 24)
            The first addition of a group and of a run adds to an exact zero, so (D + ceil(D / 4) + 1) overcounts
            by up to ceil(D / 4) + 1 additions - kept, as a bound.
  k_painn_interaction_fwd<R> and k_painn_interaction_fwd_mol<R> (fp32 vector arithmetic), u = 2^-24 (U24):
            W: the bias is the accumulator's exact starting value, then R fused multiply-adds, one rounding each: R;
            W fcut, W x: 2; x1 d + x2 mu_j: at most 3; D sequential additions in incidence order; the residual: 1.
            c_fwd_atom(R, D) = R + 2 + 3 + D + 1 = R + D + 6            (R = 20, D = 70 -> 96; R = 32 -> 108)
            (the bias costs no rounding of its own: it is where the chain starts.)"""
import math

import torch

U = 2.0 ** -22
U24 = 2.0 ** -24


def c_fwd(max_degree):
    return 9.0 + 1.25 + (32 * math.ceil(max_degree / 32) + 2) / 4.0


def c_bwd(max_degree):
    return 9.0 + 0.75 + 0.75 + (16 * math.ceil(max_degree / 32) + 2) / 4.0


def c_wgrad(tiles):
    return 2.0 + (48 * tiles + 6) / 4.0


def c_fwd_mma(max_degree):
    """k_painn_fwd_mma, in units of U = 2^-22."""
    return 9.0 + 1.25 + (max_degree + math.ceil(max_degree / 4) + 1) / 4.0


def c_fwd_atom(R, max_degree):
    """k_painn_interaction_fwd / _fwd_mol, in units of U24 = 2^-24."""
    return float(R + 2 + 3 + max_degree + 1)


MAX_DEGREE = 70                 # of the GPU test's edge list, either side
C_FWD, C_BWD = c_fwd(MAX_DEGREE), c_bwd(MAX_DEGREE)
C_WGRAD = c_wgrad(math.ceil(MAX_DEGREE / 32))   # one atom per block (96 atoms on 96 blocks)


def _d(t, device="cpu"):
    return None if t is None else t.detach().double().to(device)


def filters(phi, fcut, Wf, bf, device="cpu"):
    """-> W [E, 3F], Wabs [E, 3F]."""
    phi, fcut, Wf, bf = _d(phi, device), _d(fcut, device), _d(Wf, device), _d(bf, device)
    W = (phi @ Wf.t() + bf) * fcut[:, None]
    Wabs = (phi.abs() @ Wf.abs().t() + bf.abs()) * fcut.abs()[:, None]
    return W, Wabs


def _scatter(terms, index, n):
    out = torch.zeros((n,) + tuple(terms.shape[1:]), dtype=torch.float64, device=terms.device)
    return out.index_add_(0, index, terms)


def forward(q, mu, xc, idx_i, idx_j, phi, fcut, dirv, Wf, bf, device="cpu"):
    """mu None: identically zero.  -> dict(q_out, mu_out: (ref, S), terms_q [E, F], terms_mu [E, 3, F], abs_q, abs_mu,
    and the two parts of terms_mu: terms_mu_r = W_1 x_1 dir, terms_mu_m = W_2 x_2 mu_j).  `device`: where the fp64
    tensors live (the batches of a thousand molecules are evaluated on the device they are on, in one pass)."""
    q, mu, xc, dirv = _d(q, device), _d(mu, device), _d(xc, device), _d(dirv, device)
    N, F = q.shape
    if mu is None:
        mu = torch.zeros(N, 3, F, dtype=torch.float64, device=device)
    i, j = idx_i.to(device).long(), idx_j.to(device).long()
    W, Wabs = filters(phi, fcut, Wf, bf, device)
    x = xc[j]                                                                  # [E, 3F]
    t_q = W[:, :F] * x[:, :F]
    a_q = Wabs[:, :F] * x[:, :F].abs()
    r_part = (W[:, F:2 * F] * x[:, F:2 * F])[:, None, :] * dirv[:, :, None]
    m_part = (W[:, 2 * F:] * x[:, 2 * F:])[:, None, :] * mu[j]
    t_mu = r_part + m_part
    a_mu = (Wabs[:, F:2 * F] * x[:, F:2 * F].abs())[:, None, :] * dirv.abs()[:, :, None] + \
           (Wabs[:, 2 * F:] * x[:, 2 * F:].abs())[:, None, :] * mu[j].abs()
    return dict(q_out=(q + _scatter(t_q, i, N), q.abs() + _scatter(a_q, i, N)),
                mu_out=(mu + _scatter(t_mu, i, N), mu.abs() + _scatter(a_mu, i, N)),
                terms_q=t_q, terms_mu=t_mu, abs_q=a_q, abs_mu=a_mu, terms_mu_r=r_part, terms_mu_m=m_part)


def backward(dq_out, dmu_out, mu, xc, idx_i, idx_j, phi, fcut, dirv, Wf, bf, atoms=None):
    """mu None: identically zero (dmu_in is then None).  `atoms`: the source atoms whose edges enter dWf / dbf (a list of
    atoms; default all).  -> dict(dxc, dmu_in, dWf, dbf: (ref, S), terms_dxc [E, 3F], terms_dmu [E, 3, F],
    terms_dWf [E, 3F, R], terms_dbf [E, 3F] and abs_* likewise)."""
    gq, gm, xc, dirv, phi_, fc = _d(dq_out), _d(dmu_out), _d(xc), _d(dirv), _d(phi), _d(fcut)
    N, F = gq.shape
    mz = mu is None
    mu = torch.zeros(N, 3, F, dtype=torch.float64) if mz else _d(mu)
    i, j = idx_i.cpu().long(), idx_j.cpu().long()
    W, Wabs = filters(phi, fcut, Wf, bf)
    gqe, gme = gq[i], gm[i]                                                    # [E, F], [E, 3, F]
    g = torch.cat([gqe, (gme * dirv[:, :, None]).sum(1), (gme * mu[j]).sum(1)], 1)                 # [E, 3F]
    gabs = torch.cat([gqe.abs(), (gme.abs() * dirv.abs()[:, :, None]).sum(1), (gme.abs() * mu[j].abs()).sum(1)], 1)
    t_dxc, a_dxc = g * W, gabs * Wabs
    x2 = xc[j][:, 2 * F:]
    t_dmu = gme * (W[:, 2 * F:] * x2)[:, None, :]
    a_dmu = gme.abs() * (Wabs[:, 2 * F:] * x2.abs())[:, None, :]
    t = g * xc[j] * fc[:, None]
    tabs = gabs * xc[j].abs() * fc.abs()[:, None]
    if atoms is not None:
        keep = torch.zeros(N, dtype=torch.bool)
        keep[torch.as_tensor(atoms).cpu().long()] = True
        t, tabs = t * keep[j][:, None], tabs * keep[j][:, None]
    t_w, a_w = t[:, :, None] * phi_[:, None, :], tabs[:, :, None] * phi_.abs()[:, None, :]
    out = dict(dxc=(_scatter(t_dxc, j, N), _scatter(a_dxc, j, N)),
               dmu_in=None if mz else (gm + _scatter(t_dmu, j, N), gm.abs() + _scatter(a_dmu, j, N)),
               dWf=(t_w.sum(0), a_w.sum(0)), dbf=(t.sum(0), tabs.sum(0)),
               terms_dxc=t_dxc, terms_dmu=t_dmu, terms_dWf=t_w, terms_dbf=t,
               abs_dxc=a_dxc, abs_dmu=a_dmu, abs_dWf=a_w, abs_dbf=tabs)
    return out


# ---- a plain restatement (painn.py:54-64, :241-245) for the CPU test: differentiable fp64 tensors in, (q_out, mu_out) out
def plain_forward(q, mu, xc, idx_i, idx_j, phi, fcut, dirv, Wf, bf):
    N, F = q.shape
    filt = (phi @ Wf.t() + bf) * fcut[:, None]                    # :241-245 (one interaction's slice of the filter)
    Wq, WR, Wmu = torch.split(filt, F, dim=-1)
    xq, xR, xmu = torch.split(xc[idx_j], F, dim=-1)               # :56-57
    dq = torch.zeros_like(q).index_add_(0, idx_i, Wq * xq)        # :59
    dmu = (WR * xR)[:, None, :] * dirv[:, :, None] + (Wmu * xmu)[:, None, :] * mu[idx_j]   # :60-61
    dmu = torch.zeros_like(mu).index_add_(0, idx_i, dmu)
    return q + dq, mu + dmu                                       # :63-64
