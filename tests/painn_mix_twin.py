"""fp64 restatement of PaiNN's four mixing kernels (csrc/painn.hip: k_painn_mix_pre_fwd, _post_fwd, _post_bwd, _pre_bwd;
the block is Geom3D/models/painn.py:100-113) for element-wise checks: per output the reference value and the magnitude
sum S of the terms that enter it, in the layouts of the kernels:

    mm  [N][3][2F]   mu_channel_mix(mu): V = mm[:, k, :F], W = mm[:, k, F:] of component k
    ctx [N][2F]      [q, |V|],  |V| = sqrt(V_x^2 + V_y^2 + V_z^2 + eps)
    dot [N][F]       sum_k V_k W_k
    xx  [N][3F]      [dq_intra, dmu_intra, dqmu_intra]
    q' = q + xx_0 + xx_2 dot,      mu'[k] = mu[k] + xx_1 W_k                       (mu_out NULL: not formed)
and backward, with gq = dq', gm = dmu' (NULL: zero), ddot = gq xx_2:
    dxx = [gq, sum_k gm_k W_k, gq dot]
    dmm_V[k] = ddot W_k (post_bwd)  + dctx_n V_k / ctx_n (added by pre_bwd),     dmm_W[k] = gm_k xx_1 + ddot V_k
    dq_in = gq + dctx_q

Every function returns {name: (ref, S)}; `dot` and `ctx` enter the later kernels as the fp32 tensors they are handed, so
each kernel is held to its own arithmetic.  The bound is |got - ref| <= C[name] u S, u = 2^-24, with C the number of
fp32 roundings on the way to the element, every operation counted uncontracted (a fused multiply-add only removes one).
Division and square root count one rounding each: the library is built with `-O3` and no fast-math or
`-fno-hip-fp32-correctly-rounded-divide-sqrt` flag (geossl_amd/build.py, the hipcc line), so both are correctly rounded.
Under the root all terms are non-negative, so S of ctx[:, F:] is the value itself (a relative error of the radicand is
halved by the root; counted in full).

    ctx_q   copy                                                            0     (exact)
    ctx_n   three squares, three additions (eps included), the root         7
    dot     three products, two additions                                   5
    q_out   xx_2 dot, two additions                                         3
    mu_out  xx_1 W_k, one addition                                          2
    dxx_0   copy                                                            0
    dxx_1   three products, three additions (the first onto an exact zero)  6
    dxx_2   one product                                                     1
    dmm_V   post_bwd: ddot, ddot W_k                                        2
    dmm_W   gm xx_1, ddot, ddot V_k, one addition                           4
    dq_in   one addition                                                    1
    dmm_V   after pre_bwd: the 2 above + the quotient, its product with V_k, the addition onto what is there    5
These are counts of operations in the kernel sources, not figures measured on the kernels."""
import torch

U = 2.0 ** -24
C = dict(ctx_q=0.0, ctx_n=7.0, dot=5.0, q_out=3.0, mu_out=2.0, dxx_0=0.0, dxx_1=6.0, dxx_2=1.0, dmm_V_post=2.0, dmm_W=4.0,
         dq_in=1.0, dmm_V=5.0)


def _d(t):
    return None if t is None else t.detach().double()


def _vw(mm, F):
    mm = mm.reshape(-1, 3, 2 * F)
    return mm[:, :, :F], mm[:, :, F:]


def pre_fwd(q, mm, eps):
    """-> ctx_q [N, F], ctx_n [N, F], dot [N, F]."""
    q, mm = _d(q), _d(mm)
    F = q.shape[1]
    V, W = _vw(mm, F)
    n = torch.sqrt((V * V).sum(1) + eps)
    return dict(ctx_q=(q, q.abs()), ctx_n=(n, n), dot=((V * W).sum(1), (V * W).abs().sum(1)))


def post_fwd(q, mu, mm, xx, dot, with_mu_out=True):
    """-> q_out [N, F], mu_out [N, 3, F] (absent when with_mu_out is False: the kernel's mu_out == NULL)."""
    q, mu, mm, xx, dot = _d(q), _d(mu), _d(mm), _d(xx), _d(dot)
    F = q.shape[1]
    _, W = _vw(mm, F)
    x0, x1, x2 = xx[:, :F], xx[:, F:2 * F], xx[:, 2 * F:]
    out = dict(q_out=(q + x0 + x2 * dot, q.abs() + x0.abs() + (x2 * dot).abs()))
    if with_mu_out:
        mu = mu.reshape(-1, 3, F)
        t = x1[:, None, :] * W
        out["mu_out"] = (mu + t, mu.abs() + t.abs())
    return out


def post_bwd(dq_new, dmu_new, mm, xx, dot):
    """dmu_new None: zero.  -> dxx_0, dxx_1, dxx_2 [N, F], dmm_V_post, dmm_W [N, 3, F], and the two terms of dmm_W
    (term_W_gm = gm xx_1, term_W_dot = ddot V: plain tensors)."""
    gq, gm, mm, xx, dot = _d(dq_new), _d(dmu_new), _d(mm), _d(xx), _d(dot)
    F = gq.shape[1]
    V, W = _vw(mm, F)
    if gm is None:
        gm = torch.zeros_like(V)
    gm = gm.reshape(-1, 3, F)
    x1, x2 = xx[:, F:2 * F], xx[:, 2 * F:]
    ddot = (gq * x2)[:, None, :]
    t_gm, t_dot = gm * x1[:, None, :], ddot * V
    return dict(dxx_0=(gq, gq.abs()), dxx_1=((gm * W).sum(1), (gm * W).abs().sum(1)), dxx_2=(gq * dot, (gq * dot).abs()),
                dmm_V_post=(ddot * W, (ddot * W).abs()), dmm_W=(t_gm + t_dot, t_gm.abs() + t_dot.abs()),
                term_W_gm=t_gm, term_W_dot=t_dot)


def pre_bwd(dq_new, dctx, ctx, mm, dmm_V_post):
    """dmm_V_post: (ref, S) of post_bwd.  -> dq_in [N, F], dmm_V [N, 3, F] = post_bwd's value + dctx_n V / ctx_n."""
    gq, dctx, ctx, mm = _d(dq_new), _d(dctx), _d(ctx), _d(mm)
    F = gq.shape[1]
    V, _ = _vw(mm, F)
    t = (dctx[:, F:] / ctx[:, F:])[:, None, :] * V
    return dict(dq_in=(gq + dctx[:, :F], gq.abs() + dctx[:, :F].abs()),
                dmm_V=(dmm_V_post[0] + t, dmm_V_post[1] + t.abs()), term_V_norm=t)


def pack_dmm(dmm_V, dmm_W):
    """[N, 3, F] x 2 -> the kernels' dmm [N, 3, 2F]."""
    return torch.cat([dmm_V, dmm_W], dim=2)
