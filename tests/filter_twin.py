"""fp64 twin of the filter-network kernels (filter_fwd.hip, filter_bwd.hip, filter_dpos.hip) with element-wise bounds.

A plain module (no tests): every function takes the tensors the C ABI takes, on the CPU or the GPU, and returns the fp64
value `ref` of each output element and `S`, the same expression evaluated on absolute values (sum of |terms|), so that a
kernel is checked per element by |got - ref| <= c u S (tests/test_gpu_packed_kernels.py: flagged / assert_within).

Operand model of the split products (csrc/split.h): two fp16 pieces under power-of-two block scales keep an operand
element exact to 22 bits of itself, or to 2^-12 of the largest element of its operand where it is smaller than that:
`fl_(a) = |a| + 2^-12 max|a|`, u = 2^-22.  The three-bf16-piece forms carry 24 bits: the same S with u = 2^-24.

Arguments evaluated in fp32 before a transcendental carry their own term: exp(x) of an argument with relative error u is
off by |x| u of itself (S(rbf) = rbf (1 + |x|)); sin(theta) by |theta cos(theta)| u."""
import math

import torch

LOG2 = math.log(2.0)


def fl_(a):
    """|a| plus the floor of a two-piece operand: 2^-12 of its largest element."""
    return a.abs() + 2.0 ** -12 * a.abs().max()


def gaussians(pair_d, offset, coeff):
    """rbf_g = exp(coeff (d - mu_g)^2) (schnet.py:205-207) in fp64: (rbf [P, G], S(rbf), d - mu)."""
    diff = pair_d.double()[:, None] - offset.double()[None, :]
    arg = coeff * diff ** 2
    rbf = torch.exp(arg)
    return rbf, rbf * (1.0 + arg.abs()), diff


def _layer_forward(rbf, Srbf, w1, b1, w2, b2, C):
    """One block's filter rows from its Gaussians (schnet.py:141-145, 186-187): every intermediate and its S."""
    w1, b1, w2, b2 = w1.double(), b1.double(), w2.double(), b2.double()
    u = rbf @ w1.t() + b1
    Su = fl_(Srbf) @ fl_(w1).t() + b1.abs()
    sg = torch.sigmoid(u)
    sp = torch.nn.functional.softplus(u)
    T, ST = sp - LOG2, sp + LOG2 + sg * Su
    O = T @ w2.t() + b2
    SO = fl_(ST) @ fl_(w2).t() + b2.abs()
    return dict(u=u, Su=Su, sg=sg, T=T, ST=ST, O=O, SO=SO, Wf=C[:, None] * O, SWf=C.abs()[:, None] * SO)


def filter_forward(pair_d, pair_c, ws, offset, coeff):
    """geossl_cfconv_filter_fwd: per layer dict(T, ST, Wf, SWf, ...).  The envelope C = pair_c is an INPUT of the kernels:
    it is taken as given (fp64 of the fp32 value), never recomputed from d."""
    rbf, Srbf, _ = gaussians(pair_d, offset, coeff)
    C = pair_c.double()
    return [_layer_forward(rbf, Srbf, *w, C) for w in ws]


def forward_gaussian_terms(pair_d, ws, offset, coeff, l, g, centre=None, column=None):
    """What Gaussian `g` of layer `l` contributes to the pre-activations u [P, F]: w1[:, column] rbf_g.  With `centre`
    and `column` given: what a Gaussian at that centre, weighted by that column of w1, WOULD contribute (a kernel that
    reads one Gaussian too many)."""
    mu = offset.double()[g] if centre is None else centre
    col = g if column is None else column
    r = torch.exp(coeff * (pair_d.double() - mu) ** 2)
    return r[:, None] * ws[l][0].double()[:, col][None, :]


def without_pre_activation_term(layer, w2, b2, C, du, rows):
    """T and Wf of the pair rows `rows` when `du` [len(rows), F] is taken away from their pre-activations."""
    u = layer["u"][rows] - du
    T = torch.nn.functional.softplus(u) - LOG2
    return T, C.double()[rows, None] * (T @ w2.double().t() + b2.double())


def _filter_ref_and_bound(run, daggs):
    """fp64 weight gradients and their S (schnet.py:141-145,186-195 differentiated w.r.t. the filter weights; the
    hidden rows T = softplus(u) - log 2 with S(T) = softplus(u) + log 2 + sigmoid(u) S(u))."""
    inp, lay = run.inputs, run.lay
    i, j = lay.pair_i.long(), lay.pair_j.long()
    fl = inp["pair_flag"].long()
    c = inp["pair_c"].double()
    m0, m1 = ((fl & 1) > 0).double() * c, ((fl & 2) > 0).double() * c
    rbf = torch.exp(inp["coeff"] * (inp["pair_d"].double()[:, None] - inp["offset"].double()[None, :]) ** 2)
    # two fp16 pieces under power-of-two block scales: an operand element is exact to 22 bits of itself, or of 2^-12 of
    # the largest element of its operand where it is smaller than that
    fl_ = lambda a: a.abs() + 2.0 ** -12 * a.abs().max()
    out = []
    for l, (w1, b1, w2, b2) in enumerate(inp["ws"]):
        x, dg = inp["xs"][l].double(), daggs[l].double()
        dO = m0[:, None] * (dg[i] * x[j]) + m1[:, None] * (dg[j] * x[i])
        SdO = m0[:, None] * (fl_(dg)[i] * fl_(x)[j]) + m1[:, None] * (fl_(dg)[j] * fl_(x)[i])
        u = rbf @ w1.double().t() + b1.double()
        Su = fl_(rbf) @ fl_(w1.double()).t() + b1.double().abs()
        sg = torch.sigmoid(u)
        sp_ = torch.nn.functional.softplus(u)
        tt, Stt = sp_ - math.log(2.0), sp_ + math.log(2.0) + sg * Su
        g = dO @ w2.double()
        dU, SdU = g * sg, (SdO @ fl_(w2.double())) * sg + g.abs() * 0.25 * Su
        out.append(dict(ref=[dU.t() @ rbf, dU.sum(0), dO.t() @ tt, dO.sum(0)],
                        S=[SdU.t() @ fl_(rbf), SdU.sum(0), SdO.t() @ fl_(Stt), SdO.sum(0)], dO=dO, tt=tt, Stt=Stt))
    return out


def envelope(d, cutoff):
    """C(d) = (cos(pi d / r_c) + 1) / 2 (schnet.py:186) and C'(d), S(C') in the dtype of d."""
    th = d * (math.pi / cutoff)
    k = 0.5 * math.pi / cutoff
    return 0.5 * (torch.cos(th) + 1.0), -k * torch.sin(th), k * (torch.sin(th).abs() + (th * torch.cos(th)).abs())


def upstream_rows(pair_flag, pair_i, pair_j, x, dagg):
    """g[p][c] = f0 dagg[i][c] x[j][c] + f1 dagg[j][c] x[i][c]: the gradient that reaches filter row p from the two
    directions of its pair (fp32 vector arithmetic in the kernels: S on plain absolute values).  (g, S(g))."""
    i, j = pair_i.long(), pair_j.long()
    fl = pair_flag.long()
    f0, f1 = ((fl & 1) > 0).double()[:, None], ((fl & 2) > 0).double()[:, None]
    x, dg = x.double(), dagg.double()
    return f0 * (dg[i] * x[j]) + f1 * (dg[j] * x[i]), f0 * (dg[i] * x[j]).abs() + f1 * (dg[j] * x[i]).abs()


def _layer_dpos(rbf, Srbf, diff, coeff, C, Cp, SCp, w, g, Sg, drop_where_c_is_zero):
    w1, b1, w2, b2 = (t.double() for t in w)
    f = _layer_forward(rbf, Srbf, w1, b1, w2, b2, C)
    drbf = 2.0 * coeff * diff * rbf                        # rbf'_g = 2 coeff (d - mu_g) rbf_g
    Sdrbf = 2.0 * abs(coeff) * diff.abs() * Srbf
    a = drbf @ w1.t()                                      # du/dd
    Sa = fl_(Sdrbf) @ fl_(w1).t()
    sg = f["sg"]
    v = sg * a                                             # ssp'(u) from the saved rows T: sigmoid = 1 - exp(-(T + log 2))
    Sv = sg * Sa + a.abs() * (1.0 - sg) * f["ST"]
    z = v @ w2.t()                                         # dO/dd
    Sz = fl_(Sv) @ fl_(w2).t()
    env = (Cp[:, None] * f["O"], SCp[:, None] * f["SO"])   # the C'(d) O term
    zero = (C == 0)[:, None]
    J = C[:, None] * z
    SJ = C.abs()[:, None] * Sz
    extra = torch.zeros_like(C)
    if drop_where_c_is_zero:
        # the kernel forms C' O as (C' / C) Wf and leaves the term out where the fp32 envelope rounded to zero
        extra = (zero * (g * env[0])).sum(1).abs()
        J = J + (~zero) * env[0]
        SJ = SJ + (~zero) * env[1]
    else:
        J, SJ = J + env[0], SJ + env[1]
    return dict(dd=(g * J).sum(1), S=(Sg * SJ).sum(1), extra=extra, J=J, z=z, a=a, sg=sg, g=g, fwd=f)


def filter_dpos(pair_d, pair_c, pair_flag, pair_i, pair_j, ws, offset, coeff, cutoff, xs, daggs, drop_where_c_is_zero=True):
    """geossl_cfconv_filter_dpos (filter_dpos.hip, header): dd[l][p] = sum_c g[p][c] J[p][c], J = C z + C'(d) O,
    z = W2 (sigmoid(u) * (W1 rbf')).  Per layer dict(dd, S, extra, ...): `extra` is the magnitude of the C' O term on
    the slots with pair_c == 0, where the kernel drops it by design, and 0 everywhere else."""
    rbf, Srbf, diff = gaussians(pair_d, offset, coeff)
    C = pair_c.double()
    _, Cp, SCp = envelope(pair_d.double(), cutoff)
    out = []
    for l, w in enumerate(ws):
        g, Sg = upstream_rows(pair_flag, pair_i, pair_j, xs[l], daggs[l])
        out.append(_layer_dpos(rbf, Srbf, diff, coeff, C, Cp, SCp, w, g, Sg, drop_where_c_is_zero))
    return out


def dpos_gaussian_term(layer, pair_d, pair_c, w, offset, coeff, gidx, centre=None, column=None):
    """What Gaussian `gidx` contributes to dd [P] of a layer (`layer`: its dict from filter_dpos) through z, the
    pre-activations held fixed: sum_c g C (W2 (sigmoid(u) w1[:, column] rbf'_g))_c.  `centre`, `column`: as in
    forward_gaussian_terms."""
    mu = offset.double()[gidx] if centre is None else centre
    col = gidx if column is None else column
    diff = pair_d.double() - mu
    dr = 2.0 * coeff * diff * torch.exp(coeff * diff ** 2)
    v = layer["sg"] * (dr[:, None] * w[0].double()[:, col][None, :])
    return (layer["g"] * (pair_c.double()[:, None] * (v @ w[2].double().t()))).sum(1)


def pair_slots(mol_ptr, pair_ptr):
    """Dense over every molecule: for each atom a and every other atom b of its molecule the pair slot of (a, b),
    slot = base + lo n - lo (lo + 1) / 2 - lo - 1 + hi with lo < hi the two local indices (k_pair_position_grad).
    (atom [K], other [K], slot [K]) as int64, atoms ascending, b ascending."""
    mp, pp = mol_ptr.long(), pair_ptr.long()
    n = mp[1:] - mp[:-1]
    B = n.numel()
    dev = mp.device
    if B == 0 or int(n.sum()) == 0:
        e = torch.zeros(0, dtype=torch.long, device=dev)
        return e, e, e
    mol = torch.repeat_interleave(torch.arange(B, device=dev), n)
    a_loc = torch.arange(int(n.sum()), device=dev) - mp[:-1][mol]
    nmax = int(n.max())
    b_loc = torch.arange(nmax, device=dev)[None, :].expand(mol.numel(), nmax)
    keep = (b_loc < n[mol][:, None]) & (b_loc != a_loc[:, None])
    A = a_loc[:, None].expand_as(b_loc)[keep]
    Bl = b_loc[keep]
    M = mol[:, None].expand_as(b_loc)[keep]
    lo, hi = torch.minimum(A, Bl), torch.maximum(A, Bl)
    slot = pp[:-1][M] + lo * n[M] - lo * (lo + 1) // 2 - lo - 1 + hi
    return mp[:-1][M] + A, mp[:-1][M] + Bl, slot


def pair_position_grad(pos, pair_d, dd, mol_ptr, pair_ptr):
    """geossl_pair_position_grad: dpos[a] = sum_b (sum_l dd[l][slot(a, b)]) (pos_a - pos_b) / d(a, b) over the other
    atoms of a's molecule, slots with a zero sum or a zero distance skipped.  (ref [N, 3], S [N, 3], terms [K, 3],
    atom [K]): S sums |dd| over the layers and |terms| over b."""
    atom, other, slot = pair_slots(mol_ptr, pair_ptr)
    dd = dd.double()
    s, Ss = dd[:, slot].sum(0), dd[:, slot].abs().sum(0)
    dist = pair_d.double()[slot]
    live = (s != 0) & (dist > 0)
    k = torch.where(live, s / dist.clamp_min(1e-300), torch.zeros_like(s))
    Sk = torch.where(live, Ss / dist.clamp_min(1e-300), torch.zeros_like(s))
    delta = pos.double()[atom] - pos.double()[other]
    terms = k[:, None] * delta
    ref = torch.zeros(pos.size(0), 3, dtype=torch.float64, device=pos.device).index_add(0, atom, terms)
    S = torch.zeros_like(ref).index_add(0, atom, Sk[:, None] * delta.abs())
    return ref, S, terms, atom
