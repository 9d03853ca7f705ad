"""fp64 twins of the row kernels at the two ends of both backbones (csrc/schnet.hip, readout columns in csrc/common.h):
geossl_embedding_bwd[_dyn] (k_embedding_bwd_partial<NG>, k_embedding_bwd_reduce), geossl_segment_reduce_fwd / _bwd
(readout_col, scatter_readout_col) and geossl_row_normalize_fwd / _bwd, with element-wise bounds, a restatement of the
embedding launcher's chunk rule, and the seeded inputs the tests run them on.

A plain module (no tests).  Every twin returns (ref, S, c): the fp64 value, the same expression on absolute values and
the number of fp32 roundings on the longest path to an element, counted from the kernel's own summation order, so that a
kernel is held to |got - ref| <= c u S per element (tests/elementwise.py), u = 2^-24.  c is a count (a number, or a
column of numbers where it differs by row): it is never fitted to a kernel's output.  The build has no fast-math flag:
`/` and sqrtf are one correctly rounded operation each."""
import functools
import math

import numpy as np
import torch

from elementwise import pick_term

U = 2.0 ** -24
EMB_CHUNKS = 512                  # GEOSSL_EMB_CHUNKS
LDS_LIMIT = 160 * 1024
INT_MAX = 2 ** 31 - 1
HIP_ERROR_INVALID_VALUE = 1
EPS = 1e-12                       # ops.row_normalize's default


def _ceil(a, b):
    return -(-a // b)


def eps32(eps):
    """The clamp as the kernels see it: the entry points take a float."""
    return float(np.float32(eps))


# ------------------------------------------------------------------------------------------ embedding backward: launch
def plan(N_cap, C, F):
    """(ng, nchunks) of a launch over a capacity of N_cap rows.  Restates geossl_embedding_bwd_dyn (csrc/schnet.hip):

        const int TF = (F + 63) / 64 * 64;
        const int ng = ((size_t)4 * num_classes * F * sizeof(float) <= 48 * 1024 && 4 * TF <= 1024) ? 4 : 1;
        int nchunks = (int)((N + 32 * ng - 1) / (32 * ng));
        nchunks = nchunks < 16 ? 16 : (nchunks > GEOSSL_EMB_CHUNKS ? GEOSSL_EMB_CHUNKS : (nchunks + 3) / 4 * 4);

    The GPU test counts the band slots a launch overwrote against nchunks, so the restatement cannot drift."""
    TF = _ceil(F, 64) * 64
    ng = 4 if (4 * C * F * 4 <= 48 * 1024 and 4 * TF <= 1024) else 1
    n = (N_cap + 32 * ng - 1) // (32 * ng)
    n = 16 if n < 16 else (EMB_CHUNKS if n > EMB_CHUNKS else (n + 3) // 4 * 4)
    return ng, n


def launch(N_cap, C, F, N_real=None):
    """The launch in full: refused (hipErrorInvalidValue before anything is launched: F > 256, more rows than an int,
    or more LDS than a CU has - `lds` is what the launch asks for: the group tables and one int2 band per group), ng,
    nchunks, threads per block, lds, and with the real row count: per (rows per chunk, k_embedding_bwd_partial's
    `(N + gridDim.x - 1) / gridDim.x`), PER (chunks per slice of k_embedding_bwd_reduce), used / empty chunks."""
    ng, nchunks = plan(N_cap, C, F)
    lds = ng * C * F * 4 + ng * 8
    d = dict(ng=ng, nchunks=nchunks, threads=ng * _ceil(F, 64) * 64, lds=lds, PER=nchunks // 4,
             refused=F > 256 or N_cap > INT_MAX or lds > LDS_LIMIT)
    if N_real is not None:
        per = _ceil(N_real, nchunks)
        used = _ceil(N_real, per) if per else 0
        d.update(per=per, used=used, empty=nchunks - used)
    return d


def workspace_floats(C, F):
    """geossl_embedding_bwd_workspace_floats: the partial tables [EMB_CHUNKS][C][F], then EMB_CHUNKS int2 bands."""
    return EMB_CHUNKS * C * F + 2 * EMB_CHUNKS


def bands(z, C, N_real, nchunks):
    """The band [cmin, cmax] every chunk records ((C, -1): none of its rows has a class of the table): int64
    [nchunks, 2]."""
    out = torch.empty(nchunks, 2, dtype=torch.int64)
    out[:, 0], out[:, 1] = C, -1
    per = _ceil(N_real, nchunks)
    if per:
        zz = z[:N_real]
        ok = (zz >= 0) & (zz < C)
        chunk = (torch.arange(N_real) // per)[ok]
        out[:, 0].scatter_reduce_(0, chunk, zz[ok], "amin")
        out[:, 1].scatter_reduce_(0, chunk, zz[ok], "amax")
    return out


# ------------------------------------------------------------------------------------------------ embedding backward
def embedding_bwd(z, dh, C, N_real, prior=None, N_cap=None):
    """dtable[c][f] = sum of dh[a][f] over the rows a < N_real with z[a] == c (+ prior[c][f] under accumulate); a row
    whose class is outside [0, C) AS A 64-BIT VALUE contributes nothing.  S: the same sum of absolute values.

    c, from plan(N_cap, C, F) and per = ceil(N_real / nchunks) rows in a chunk:
      ceil(per / ng) - 1   a group adds its rows of a chunk (every ng-th) to its LDS column one after the other, the
                           first onto 0.0 (exact)
      ng - 1               the group tables are added in group order
      2                    k_embedding_bwd_reduce sums a slice's chunks compensated (Kahan): first order 2 u whatever
                           the number of chunks.  Its second-order term is about n u^2 for the n chunks of a slice:
                           n u = 2^-15 of one u even if all 512 chunks sat in one slice - far below 1 u, not carried
      3                    red[0] is added to 0.0 (exact), then the three other slices
      1                    under accumulate: the prior is there first, red[0] is one more addition; S holds |prior|."""
    N_cap = z.size(0) if N_cap is None else N_cap
    F = dh.size(1)
    zz, d = z[:N_real], dh[:N_real].double()
    ok = (zz >= 0) & (zz < C)
    ref = torch.zeros(C, F, dtype=torch.float64).index_add_(0, zz[ok], d[ok])
    S = torch.zeros(C, F, dtype=torch.float64).index_add_(0, zz[ok], d[ok].abs())
    if prior is not None:
        ref, S = ref + prior.double(), S + prior.double().abs()
    return ref, S, embedding_bwd_c(N_cap, C, F, N_real, prior is not None)


def embedding_bwd_c(N_cap, C, F, N_real, accumulate):
    ng, nchunks = plan(N_cap, C, F)
    per = _ceil(N_real, nchunks)
    return float(max(_ceil(per, ng) - 1, 0) + (ng - 1) + 2 + 3 + (1 if accumulate else 0))


# ------------------------------------------------------------------------------------------------------------ readout
def _sizes(mol_ptr):
    p = [int(v) for v in mol_ptr]
    return [(p[m], p[m + 1]) for m in range(len(p) - 1)]


def segment_reduce_fwd(h, mol_ptr, mean):
    """out[m] = the rows [mol_ptr[m], mol_ptr[m + 1]) of h added in atom order (readout_col), "mean": / max(n, 1).  An
    empty molecule gives 0.  c [B, 1] = n - 1 sequential additions (the first onto 0.0 is exact), + 1 for the mean's
    division."""
    x = h.double()
    ref, S, c = [], [], []
    for a0, a1 in _sizes(mol_ptr):
        div = float(max(a1 - a0, 1)) if mean else 1.0
        ref.append(x[a0:a1].sum(0) / div)
        S.append(x[a0:a1].abs().sum(0) / div)
        c.append(float(max(a1 - a0 - 1, 0) + (1 if mean else 0)))
    return torch.stack(ref), torch.stack(S), torch.tensor(c, dtype=torch.float64)[:, None]


def segment_reduce_bwd(dout, mol_ptr, mean, prior=None):
    """dh[a] = dout[m] for the rows of molecule m ("mean": / max(n, 1)), + prior under accumulate (scatter_readout_col).
    c: "add" copies (0: exact), "mean" rounds once, accumulate once more."""
    g = dout.double()
    N = int(mol_ptr[-1])
    ref = torch.zeros(N, g.size(1), dtype=torch.float64)
    for m, (a0, a1) in enumerate(_sizes(mol_ptr)):
        ref[a0:a1] = g[m] / (float(max(a1 - a0, 1)) if mean else 1.0)
    S = ref.abs()
    if prior is not None:
        ref, S = ref + prior.double(), S + prior.double().abs()
    return ref, S, float((1 if mean else 0) + (1 if prior is not None else 0))


def row_of_molecule(mol_ptr):
    p = torch.as_tensor(mol_ptr, dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(p.numel() - 1), p[1:] - p[:-1])


# ------------------------------------------------------------------------------------------------------ row normalize
def _norm_parts(h, eps, drop):
    x = h.double()
    sq = x * x
    if drop is not None:
        sq = sq.clone()
        sq[drop] = 0.0
    nr = sq.sum(1, keepdim=True).sqrt()
    return x, nr, nr < eps32(eps)


def row_normalize_fwd(h, eps=EPS, drop=None):
    """y = h / max(||h||, eps) (k_row_normalize_fwd: one wave per row).  S = |y|.  c [N, 1], with k = ceil(F / 64):
      k     fused multiply-adds per lane into the sum of squares (all terms >= 0: its error is relative)
      6     butterfly steps of wave_sum
      2     the square root and the division
    and on a row clamped at eps the division alone: 1.  `drop` = (row, column): that square is left out of the row's
    norm (what the checker must see)."""
    x, nr, clamped = _norm_parts(h, eps, drop)
    y = x / torch.where(clamped, torch.full_like(nr, eps32(eps)), nr)
    k = _ceil(h.size(1), 64)
    return y, y.abs(), torch.where(clamped, 1.0, k + 8.0).double()


def row_norm(h, eps=EPS):
    """The norm the forward keeps for the backward: (ref, S, c, extra) [N, 1].  c = k + 6 + 1 (no division).  extra:
    a square or a partial sum below 2^-126 is rounded absolutely, by at most 2^-150 in each of the F fused multiply-adds
    and 63 additions behind lane 0's result, and sqrt passes d(ss) on as d(ss) / (2 norm).  It is 1e-43 / norm: nothing
    against u norm on any row but one of elements near 1e-20, and 0 on an all-zero row, whose norm is exactly 0."""
    x, nr, _ = _norm_parts(h, eps, None)
    F = h.size(1)
    extra = torch.where(nr > 0, (F + 63) * 2.0 ** -150 / (2.0 * nr.clamp_min(1e-300)), torch.zeros_like(nr))
    return nr, nr, float(_ceil(F, 64) + 7), extra


def row_normalize_bwd(g, y, norm, eps=EPS, drop=None):
    """dh = (g - y (g . y)) / max(norm, eps), and g / eps on a row with norm < eps (k_row_normalize_bwd); y and norm are
    taken as given, as the kernel takes them.  S = (|g_f| + |y_f| sum |g y|) / max(norm, eps): the cancellation in
    g - y (g . y) is held against the magnitudes of its terms.  c [N, 1], with k = ceil(F / 64):
      k + 6  the dot product: k fused multiply-adds per lane, six butterfly steps (they act on |y_f| sum |g y|)
      2      the product y_f dot and the subtraction
      2      the reciprocal of max(norm, eps) and the multiplication by it
    and on a clamped row the last two alone: 2, S = |g| / eps.  `drop` = (row, column): that product is left out of the
    row's dot."""
    gd, yd, nd = g.double(), y.double(), norm.double().reshape(-1, 1)
    e = eps32(eps)
    clamped = nd < e
    den = torch.where(clamped, torch.full_like(nd, e), nd)
    prod = gd * yd
    if drop is not None:
        prod = prod.clone()
        prod[drop] = 0.0
    dot, A = prod.sum(1, keepdim=True), prod.abs().sum(1, keepdim=True)
    ref = torch.where(clamped, gd, gd - yd * dot) / den
    S = torch.where(clamped, gd.abs(), gd.abs() + yd.abs() * A) / den
    k = _ceil(g.size(1), 64)
    return ref, S, torch.where(clamped, 2.0, k + 10.0).double()


# ------------------------------------------------------------------------------------------- the dropped-term choice
def pick(terms, bound, where):
    """elementwise.pick_term, with an element of bound 0 (it must come out exactly) taken first: any term there stands
    infinitely above its bound.  (flat position, ratio) or None without a candidate."""
    if terms.numel() == 0 or not bool(where.any()):
        return None
    exact = where & (bound == 0) & (terms != 0)
    if bool(exact.any()):
        return int(torch.where(exact, terms.abs(), torch.zeros_like(terms)).argmax()), float("inf")
    return pick_term(terms, bound, where)


# ================================================================================================= the GPU test's cases
# ---- embedding backward.  name -> C, F, N (capacity), pattern, and: zs (stride of z), acc, dyn (real rows), scale
# (dh times 2^scale), seed (cases that share one share their draws)
def _e(C, F, N, pattern="shuffled", **kw):
    return dict(dict(C=C, F=F, N=N, pattern=pattern, zs=1, acc=False, dyn=None, scale=0, seed=None), **kw)


EMB_BWD = {
    # group plans: (ng, threads per block)
    "plan C=9 F=128": _e(9, 128, 700),              # 4, 512
    "plan C=100 F=128": _e(100, 128, 700),          # 1, 128: PaiNN's table
    "plan C=9 F=256": _e(9, 256, 700),              # 4, 1024
    "plan C=13 F=256": _e(13, 256, 700),            # 1, 256
    "plan C=9 F=48": _e(9, 48, 700),                # 4, 256: 48 of each group's 64 lanes live
    # row counts
    "rows 0": _e(9, 128, 0),
    "rows 0 accumulate": _e(9, 128, 0, acc=True),
    "rows 1": _e(9, 128, 1),
    "rows 2049": _e(9, 128, 2049, seed=2049),       # 17 chunks rounded to 20
    "rows 32768": _e(9, 128, 32768),                # PER = 64: the first ballot round full, the second empty
    "rows 32769": _e(9, 128, 32769),                # PER = 65: one lane in the second round
    "rows 65537": _e(9, 128, 65537),                # 513 chunks capped at 512, per = 129, empty trailing chunks
    "one group rows 8193": _e(100, 128, 8193),      # PER = 65 on the one-group plan
    "one group rows 16385": _e(100, 128, 16385),    # capped on the one-group plan, per = 33
    # class patterns
    "sorted": _e(9, 128, 2049, "sorted"),
    "sorted rows 32769": _e(9, 128, 32769, "sorted"),
    "classes 1 and 8": _e(9, 128, 2049, "two"),
    "one chunk, one absent": _e(9, 128, 2049, "one_chunk"),
    "one chunk, one absent, accumulate": _e(9, 128, 2049, "one_chunk", acc=True),
    "z stride 2": _e(9, 128, 2049, zs=2),
    "out of range": _e(9, 128, 2049, "out_of_range"),
    "out of range, one group": _e(100, 128, 2049, "out_of_range"),
    "accumulate": _e(9, 128, 2049, acc=True),
    "accumulate, one group": _e(100, 128, 700, acc=True),
    "dyn 5000 of 8203": _e(9, 128, 8203, dyn=5000),
    "dh 2^-20": _e(9, 128, 2049, scale=-20, seed=2049),
    "dh 2^20": _e(9, 128, 2049, scale=20, seed=2049),
}
OUT_OF_RANGE = (-1, None, 2 ** 32 + 1)              # None: C itself
ONE_CHUNK, ONE_CHUNK_CLASS, ABSENT_CLASS = 5, 8, 4


@functools.lru_cache(maxsize=None)
def emb_bwd_case(name):
    """The seeded operands of one case (CPU tensors), its twin and its dropped term: z_store [N, zs] (z is column 0, the
    other column holds 99), dh, prior, ref, S, c, absent (classes without a row), pick = (index, term, ratio) or None."""
    s = EMB_BWD[name]
    C, F, N = s["C"], s["F"], s["N"]
    seed = s["seed"] if s["seed"] is not None else 7919 * sorted(EMB_BWD).index(name) + 13
    g = torch.Generator().manual_seed(seed)
    N_real = N if s["dyn"] is None else s["dyn"]
    L = launch(N, C, F, N_real)
    z = torch.randint(0, C, (N,), generator=g)
    dh = torch.randn(N, F, generator=g)
    prior = torch.randn(C, F, generator=g) if s["acc"] else None
    if s["pattern"] == "sorted":
        z = z.sort().values
    elif s["pattern"] == "two":
        z = torch.where(z % 2 == 0, 1, 8)
    elif s["pattern"] == "one_chunk":
        allowed = torch.tensor([c for c in range(C) if c not in (ONE_CHUNK_CLASS, ABSENT_CLASS)])
        z = allowed[z % allowed.numel()]
        z[ONE_CHUNK * L["per"]:ONE_CHUNK * L["per"] + 3] = ONE_CHUNK_CLASS
    elif s["pattern"] == "out_of_range":
        for k, v in enumerate(OUT_OF_RANGE):
            z[3 + 7 * k::21] = C if v is None else v
    if s["scale"]:
        dh = dh * 2.0 ** s["scale"]
    if s["dyn"] is not None:
        z[N_real:], dh[N_real:] = 99, float("nan")
    z_store = torch.full((N, s["zs"]), 99, dtype=torch.int64)
    z_store[:, 0] = z
    ref, S, c = embedding_bwd(z, dh, C, N_real, prior, N_cap=N)
    ok = (z[:N_real] >= 0) & (z[:N_real] < C)
    zc = z[:N_real].clamp(0, C - 1)
    p = pick(dh[:N_real].double(), c * U * S[zc], ok[:, None].expand(N_real, F))
    if p is not None:
        a, f = divmod(p[0], F)
        p = ((int(z[a]), f), float(dh[a, f]), p[1])
    present = set(int(v) for v in z[:N_real][ok].unique())
    return dict(s, name=name, N_real=N_real, launch=L, z_store=z_store, z=z, dh=dh, prior=prior, ref=ref, S=S, c=c,
                absent=[k for k in range(C) if k not in present], pick=p, bands=bands(z, C, N_real, L["nchunks"]))


# ---- readout: one ragged batch
SEG_SIZES = (0, 1, 2, 33, 255, 0)
SEG_F = (48, 128, 300)                              # 300: the 256-thread block's stride loop takes a second pass


def seg_mol_ptr():
    return torch.tensor([0] + list(np.cumsum(SEG_SIZES)), dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def seg_case(F, mean, accumulate):
    """h [N, F], dout [B, F], prior [N, F] or None; fwd / bwd: (ref, S, c); pick_fwd / pick_bwd: (index, term, ratio)."""
    g = torch.Generator().manual_seed(1000 * F + 10 * int(mean) + int(accumulate))
    mp = seg_mol_ptr()
    N, B = int(mp[-1]), len(SEG_SIZES)
    h, dout = torch.randn(N, F, generator=g), torch.randn(B, F, generator=g)
    prior = torch.randn(N, F, generator=g) if accumulate else None
    fwd, bwd = segment_reduce_fwd(h, mp, mean), segment_reduce_bwd(dout, mp, mean, prior)
    mol = row_of_molecule(mp)
    n = torch.tensor([max(s, 1) if mean else 1 for s in SEG_SIZES], dtype=torch.float64)
    terms = h.double() / n[mol][:, None]
    p = pick(terms, (fwd[2] * U * fwd[1])[mol], torch.ones_like(terms, dtype=torch.bool))
    a, f = divmod(p[0], F)
    pick_fwd = ((int(mol[a]), f), float(terms[a, f]), p[1])
    terms = dout.double()[mol] / n[mol][:, None]
    p = pick(terms, bwd[2] * U * bwd[1], torch.ones_like(terms, dtype=torch.bool))
    a, f = divmod(p[0], F)
    return dict(F=F, mean=mean, accumulate=accumulate, mol_ptr=mp, h=h, dout=dout, prior=prior, fwd=fwd, bwd=bwd,
                pick_fwd=pick_fwd, pick_bwd=((a, f), float(terms[a, f]), p[1]))


# ---- row normalize
RN_ROWS = (1, 5, 333)           # one live wave of four in a block; a partial last block; 84 blocks
RN_F = (48, 64, 128, 300)
# which row holds what (row counts that have the row)
RN_ZERO, RN_TINY, RN_ABOVE_EPS = {5: 1, 333: 3}, {5: 2, 333: 7}, {5: 3, 333: 11}
RN_SMALL, RN_LARGE = {333: range(20, 30)}, {5: range(4, 5), 333: range(30, 40)}


@functools.lru_cache(maxsize=None)
def rn_case(N, F):
    """h, g [N, F]; y32 / norm32: the twin's y and norm rounded to fp32 (what the backward is given); fwd, norm, bwd:
    the twins; drop_row: an ordinary row whose largest square (the forward) / largest product (the backward) is dropped
    from the reduction; pick_*: the element of that row where the effect stands highest above its bound; pick_g: one
    term g_f / max(norm, eps) of the backward: (index, term, ratio)."""
    gen = torch.Generator().manual_seed(100 * N + F)
    h, g = torch.randn(N, F, generator=gen), torch.randn(N, F, generator=gen)
    sign = torch.where(torch.arange(F) % 3 == 0, -1.0, 1.0)
    if N in RN_ZERO:
        h[RN_ZERO[N]] = 0.0
        h[RN_TINY[N]] = 1e-20
        h[RN_ABOVE_EPS[N]] = sign * 4.0 * EPS / math.sqrt(F)           # norm = 4 eps
    for r in RN_SMALL.get(N, ()):
        h[r] *= 2.0 ** -40
    for r in RN_LARGE.get(N, ()):
        h[r] *= 2.0 ** 40
    fwd, norm = row_normalize_fwd(h), row_norm(h)
    y32, norm32 = fwd[0].float(), norm[0].float().reshape(-1)
    bwd = row_normalize_bwd(g, y32, norm32)
    r = 0 if N < 333 else 100
    d = dict(N=N, F=F, h=h, g=g, y32=y32, norm32=norm32, fwd=fwd, norm=norm, bwd=bwd, drop_row=r)
    row = torch.zeros(N, 1, dtype=torch.bool)
    row[r] = True
    for key, ref, S, c, dropped in (
            ("fwd", fwd[0], fwd[1], fwd[2], row_normalize_fwd(h, drop=(r, int(h[r].abs().argmax())))[0]),
            ("bwd", bwd[0], bwd[1], bwd[2], row_normalize_bwd(g, y32, norm32, drop=(r, int((g[r] * y32[r]).abs().argmax())))[0])):
        effect = ref - dropped
        assert bool((effect[~row.expand_as(effect)] == 0).all())
        p = pick(effect, c * U * S, row.expand_as(effect))
        d["drop_" + key] = dropped
        d["pick_" + key] = (divmod(p[0], F), float(effect.reshape(-1)[p[0]]), p[1])
    den = torch.where(norm32[:, None].double() < eps32(EPS), eps32(EPS), norm32[:, None].double())
    terms = g.double() / den
    p = pick(terms, bwd[2] * U * bwd[1], torch.ones_like(terms, dtype=torch.bool))
    d["pick_g"] = (divmod(p[0], F), float(terms.reshape(-1)[p[0]]), p[1])
    return d
