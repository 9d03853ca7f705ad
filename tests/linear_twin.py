"""fp64 twin of the single-layer row GEMM (csrc/gemm.hip: geossl_linear, geossl_linear_prepared; kernels k_linear<NC>,
k_linear_split<KS, E0, E1>, k_linear_prepare<KS>) with element-wise bounds, a mirror of the launch arithmetic and the
operands the tests run it on.

A plain module (no tests).  `reference` takes the operands `ops.linear` takes, on the CPU or the GPU, and returns the
fp64 value `ref` of the result and `S`, the same expression on absolute values, so that a kernel is held to
|got - ref| <= c u S per element (tests/elementwise.py).

Operand model: the split kernel (K = 32 / 64 / 128) cuts every fp32 operand EXACTLY into three bf16 pieces and sums six
of the nine piece products in fp32; the f32-MFMA kernel (every other K = 0 mod 8 up to 256) multiplies fp32 operands.
For both fl(x) = |x| and u = 2^-24.

S through the epilogue, in the kernels' order (chain_twin has the same rules): the bias starts the accumulator: + |b|;
ssp is 1-Lipschitz and adds the magnitudes of its own terms: softplus + log 2 + sigmoid S; the factor ssp'(v) is
computed in fp32 from the saved output t = ssp(v) as 1 - exp(-t) / 2 and carries the rounding of its exp argument: it
multiplies S by 1 + exp(-t) (1 + |t|) / 2; the residual adds |res|.

`emulate` is the kernels' arithmetic on the CPU (numpy): the constants c of the bound are fixed from its error against
`reference` (tests/test_linear_twin_cpu.py), never from the kernels under test."""
import math

import numpy as np
import torch

import chain_twin as ct

LOG2 = ct.LOG2
EPI_BIAS, EPI_SSP, EPI_RESIDUAL, EPI_MUL_DSSP = 1, 2, 4, 8     # geossl_amd._lib (checked by the CPU test)
U = 2.0 ** -24
SPLIT_K = (32, 64, 128)
INT_MAX = 2 ** 31 - 1
HIP_ERROR_INVALID_VALUE = 1
# c of |got - ref| <= c u S: four times the worst err / (u S) of `emulate` against `reference` over the CPU grid, rounded
# up to a power of two and not below 8 (test_linear_twin_cpu.py: test_bound_constants_are_the_emulated_ones; DESIGN.md
# section 4).  "fp32" is keyed by K class: the f32-MFMA kernel rounds once per product, so its worst ratio grows with K.
C_BOUND = {"split": 32.0, "fp32": {64: 32.0, 256: 128.0}}
KINDS = ct.KINDS
BLOCK_SCALES = ct.BLOCK_SCALES
# which operands a launch has: (bias, ssp, tprev, res).  W [NO][K]: bias x ssp x residual; W [K][NO]: bias x tprev x
# residual; one launch with all four
FLAGSETS = ([(True, b, s, False, r) for b in (0, 1) for s in (0, 1) for r in (0, 1)] +
            [(False, b, False, t, r) for b in (0, 1) for t in (0, 1) for r in (0, 1)] + [(True, 1, 1, 1, 1)])
FLAGSETS = [(tb, bool(b), bool(s), bool(t), bool(r)) for tb, b, s, t, r in FLAGSETS]
FULL = {True: (True, True, True, False, True), False: (False, True, False, True, True)}   # the richest set per layout


def family(K):
    return "split" if K in SPLIT_K else "fp32"


def c_bound(K):
    if K in SPLIT_K:
        return C_BOUND["split"]
    return C_BOUND["fp32"][min(k for k in C_BOUND["fp32"] if K <= k)]


def flagset_name(fs):
    tb, b, s, t, r = fs
    return ("NT" if tb else "NN") + "".join(n for n, on in (("+bias", b), ("+ssp", s), ("+tprev", t), ("+res", r)) if on)


# ----------------------------------------------------------------------------------------------------------- fp64 twin
def reference(X, W, bias, res, tprev, transB, flags):
    """dict: ref, S (the stored result and its bound sum), and what the dropped-term proofs need: X, B ([K][NO] of
    Y = X B), pre (the value the epilogue is applied to), ssp, factor, bias, res."""
    x = X.double()
    B = W.double().t() if transB else W.double()
    pre, Spre = x @ B, x.abs() @ B.abs()
    if bias is not None:
        pre, Spre = pre + bias.double(), Spre + bias.double().abs()
    y, Sy = pre, Spre
    ssp = bool(flags & EPI_SSP)
    if ssp:
        sp = torch.nn.functional.softplus(pre)
        y, Sy = sp - LOG2, sp + LOG2 + torch.sigmoid(pre) * Spre
    factor = None
    if tprev is not None:
        factor, Sf = ct._factor(tprev.double(), False)
        y, Sy = y * factor, Sy * Sf
    if res is not None:
        y, Sy = y + res.double(), Sy + res.double().abs()
    return dict(ref=y, S=Sy, X=x, B=B, pre=pre, ssp=ssp, factor=factor, bias=None if bias is None else bias.double(),
                res=None if res is None else res.double())


def effect_on_output(d, term, after_epilogue=False):
    """What taking `term` [R, NO] out of the pre-epilogue value takes out of the stored result (the epilogue is
    element-wise); `after_epilogue`: the term is added behind the activation and the factor (the residual)."""
    if after_epilogue:
        return term
    a, b = d["pre"], d["pre"] - term
    if d["ssp"]:
        a, b = torch.nn.functional.softplus(a), torch.nn.functional.softplus(b)
    e = a - b
    return e if d["factor"] is None else e * d["factor"]


def dropped_terms(d):
    """Term lists of the dropped-term proofs: (what, effect [R, NO] on the stored result) for one product x_rk w_kn per
    32-wide group of the contraction (the k of the group with the largest input element), the bias and the residual."""
    K = d["X"].size(1)
    for g in range((K + 31) // 32):
        k = 32 * g + int(d["X"][:, 32 * g:32 * g + 32].abs().amax(0).argmax())
        yield "product", effect_on_output(d, d["X"][:, k:k + 1] * d["B"][k:k + 1, :])
    if d["bias"] is not None:
        yield "bias", effect_on_output(d, d["bias"][None, :].expand_as(d["pre"]))
    if d["res"] is not None:
        yield "res", effect_on_output(d, d["res"], after_epilogue=True)


def proofs(d, c, u):
    """Per kind of term the element where it is largest against its bound: (what, index, term, ratio).
    elementwise.pick_term's rule applies: a ratio under 2 cannot be told from rounding."""
    from elementwise import pick_term
    NO = d["ref"].size(1)
    best = {}
    for what, effect in dropped_terms(d):
        pos, r = pick_term(effect, c * u * d["S"], torch.ones_like(effect, dtype=torch.bool))
        if what not in best or r > best[what][2]:
            idx = (pos // NO, pos % NO)
            best[what] = (idx, effect[idx], r)
    for what, (idx, term, r) in best.items():
        yield what, idx, term, r


# ---------------------------------------------------------------------------------------------------- arithmetic model
def emulate(X, W, bias, res, tprev, transB, flags):
    """The kernels' arithmetic on the CPU, a float32 array [R, NO].  Split path (K = 32 / 64 / 128): three bf16 pieces of
    both operands, per 16-wide k-step the six piece products smallest first, one fp32 rounding per MFMA
    (chain_twin._mfma_sum), the accumulator started from the bias.  Other K: fp32 products added to the fp32 accumulator
    (started from the bias) one at a time in the order of the 32x32x2 MFMAs: step (q, s) takes k = 8 q + s, then
    8 q + 4 + s.  Epilogues in fp32.  A model for fixing c: it need not give the GPU's bits."""
    x = ct._f32(ct._np(X))
    w = ct._f32(ct._np(W))
    B = np.ascontiguousarray(w.T if transB else w)
    R, K = x.shape
    NO = B.shape[1]
    acc = np.zeros((R, NO), np.float32) if bias is None else np.broadcast_to(ct._f32(ct._np(bias)), (R, NO)).astype(np.float32)
    if K in SPLIT_K:
        (xh, xm, xl), (wh, wm, wl) = ct._split_bf16(x), ct._split_bf16(B)
        acc = ct._mfma_sum(acc, ((xh, wl), (xl, wh), (xm, wm), (xh, wm), (xm, wh), (xh, wh)))
    else:
        x64, B64 = x.astype(np.float64), B.astype(np.float64)
        for q in range(K // 8):
            for s in range(4):
                for k in (8 * q + s, 8 * q + 4 + s):
                    acc = ct._f32(acc.astype(np.float64) + x64[:, k:k + 1] * B64[k:k + 1, :])
    y = acc
    if flags & EPI_SSP:
        y = ct._ssp32(y)
    if tprev is not None:
        t = ct._f32(ct._np(tprev))
        y = y * (np.float32(1.0) - np.float32(0.5) * np.exp(-t, dtype=np.float32))
    if res is not None:
        y = y + ct._f32(ct._np(res))
    return ct._f32(y)


# ------------------------------------------------------------------------------------------- the launch, from gemm.hip
def plan(R, K, NO, prepared=False, ldx=None, ldy=None):
    """What geossl_linear (`prepared`: geossl_linear_prepared) does with R rows of width K -> NO: a dict with `refused`
    (True: hipErrorInvalidValue before any launch) or the launch: kernel ("split" / "fp32"), KS or NC, ny, nmb (32-column
    blocks per thread block), nx, and per kernel
      split: nrb, n_whole (row blocks taken whole by waves 0-3), n_tasks ((row block, column block) tasks of waves 4-7),
             rounds (row blocks of the busiest primary wave), task_rounds (tasks of the busiest secondary wave),
             idle_primaries, ragged (a block owns column blocks past NO)
      fp32:  ntiles, tiles_per_block (of block 0, the busiest), last_tile_rows, lds, big_lds."""
    ldx, ldy = K if ldx is None else ldx, NO if ldy is None else ldy
    refused = dict(refused=True)
    if R <= 0:
        return dict(refused=False, kernel=None)
    if R > INT_MAX:
        return refused
    if prepared:
        if K not in SPLIT_K or NO <= 0 or NO > 256 or NO & 3:
            return refused
    elif K % 8 or K > 256 or NO > 256 or NO & 3:
        return refused
    if ldx < K or ldy < NO or ldx & 3 or ldy & 3:
        return refused
    if K in SPLIT_K:
        KS = K // 16
        nmb_all = (NO + 31) // 32
        cap = 108 // (3 * KS)
        ny = 1
        while (nmb_all + ny - 1) // ny > cap:
            ny += 1
        if prepared and nmb_all % ny:
            return refused
        nmb = (nmb_all + ny - 1) // ny
        nrb = (R + 31) // 32
        nx = min((nrb + 3) // 4, 256)
        nprim = 4 * nx
        n_whole = nrb // nprim * nprim if nrb >= nprim else nrb
        n_tasks = (nrb - n_whole) * nmb
        return dict(refused=False, kernel="split", KS=KS, ny=ny, nmb=nmb, nx=nx, nrb=nrb, n_whole=n_whole, n_tasks=n_tasks,
                    rounds=-(-n_whole // nprim), task_rounds=-(-n_tasks // nprim), idle_primaries=max(0, nprim - n_whole),
                    ragged=ny * nmb > nmb_all, last_rows=R - 32 * (nrb - 1),
                    lds=nmb * KS * 3 * 1024 + (nmb * 32 + 8 * 32 * 36) * 4)
    ntiles = (R + 127) // 128
    NOp = (NO + 31) // 32 * 32
    NC = 4 if NOp % 128 == 0 else (2 if NOp % 64 == 0 else 1)
    if NC == 4 and ntiles < 512:
        NC = 2
    nx = min(ntiles, 1024)
    lds = (((K * (32 * NC + 1) + 3) & ~3) + 4 * 512) * 4
    return dict(refused=False, kernel="fp32", NC=NC, ny=NOp // (32 * NC), nmb=NC, nx=nx, ntiles=ntiles,
                tiles_per_block=-(-ntiles // nx), last_tile_rows=R - 128 * (ntiles - 1), lds=lds, big_lds=lds > 64 * 1024)


# ------------------------------------------------------------------------------------------------------------ operands
def ssp_output(pre):
    """A real ssp output in fp32 (what a launch's tprev holds)."""
    return (torch.nn.functional.softplus(pre.double()) - LOG2).float()


def operands(kind, R, K, NO, flagset, device="cpu", seed=0):
    """dict(X, W, bias, res, tprev, transB, flags) of one launch on `kind` operands (`slices` has the data of `main`:
    the test places it), drawn on `device` from its own generator.  flags holds EPI_SSP alone: ops.linear derives the
    others from the operands."""
    transB, has_bias, ssp, has_tprev, has_res = flagset
    g = torch.Generator(device=device).manual_seed(100003 * K + 1009 * NO + 7 * R + seed + sum(1 << i for i, f in enumerate(flagset) if f))
    rn = lambda *shape: torch.randn(*shape, generator=g, device=device)
    nb = (NO + 31) // 32
    rows = torch.arange(R, device=device)
    X = rn(R, K)
    W = rn(NO, K) / K ** 0.5                   # drawn as [NO][K]; W [K][NO] is its transpose (the same matrix B)
    bias = rn(NO) * 0.1 if has_bias else None
    res = rn(R, NO) if has_res else None
    tprev = ssp_output(3.0 * rn(R, NO)) if has_tprev else None
    if kind == "blocks":
        sc = torch.exp2(torch.tensor([BLOCK_SCALES[b % 4] for b in range(nb)], dtype=torch.float32, device=device))
        sc = sc.repeat_interleave(32)[:NO]
        W = W * sc[:, None]
        bias = None if bias is None else bias * sc
    if kind == "rows":
        row_scale = torch.exp2(((rows * 7) % 25 - 12).double()).float()[:, None]
        ng = (K + 31) // 32
        group = torch.where(torch.arange(K, device=device)[None, :] // 32 == (rows % ng)[:, None], 1024.0, 1.0)
        X = X * row_scale * group
        res = None if res is None else res * row_scale
    if kind == "zeros":
        X[rows % 5 == 0] = 0.0
        b = 1 % nb                              # one all-zero weight block (its first half where NO has a single block)
        W[32 * b:(32 * b + 32 if nb > 1 else max(NO // 2, 1))] = 0.0
    W = W.contiguous() if transB else W.t().contiguous()
    return dict(X=X, W=W, bias=bias, res=res, tprev=tprev, transB=transB, flags=EPI_SSP if ssp else 0)
