"""fp64 twin of the chained row GEMMs (csrc/chain.hip: geossl_linear_chain) with element-wise bounds, the catalogue of
chain forms the models launch, and the operands the tests run them on.

A plain module (no tests).  `chain` takes the stage dicts `ops.linear_chain` takes, with the weight `W` and its
`transB` in place of the operand image, on the CPU or the GPU, and returns per stage the fp64 value `ref` of the result
and `S`, the same expression on absolute values, so that a kernel is held to |got - ref| <= c u S per element
(tests/elementwise.py).

Operand model, per scale group of the kernel and not coarser:
  F = 128 (k_row_chain_cu: two fp16 pieces, u = 2^-22): an input row has ONE power-of-two scale over its 128 columns and
  a weight one per 32-output-column block (k_chain_prepare<8>), so an operand element is exact to 22 bits of itself or
  to 2^-12 of the largest element of its group: fl(x_ik) = |x_ik| + 2^-12 max_k |x_ik|, fl(w_jk) = |w_jk| + 2^-12 max
  |w| over the block that holds j.  The scale of a handed-on row is taken from the stage result BEFORE the silu of an
  EPI_SILU hand-on (|silu(y)| <= |y|), so the floor of such a row is 2^-12 max_k S(y).
  F = 64 / 32 (k_row_chain8: three bf16 pieces, no scales, u = 2^-24): fl(a) = |a|.

S through the epilogues (filter_twin._layer_forward): ssp: |ssp| + log 2 + sigmoid S; a factor computed in fp32 from a
given input t (ssp'(t) from the saved output, silu'(t)) carries the rounding of its exp argument, S(exp(-t)) =
exp(-t) (1 + |t|); res adds |res|; add_prev adds the S of the stage before; silu hand-on: |silu(y)| + |silu'(y)| S(y).

`emulate` is the kernels' arithmetic on the CPU (numpy): the constants c of the bound are fixed from its error against
`ref` (tests/test_chain_twin_cpu.py), never from the kernels under test."""
import math

import numpy as np
import torch

LOG2 = math.log(2.0)
EPI_SSP, EPI_SILU, EPI_MUL_DSILU = 2, 128, 256          # geossl_amd._lib (checked by the CPU test)
U = {128: 2.0 ** -22, 64: 2.0 ** -24, 32: 2.0 ** -24}
FAMILY = {128: "two-piece", 64: "bf16x3", 32: "bf16x3"}
# c of |got - ref| <= c u S: four times the worst err / (u S) of `emulate` against `ref` over the CPU grid, rounded up to
# a power of two (test_chain_twin_cpu.py: test_bound_constants_are_the_emulated_ones)
C_BOUND = {"two-piece": 8.0, "bf16x3": 32.0}
# absolute term of the activated copy: silu_f(y) = y / (1 + expf(-y)) is -0 once expf(-y) overflows (y < -88.7), where
# silu(y) is as large as 89 e^-89 = 2^-122: below the range of the format, not a matter of u S
ACT_FLOOR = 2.0 ** -120


# ----------------------------------------------------------------------------------------------------------- fp64 twin
def _silu(v):
    return v * torch.sigmoid(v)


def _dsilu(v):
    sg = torch.sigmoid(v)
    return sg * (1.0 + v * (1.0 - sg))


def _factor(t, dsilu):
    """The fp32 factor a stage multiplies by, from the given input t, and its S: (f, S(f))."""
    e = torch.exp(-t)
    Se = e * (1.0 + t.abs())
    if not dsilu:                                  # dssp_from_out: 1 - exp(-t) / 2
        return 1.0 - 0.5 * e, 1.0 + 0.5 * Se
    sg = 1.0 / (1.0 + e)                           # dsilu_f: sg (1 + t (1 - sg))
    Ssg = sg * (1.0 + Se / (1.0 + e))
    one_m = 1.0 - sg
    return sg * (1.0 + t * one_m), Ssg * (1.0 + t.abs() * one_m) + sg * t.abs() * (one_m + Ssg)


def _matrix(st):
    """B [K][NO] of Y = X B: W^T for transB (torch layout) else W."""
    W = st["W"].double()
    return W.t() if st.get("transB", True) else W


def _fl_weight(B, F):
    """fl of the operand matrix B [K][NO]: per 32-output-column block (all k) at F = 128, plain |B| else."""
    A = B.abs()
    if F != 128:
        return A
    blk = A.reshape(F, F // 32, 32).amax(dim=(0, 2))
    return A + 2.0 ** -12 * blk.repeat_interleave(32)[None, :]


def _fl_rows(S, F, floor_of=None):
    """fl of input rows with magnitudes S: one scale per row over all columns at F = 128 (from `floor_of` if given)."""
    if F != 128:
        return S
    return S + 2.0 ** -12 * (S if floor_of is None else floor_of).amax(dim=1, keepdim=True)


def chain(X, stages):
    """One dict per stage: ref, S (the stored result), ref_act, S_act (silu of it where EPI_SILU is set, else None), and
    what the dropped-term proofs need: xin, Sxin (the stage's input rows and their S), B, pre (the value the epilogue is
    applied to, add_prev summand included), factor, res, handon (the stage whose silu is this stage's input, or None)."""
    F = X.size(1)
    x, Sx, floor_of, handon = X.double(), X.double().abs(), None, None
    out = []
    v = Sv = None
    for s, st in enumerate(stages):
        flags = int(st.get("flags", 0))
        if st.get("x") is not None:
            x, Sx, floor_of, handon = st["x"].double(), st["x"].double().abs(), None, None
        elif s > 0 and not st.get("same_input"):
            prev = stages[s - 1]
            if int(prev.get("flags", 0)) & EPI_SILU:
                x, Sx, floor_of, handon = _silu(v), _silu(v).abs() + _dsilu(v).abs() * Sv, Sv, s - 1
            else:
                x, Sx, floor_of, handon = v, Sv, None, None
        B = _matrix(st)
        pre = x @ B
        Spre = _fl_rows(Sx, F, floor_of) @ _fl_weight(B, F)
        if st.get("bias") is not None:
            pre = pre + st["bias"].double()
            Spre = Spre + st["bias"].double().abs()
        prev_v = None
        if st.get("add_prev"):
            prev_v = v
            pre, Spre = pre + v, Spre + Sv
        y, Sy = pre, Spre
        if flags & EPI_SSP:
            sp = torch.nn.functional.softplus(pre)
            y, Sy = sp - LOG2, sp + LOG2 + torch.sigmoid(pre) * Spre
        factor = None
        if st.get("tprev") is not None:
            factor, Sf = _factor(st["tprev"].double(), bool(flags & EPI_MUL_DSILU))
            y, Sy = y * factor, Sy * Sf
        if st.get("res") is not None:
            y, Sy = y + st["res"].double(), Sy + st["res"].double().abs()
        v, Sv = y, Sy
        d = dict(ref=y, S=Sy, ref_act=None, S_act=None, xin=x, Sxin=Sx, B=B, pre=pre, prev=prev_v, factor=factor,
                 ssp=bool(flags & EPI_SSP), res=st.get("res"), handon=handon)
        if flags & EPI_SILU:
            d["ref_act"], d["S_act"] = _silu(y), _silu(y).abs() + _dsilu(y).abs() * Sy
        out.append(d)
    return out


def product_terms(stage, k):
    """What contraction index k contributes to the pre-epilogue value of a stage (`stage`: its dict from `chain`):
    dict(product [R, F], add_prev (the summand of the stage before, or None), res (the residual summand, or None))."""
    return dict(product=stage["xin"][:, k:k + 1] * stage["B"][k:k + 1, :], add_prev=stage["prev"],
                res=None if stage["res"] is None else stage["res"].double())


def effect_on_output(stage, term, after_epilogue=False):
    """What taking `term` [R, F] out of a stage's pre-epilogue value takes out of its stored result (the epilogue is
    element-wise); `after_epilogue`: the term is added behind the activation and the factor (the res summand)."""
    if after_epilogue:
        return term
    a, b = stage["pre"], stage["pre"] - term
    if stage["ssp"]:
        a, b = torch.nn.functional.softplus(a), torch.nn.functional.softplus(b)
    d = a - b
    return d if stage["factor"] is None else d * stage["factor"]


def effect_on_act(stage, effect):
    """What `effect` on the stored result takes out of silu of it (out_act)."""
    return _silu(stage["ref"]) - _silu(stage["ref"] - effect)


def handon_terms(prev_stage, stage, k):
    """What stage `stage` loses at contraction index k when the EPI_SILU hand-on of the stage before it is left out
    (it reads y where it should read silu(y))."""
    y = prev_stage["ref"][:, k:k + 1]
    return (_silu(y) - y) * stage["B"][k:k + 1, :]


def dropped_terms(res, form, g):
    """What the dropped-term proofs take out of the STORED results of a chain (`res` from `chain`): (stage, what,
    effect [R, F]) for the product term of one contraction index of 32-column group g (the input column of the group
    with the largest element), the add_prev summand, the res summand and the silu hand-on at one index of the group
    (the one where silu(y) - y is largest), where the stage has them."""
    grp = slice(32 * g, 32 * g + 32)
    for s, (d, sp) in enumerate(zip(res, form)):
        if not sp["store"]:
            continue
        k = 32 * g + int(d["xin"][:, grp].abs().amax(0).argmax())
        t = product_terms(d, k)
        yield s, "product", effect_on_output(d, t["product"])
        if t["add_prev"] is not None:
            yield s, "add_prev", effect_on_output(d, t["add_prev"])
        if t["res"] is not None:
            yield s, "res", effect_on_output(d, t["res"], after_epilogue=True)
        if d["handon"] is not None:
            y = res[d["handon"]]["ref"][:, grp]
            k = 32 * g + int((_silu(y) - y).abs().amax(0).argmax())
            yield s, "hand-on", effect_on_output(d, handon_terms(res[d["handon"]], d, k))


def proofs(res, form, F, c, u):
    """The dropped-term proofs of a chain: for every stored result (and its activated copy) and every kind of term it
    has, the element where the term is largest against its bound, over one contraction index per 32-column group (a
    stage's input columns differ by orders of magnitude on the `blocks` operands).  Yields (stage, what, act, index,
    term, ratio); elementwise.pick_term's rule applies: a ratio under 2 cannot be told from rounding."""
    from elementwise import pick_term
    best = {}
    for g in range(F // 32):
        for s, what, effect in dropped_terms(res, form, g):
            d = res[s]
            for act in (False, True) if d["ref_act"] is not None else (False,):
                e = effect_on_act(d, effect) if act else effect
                bound = c * u * (d["S_act"] if act else d["S"]) + (ACT_FLOOR if act else 0.0)
                pos, r = pick_term(e, bound, torch.ones_like(e, dtype=torch.bool))
                if (s, what, act) not in best or r > best[(s, what, act)][2]:
                    idx = (pos // F, pos % F)
                    best[(s, what, act)] = (idx, e[idx], r)
    for (s, what, act), (idx, term, r) in best.items():
        yield s, what, act, idx, term, r


# ---------------------------------------------------------------------------------------------------- arithmetic model
def _f32(a):
    return np.asarray(a, dtype=np.float32)


def mag_exponent(m):
    """split.h: exponent e of m = f 2^e, f in [0.5, 1), floored at -100; zero maps to the floor."""
    e = np.frexp(_f32(m))[1]
    return np.where(_f32(m) > 0, np.maximum(e, -100), -100).astype(np.int64)


def _split_fp16(v64):
    """Two fp16 pieces of exactly known values (float64 holds the scaled fp32 operand exactly): h = fp16(v), l =
    fp16(v - h), each rounded once."""
    h = v64.astype(np.float16)
    l = (v64 - h.astype(np.float64)).astype(np.float16)
    return h.astype(np.float32), l.astype(np.float32)


def _bf16(a):
    """Round-to-nearest-even bf16 of fp32 values, returned as fp32."""
    b = _f32(a).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def _split_bf16(a):
    a = _f32(a)
    h = _bf16(a)
    r = a - h
    m = _bf16(r)
    return h, m, _bf16(r - m)


def _ssp32(x):
    z = np.exp(-np.abs(x), dtype=np.float32)
    l = np.log2(np.float32(1.0) + z, dtype=np.float32)
    return _f32(l.astype(np.float64) * np.float64(np.float32(LOG2)) + np.maximum(x, 0).astype(np.float64)) - np.float32(LOG2)


def _silu32(x):
    return x / (np.float32(1.0) + np.exp(-x, dtype=np.float32))


def _dsilu32(x):
    sg = np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))
    return sg * (np.float32(1.0) + x * (np.float32(1.0) - sg))


def _mfma_sum(acc, pairs):
    """acc += sum over the piece products of `pairs` (x piece [R, K], weight piece [K, F]) the way the kernels issue
    them: per 16-wide k-step one MFMA per pair, smallest products first.  One MFMA adds the sum of its 16 products (exact
    here: float64 holds it) to the fp32 accumulator with one rounding."""
    K = pairs[0][0].shape[1]
    for ks in range(K // 16):
        k = slice(16 * ks, 16 * ks + 16)
        for a, b in pairs:
            acc = _f32(acc.astype(np.float64) + a[:, k].astype(np.float64) @ b[k, :].astype(np.float64))
    return acc


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def emulate(X, stages, F):
    """The kernels' arithmetic on the CPU: operands cut to two fp16 pieces under the kernel's power-of-two scales (F =
    128) or to three bf16 pieces (F = 64 / 32), piece products summed in fp32 (one rounding per MFMA: _mfma_sum), epilogues
    in fp32.  Returns per stage
    (out, out_act or None) as float32 arrays.  A model for fixing c: it need not give the GPU's bits."""
    two = F == 128

    def frag_rows(x, scale_from=None):
        if not two:
            return _split_bf16(x), None
        e = mag_exponent(np.abs(x if scale_from is None else scale_from).max(axis=1))
        h, l = _split_fp16(x.astype(np.float64) * np.exp2((14 - e).astype(np.float64))[:, None])
        return (h, l), np.exp2((e - 14).astype(np.float64))

    def frag_weight(B):
        if not two:
            return _split_bf16(B), None
        e = mag_exponent(np.abs(B).reshape(F, F // 32, 32).max(axis=(0, 2)))
        e = np.repeat(e, 32)
        h, l = _split_fp16(B.astype(np.float64) * np.exp2((14 - e).astype(np.float64))[None, :])
        return (h, l), np.exp2((e - 14).astype(np.float64))

    xf, krow = frag_rows(_f32(_np(X)))
    v = None
    out = []
    for s, st in enumerate(stages):
        flags = int(st.get("flags", 0))
        if st.get("x") is not None:
            xf, krow = frag_rows(_f32(_np(st["x"])))
        elif s > 0 and not st.get("same_input"):
            hand = _silu32(v) if int(stages[s - 1].get("flags", 0)) & EPI_SILU else v
            xf, krow = frag_rows(hand, scale_from=v)
        W = _f32(_np(st["W"]))
        wf, kw = frag_weight(np.ascontiguousarray(W.T if st.get("transB", True) else W))
        bias = np.zeros(F, np.float32) if st.get("bias") is None else _f32(_np(st["bias"]))
        if two:
            (xh, xl), (wh, wl) = xf, wf
            acc = _mfma_sum(np.zeros((xh.shape[0], F), np.float32), ((xh, wl), (xl, wh), (xh, wh)))
            acc = _f32(acc.astype(np.float64) * (krow[:, None] * kw[None, :]) + bias.astype(np.float64))   # one fma
        else:
            (xh, xm, xl), (wh, wm, wl) = xf, wf
            acc = _mfma_sum(np.broadcast_to(bias, (xh.shape[0], F)).astype(np.float32),
                            ((xh, wl), (xl, wh), (xm, wm), (xh, wm), (xm, wh), (xh, wh)))
        y = acc + v if st.get("add_prev") else acc
        if flags & EPI_SSP:
            y = _ssp32(y)
        if st.get("tprev") is not None:
            t = _f32(_np(st["tprev"]))
            y = y * (_dsilu32(t) if flags & EPI_MUL_DSILU else np.float32(1.0) - np.float32(0.5) * np.exp(-t, dtype=np.float32))
        if st.get("res") is not None:
            y = y + _f32(_np(st["res"]))
        v = _f32(y)
        out.append((v, _silu32(v) if flags & EPI_SILU else None))
    return out


# ------------------------------------------------------------------------------------------------- catalogue of forms
def _st(**kw):
    """A stage of a form: which operands it has.  bias / res / x / out_act: present or not; tprev: None, "dssp" or
    "dsilu"; store: the result is written."""
    d = dict(bias=False, ssp=False, silu=False, res=False, tprev=None, store=True, out_act=False, same_input=False,
             x=False, add_prev=False)
    d.update(kw)
    return d


_B = dict(bias=True)
_FAN = [_st(bias=True), _st(bias=True, same_input=True), _st(bias=True, same_input=True)]
_WIDE3 = [_st(store=False), _st(x=True, add_prev=True, store=False), _st(x=True, add_prev=True, tprev="dsilu")]
FORMS = {
    128: {
        # SchNet, forward (schnet.py: conv.lin1; conv.lin2 + act, lin + residual, next conv.lin1 or the head) ...
        "lin": [_st()],
        "lin-bias": [_st(**_B)],
        "ssp": [_st(ssp=True, **_B)],
        "ssp-res": [_st(ssp=True, **_B), _st(res=True, **_B)],
        "ssp-res-lin": [_st(ssp=True, **_B), _st(res=True, **_B), _st()],
        "ssp-res-ssp": [_st(ssp=True, **_B), _st(res=True, **_B), _st(ssp=True, **_B)],
        "ssp-unstored-tprev": [_st(ssp=True, **_B), _st(res=True, store=False, **_B), _st(tprev="dssp")],
        # ... and backward (through lin2 of the head and act; conv.lin1 + residual, through lin and act, conv.lin2)
        "tprev-lin": [_st(tprev="dssp"), _st()],
        "res": [_st(res=True)],
        "bias-res": [_st(res=True, **_B)],
        "res-tprev-lin": [_st(res=True), _st(tprev="dssp"), _st()],
        # PaiNN, forward: Dense(F, F, silu) + Dense(F, 3F); the channel mix; Dense(2F, F, silu) + Dense(F, 3F)
        "silu-fan": [_st(silu=True, out_act=True, **_B)] + _FAN,
        "fan2": [_st(), _st(same_input=True)],
        "fan3-bias": list(_FAN),
        "wide-silu-fan": [_st(store=False, **_B), _st(x=True, add_prev=True, silu=True, out_act=True)] + _FAN,
        "wide2": [_st(store=False, **_B), _st(x=True, add_prev=True)],
        # PaiNN, backward: sum_c dx_c W_c * silu'(u), then the Dense before it (two column slices; or + residual)
        "wide3-dsilu-fan2": _WIDE3 + [_st(), _st(same_input=True)],
        "wide3-dsilu-res": _WIDE3 + [_st(res=True)],
        "wide2-back": [_st(store=False), _st(x=True, add_prev=True)],
        "wide2-back-res": [_st(store=False), _st(x=True, add_prev=True, res=True)],
        # not launched by a model today
        "four": [_st(ssp=True, **_B), _st(res=True, **_B), _st(tprev="dssp"), _st(ssp=True, **_B)],
        "new-input": [_st(**_B), _st(x=True, **_B)],
    },
}
for _F in (64, 32):  # the streaming form: bias, ssp, * ssp'(tprev), + res; up to three stages
    FORMS[_F] = {k: FORMS[128][k] for k in ("lin", "lin-bias", "ssp", "ssp-res", "ssp-res-lin", "ssp-res-ssp",
                                            "ssp-unstored-tprev", "tprev-lin", "res", "bias-res", "res-tprev-lin")}
LONGEST = ("wide-silu-fan", "wide3-dsilu-fan2")      # the two five-stage forms
SCHNET3 = "ssp-res-lin"
KINDS = ("main", "blocks", "rows", "zeros", "slices")
BLOCK_SCALES = (0, 7, -9, 3)


def stage_flags(sp):
    return (EPI_SSP if sp["ssp"] else 0) | (EPI_SILU if sp["silu"] else 0) | (EPI_MUL_DSILU if sp["tprev"] == "dsilu" else 0)


def form_signature(F, form):
    """What the completeness check compares: per stage (flags, bias, res, tprev, out, out_act, x, same_input,
    add_prev)."""
    return (F, tuple((stage_flags(sp), sp["bias"], sp["res"], sp["tprev"] is not None, sp["store"], sp["out_act"],
                      sp["x"], sp["same_input"], sp["add_prev"]) for sp in form))


def operands(F, name, R, transB, kind, device="cpu", seed=0):
    """(X, stages) of form `name` on `kind` operands (`slices` has the data of `main`: the test places it), stages as
    `chain` takes them, with `store` and `out_act` (bool) carried along.  Drawn on `device` from its own generator."""
    form = FORMS[F][name]
    g = torch.Generator(device=device).manual_seed(1000 * F + 10 * len(name) + seed + (1 if transB else 0) + 7 * R)
    rn = lambda *shape: torch.randn(*shape, generator=g, device=device)
    nb = F // 32
    rows = torch.arange(R, device=device)
    row_scale = torch.exp2(((rows * 7) % 25 - 12).double()).float()[:, None]
    group = torch.where(torch.arange(F, device=device)[None, :] // 32 == (rows % nb)[:, None], 1024.0, 1.0)

    def input_rows():
        x = rn(R, F)
        if kind == "rows":
            x = x * row_scale * group
        if kind == "zeros":
            x[rows % 5 == 0] = 0.0
        return x

    X = input_rows()
    stages = []
    for s, sp in enumerate(form):
        W = rn(F, F) / F ** 0.5
        bias = rn(F) * 0.1 if sp["bias"] else None
        if kind == "blocks":
            perm = [BLOCK_SCALES[(b + s) % 4] for b in range(nb)]
            sc = torch.exp2(torch.tensor(perm, dtype=torch.float32, device=device)).repeat_interleave(32)
            W = W * (sc[:, None] if transB else sc[None, :])
            bias = None if bias is None else bias * sc
        if kind == "zeros" and s == 0:
            blk = slice(32 * (1 % nb), 32 * (1 % nb) + 32)   # one all-zero weight block
            if transB:
                W[blk, :] = 0.0
            else:
                W[:, blk] = 0.0
            if bias is not None:   # zero rows then give exact zeros (ssp(0) = 0): the next stage's row scale is the floor
                bias = torch.zeros(F, device=device)
        st = dict(W=W.contiguous(), transB=transB, bias=bias, flags=stage_flags(sp), same_input=sp["same_input"],
                  add_prev=sp["add_prev"], store=sp["store"], out_act=sp["out_act"])
        st["res"] = rn(R, F) * (row_scale if kind == "rows" else 1.0) if sp["res"] else None
        st["tprev"] = rn(R, F) if sp["tprev"] else None
        st["x"] = input_rows() if sp["x"] else None
        stages.append(st)
    return X, stages
