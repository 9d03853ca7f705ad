"""GPU tests of PaiNN's four mixing kernels (csrc/painn.hip: k_painn_mix_pre_fwd, _post_fwd, _post_bwd, _pre_bwd) through
both entry points (exact and _dyn): every output element against the fp64 twin with the rounding counts of
tests/painn_mix_twin.py as the bound (u = 2^-24), outputs pre-filled with NaN.
  shapes:  F = 128 and 48; N = 8203 (N * 128 is just above 4096 blocks of 256 threads: the grid-stride loop runs a second,
           partial round) and N = 1
  forms:   mu_out == NULL, dmu_new == NULL; dyn_N = 5000 in a capacity of 8203 (rows from 5000 on keep their bits in every
           output, dmm's prior contents under pre_bwd included)
  edges:   rows with mu_V = 0 exactly (ctx = sqrt(eps), a finite gradient); pre_bwd adds onto what post_bwd wrote
  proof:   the ddot * v term removed from the reference of one dmm_W element - flagged, and only it."""
import numpy as np
import pytest
import torch

import painn_mix_twin as mx
from elementwise import assert_sees_a_dropped_term, assert_within, pick_term

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
EPS = 1e-8
N_BIG, N_DYN = 8203, 5000
ZERO_ROWS = (0, 3, 4097, 4999, 5000, 8202)


def _ptr(x):
    return None if x is None else x.data_ptr()


_CASES = {}


def _inputs(N, F):
    if (N, F) not in _CASES:
        g = torch.Generator().manual_seed(1000 * F + N)
        rnd = lambda *s: torch.randn(*s, generator=g)
        c = dict(q=rnd(N, F), mu=rnd(N, 3, F), mm=rnd(N, 3, 2 * F), xx=rnd(N, 3 * F), gq=rnd(N, F), gm=rnd(N, 3, F),
                 dctx=rnd(N, 2 * F))
        if N > 1:
            for r in ZERO_ROWS:
                c["mm"][r, :, :F] = 0.0                         # mu_V = 0 exactly
        else:
            c["mm"][0, :, :F // 2] = 0.0                        # (one atom: half of its features)
        _CASES[(N, F)] = {k: v.to(DEV) for k, v in c.items()}
    return _CASES[(N, F)]


def _nan(*s):
    return torch.full(s, NAN, device=DEV)


def _run(c, N, F, dyn=None, null_forms=False, dmm_prior=None):
    """The four kernels in the order of a step: pre_fwd, post_fwd, post_bwd, pre_bwd (on the dmm post_bwd wrote, or on
    `dmm_prior` rows where given) -> dict of fp32 outputs (dmm both after post_bwd and after pre_bwd)."""
    from geossl_amd import _lib
    st = _lib.stream()
    sfx, tail = ("", ()) if dyn is None else ("_dyn", (_ptr(dyn),))
    o = dict(ctx=_nan(N, 2 * F), dot=_nan(N, F), q_out=_nan(N, F), mu_out=None if null_forms else _nan(N, 3, F),
             dxx=_nan(N, 3 * F), dmm=_nan(N, 3, 2 * F), dq_in=_nan(N, F))
    _lib.call("geossl_painn_mix_pre_fwd" + sfx, _ptr(c["q"]), _ptr(c["mm"]), N, F, EPS, _ptr(o["ctx"]), _ptr(o["dot"]), *tail, st)
    ctx_in, dot_in = o["ctx"], o["dot"]
    if dyn is not None:   # (the later kernels read only the live rows; finite stand-ins keep the NaN rows out of their inputs)
        ctx_in, dot_in = torch.nan_to_num(o["ctx"], nan=1.0), torch.nan_to_num(o["dot"], nan=1.0)
    o["ctx_in"], o["dot_in"] = ctx_in, dot_in
    _lib.call("geossl_painn_mix_post_fwd" + sfx, _ptr(c["q"]), _ptr(c["mu"]), _ptr(c["mm"]), _ptr(c["xx"]), _ptr(dot_in), N, F,
              _ptr(o["q_out"]), _ptr(o["mu_out"]), *tail, st)
    _lib.call("geossl_painn_mix_post_bwd" + sfx, _ptr(c["gq"]), None if null_forms else _ptr(c["gm"]), _ptr(c["mm"]),
              _ptr(c["xx"]), _ptr(dot_in), N, F, _ptr(o["dxx"]), _ptr(o["dmm"]), *tail, st)
    o["dmm_post"] = o["dmm"].clone()
    if dmm_prior is not None:
        o["dmm"][dmm_prior[0]:] = dmm_prior[1]
    _lib.call("geossl_painn_mix_pre_bwd" + sfx, _ptr(c["gq"]), _ptr(c["dctx"]), _ptr(ctx_in), _ptr(c["mm"]), N, F,
              _ptr(o["dq_in"]), _ptr(o["dmm"]), *tail, st)
    torch.cuda.synchronize()
    return o


def _twin(c, o, F, null_forms):
    """The fp64 references of every output, each kernel on the fp32 inputs it was handed (ctx, dot: the kernels' own)."""
    cpu = {k: v.cpu() for k, v in c.items()}
    pre = mx.pre_fwd(cpu["q"], cpu["mm"], float(np.float32(EPS)))
    fw = mx.post_fwd(cpu["q"], cpu["mu"], cpu["mm"], cpu["xx"], o["dot_in"].cpu(), with_mu_out=not null_forms)
    pb = mx.post_bwd(cpu["gq"], None if null_forms else cpu["gm"], cpu["mm"], cpu["xx"], o["dot_in"].cpu())
    rb = mx.pre_bwd(cpu["gq"], cpu["dctx"], o["ctx_in"].cpu(), cpu["mm"], pb["dmm_V_post"])
    return pre, fw, pb, rb


def _pairs(o, F, pre, fw, pb, rb, null_forms):
    """(name of the constant, got, (ref, S)) for every output element of the four kernels."""
    out = [("ctx_q", o["ctx"][:, :F], pre["ctx_q"]), ("ctx_n", o["ctx"][:, F:], pre["ctx_n"]), ("dot", o["dot"], pre["dot"]),
           ("q_out", o["q_out"], fw["q_out"]),
           ("dxx_0", o["dxx"][:, :F], pb["dxx_0"]), ("dxx_1", o["dxx"][:, F:2 * F], pb["dxx_1"]),
           ("dxx_2", o["dxx"][:, 2 * F:], pb["dxx_2"]),
           ("dmm_V_post", o["dmm_post"][:, :, :F], pb["dmm_V_post"]), ("dmm_W", o["dmm_post"][:, :, F:], pb["dmm_W"]),
           ("dq_in", o["dq_in"], rb["dq_in"]), ("dmm_V", o["dmm"][:, :, :F], rb["dmm_V"]),
           ("dmm_W", o["dmm"][:, :, F:], pb["dmm_W"])]
    if not null_forms:
        out.append(("mu_out", o["mu_out"], fw["mu_out"]))
    return out


@pytest.mark.parametrize("null_forms", [False, True], ids=["general", "null"])
@pytest.mark.parametrize("N", [N_BIG, 1])
@pytest.mark.parametrize("F", [128, 48])
def test_mixing_kernels_every_element_against_the_twin(F, N, null_forms):
    c = _inputs(N, F)
    if N == N_BIG and F == 128:
        assert 4096 * 256 < N * F < 4096 * 256 + 4096 * 256 // 8   # a second, partial round of the grid-stride loop
    o = _run(c, N, F, null_forms=null_forms)
    pre, fw, pb, rb = _twin(c, o, F, null_forms)
    for name, got, (ref, S) in _pairs(o, F, pre, fw, pb, rb, null_forms):
        got = got.cpu()
        live = S > 0
        w = float(((got.double() - ref).abs()[live] / (mx.U * S[live])).max()) if bool(live.any()) else 0.0
        print("mix F=%d N=%d %s %s: worst error %.2f u S (bound %g)" % (F, N, "null" if null_forms else "general", name, w,
                                                                       mx.C[name]))
        assert_within(got, ref, S, mx.C[name], mx.U, name)
    # pre_bwd leaves the W columns of dmm as post_bwd wrote them
    assert torch.equal(o["dmm"][:, :, F:], o["dmm_post"][:, :, F:])
    # mu_V = 0 exactly: ctx = sqrt(eps) to the bit, and the gradient through the norm is an exact, finite zero
    zero = torch.tensor(ZERO_ROWS, device=DEV) if N > 1 else torch.tensor([0], device=DEV)
    fs = slice(0, F) if N > 1 else slice(0, F // 2)
    root = float(np.sqrt(np.float32(EPS)))
    assert bool((o["ctx"][zero][:, F:][:, fs] == root).all())
    assert bool(torch.isfinite(o["dmm"]).all()) and bool(torch.isfinite(o["dq_in"]).all())
    assert torch.equal(o["dmm"][zero][:, :, fs], o["dmm_post"][zero][:, :, fs])
    # the ddot * v term removed from the reference of one dmm_W element: flagged, and only that element
    got, (ref, S) = o["dmm_post"][:, :, F:].cpu(), pb["dmm_W"]
    cc = mx.C["dmm_W"]
    bound = cc * mx.U * S + (got.double() - ref).abs()
    k, ratio = pick_term(pb["term_W_dot"], bound, torch.ones_like(ref, dtype=torch.bool))
    assert ratio >= 2.0, ratio
    idx = tuple(int(v) for v in np.unravel_index(k, tuple(ref.shape)))
    assert_sees_a_dropped_term(got, ref, S, cc, mx.U, idx, float(pb["term_W_dot"][idx]), "dmm_W without ddot * v")
    # and the |mu_V| term of pre_bwd from one dmm_V element
    got, (ref, S) = o["dmm"][:, :, :F].cpu(), rb["dmm_V"]
    cc = mx.C["dmm_V"]
    bound = cc * mx.U * S + (got.double() - ref).abs()
    k, ratio = pick_term(rb["term_V_norm"], bound, torch.ones_like(ref, dtype=torch.bool))
    assert ratio >= 2.0, ratio
    idx = tuple(int(v) for v in np.unravel_index(k, tuple(ref.shape)))
    assert_sees_a_dropped_term(got, ref, S, cc, mx.U, idx, float(rb["term_V_norm"][idx]), "dmm_V without the norm term")


@pytest.mark.parametrize("null_forms", [False, True], ids=["general", "null"])
@pytest.mark.parametrize("F", [128, 48])
def test_dyn_row_count_leaves_the_rows_behind_it_alone(F, null_forms):
    """dyn_N = 5000 in a capacity of 8203: the live rows carry the bits of the exact entry points, the rows from 5000 on
    keep their NaN fill in every output - and, under pre_bwd, dmm's prior contents."""
    N = N_BIG
    c = _inputs(N, F)
    exact = _run(c, N, F, null_forms=null_forms)
    dyn = torch.tensor([N_DYN], dtype=torch.int32, device=DEV)
    prior = 3.5
    o = _run(c, N, F, dyn=dyn, null_forms=null_forms, dmm_prior=(N_DYN, prior))
    fill = torch.full((1,), NAN, device=DEV).view(torch.int32)
    names = ["ctx", "dot", "q_out", "dxx", "dmm_post", "dq_in"] + ([] if null_forms else ["mu_out"])
    for name in names:
        assert torch.equal(o[name][:N_DYN], exact[name][:N_DYN]), name
        assert bool((o[name][N_DYN:].view(torch.int32) == fill).all()), name
    assert torch.equal(o["dmm"][:N_DYN], exact["dmm"][:N_DYN])
    assert bool((o["dmm"][N_DYN:] == prior).all())
    # a count above the capacity is the capacity
    over = torch.tensor([N + 77], dtype=torch.int32, device=DEV)
    o2 = _run(c, N, F, dyn=over, null_forms=null_forms)
    for name in names + ["dmm"]:
        assert torch.equal(o2[name], exact[name]), name
