"""The fp64 twin of the chained row GEMMs (tests/chain_twin.py) against a plain torch.float64 evaluation, the validity of
the inputs of tests/test_gpu_chain_elementwise.py (the arithmetic model alone stays inside the bound, the checker sees
one removed term in exactly one element) and the constants c of the bound |got - ref| <= c u S."""
import math

import pytest
import torch
import torch.nn.functional as nnf

import chain_twin as tw
from elementwise import assert_sees_a_dropped_term, assert_within, flagged

CPU_ROWS = (1, 33, 293)         # the arithmetic model has no path that depends on the row count: the GPU grid, capped
GRID = [(F, name, transB) for F in (128, 64, 32) for name in tw.FORMS[F] for transB in (True, False)]


def test_flag_values_are_the_library_ones():
    from geossl_amd import _lib
    assert (tw.EPI_SSP, tw.EPI_SILU, tw.EPI_MUL_DSILU) == (_lib.EPI_SSP, _lib.EPI_SILU, _lib.EPI_MUL_DSILU)
    assert max(len(f) for f in tw.FORMS[128].values()) == _lib.CHAIN_MAX


def _plain(X, stages):
    """The chain layer by layer in torch.float64 with torch.nn.functional, written from the stage dicts alone."""
    outs, inp, y = [], X.double(), None
    for s, st in enumerate(stages):
        if st["x"] is not None:
            inp = st["x"].double()
        elif s > 0 and not st["same_input"]:
            inp = nnf.silu(y) if stages[s - 1]["flags"] & tw.EPI_SILU else y
        W = st["W"].double()
        z = nnf.linear(inp, W if st["transB"] else W.t(), None if st["bias"] is None else st["bias"].double())
        if st["add_prev"]:
            z = z + y
        if st["flags"] & tw.EPI_SSP:
            z = nnf.softplus(z) - math.log(2.0)
        if st["tprev"] is not None:
            t = st["tprev"].double().requires_grad_()
            if st["flags"] & tw.EPI_MUL_DSILU:                 # silu'(t) by autograd
                z = z * torch.autograd.grad(nnf.silu(t).sum(), t)[0]
            else:                                              # ssp'(v) from the saved t = ssp(v): sigmoid(v), v = ssp^-1(t)
                v = torch.log(torch.expm1(t.detach() + math.log(2.0)))
                z = z * torch.sigmoid(v)
        if st["res"] is not None:
            z = z + st["res"].double()
        y = z
        outs.append((y, nnf.silu(y) if st["flags"] & tw.EPI_SILU else None))
    return outs


@pytest.mark.parametrize("F,name,transB", GRID)
def test_twin_equals_a_plain_fp64_evaluation(F, name, transB):
    X, stages = tw.operands(F, name, 37, transB, "main")
    for st in stages:        # a saved ssp output is > -log 2: only there is ssp'(v) = 1 - exp(-t) / 2 a sigmoid
        if st["tprev"] is not None and not st["flags"] & tw.EPI_MUL_DSILU:
            st["tprev"] = st["tprev"].abs()
    got, want = tw.chain(X, stages), _plain(X, stages)
    for s, (d, (y, ya)) in enumerate(zip(got, want)):
        scale = float(y.abs().max())
        assert float((d["ref"] - y).abs().max()) <= 1e-12 * scale, s
        assert bool((d["S"] >= d["ref"].abs() * (1 - 1e-12)).all()), s
        assert (ya is None) == (d["ref_act"] is None)
        if ya is not None:
            assert float((d["ref_act"] - ya).abs().max()) <= 1e-12 * scale, s
            assert bool((d["S_act"] >= d["ref_act"].abs() * (1 - 1e-12)).all()), s


def _ratio(got, ref, S, floor=0.0):
    err = ((torch.from_numpy(got).double() - ref).abs() - floor).clamp_min(0.0)
    assert bool((err[S == 0] == 0).all())
    return float((err / S.clamp_min(1e-300)).max())


def _case(F, name, transB, kind, R):
    """Worst err / (u S) of the arithmetic model on one case, the bound and the dropped-term proofs on its outputs."""
    fam, u = tw.FAMILY[F], tw.U[F]
    c = tw.C_BOUND[fam]
    X, stages = tw.operands(F, name, R, transB, kind)
    form = tw.FORMS[F][name]
    ref, emu = tw.chain(X, stages), tw.emulate(X, stages, F)
    worst = 0.0
    for s, (d, (y, ya)) in enumerate(zip(ref, emu)):
        assert not bool(torch.from_numpy(y).isnan().any())
        worst = max(worst, _ratio(y, d["ref"], d["S"]) / u)
        if ya is not None:
            worst = max(worst, _ratio(ya, d["ref_act"], d["S_act"], tw.ACT_FLOOR) / u)
        if form[s]["store"]:
            what = "%d %s %s %s R=%d stage %d" % (F, name, transB, kind, R, s)
            assert_within(torch.from_numpy(y), d["ref"], d["S"], c, u, what)
            if ya is not None:
                assert_within(torch.from_numpy(ya), d["ref_act"], d["S_act"], c, u, what + " act", extra=tw.ACT_FLOOR)
    if kind in ("main", "blocks"):
        for s, which, act, idx, term, r in tw.proofs(ref, form, F, c, u):
            d, y = ref[s], torch.from_numpy(emu[s][1 if act else 0])
            what = "%d %s %s %s R=%d stage %d %s%s" % (F, name, transB, kind, R, s, which, " act" if act else "")
            assert r >= 2.0, (what, r)
            if act:
                assert_sees_a_dropped_term(y, d["ref_act"], d["S_act"], c, u, idx, term, what, extra=tw.ACT_FLOOR)
            else:
                assert_sees_a_dropped_term(y, d["ref"], d["S"], c, u, idx, term, what)
    return worst


_W = {}


def _grid_worst(F, name, transB):
    key = (F, name, transB)
    if key not in _W:
        _W[key] = max(_case(F, name, transB, kind, R) for kind in tw.KINDS for R in CPU_ROWS)
    return _W[key]


@pytest.mark.parametrize("F,name,transB", GRID)
def test_arithmetic_model_stays_inside_the_bound_and_a_dropped_term_is_seen(F, name, transB):
    """Every operand kind of the GPU grid at the capped row counts: `emulate` within c u S per element, no NaN, and on
    `main` and `blocks` one removed product term (add_prev summand, res summand, silu hand-on) flagged in exactly one
    element with a ratio >= 2.  Prints the worst err / (u S): c is fixed from these figures."""
    print("emulated err/(u S) %-9s F=%-3d %-22s transB=%-5s %7.3f" % (tw.FAMILY[F], F, name, transB,
                                                                      _grid_worst(F, name, transB)))


def test_bound_constants_are_the_emulated_ones():
    """C_BOUND is exactly four times the worst emulated ratio of its family over the grid, rounded up to a power of two
    (the factor covers the hardware's exp / log / reciprocal, a few fp32 ulp each, and the MFMA's summation order)."""
    for fam in sorted(set(tw.FAMILY.values())):
        w, where = max((_grid_worst(F, name, transB), "F=%d %s transB=%s" % (F, name, transB))
                       for F, name, transB in GRID if tw.FAMILY[F] == fam)
        c = 2.0 ** math.ceil(math.log2(4.0 * w))
        print("worst emulated err/(u S) %-9s %7.3f at %s -> c = %g" % (fam, w, where, c))
        assert tw.C_BOUND[fam] == c, (fam, w, where)


def test_the_checker_flags_a_wrong_weight_block_exponent():
    """The `blocks` operands do what they are for: results computed with the weight-block exponents rotated by one block
    (what a kernel reading the wrong eW gives) are flagged."""
    F = 128
    X, stages = tw.operands(F, "lin-bias", 33, True, "blocks")
    d = tw.chain(X, stages)[0]
    y = torch.from_numpy(tw.emulate(X, stages, F)[0][0]).double()
    sc = torch.exp2(torch.tensor([float(tw.BLOCK_SCALES[(b + 1) % 4] - tw.BLOCK_SCALES[b]) for b in range(4)]))
    wrong = ((y - stages[0]["bias"].double()) * sc.double().repeat_interleave(32) + stages[0]["bias"].double()).float()
    assert int(flagged(wrong, d["ref"], d["S"], tw.C_BOUND["two-piece"], tw.U[F]).sum()) > 0.9 * y.numel()
    Xm, sm = tw.operands(F, "lin-bias", 33, True, "main")
    dm = tw.chain(Xm, sm)[0]
    same = torch.from_numpy(tw.emulate(Xm, sm, F)[0][0])
    assert int(flagged(same, dm["ref"], dm["S"], tw.C_BOUND["two-piece"], tw.U[F]).sum()) == 0
