"""The fp64 twin of the single-layer row GEMM (tests/linear_twin.py) against a plain torch.float64 evaluation, the
validity of the inputs of tests/test_gpu_linear_elementwise.py (the arithmetic model alone stays inside the bound, the
checker sees one removed term in exactly one element), the constants c of the bound |got - ref| <= c u S, and the
launch regimes the GPU test's row counts and widths are named for (linear_twin.plan, a mirror of gemm.hip)."""
import math

import pytest
import torch
import torch.nn.functional as nnf

import linear_twin as tw
from elementwise import assert_sees_a_dropped_term, assert_within

CPU_ROWS = 37                    # the arithmetic model has no path that depends on the row count
GRID_K = (8, 24, 32, 56, 64, 128, 200, 256)
GRID_NO = (4, 36, 64, 100, 128, 160, 256)


def test_flag_values_are_the_library_ones():
    from geossl_amd import _lib
    assert (tw.EPI_BIAS, tw.EPI_SSP, tw.EPI_RESIDUAL, tw.EPI_MUL_DSSP) == (_lib.EPI_BIAS, _lib.EPI_SSP, _lib.EPI_RESIDUAL,
                                                                          _lib.EPI_MUL_DSSP)


def test_flag_sets_cover_every_epilogue_combination():
    nt = [fs for fs in tw.FLAGSETS if fs[0] and not fs[3]]
    nn = [fs for fs in tw.FLAGSETS if not fs[0]]
    assert len(set(nt)) == 8 and len(set(nn)) == 8 and len(tw.FLAGSETS) == 17
    assert {(b, s, r) for _, b, s, _, r in nt} == {(b, s, r) for b in (False, True) for s in (False, True) for r in (False, True)}
    assert {(b, t, r) for _, b, _, t, r in nn} == {(b, t, r) for b in (False, True) for t in (False, True) for r in (False, True)}
    assert all(not s for _, _, s, _, _ in nn) and (True, True, True, True, True) in tw.FLAGSETS


@pytest.mark.parametrize("fs", tw.FLAGSETS, ids=tw.flagset_name)
@pytest.mark.parametrize("K,NO", [(24, 36), (64, 100), (128, 160)])
def test_twin_equals_a_plain_fp64_evaluation(K, NO, fs):
    o = tw.operands("main", 37, K, NO, fs)
    d = tw.reference(**o)
    W = o["W"].double()
    z = nnf.linear(o["X"].double(), W if o["transB"] else W.t(), None if o["bias"] is None else o["bias"].double())
    if o["flags"] & tw.EPI_SSP:
        z = nnf.softplus(z) - math.log(2.0)
    if o["tprev"] is not None:      # ssp'(v) from the saved t = ssp(v): sigmoid(v), v = ssp^-1(t)
        assert float(o["tprev"].min()) > -math.log(2.0)
        z = z * torch.sigmoid(torch.log(torch.expm1(o["tprev"].double() + math.log(2.0))))
    if o["res"] is not None:
        z = z + o["res"].double()
    assert float((d["ref"] - z).abs().max()) <= 1e-12 * float(z.abs().max())
    assert bool((d["S"] >= d["ref"].abs() * (1 - 1e-12)).all())


def _case(K, NO, kind, fs):
    """Worst err / (u S) of the arithmetic model on one case; the bound and the dropped-term proofs on its output."""
    c, u = tw.c_bound(K), tw.U
    o = tw.operands("main" if kind == "slices" else kind, CPU_ROWS, K, NO, fs)
    d = tw.reference(**o)
    y = torch.from_numpy(tw.emulate(**o))
    what = "K=%d NO=%d %s %s" % (K, NO, kind, tw.flagset_name(fs))
    assert not bool(y.isnan().any()), what
    err = (y.double() - d["ref"]).abs()
    assert bool((err[d["S"] == 0] == 0).all()), what
    worst = float((err / d["S"].clamp_min(1e-300)).max()) / u
    assert_within(y, d["ref"], d["S"], c, u, what)
    if kind in ("main", "blocks"):
        for which, idx, term, r in tw.proofs(d, c, u):
            assert r > 2.0, (what, which, r)
            assert_sees_a_dropped_term(y, d["ref"], d["S"], c, u, idx, term, "%s %s" % (what, which))
    return worst


_W = {}


def _grid_worst(K):
    if K not in _W:
        _W[K] = max((_case(K, NO, kind, fs), "NO=%d %s %s" % (NO, kind, tw.flagset_name(fs)))
                    for NO in GRID_NO for kind in tw.KINDS for fs in tw.FLAGSETS)
    return _W[K]


@pytest.mark.parametrize("K", GRID_K)
def test_arithmetic_model_stays_inside_the_bound_and_a_dropped_term_is_seen(K):
    """Every width, operand kind and flag set of the GPU grid at 37 rows: `emulate` within c u S per element, no NaN, and
    on `main` and `blocks` one removed product term, bias or residual flagged in exactly one element with a ratio > 2.
    Prints the worst err / (u S): c is fixed from these figures."""
    print("emulated err/(u S) %-5s K=%-3d %7.3f at %s" % ((tw.family(K), K) + _grid_worst(K)))


def test_bound_constants_are_the_emulated_ones():
    """c is exactly four times the worst emulated ratio over the grid, rounded up to a power of two and not below 8 (the
    factor covers the hardware's exp / log and the MFMA's internal summation): one c for the split kernel, one per K
    class (K <= 64, K <= 256) for the f32-MFMA kernel, whose accumulator is rounded once per product."""
    classes = {"split": [K for K in GRID_K if K in tw.SPLIT_K]}
    for top in sorted(tw.C_BOUND["fp32"]):
        lower = max([t for t in tw.C_BOUND["fp32"] if t < top], default=0)
        classes["fp32 K<=%d" % top] = [K for K in GRID_K if K not in tw.SPLIT_K and lower < K <= top]
    for name, Ks in classes.items():
        assert Ks, name
        (w, where), K = max((_grid_worst(K), K) for K in Ks)
        c = max(8.0, 2.0 ** math.ceil(math.log2(4.0 * w)))
        print("worst emulated err/(u S) %-12s %7.3f at K=%d %s -> c = %g" % (name, w, K, where, c))
        assert all(tw.c_bound(k) == c for k in Ks), (name, w, where, c)


# ----------------------------------------------------------------------------------------------------- launch regimes
def test_plan_of_the_split_kernel_row_counts():
    """The row counts of test_gpu_linear_elementwise.py are the smallest at which each regime of launch_linear_split
    exists."""
    for K in tw.SPLIT_K:
        for R in (1, 31, 32, 33):
            p = tw.plan(R, K, 128)
            assert (p["kernel"], p["nx"], p["nrb"] <= 2, p["n_tasks"], p["rounds"]) == ("split", 1, True, 0, 1), (K, R)
        p = tw.plan(129, K, 128)
        assert (p["nrb"], p["nx"], p["idle_primaries"], p["n_tasks"]) == (5, 2, 3, 0)
        p = tw.plan(32768, K, 128)
        assert (p["nx"], p["n_whole"], p["n_tasks"], p["rounds"], p["idle_primaries"]) == (256, 1024, 0, 1, 0)
        assert tw.plan(32736, K, 128)["idle_primaries"] == 1
        p = tw.plan(32769, K, 128)
        assert (p["n_whole"], p["n_tasks"], p["task_rounds"], p["last_rows"], p["rounds"]) == (1024, p["nmb"], 1, 1, 1)
        p = tw.plan(32833, K, 128)
        assert (p["n_whole"], p["n_tasks"], p["last_rows"]) == (1024, 3 * p["nmb"], 1)
        assert p["nrb"] - p["n_whole"] == 3 and 0 < p["last_rows"] < 32
        assert tw.plan(65504, K, 128)["rounds"] == 1 and tw.plan(65505, K, 128)["n_whole"] == 2048
        p = tw.plan(65536, K, 128)
        assert (p["n_whole"], p["n_tasks"], p["rounds"]) == (2048, 0, 2)
        p = tw.plan(65569, K, 128)
        assert (p["n_whole"], p["nrb"] - p["n_whole"], p["rounds"], p["last_rows"]) == (2048, 2, 2, 1)
    p = tw.plan(42368, 64, 256)
    assert (p["nmb"], p["ny"], p["nrb"] - p["n_whole"], p["n_tasks"], p["task_rounds"]) == (8, 1, 300, 2400, 3)


def test_plan_of_the_split_kernel_widths():
    for K in (32, 64):
        for NO in (4, 36, 64, 100, 128, 160, 192, 256):
            p = tw.plan(33, K, NO)
            assert (p["ny"], p["nmb"], p["ragged"]) == (1, (NO + 31) // 32, False)
            assert not tw.plan(33, K, NO, prepared=True)["refused"]
    want = {4: (1, 1, False), 36: (1, 2, False), 64: (1, 2, False), 100: (1, 4, False), 128: (1, 4, False),
            160: (2, 3, True), 192: (2, 3, False), 256: (2, 4, False)}
    for NO, w in want.items():
        p = tw.plan(33, 128, NO)
        assert (p["ny"], p["nmb"], p["ragged"]) == w, NO
        assert p["lds"] <= 160 * 1024
        assert tw.plan(33, 128, NO, prepared=True)["refused"] == (NO == 160), NO


def test_plan_of_the_f32_kernel():
    for K in (8, 24, 56, 200, 256):
        for R, last in ((1, 1), (33, 33), (97, 97), (128, 128), (129, 1)):
            p = tw.plan(R, K, 128)
            assert (p["kernel"], p["ntiles"], p["last_tile_rows"], p["tiles_per_block"]) == ("fp32", 1 + (R > 128), last, 1)
        want = {4: (1, 1), 36: (2, 1), 64: (2, 1), 100: (2, 2), 128: (2, 2), 160: (1, 5), 192: (2, 3), 256: (2, 4)}
        for NO, w in want.items():
            p = tw.plan(97, K, NO)
            assert (p["NC"], p["ny"]) == w, (K, NO)
            assert p["lds"] <= 160 * 1024 and p["big_lds"] == (p["lds"] > 64 * 1024)
    assert tw.plan(97, 256, 128)["big_lds"] and not tw.plan(97, 200, 128)["big_lds"]
    assert {tw.plan(97, K, NO)["ny"] for K in (8,) for NO in want} >= {1, 2, 3, 4, 5}
    for K in (8, 56):
        for NO, ny in ((128, 1), (256, 2)):
            lo, hi = tw.plan(65408, K, NO), tw.plan(65409, K, NO)
            assert (lo["NC"], lo["ntiles"], lo["ny"]) == (2, 511, 2 * ny) and (hi["NC"], hi["ntiles"], hi["ny"]) == (4, 512, ny)
            assert hi["last_tile_rows"] == 1
        lo, hi = tw.plan(131072, K, 128), tw.plan(131073, K, 128)
        assert (lo["nx"], lo["tiles_per_block"], hi["nx"], hi["tiles_per_block"], hi["last_tile_rows"]) == (1024, 1, 1024, 2, 1)
        assert hi["NC"] == 4
    assert tw.plan(65409, 56, 128)["lds"] <= 64 * 1024


def test_plan_refusals():
    assert tw.plan(33, 128, 160, prepared=True)["refused"]
    for K, NO in ((12, 64), (264, 64), (64, 258), (56, 258), (64, 260)):
        assert tw.plan(33, K, NO)["refused"], (K, NO)
    assert tw.plan(33, 56, 64, prepared=True)["refused"]
    assert tw.plan(33, 64, 64, ldx=60)["refused"] and tw.plan(33, 64, 64, ldy=66)["refused"]
    assert tw.plan(2 ** 31, 64, 64)["refused"] and tw.plan(2 ** 31, 56, 64)["refused"]
    assert tw.plan(2 ** 31, 64, 64, prepared=True)["refused"]
    assert not tw.plan(2 ** 31 - 1, 64, 64)["refused"]
