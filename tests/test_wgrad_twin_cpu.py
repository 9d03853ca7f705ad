"""The fp64 twin of the weight-gradient column GEMM (tests/wgrad_twin.py) against a plain torch.float64 evaluation, the
constants c of the bound |got - ref| <= c u S fixed from the twin's arithmetic model, the row counts of
tests/test_gpu_wgrad_elementwise.py against geossl_tn_plan, and the argument refusals of geossl_linear_wgrad[_dyn]
(they return before any HIP call: null pointers, no GPU)."""
import ctypes as C
import math

import pytest
import torch

import wgrad_twin as tw
from elementwise import assert_sees_a_dropped_term, assert_within

WIDTHS = (32, 64, 128, 36, 100)
# (R, chunk): one row; two tiles, the second partial; two chunks of 64; three chunks of 128 (reduction slice 3 empty),
# the last partial; 449 rows in eight chunks of 64 (two per slice); 700 and 1100 rows in chunks of 256 (eight tiles,
# three and five chunks)
CPU_ROWS = ((1, 64), (33, 64), (97, 64), (300, 128), (449, 64), (700, 256), (1100, 256))
KINDS_3 = ("main", "blocks", "rising", "zeros")       # the kinds the three-piece form runs on
NPROB = {"blocks": 3, "zeros": 3}
GRID = [(M, N) for M in WIDTHS for N in WIDTHS]


def _ratio(got, ref, S):
    err = (torch.from_numpy(got).double() - ref).abs()
    assert bool((err[S == 0] == 0).all())
    return float((err / S.clamp_min(1e-300)).max())


def _case(kind, M, N, R, chunk, pieces, accumulate=False):
    """Worst err / (u S) of the arithmetic model on one case (dW, db); the bound and the dropped-term proofs on it."""
    fam = tw.family(pieces)
    nprob = NPROB.get(kind, 1)
    probs = tw.operands("main" if kind == "slices" else kind, nprob, R, M, N, chunk)
    prior = tw.priors(probs, M, N, [True] * len(probs)) if accumulate else None
    ref = tw.wgrad(probs, R, M, N, chunk, prior=prior, pieces=pieces)
    emu = tw.emulate(probs, R, M, N, chunk, prior=prior, pieces=pieces)
    what = "%s M=%d N=%d R=%d chunk=%d pieces=%d acc=%s" % (kind, M, N, R, chunk, pieces, accumulate)
    w = wb = 0.0
    for z, (d, (dW, db)) in enumerate(zip(ref, emu)):
        w = max(w, _ratio(dW, d["ref_dW"], d["S_dW"]) / tw.U[fam])
        wb = max(wb, _ratio(db, d["ref_db"], d["S_db"]) / tw.U["db"])
        assert_within(torch.from_numpy(dW), d["ref_dW"], d["S_dW"], tw.C_BOUND[fam], tw.U[fam], what)
        assert_within(torch.from_numpy(db), d["ref_db"], d["S_db"], tw.C_BOUND["db"], tw.U["db"], what + " db")
        if kind in ("main", "blocks", "spike") and not accumulate:
            for name, r in tw.proof_rows(R, chunk).items():
                idx, term, ratio = tw.pick_dropped_term(d, r, tw.C_BOUND[fam], tw.U[fam])
                assert ratio >= 2.0, (what, name, r, ratio)
                assert_sees_a_dropped_term(torch.from_numpy(dW), d["ref_dW"], d["S_dW"], tw.C_BOUND[fam], tw.U[fam], idx,
                                           term, "%s %s row %d" % (what, name, r))
    return w, wb


_W = {}


def _grid_worst(M, N):
    if (M, N) not in _W:
        worst = {"two-piece": (0.0, ""), "bf16x3": (0.0, ""), "db": (0.0, "")}

        def take(fam, v, where):
            if v > worst[fam][0]:
                worst[fam] = (v, where)
        for R, chunk in CPU_ROWS:
            for pieces in (2, 3):
                for kind in (tw.KINDS if pieces == 2 else KINDS_3):
                    where = "%s M=%d N=%d R=%d chunk=%d" % (kind, M, N, R, chunk)
                    w, wb = _case(kind, M, N, R, chunk, pieces)
                    take(tw.family(pieces), w, where)
                    take("db", wb, where)
            w, wb = _case("main", M, N, R, chunk, 2, accumulate=True)
            take("two-piece", w, "accumulate M=%d N=%d R=%d chunk=%d" % (M, N, R, chunk))
            take("db", wb, "accumulate M=%d N=%d R=%d chunk=%d" % (M, N, R, chunk))
        _W[(M, N)] = worst
    return _W[(M, N)]


@pytest.mark.parametrize("M,N", GRID)
def test_arithmetic_model_stays_inside_the_bound_and_a_dropped_term_is_seen(M, N):
    """Every operand kind at the CPU row counts: `emulate` within c u S per element of dW and db, and on `main`,
    `blocks` and `spike` one removed product a[r][m] b[r][n] per proof row flagged in exactly one element with a ratio
    >= 2.  Prints the worst err / (u S): c is fixed from these figures."""
    for fam, (v, where) in sorted(_grid_worst(M, N).items()):
        print("emulated err/(u S) %-9s M=%-3d N=%-3d %7.3f at %s" % (fam, M, N, v, where))


def test_bound_constants_are_the_emulated_ones():
    """C_BOUND is exactly four times the worst emulated ratio of its family over the grid, rounded up to a power of two
    (the factor covers the MFMA's summation order inside one instruction and the hardware's handling of the smallest
    pieces).  The worst values of the grid are recorded here: two-piece 2.04 (one row, `blocks`), bf16x3 3.66 (33 rows, `blocks`), db 2.56 (700 rows, `falling`)."""
    recorded = {"two-piece": 2.04, "bf16x3": 3.66, "db": 2.56}
    found = {fam: max(_grid_worst(M, N)[fam] for M, N in GRID) for fam in recorded}
    for fam, (w, where) in sorted(found.items()):
        print("worst emulated err/(u S) %-9s %7.3f at %s -> c = %g" % (fam, w, where, 2.0 ** math.ceil(math.log2(4.0 * w))))
    for fam, (w, where) in sorted(found.items()):
        assert tw.C_BOUND[fam] == 2.0 ** math.ceil(math.log2(4.0 * w)), (fam, w, where)
        assert abs(w - recorded[fam]) < 0.006, (fam, w)


@pytest.mark.parametrize("M,N", [(128, 128), (36, 100), (64, 32)])
def test_twin_equals_a_plain_fp64_evaluation(M, N):
    R, chunk = 300, 128
    for kind in tw.KINDS:
        probs = tw.operands("main" if kind == "slices" else kind, 3, R, M, N, chunk)
        for pieces in (2, 3):
            for prior in (None, tw.priors(probs, M, N, [True, False, True])):
                for z, d in enumerate(tw.wgrad(probs, R, M, N, chunk, prior=prior, pieces=pieces)):
                    A, B = probs[z][0].double(), probs[z][1].double()
                    dW, db = torch.matmul(A.t(), B), A.sum(0)
                    if prior is not None:
                        dW = dW + prior[z][0].double()
                        db = db + (0 if prior[z][1] is None else prior[z][1].double())
                    assert float((d["ref_dW"] - dW).abs().max()) <= 1e-12 * float(dW.abs().max().clamp_min(1e-300))
                    assert float((d["ref_db"] - db).abs().max()) <= 1e-12 * float(db.abs().max().clamp_min(1e-300))
                    assert bool((d["S_dW"] >= d["ref_dW"].abs() * (1 - 1e-12)).all()), (kind, z)
                    assert bool((d["S_db"] >= d["ref_db"].abs() * (1 - 1e-12)).all()), (kind, z)


def test_extra_rows_and_columns_of_the_operands_are_not_part_of_the_product():
    A, B = torch.randn(40, 48), torch.randn(40, 72)
    d = tw.wgrad([(A, B)], 33, 36, 68, 64)[0]
    assert torch.equal(d["ref_dW"], A[:33, :36].double().t() @ B[:33, :68].double())
    assert d["S_dW"].shape == (36, 68) and d["S_db"].shape == (36,)


def test_floor_factor_is_the_one_of_the_fp16_split():
    """f from split.h: under a block maximum scaled into [2^13, 2^14) an element far below it is cut to fp16's subnormal
    grid, spacing 2^-24: its error is at most 2^-25 of the scaled value, 2^-38 = u f of the maximum, and that is
    attained (to a factor of two: the maximum may sit anywhere in its binade)."""
    import numpy as np
    from chain_twin import _split_fp16, mag_exponent
    assert tw.FLOOR_F * tw.U["two-piece"] == 2.0 ** -25 / 2.0 ** 13
    worst = 0.0
    for mx in (1.0, 1.999, 3.0e4, 7.7e-9):
        e = int(mag_exponent(np.float32(mx)))
        x = (np.float32(mx) * np.exp2(-np.linspace(12.0, 40.0, 4001))).astype(np.float32)
        h, l = _split_fp16(x.astype(np.float64) * 2.0 ** (14 - e))
        err = np.abs((h.astype(np.float64) + l.astype(np.float64)) * 2.0 ** (e - 14) - x.astype(np.float64))
        bound = tw.U["two-piece"] * (np.abs(x.astype(np.float64)) + tw.FLOOR_F * mx)
        assert (err <= bound).all(), mx
        rest = (err - tw.U["two-piece"] * np.abs(x.astype(np.float64))).clip(0.0)      # what the floor term has to cover
        worst = max(worst, float((rest / (tw.U["two-piece"] * tw.FLOOR_F * mx)).max()))
    assert 0.45 <= worst <= 1.0, worst


def test_running_maxima_are_tighter_than_chunk_maxima_on_a_spike():
    """One element of 2^20 in the LAST row of a 256-row chunk: the seven tiles before it were cut under their own block
    maxima, so the bound of the elements of the spike's blocks (other than its own row and column of dW) must not carry
    its floor for all 256 rows.  A twin coarsened to chunk-wide maxima is looser by a factor of about 8 there (256 rows
    against 32 at the raised floor); this test fails it."""
    R = chunk = 256
    M = N = 128
    probs = tw.operands("spike", 1, R, M, N, chunk)
    assert float(probs[0][0][R - 1, 5]) == tw.SPIKE and float(probs[0][1][R - 1, N - 3]) == -tw.SPIKE
    fine = tw.wgrad(probs, R, M, N, chunk)[0]["S_dW"]
    coarse = tw.wgrad(probs, R, M, N, chunk, running=False)[0]["S_dW"]
    assert bool((coarse >= fine * (1 - 1e-12)).all())
    rows = [m for m in range(32) if m != 5]
    cols = [n for n in range(96, 128) if n != N - 3]
    ratio = (coarse / fine)[rows][:, cols]
    print("chunk-max S / running-max S over the spike's blocks: min %.2f median %.2f" % (float(ratio.min()),
                                                                                         float(ratio.median())))
    assert float(ratio.min()) >= 4.0


# ------------------------------------------------------------------------------------------ the GPU test's row counts
def test_row_counts_of_the_gpu_test_hit_their_plan_conditions():
    import test_gpu_wgrad_elementwise as g
    for R in (1, 31, 32, 33, 63, 64):
        assert tw.plan(R, 1) == (64, 1), R
    assert g.ROWS_ONE[:6] == (1, 31, 32, 33, 63, 64)
    for R, rows_last in ((65, 1), (97, 33)):                 # two chunks: reduction slices 2 and 3 empty, six dead slots
        assert tw.plan(R, 1) == (64, 2) and R - 64 == rows_last and R in g.ROWS_ONE
    assert tw.plan(448, 1) == (64, 7) and tw.plan(449, 1) == (64, 8) and tw.plan(512, 1) == (64, 8)
    assert tw.plan(513, 1) == (64, 9) and 449 in g.ROWS_ONE and 513 in g.ROWS_ONE
    # chunk = 128 from 32 641 rows of one problem on (the first refill, four tiles per chunk); its last chunk has one row
    assert tw.plan(32640, 1) == (64, 510) and tw.plan(32641, 1) == (128, 256) and 32641 - 255 * 128 == 1
    # chunk = 256 from 65 281 rows on (eight tiles, the refill repeats); 65 313: the last chunk has 33 rows
    assert tw.plan(65280, 1) == (128, 510) and tw.plan(65281, 1) == (256, 256) and tw.plan(65313, 1) == (256, 256)
    assert 65313 - 255 * 256 == 33
    assert g.ROWS_LONG == (32641, 65313)
    # several problems: chunk = 256 with nblk = 0, 1 and 7 mod 8
    assert sorted(g.ROWS_MULTI) == [3, 18, 32] and tw.TN_MAX == 32
    for nprob, rows in g.ROWS_MULTI.items():
        plans = [tw.plan(R, nprob) for R in rows]
        assert [c for c, _ in plans] == [256] * 3, (nprob, plans)
        assert [n % 8 for _, n in plans] == [0, 1, 7], (nprob, plans)
        assert rows[2] % 32 != 0                               # (and a partial last tile)
    assert g.ROWS_FORMS == (33, 513)
    for nprob in range(2, tw.TN_MAX + 1):                      # the catalogue's third row count, per problem count
        R = g.rows_256(nprob)
        assert tw.plan(R, nprob)[0] == 256 and tw.plan(R - 256, nprob)[0] < 256 and R % 32 == 1, nprob
    assert g.PROOF_ROWS_MAX <= 40000


def test_the_catalogue_builds_the_db_pattern_it_names():
    for name, f in tw.FORMS.items():
        assert 1 <= f["nprob"] <= tw.TN_MAX and (f["db"] != "mixed" or f["nprob"] >= 2), name
        assert tw.db_class([True if g else None for g in tw.db_given(f["db"], f["nprob"])]) == f["db"], name


# --------------------------------------------------------------------------------------------------- argument refusals
INVALID = 1      # hipErrorInvalidValue


def _call(dyn, nprob=1, R=64, M=128, N=128, lda=None, ldb=None, ldw=None):
    from geossl_amd import _lib
    lib = _lib.load()
    tb = _lib.TnBatch()
    lda, ldb, ldw = lda or M, ldb or N, ldw or N
    if dyn:
        return lib.geossl_linear_wgrad_dyn(C.byref(tb), nprob, R, M, N, lda, ldb, ldw, None, 0, None, None)
    return lib.geossl_linear_wgrad(C.byref(tb), nprob, R, M, N, lda, ldb, ldw, None, 0, None)


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("what,kw", [
    ("lda < M", dict(lda=124)), ("ldb < N", dict(ldb=124)), ("ldw < N", dict(ldw=124)),
    ("lda & 3", dict(lda=130)), ("ldb & 3", dict(ldb=130)),
    ("M & 3", dict(M=126, lda=128)), ("N & 3", dict(N=126, ldb=128, ldw=128)),
    ("ceil(M/32) = 3", dict(M=68)), ("ceil(M/32) = 3", dict(M=96)),
    ("ceil(N/32) = 3", dict(N=68)), ("ceil(N/32) = 3", dict(N=96)),
    ("M > 128", dict(M=132)), ("N > 128", dict(N=160)),
    ("nprob > GEOSSL_TN_MAX", dict(nprob=tw.TN_MAX + 1)),
    ("R > INT_MAX", dict(R=2 ** 31)), ("R > INT_MAX", dict(R=2 ** 32 + 64)), ("R > INT_MAX", dict(R=2 ** 31, nprob=32)),
])
def test_arguments_the_kernel_cannot_serve_are_refused_before_any_launch(what, kw, dyn):
    """Every one of these returns hipErrorInvalidValue before the first HIP call (null operands, no GPU here).  A row
    count above INT_MAX used to be cut to 32 bits on its way into the kernel (2^32 + 64 rows ran as 64)."""
    assert _call(dyn, **kw) == INVALID, what


@pytest.mark.parametrize("dyn", [False, True])
def test_an_empty_launch_is_no_error(dyn):
    assert _call(dyn, R=0) == 0 and _call(dyn, nprob=0) == 0
