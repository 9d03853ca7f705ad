"""geossl_linear / geossl_linear_prepared (csrc/gemm.hip: k_linear<NC>, k_linear_split<KS, E0, E1>, k_linear_prepare<KS>)
through ops.linear / ops.prepare_linear against the fp64 twin (tests/linear_twin.py), element by element, at the row
counts and widths where the launch changes shape (linear_twin.plan mirrors the launch arithmetic; the CPU test pins the
regime of every shape used here).

Split kernel, K = 32 / 64 / 128: 1, 31, 32, 33 rows (one row block); 129 (5 row blocks on 2 blocks, idle primary waves);
32768 (1024 whole row blocks, no tasks); 32769 (one leftover row block of one row: nmb tasks on waves 4-7); 32833 (three
leftover row blocks, the last partial); 42368 at K = 64, NO = 256 (2400 tasks on 1024 secondary waves: they loop);
65536 (a second whole round: the X prefetch behind the MFMAs); 65569 (second round plus leftover).
f32-MFMA kernel, K = 8 / 24 / 56 / 200 / 256: 1, 33, 97 rows (the last wave has one live row); 128, 129 (tile boundary);
65408 / 65409 at NO = 128 and 256 (NC 2 -> 4); 131072 / 131073 (grid cap of 1024 tiles; block 0's second tile holds one
row).
Widths NO = 4, 36, 64, 100, 128, 160, 192, 256 in both weight layouts (K != NO); K = 128 splits the column blocks over
gridDim.y from NO = 160 on, ragged at 160.
Operands: `main` (randn); `blocks` (the 32-output-column blocks of W scaled by 2^{0, 7, -9, 3}); `rows` (row magnitudes
2^-12 .. 2^12, one 32-column group of each row 2^10 above the rest); `zeros` (zero rows, a zero weight block); `slices`
(X, Y, res, tprev column slices of NaN-filled [R + 2 GUARD, ld] tensors, ld > width, ldx != ldy).
Every case: the output lies inside a NaN-filled tensor with GUARD rows above and below that must keep their bits, every
element is held to |got - ref| <= c u S, elementwise.REPEATS launches agree bit for bit, the prepared image (where the
launch takes one) gives torch.equal results, and on `main` and `blocks` one removed product, bias or residual is flagged
in exactly one element.  c comes from the twin's arithmetic model (tests/test_linear_twin_cpu.py); the worst
err / (u S) measured here is printed and recorded in DESIGN.md section 4."""
import pytest
import torch

import linear_twin as tw
from elementwise import assert_repeatable, assert_sees_a_dropped_term, assert_within
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC00000
GUARD = 40
WIDTHS = (4, 36, 64, 100, 128, 160, 192, 256)
K_SPLIT, K_F32 = (32, 64, 128), (8, 24, 56, 200, 256)
ROWS_SMALL = {"split": (1, 31, 32, 33, 129), "fp32": (1, 33, 97, 128, 129)}
ROWS_SPLIT_LARGE = (32768, 32769, 32833, 65536, 65569)
WIDTH_AT_LARGE = {32: 100, 64: 256, 128: 160}        # one width per K at the large row counts


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The worst err / (u S) per kernel over the cases that ran (what DESIGN.md section 4 records)."""
    yield
    for k in sorted(WORST):
        print("worst err/(u S)  %-12s %8.3f  at %s" % ((k,) + WORST[k]))


def note(fam, got, ref, S, u, where):
    """err / (u S) of a tensor, recorded before it is asserted on."""
    err = (got.double() - ref).abs()
    r = torch.where(S > 0, err / (u * S), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = float(r.max()) if r.numel() else 0.0
    if fam not in WORST or not r <= WORST[fam][0]:
        WORST[fam] = (r, where)
    return r


def _family(K):
    return "split" if K in tw.SPLIT_K else ("fp32 K<=64" if K <= 64 else "fp32 K<=256")


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _wide(t, R, width, ld, col):
    """A NaN-filled [R + 2 GUARD, ld] tensor and its [R, width] slice behind GUARD rows at column `col` (holding t)."""
    base = _nan(R + 2 * GUARD, ld)
    view = base[GUARD:GUARD + R, col:col + width]
    if t is not None:
        view.copy_(t)
    return base, view


def _strides(K, NO, sliced):
    if not sliced:
        return K, 0, NO, 0
    ldx, ldy = K + 12, NO + 20
    if ldx == ldy:
        ldx += 8
    return ldx, 8, ldy, 12


class Launch:
    """The device operands of one case and its launches into fresh NaN-filled outputs."""

    def __init__(self, o, sliced):
        self.o, (self.R, self.K), self.NO = o, o["X"].shape, o["W"].size(0 if o["transB"] else 1)
        self.ldx, self.cx, self.ldy, self.cy = _strides(self.K, self.NO, sliced)
        self.inputs = []
        place = lambda t, w, ld, col: None if t is None else self._keep(*_wide(t, self.R, w, ld, col))
        self.X = place(o["X"], self.K, self.ldx, self.cx)
        self.res = place(o["res"], self.NO, self.ldy, self.cy)
        self.tprev = place(o["tprev"], self.NO, self.ldy, self.cy)

    def _keep(self, base, view):
        self.inputs.append((base, base.clone()))
        return view

    def fire(self, w=None, out=None, res="own"):
        from geossl_amd import ops
        o = self.o
        base = None
        if out is None:
            base, out = _wide(None, self.R, self.NO, self.ldy, self.cy)
        ops.linear(self.X, o["W"] if w is None else w, bias=o["bias"], res=self.res if res == "own" else res,
                   tprev=self.tprev, transB=o["transB"], flags=o["flags"], out=out)
        return out, base

    def inputs_unchanged(self):
        return all(torch.equal(b.view(torch.int32), c.view(torch.int32)) for b, c in self.inputs)


def _guards_intact(base, view):
    """Everything around the slice keeps the NaN bits it was filled with."""
    return int((base.view(torch.int32) != NAN_BITS).sum()) == int((view.view(torch.int32) != NAN_BITS).sum())


def _operands(kind, R, K, NO, fs, seed=0):
    o = tw.operands("main" if kind == "slices" else kind, R, K, NO, fs, device=DEV, seed=seed)
    return o, tw.reference(**o)


def _check_case(K, NO, kind, fs, R):
    from geossl_amd import ops
    fam, u, c = _family(K), tw.U, tw.c_bound(K)
    where = "K=%d NO=%d %s %s R=%d" % (K, NO, tw.flagset_name(fs), kind, R)
    p = tw.plan(R, K, NO)
    assert not p["refused"] and p["kernel"] == tw.family(K), where
    o, d = _operands(kind, R, K, NO, fs)
    L = Launch(o, kind == "slices")
    got, base = L.fire()
    print("ratio %-12s %-60s %8.3f" % (fam, where, note(fam, got, d["ref"], d["S"], u, where)))
    assert_within(got, d["ref"], d["S"], c, u, where)
    assert _guards_intact(base, got), where
    if kind in ("main", "blocks"):
        for what, idx, term, r in tw.proofs(d, c, u):
            assert r > 2.0, (where, what, r)
            assert_sees_a_dropped_term(got, d["ref"], d["S"], c, u, idx, term, "%s %s" % (where, what))
    assert_repeatable(lambda: [L.fire()[0]], [got], where)
    if not tw.plan(R, K, NO, prepared=True, ldx=L.ldx, ldy=L.ldy)["refused"]:
        img = ops.prepare_linear([o["W"]], transB=o["transB"])[0]
        gp, bp = L.fire(w=img)
        assert torch.equal(gp, got) and not bool(gp.isnan().any()), where + " prepared"
        assert _guards_intact(bp, gp), where + " prepared"
    assert L.inputs_unchanged(), where


# ----------------------------------------------------------------------------- widths, layouts and kinds, few rows
def _small_cases():
    for K in K_SPLIT + K_F32:
        for tb in (True, False):
            for NO in WIDTHS:
                for kind in ("main", "slices"):
                    yield K, NO, tb, kind
            for NO in (100, 160):
                for kind in ("blocks", "rows", "zeros"):
                    yield K, NO, tb, kind


@pytest.mark.parametrize("K,NO,transB,kind", list(_small_cases()))
def test_widths_layouts_and_kinds_at_few_rows(K, NO, transB, kind):
    for R in ROWS_SMALL[tw.family(K)]:
        _check_case(K, NO, kind, tw.FULL[transB], R)


# ------------------------------------------------------------------------------------------------- every flag set
def _flag_cases():
    for K in (32, 64, 128):
        for fs in tw.FLAGSETS:
            yield K, 160 if K == 128 else 100, fs, (33, 32833)
    for K in (24, 200):
        for fs in tw.FLAGSETS:
            yield K, 100, fs, (97,)
    for fs in tw.FLAGSETS:
        yield 8, 128, fs, (65409,)                      # k_linear<4>


@pytest.mark.parametrize("K,NO,fs,rows", list(_flag_cases()), ids=lambda v: tw.flagset_name(v) if isinstance(v, tuple) and len(v) == 5 else None)
def test_every_flag_set(K, NO, fs, rows):
    """bias x ssp x residual on W [NO][K], bias x tprev x residual on W [K][NO], all four once: every (E0, E1)
    instantiation of the split kernel at each KS (K = 128 with both is the LATE_RES path), with and without leftover
    tasks; the f32-MFMA kernel at NC = 2 and NC = 4."""
    for R in rows:
        _check_case(K, NO, "main", fs, R)


# ------------------------------------------------------------------------------------------------ large row counts
def _large_split_cases():
    shapes = [(R, K, WIDTH_AT_LARGE[K]) for R in ROWS_SPLIT_LARGE for K in K_SPLIT]
    shapes += [(42368, 64, 256), (32833, 128, 256), (65569, 128, 192)]
    for R, K, NO in shapes:
        for tb in (True, False):
            for kind in tw.KINDS:
                yield R, K, NO, tb, kind


@pytest.mark.parametrize("R,K,NO,transB,kind", list(_large_split_cases()))
def test_split_kernel_at_the_row_counts_where_the_launch_changes(R, K, NO, transB, kind):
    _check_case(K, NO, kind, tw.FULL[transB], R)


def _large_f32_cases():
    shapes = [(R, K, NO) for R in (65408, 65409) for K in (8, 56) for NO in (128, 256)]
    shapes += [(R, K, NO) for R in (131072, 131073) for K, NO in ((56, 128), (8, 36))]
    for R, K, NO in shapes:
        for tb in (True, False):
            for kind in tw.KINDS:
                yield R, K, NO, tb, kind


@pytest.mark.parametrize("R,K,NO,transB,kind", list(_large_f32_cases()))
def test_f32_kernel_at_the_row_counts_where_the_launch_changes(R, K, NO, transB, kind):
    _check_case(K, NO, kind, tw.FULL[transB], R)


# ------------------------------------------------------------------------------------------- in-place accumulation
@pytest.mark.parametrize("R", [33, 32833])
@pytest.mark.parametrize("K,NO", [(32, 100), (64, 256), (128, 160), (128, 256), (56, 128), (256, 100)])
@pytest.mark.parametrize("transB", [True, False])
def test_residual_read_from_the_output(K, NO, transB, R):
    """res is out (tape._mm_launch accumulates contraction passes that way): the same bits as with a separate copy."""
    fs = (transB, True, False, not transB, True)
    where = "K=%d NO=%d %s R=%d in place" % (K, NO, tw.flagset_name(fs), R)
    o, d = _operands("main", R, K, NO, fs, seed=1)
    L = Launch(o, True)
    apart, _ = L.fire()
    base, out = _wide(o["res"], R, NO, L.ldy, L.cy)
    L.fire(out=out, res=out)
    note(_family(K), out, d["ref"], d["S"], tw.U, where)
    assert_within(out, d["ref"], d["S"], tw.c_bound(K), tw.U, where)
    assert torch.equal(out, apart), where
    assert _guards_intact(base, out), where


# ------------------------------------------------------------------------------------------------ through the tape
def _tape_operands(R, K, NO, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(R, K, generator=g, device=DEV), torch.randn(NO, K, generator=g, device=DEV) / K ** 0.5,
            0.1 * torch.randn(NO, generator=g, device=DEV))


def test_tape_nt_with_bias_on_the_four_column_block_kernel():
    """tape.mm_raw "nt" at K = 50 (padded to 56 with zero columns: exact) and 65409 rows: k_linear<4>."""
    from geossl_amd import tape as tp
    R, K, NO = 65409, 50, 128
    assert tw.plan(R, 56, NO)["NC"] == 4
    a, w, bias = _tape_operands(R, K, NO, 50)
    got = tp.mm_raw(a, w, "nt", bias=bias)
    ref = a.double() @ w.double().t() + bias.double()
    S = a.double().abs() @ w.double().abs().t() + bias.double().abs()
    where = "tape nt R=%d K=%d NO=%d bias" % (R, K, NO)
    print("ratio %-12s %-60s %8.3f" % (_family(56), where, note(_family(56), got, ref, S, tw.U, where)))
    assert got.shape == (R, NO)
    assert_within(got, ref, S, tw.c_bound(56), tw.U, where)


def test_tape_nn_on_the_four_column_block_kernel():
    from geossl_amd import tape as tp
    R, K, NO = 65409, 50, 128
    a, w, _ = _tape_operands(R, K, NO, 51)
    b = w.t().contiguous()                                      # [K][NO]
    got = tp.mm_raw(a, b, "nn")
    ref, S = a.double() @ b.double(), a.double().abs() @ b.double().abs()
    where = "tape nn R=%d K=%d NO=%d" % (R, K, NO)
    print("ratio %-12s %-60s %8.3f" % (_family(56), where, note(_family(56), got, ref, S, tw.U, where)))
    assert got.shape == (R, NO)
    assert_within(got, ref, S, tw.c_bound(56), tw.U, where)


def test_tape_nt_in_two_contraction_passes():
    """K = 264: a pass over k < 256 (c = c(256)), then one over the last 8 with the first pass's result as the in-place
    residual.  The passes' bounds add: c(256) u S1 + c(8) u (S2 + |y1|) with |y1| <= (1 + c u) S1, so with c = c(256)
    for both: c u (1 + c u) (2 S1 + S2)."""
    from geossl_amd import tape as tp
    R, K, NO = 33, 264, 100
    a, w, bias = _tape_operands(R, K, NO, 52)
    got = tp.mm_raw(a, w, "nt", bias=bias)
    ad, wd = a.double(), w.double()
    ref = ad @ wd.t() + bias.double()
    S1 = ad[:, :256].abs() @ wd[:, :256].abs().t() + bias.double().abs()
    S2 = ad[:, 256:].abs() @ wd[:, 256:].abs().t()
    c = tw.c_bound(256)
    S = (1.0 + c * tw.U) * (2.0 * S1 + S2)
    where = "tape nt R=%d K=%d NO=%d two passes" % (R, K, NO)
    print("ratio %-12s %-60s %8.3f" % ("tape 2-pass", where, note("tape 2-pass", got, ref, S, tw.U, where)))
    assert_within(got, ref, S, c, tw.U, where)


# ------------------------------------------------------------------------------------------------------- refusals
def _abi_call(prepared, R, K, NO, ldx=None, ldy=None, alloc_rows=33):
    """geossl_linear[_prepared] straight through the C ABI on valid buffers of `alloc_rows` rows: (return code, out)."""
    from geossl_amd import _lib
    lib = _lib.load()
    ldx, ldy = K if ldx is None else ldx, NO if ldy is None else ldy
    x = torch.randn(alloc_rows, max(ldx, K), device=DEV)
    w = torch.randn(max(NO, 1) * max(K, 1), device=DEV)
    out = _nan(alloc_rows, max(ldy, NO))
    if prepared:
        image = torch.zeros(max(int(lib.geossl_linear_image_words(K, NO)), 4), dtype=torch.int32, device=DEV)
        rc = lib.geossl_linear_prepared(_lib.ptr(x), ldx, _lib.ptr(image), None, None, None, _lib.ptr(out), ldy, R, K, NO,
                                        0, _lib.stream())
    else:
        rc = lib.geossl_linear(_lib.ptr(x), ldx, _lib.ptr(w), None, None, None, _lib.ptr(out), ldy, R, K, NO, 1, 0,
                               _lib.stream())
    torch.cuda.synchronize()
    return rc, out


REFUSALS = [("prepared K=128 NO=160", dict(prepared=True, R=33, K=128, NO=160)),
            ("K=12", dict(prepared=False, R=33, K=12, NO=64)),
            ("K=264", dict(prepared=False, R=33, K=264, NO=64)),
            ("NO=258", dict(prepared=False, R=33, K=64, NO=258)),
            ("ldx < K", dict(prepared=False, R=33, K=64, NO=64, ldx=60)),
            ("ldy not a multiple of 4", dict(prepared=False, R=33, K=64, NO=64, ldy=66)),
            ("ldy not a multiple of 4, f32 kernel", dict(prepared=False, R=33, K=56, NO=64, ldy=66)),
            ("prepared ldx < K", dict(prepared=True, R=33, K=64, NO=64, ldx=60))]


@pytest.mark.parametrize("what,kw", REFUSALS, ids=[w for w, _ in REFUSALS])
def test_refused_shapes_return_an_error_and_launch_nothing(what, kw):
    p = tw.plan(kw["R"], kw["K"], kw["NO"], prepared=kw["prepared"], ldx=kw.get("ldx"), ldy=kw.get("ldy"))
    assert p["refused"], what
    rc, out = _abi_call(**kw)
    assert rc == tw.HIP_ERROR_INVALID_VALUE, (what, rc)
    assert bool((out.view(torch.int32) == NAN_BITS).all()), what


def test_ops_linear_raises_on_a_refused_prepared_shape():
    from geossl_amd import _lib, ops
    W = torch.randn(160, 128, device=DEV)
    img = ops.prepare_linear([W])[0]
    out = _nan(33, 160)
    with pytest.raises(_lib.GeosslHipError):
        ops.linear(torch.randn(33, 128, device=DEV), img, out=out)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == NAN_BITS).all())


@pytest.mark.parametrize("prepared,K", [(False, 64), (False, 56), (True, 64), (True, 128)])
def test_row_counts_past_32_bits_are_refused(prepared, K):
    """R = 2^31 on buffers of 33 rows: both entry points return hipErrorInvalidValue before any launch (they cast R to
    int for the kernels; the refusal is the first statement after the R <= 0 return)."""
    assert tw.plan(2 ** 31, K, 64, prepared=prepared)["refused"]
    rc, out = _abi_call(prepared, 2 ** 31, K, 64)
    assert rc == tw.HIP_ERROR_INVALID_VALUE, rc
    assert bool((out.view(torch.int32) == NAN_BITS).all())
