"""The row kernels at the two ends of both backbones (csrc/schnet.hip) element by element against their fp64 twins
(tests/row_twin.py): geossl_embedding_bwd[_dyn] (k_embedding_bwd_partial<NG> + k_embedding_bwd_reduce),
geossl_embedding_fwd[_dyn], geossl_segment_reduce_fwd / _bwd, geossl_row_normalize_fwd / _bwd, all through the C entry
points.

Embedding backward (row_twin.EMB_BWD; test_row_twin_cpu.py pins the regime of every shape): the five group plans
(C = 9 / 100 at F = 128, C = 9 / 13 at F = 256, C = 9 at F = 48: four groups or one, 128 ... 1024 threads); 0, 1, 700,
2049, 32768, 32769, 65537 rows on four groups and 8193, 16385 on one (floor of 16 chunks, rounding to a multiple of 4,
64 / 65 chunks per slice: the second ballot round empty / one lane, the cap of 512 with empty trailing chunks); shuffled
and sorted classes, classes {1, 8} alone, a class in one chunk only, a class never present, z with stride 2, classes
-1, C and 2^32 + 1 (nothing may arrive anywhere), accumulate onto a random prior, a device-side row count with NaN rows of
class 99 behind it, dh times 2^-20 and 2^20, and the refusals (F = 257; 160 classes at F = 256, whose launch would ask
for 8 bytes more LDS than a CU has).  The workspace is filled with an integer sentinel: the band slots a launch
overwrote are counted against row_twin.plan, their contents and the partial rows written against the classes of each
chunk.
Embedding forward: torch.equal to table[z] on the vector widths 32 / 64 / 128 and on the scalar kernel (F = 48; F = 128
with the table or the output 4 bytes off a 16-byte boundary), z with stride 2, a device-side count, classes outside the
table (zeros and the status word, which stays 0 otherwise).
Readout: one ragged batch (0, 1, 2, 33, 255, 0 atoms) at F = 48 / 128 / 300, add and mean, backward with and without
accumulate.  Row normalize: 1, 5, 333 rows at F = 48 / 64 / 128 / 300 with an all-zero row, a row of 1e-20 (clamped), a
row just above eps, rows times 2^-40 and 2^40; norm = NULL.
Every case: outputs inside NaN-filled tensors whose guard rows keep their bits, every element within c u S of the twin
(exact where S = 0), elementwise.REPEATS launches bit-identical, one removed term flagged in exactly one element (row
normalize: one square or product removed from a row's reduction flags elements of that row and of no other).  c is a
count of roundings from the twin, u = 2^-24; the worst err / (u S) measured is printed and recorded in DESIGN.md
section 4."""
import pytest
import torch

import row_twin as tw
from elementwise import assert_repeatable, assert_sees_a_dropped_term, assert_within, flagged
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC00000
GUARD = 8
SENTINEL = -0x12345678            # as a float about -8e27: no sum of the tests' terms


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The worst err / (u S) per kernel family over the cases that ran, beside the c of that element."""
    yield
    print()
    for k in sorted(WORST):
        print("worst err/(u S)  %-28s %8.3f  (c = %g) at %s" % ((k,) + WORST[k]))


def note(fam, got, ref, S, c, where, extra=None):
    """err / (u S) of a tensor, recorded before it is asserted on."""
    err = (got.double() - ref).abs()
    if extra is not None:
        err = (err - extra).clamp_min(0.0)
    r = torch.where(S > 0, err / (tw.U * S), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    if not r.numel():
        return 0.0
    k = int(r.argmax())
    worst = float(r.reshape(-1)[k])
    ck = float(c.expand_as(r).reshape(-1)[k]) if torch.is_tensor(c) else float(c)
    if fam not in WORST or not worst <= WORST[fam][0]:
        WORST[fam] = (worst, ck, where)
    print("ratio %-28s %-44s %8.3f (c = %g)" % (fam, where, worst, ck))
    return worst


def _dev(t):
    return t.to(DEV) if torch.is_tensor(t) else t


def _guarded(rows, F, fill=None):
    """A NaN-filled [rows + 2 GUARD, F] tensor and its middle [rows, F] (holding `fill`)."""
    base = torch.full((rows + 2 * GUARD, F), float("nan"), device=DEV)
    view = base[GUARD:GUARD + rows]
    if fill is not None:
        view.copy_(fill)
    return base, view


def _guards_intact(base, rows):
    b = base.view(torch.int32)
    return bool((b[:GUARD] == NAN_BITS).all()) and bool((b[GUARD + rows:] == NAN_BITS).all())


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _call(name, *args):
    from geossl_amd import _lib
    _lib.call(name, *[_lib.ptr(a) if torch.is_tensor(a) or a is None else a for a in args], _lib.stream())


# ================================================================================================== embedding backward
class EmbBwd:
    """The device operands of one case and its launches into a fresh NaN-filled table and a sentinel-filled workspace."""

    def __init__(self, name):
        from geossl_amd import _lib
        self.c = c = tw.emb_bwd_case(name)
        self.z, self.dh = c["z_store"].to(DEV), c["dh"].to(DEV)
        self.prior = _dev(c["prior"])
        self.dyn = None if c["dyn"] is None else torch.tensor([c["dyn"]], dtype=torch.int32, device=DEV)
        nfl = int(_lib.load().geossl_embedding_bwd_workspace_floats(c["C"], c["F"]))
        assert nfl == tw.workspace_floats(c["C"], c["F"])
        self.ws = torch.empty(nfl, dtype=torch.int32, device=DEV)

    def fire(self):
        c = self.c
        base, table = _guarded(c["C"], c["F"], self.prior)
        self.ws.fill_(SENTINEL)
        args = (self.z, c["zs"], self.dh, c["C"], c["N"], c["F"], table, self.ws, int(c["acc"]))
        if self.dyn is None:
            _call("geossl_embedding_bwd", *args)
        else:
            _call("geossl_embedding_bwd_dyn", *args, self.dyn)
        return table, base

    def inputs_unchanged(self):
        return torch.equal(self.z.cpu(), self.c["z_store"]) and _bits_equal(self.dh.cpu(), self.c["dh"])


def _check_workspace(ws, c, name):
    """Exactly plan's nchunks band slots overwritten, each with the classes its rows hold; of the partial tables exactly
    the rows of each chunk's band."""
    C, F, n = c["C"], c["F"], c["launch"]["nchunks"]
    band = ws[tw.EMB_CHUNKS * C * F:].view(tw.EMB_CHUNKS, 2)
    written = (band != SENTINEL).any(1)
    assert int(written.sum()) == n and bool(written[:n].all()), (name, int(written.sum()), n)
    want = c["bands"].to(DEV)
    assert torch.equal(band[:n].long(), want), name
    part = ws[:tw.EMB_CHUNKS * C * F].view(tw.EMB_CHUNKS, C, F) != SENTINEL
    k = torch.arange(C, device=DEV)[None, :]
    expect = torch.zeros(tw.EMB_CHUNKS, C, dtype=torch.bool, device=DEV)
    expect[:n] = (k >= want[:, :1]) & (k <= want[:, 1:])
    assert torch.equal(part.all(2), expect) and torch.equal(part.any(2), expect), name


def _check_emb_bwd(name):
    L = EmbBwd(name)
    c = L.c
    fam = "embedding_bwd ng=%d" % c["launch"]["ng"]
    got, base = L.fire()
    torch.cuda.synchronize()
    ws = L.ws.clone()
    ref, S = c["ref"].to(DEV), c["S"].to(DEV)
    note(fam, got, ref, S, c["c"], name)
    assert_within(got, ref, S, c["c"], tw.U, name)
    assert _guards_intact(base, c["C"]), name
    for k in c["absent"]:               # a class without a row: exactly 0, or the prior's bits
        assert _bits_equal(got[k], L.prior[k]) if c["acc"] else bool((got[k] == 0).all()), (name, k)
    _check_workspace(ws, c, name)
    if c["pick"] is not None:
        index, term, ratio = c["pick"]
        assert ratio >= 2.0, (name, ratio)
        assert_sees_a_dropped_term(got, ref, S, c["c"], tw.U, index, term, name)
    assert_repeatable(lambda: [L.fire()[0]], [got], name)
    assert L.inputs_unchanged(), name
    return got


@pytest.mark.parametrize("name", [n for n in tw.EMB_BWD if not n.startswith("dh 2^")])
def test_embedding_backward(name):
    got = _check_emb_bwd(name)
    if name.startswith("out of range"):
        # the first defect: (int)(2^32 + 1) is 1.  Row 1 holds class 1's rows alone
        c = tw.emb_bwd_case(name)
        z, dh = c["z"], c["dh"].double()
        assert int((z == 2 ** 32 + 1).sum()) > 50
        wrong = c["ref"].clone()
        wrong[1] += dh[z == 2 ** 32 + 1].sum(0)
        assert int(flagged(got, wrong.to(DEV), c["S"].to(DEV), c["c"], tw.U).sum()) > 0


@pytest.mark.parametrize("scale", [-20, 20])
def test_embedding_backward_scales_with_a_power_of_two(scale):
    """dh times 2^-20 and 2^20: the same bound and the same flags, because the result is the base case's times the
    factor, bit for bit."""
    base = EmbBwd("rows 2049").fire()[0]
    got = _check_emb_bwd("dh 2^%d" % scale)
    assert torch.equal(got, base * 2.0 ** scale)


@pytest.mark.parametrize("C,F", [(9, 257), (160, 256)])
def test_embedding_backward_refusals_launch_nothing(C, F):
    """hipErrorInvalidValue from the entry point itself, table and workspace untouched.  160 x 256: the table alone is
    exactly 160 KB, the launch would ask for one band more (the second defect: it used to be admitted)."""
    from geossl_amd import _lib
    lib = _lib.load()
    assert tw.launch(33, C, F)["refused"]
    g = torch.Generator(device=DEV).manual_seed(5)
    z = torch.randint(0, C, (33,), device=DEV, generator=g)
    dh = torch.randn(33, F, device=DEV, generator=g)
    dims = torch.tensor([20], dtype=torch.int32, device=DEV)
    base, table = _guarded(C, F)
    ws = torch.full((tw.workspace_floats(C, F),), SENTINEL, dtype=torch.int32, device=DEV)
    args = (_lib.ptr(z), 1, _lib.ptr(dh), C, 33, F, _lib.ptr(table), _lib.ptr(ws), 0)
    assert lib.geossl_embedding_bwd(*args, _lib.stream()) == tw.HIP_ERROR_INVALID_VALUE
    assert lib.geossl_embedding_bwd_dyn(*args, _lib.ptr(dims), _lib.stream()) == tw.HIP_ERROR_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((base.view(torch.int32) == NAN_BITS).all()) and bool((ws == SENTINEL).all())


# =================================================================================================== embedding forward
EMB_FWD_VARIANTS = ("plain", "z stride 2", "dyn", "out of range")
EMB_FWD_PATHS = [(32, None), (64, None), (128, None), (48, None), (128, "table"), (128, "out")]


@pytest.mark.parametrize("variant", EMB_FWD_VARIANTS)
@pytest.mark.parametrize("F,offset", EMB_FWD_PATHS, ids=["F=%d%s" % (F, " %s 4 bytes off" % o if o else "") for F, o in EMB_FWD_PATHS])
def test_embedding_forward_is_the_table_row(F, offset, variant):
    """The vector kernel (F = 32 / 64 / 128, 16-byte aligned) and the scalar one (any other F, or a pointer 4 bytes off)."""
    C, N = 9, 1000
    g = torch.Generator(device=DEV).manual_seed(10 * F + EMB_FWD_VARIANTS.index(variant))
    flat = torch.randn(C * F + 4, device=DEV, generator=g)
    table = flat[1:1 + C * F].view(C, F) if offset == "table" else flat[:C * F].view(C, F)
    zs = 2 if variant == "z stride 2" else 1
    z_store = torch.full((N, zs), 99, dtype=torch.int64, device=DEV)
    z = torch.randint(0, C, (N,), device=DEV, generator=g)
    n_real = N
    dims = None
    if variant == "dyn":
        n_real = 700
        z[n_real:] = 99                                  # outside the table: must not be looked at
        dims = torch.tensor([n_real], dtype=torch.int32, device=DEV)
    if variant == "out of range":
        for k, v in enumerate(tw.OUT_OF_RANGE):
            z[3 + 7 * k::21] = C if v is None else v
    z_store[:, 0] = z
    ok = (z[:n_real] >= 0) & (z[:n_real] < C)
    want = torch.where(ok[:, None], table[z[:n_real].clamp(0, C - 1)], torch.zeros((), device=DEV))
    rows = N + 2 * GUARD

    def fire():
        oflat = torch.full((rows * F + 4,), float("nan"), device=DEV)
        base = oflat[1:1 + rows * F].view(rows, F) if offset == "out" else oflat[:rows * F].view(rows, F)
        out = base[GUARD:GUARD + N]
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        if dims is None:
            _call("geossl_embedding_fwd", z_store, zs, table, C, N, F, out, status)
        else:
            _call("geossl_embedding_fwd_dyn", z_store, zs, table, C, N, F, out, status, dims)
        return out, oflat, status

    assert (table.data_ptr() % 16 == 4) == (offset == "table")
    out, oflat, status = fire()
    assert (out.data_ptr() % 16 == 4) == (offset == "out")
    assert _bits_equal(out[:n_real], want), (F, offset, variant)
    # everything that is not a real row keeps its NaN bits: the guard rows, the rows past the device-side count
    assert int((oflat.view(torch.int32) != NAN_BITS).sum()) == n_real * F
    assert int(status) == (1 if variant == "out of range" else 0)
    if variant == "out of range":
        assert int((~ok).sum()) > 100 and bool((out[:n_real][~ok] == 0).all())
    assert_repeatable(lambda: [fire()[0][:n_real]], [out[:n_real]], "embedding_fwd F=%d %s %s" % (F, offset, variant))


# ============================================================================================================== readout
@pytest.mark.parametrize("mean", [False, True], ids=["add", "mean"])
@pytest.mark.parametrize("F", tw.SEG_F)
def test_segment_reduce_forward(F, mean):
    c = tw.seg_case(F, mean, False)
    what = "segment_reduce_fwd F=%d %s" % (F, "mean" if mean else "add")
    h, mp, B = c["h"].to(DEV), c["mol_ptr"].to(DEV), len(tw.SEG_SIZES)
    ref, S, cc = (_dev(t) for t in c["fwd"])

    def fire():
        base, out = _guarded(B, F)
        _call("geossl_segment_reduce_fwd", h, mp, B, F, int(mean), out)
        return out, base

    got, base = fire()
    note("segment_reduce_fwd", got, ref, S, cc, what)
    assert_within(got, ref, S, cc, tw.U, what)
    assert _guards_intact(base, B), what
    assert bool((got[0] == 0).all()) and bool((got[-1] == 0).all()), what          # the empty molecules
    index, term, ratio = c["pick_fwd"]
    assert ratio >= 2.0, (what, ratio)
    assert_sees_a_dropped_term(got, ref, S, cc, tw.U, index, term, what)
    assert_repeatable(lambda: [fire()[0]], [got], what)
    assert _bits_equal(h.cpu(), c["h"]), what


@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("mean", [False, True], ids=["add", "mean"])
@pytest.mark.parametrize("F", tw.SEG_F)
def test_segment_reduce_backward(F, mean, accumulate):
    c = tw.seg_case(F, mean, accumulate)
    what = "segment_reduce_bwd F=%d %s%s" % (F, "mean" if mean else "add", " accumulate" if accumulate else "")
    dout, mp, prior = c["dout"].to(DEV), c["mol_ptr"].to(DEV), _dev(c["prior"])
    N, B = int(c["mol_ptr"][-1]), len(tw.SEG_SIZES)
    ref, S, cc = (_dev(t) for t in c["bwd"])

    def fire():
        base, dh = _guarded(N, F, prior)     # (the rows of an empty molecule do not exist: the guard rows stand for them)
        _call("geossl_segment_reduce_bwd", dout, mp, B, F, int(mean), dh, int(accumulate))
        return dh, base

    got, base = fire()
    note("segment_reduce_bwd", got, ref, S, cc, what)
    assert_within(got, ref, S, cc, tw.U, what)
    if cc == 0:
        assert torch.equal(got.double(), ref), what
    assert _guards_intact(base, N), what
    index, term, ratio = c["pick_bwd"]
    assert ratio >= 2.0, (what, ratio)
    assert_sees_a_dropped_term(got, ref, S, cc, tw.U, index, term, what)
    assert_repeatable(lambda: [fire()[0]], [got], what)


# ======================================================================================================== row normalize
def _only_rows_flagged(bad, r):
    return bool(bad[r].any()) and int(bad.sum()) == int(bad[r].sum())


@pytest.mark.parametrize("F", tw.RN_F)
@pytest.mark.parametrize("N", tw.RN_ROWS)
def test_row_normalize_forward(N, F):
    c = tw.rn_case(N, F)
    what = "row_normalize_fwd N=%d F=%d" % (N, F)
    h = c["h"].to(DEV)
    ref, S, cc = (_dev(t) for t in c["fwd"])
    nref, nS, nc, nextra = (_dev(t) for t in c["norm"])

    def fire(with_norm=True):
        ybase, y = _guarded(N, F)
        nbase, norm = _guarded(N, 1)
        _call("geossl_row_normalize_fwd", h, N, F, tw.EPS, y, norm if with_norm else None)
        return y, norm, ybase, nbase

    y, norm, ybase, nbase = fire()
    note("row_normalize_fwd y", y, ref, S, cc, what)
    note("row_normalize_fwd norm", norm, nref, nS, nc, what, extra=nextra)
    assert_within(y, ref, S, cc, tw.U, what)
    assert_within(norm, nref, nS, nc, tw.U, what + " norm", extra=nextra)
    assert _guards_intact(ybase, N) and _guards_intact(nbase, N), what
    if N in tw.RN_ZERO:
        assert bool((y[tw.RN_ZERO[N]] == 0).all()) and float(norm[tw.RN_ZERO[N]]) == 0.0, what
    # one square removed from one row's norm: elements of that row are flagged, and of no other
    (r, f), term, ratio = c["pick_fwd"]
    assert ratio >= 2.0 and r == c["drop_row"], (what, ratio)
    assert _only_rows_flagged(flagged(y, c["drop_fwd"].to(DEV), S, cc, tw.U), r), what
    assert_repeatable(lambda: list(fire()[:2]), [y, norm], what)
    # norm = NULL (no gradient wanted): accepted, the same y, nothing stored
    y2, norm2, ybase2, nbase2 = fire(with_norm=False)
    assert torch.equal(y2, y) and _guards_intact(ybase2, N), what
    assert bool((nbase2.view(torch.int32) == NAN_BITS).all()), what
    assert _bits_equal(h.cpu(), c["h"]), what


@pytest.mark.parametrize("F", tw.RN_F)
@pytest.mark.parametrize("N", tw.RN_ROWS)
def test_row_normalize_backward(N, F):
    """y and norm are given (the twin's, rounded to fp32); on the clamped rows dh = g / eps on its own scale."""
    c = tw.rn_case(N, F)
    what = "row_normalize_bwd N=%d F=%d" % (N, F)
    g, y, norm = c["g"].to(DEV), c["y32"].to(DEV), c["norm32"].to(DEV)
    ref, S, cc = (_dev(t) for t in c["bwd"])

    def fire():
        base, dh = _guarded(N, F)
        _call("geossl_row_normalize_bwd", g, y, norm, N, F, tw.EPS, dh)
        return dh, base

    got, base = fire()
    note("row_normalize_bwd", got, ref, S, cc, what)
    assert_within(got, ref, S, cc, tw.U, what)
    assert _guards_intact(base, N), what
    if N in tw.RN_ZERO:
        for r in (tw.RN_ZERO[N], tw.RN_TINY[N]):
            assert float(cc[r]) == 2.0 and float((got[r].double() - ref[r]).abs().max()) <= 2.0 * tw.U * float(ref[r].abs().max())
    (r, f), term, ratio = c["pick_bwd"]
    assert ratio >= 2.0 and r == c["drop_row"], (what, ratio)
    assert _only_rows_flagged(flagged(got, c["drop_bwd"].to(DEV), S, cc, tw.U), r), what
    index, term, ratio = c["pick_g"]
    assert ratio >= 2.0, (what, ratio)
    assert_sees_a_dropped_term(got, ref, S, cc, tw.U, index, term, what + " g term")
    assert_repeatable(lambda: [fire()[0]], [got], what)
    assert _bits_equal(g.cpu(), c["g"]) and _bits_equal(y.cpu(), c["y32"]), what
