"""geossl_linear_wgrad[_dyn] (csrc/wgrad.h: k_wgrad_split<., ., PlainOps>; csrc/tn.h: k_reduce_multi) through
ops.linear_wgrad and the C ABI against the fp64 twin (tests/wgrad_twin.py), element by element of every dW and db.

Row counts (geossl_tn_plan; pinned by tests/test_wgrad_twin_cpu.py).  One problem: 1, 31, 32, 33, 63, 64 (one chunk of
64, one or two tiles; at 33 and 63 the second request set holds a partial tile); 65, 97 (two chunks: reduction slices 2
and 3 empty, six dead XCD slots, a last chunk of 1 and 33 rows); 449, 513 (eight chunks exactly, then nine: seven dead
slots in the second round); 32 641 (the first count with chunk = 128: four tiles per chunk, the refill of a request set
runs, the last chunk has one row); 65 313 (chunk = 256 from 65 281 on: eight tiles, the refill repeats; a last chunk of
33 rows).  3, 18 and 32 problems: chunk = 256 with a chunk count of 0, 1 and 7 mod 8 (ROWS_MULTI).
Operands: the twin's KINDS.  Every case checks |got - ref| <= c u S on every element, launches elementwise.REPEATS
times without a differing element, on `slices` (and every wide form) that the NaN surroundings of the outputs keep
their bits, and on `main`, `blocks` and `spike` that one removed product a[r][m] b[r][n] is flagged in exactly one
element, r taken from the first tile of a chunk, the last tile of the launch, a tile of the second request set and tiles
served after a refill.  c comes from the twin's arithmetic model; the worst err / (u S) measured here is printed per
family and recorded in DESIGN.md section 4."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import wgrad_twin as tw
from elementwise import assert_repeatable, assert_sees_a_dropped_term, assert_within
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC00000
GUARD = tw.GUARD
ROWS_ONE = (1, 31, 32, 33, 63, 64, 65, 97, 449, 513)
ROWS_LONG = (32641, 65313)
ROWS_MULTI = {3: (22528, 22529, 22050), 18: (4096, 4097, 5666), 32: (2048, 2049, 3618)}
ROWS_FORMS = (33, 513)
PROOF_ROWS_MAX = 40000
PROOF_KINDS = ("main", "blocks", "spike")
WIDTHS_OPS = [(M, N) for M in (32, 64, 128) for N in (32, 64, 128)]
WIDTHS_ABI = [(36, 100), (100, 36), (4, 124), (60, 128)]


def rows_256(nprob):
    """The smallest row count of a launch of `nprob` >= 2 problems with chunk = 256, plus a partial tile of one row."""
    return 256 * (-(-256 // nprob) - 1) + 33


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The worst err / (u S) per family over the cases that ran (what DESIGN.md section 4 records)."""
    yield
    for k in sorted(WORST):
        print("worst err/(u S)  %-12s %8.3f  at %s" % ((k,) + WORST[k]))


def note(fam, got, ref, S, where):
    """err / (u S) of a tensor, recorded before it is asserted on."""
    err = (got.double() - ref).abs()
    r = torch.where(S > 0, err / (tw.U[fam] * S), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                             torch.zeros_like(err)))
    r = float(r.max()) if r.numel() else 0.0
    if fam not in WORST or not r <= WORST[fam][0]:
        WORST[fam] = (r, where)
    return r


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _place(t, rows, cols, how, row_guard=GUARD):
    """(base, view): a [rows, cols] view holding t (or NaN).  how = 0: its own contiguous tensor; "slice": the middle
    column block behind row_guard rows of a NaN-filled [rows + 2 row_guard, 3 cols] tensor; an int p > 0: the first
    `cols` columns of a NaN-filled [rows, cols + p] tensor."""
    if how == "slice":
        base = _nan(rows + 2 * row_guard, 3 * cols)
        view = base[row_guard:row_guard + rows, cols:2 * cols]
    else:
        base = _nan(rows, cols + how)
        view = base[:, :cols]
    if t is not None:
        view.copy_(t)
    return base, view


class Launch:
    """The device side of one case: operands placed once, fresh outputs per launch."""

    def __init__(self, probs, R, M, N, given, how=0, accumulate=False, prior=None, abi=False, count=None, cap=None):
        self.R, self.M, self.N, self.given, self.how, self.accumulate = R, M, N, given, how, accumulate
        self.abi, self.cap = abi, cap or R
        placed = {}
        self.A, self.B = [], []
        for A, B in probs:      # (problems that share an operand tensor share its device copy)
            for t, w, dst in ((A, M, self.A), (B, N, self.B)):
                if id(t) not in placed:
                    placed[id(t)] = _place(t[:self.cap, :w].to(DEV), self.cap, w, how)[1]
                dst.append(placed[id(t)])
        self.prior = None if prior is None else [(w.to(DEV), None if b is None else b.to(DEV)) for w, b in prior]
        self.count = None if count is None else torch.tensor([count, 0, 0, 0], dtype=torch.int32, device=DEV)
        self.lda, self.ldb = self.A[0].stride(0), self.B[0].stride(0)

    def outputs(self):
        dWs, dbs, bases = [], [], []
        for z in range(len(self.A)):
            w0, b0 = self.prior[z] if self.prior is not None else (None, None)
            base, dW = _place(w0, self.M, self.N, self.how)
            bases.append((base, dW))
            dWs.append(dW)
            if self.given[z]:
                base, db = _place(None if b0 is None else b0[None, :], 1, self.M, self.how, row_guard=0)
                bases.append((base, db))
                dbs.append(db[0])
            else:
                dbs.append(None)
        return dWs, dbs, bases

    def fire(self, outs=None):
        """One launch into fresh outputs (or into `outs`): (dWs, dbs, bases)."""
        from geossl_amd import _lib, ops
        dWs, dbs, bases = outs or self.outputs()
        probs = list(zip(self.A, self.B, dWs, dbs))
        ldw = dWs[0].stride(0)
        if self.abi:       # the by-value entry point of the C ABI
            tb = _lib.TnBatch()
            for i, (A, B, dW, db) in enumerate(probs):
                tb.A[i], tb.B[i], tb.dW[i], tb.db[i] = _lib.ptr(A), _lib.ptr(B), _lib.ptr(dW), _lib.ptr(db)
            nfl = _lib.load().geossl_tn_workspace_floats(self.R, self.M, self.N, len(probs))
            ws = torch.empty(nfl, dtype=torch.float32, device=DEV)
            _lib.call("geossl_linear_wgrad", C.byref(tb), len(probs), self.R, self.M, self.N, self.lda, self.ldb, ldw,
                      _lib.ptr(ws), 1 if self.accumulate else 0, _lib.stream())
        else:
            ops.linear_wgrad(probs, self.R, self.M, self.N, accumulate=self.accumulate, lda=self.lda, ldb=self.ldb,
                             ldw=ldw, dyn_rows=None if self.count is None else self.count.data_ptr())
        return dWs, dbs, bases


def _flat(dWs, dbs):
    return list(dWs) + [b for b in dbs if b is not None]


def _assert_guards(bases, where):
    """What surrounds a placed output keeps the bits it was filled with (integer views)."""
    for base, view in bases:
        bits = base.view(torch.int32)
        assert int((bits != NAN_BITS).sum()) == int((view.view(torch.int32) != NAN_BITS).sum()), where


def _compare(where, ref, dWs, dbs, pieces):
    fam = tw.family(pieces)
    worst = 0.0
    for z, d in enumerate(ref):
        worst = max(worst, note(fam, dWs[z], d["ref_dW"], d["S_dW"], "%s problem %d" % (where, z)))
        if dbs[z] is not None:
            note("db", dbs[z], d["ref_db"], d["S_db"], "%s problem %d" % (where, z))
    print("ratio %-10s %-70s %8.3f" % (fam, where, worst))
    for z, d in enumerate(ref):
        assert_within(dWs[z], d["ref_dW"], d["S_dW"], tw.C_BOUND[fam], tw.U[fam], "%s dW %d" % (where, z))
        if dbs[z] is not None:
            assert_within(dbs[z], d["ref_db"], d["S_db"], tw.C_BOUND["db"], tw.U["db"], "%s db %d" % (where, z))


def _check(where, kind, nprob, R, M, N, db="all", how=0, accumulate=False, abi=False, dyn=False, pieces=2, seed=0):
    chunk, _ = tw.plan(R, 3 if kind == "shared" else nprob)
    probs = tw.operands("main" if kind == "slices" else kind, nprob, R, M, N, chunk, seed=seed)
    if kind == "slices":
        how = "slice"
    given = [True, False, False] if kind == "shared" else tw.db_given(db, len(probs))
    prior = tw.priors(probs, M, N, given, seed=seed) if accumulate else None
    L = Launch(probs, R, M, N, given, how=how, accumulate=accumulate, prior=prior, abi=abi, count=R if dyn else None)
    dev = [(a, b) for a, b in zip(L.A, L.B)]
    ref = tw.wgrad(dev, R, M, N, chunk, prior=L.prior, pieces=pieces)
    dWs, dbs, bases = L.fire()
    _compare(where, ref, dWs, dbs, pieces)
    _assert_guards(bases, where)
    if kind in PROOF_KINDS and R <= PROOF_ROWS_MAX and not accumulate:
        fam = tw.family(pieces)
        for k, (name, r) in enumerate(tw.proof_rows(R, chunk).items()):
            z = k % len(ref)
            idx, term, ratio = tw.pick_dropped_term(ref[z], r, tw.C_BOUND[fam], tw.U[fam])
            w = "%s problem %d %s row %d" % (where, z, name, r)
            assert ratio >= 2.0, (w, ratio)
            assert_sees_a_dropped_term(dWs[z], ref[z]["ref_dW"], ref[z]["S_dW"], tw.C_BOUND[fam], tw.U[fam], idx, term, w)
    assert_repeatable(lambda: _flat(*L.fire()[:2]), _flat(dWs, dbs), where)


# ------------------------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize("kind", tw.KINDS)
@pytest.mark.parametrize("R", ROWS_ONE)
def test_one_problem_at_every_short_row_count(R, kind):
    _check("one %s R=%d" % (kind, R), kind, 1, R, 128, 128)


@pytest.mark.parametrize("kind", tw.KINDS)
@pytest.mark.parametrize("R", ROWS_LONG)
def test_one_problem_at_the_row_counts_of_the_refill(R, kind):
    """chunk = 128 and 256: the request sets are refilled (once, then repeatedly)."""
    _check("one %s R=%d" % (kind, R), kind, 1, R, 128, 128)


@pytest.mark.parametrize("kind", ["main", "blocks"])
@pytest.mark.parametrize("nprob,R", [(n, R) for n in sorted(ROWS_MULTI) for R in ROWS_MULTI[n]])
def test_many_problems_with_full_and_dead_xcd_slots(nprob, R, kind):
    """Distinct operands per problem (on `blocks` distinct block scales as well): a result written to another problem's
    output or taken from another chunk is far outside the bound."""
    _check("multi %s nprob=%d R=%d" % (kind, nprob, R), kind, nprob, R, 128, 128, db="mixed")


@pytest.mark.parametrize("kind", tw.KINDS)
@pytest.mark.parametrize("M,N", WIDTHS_OPS)
def test_every_block_count_through_ops(M, N, kind):
    for R in (97, 513):
        _check("ops %s M=%d N=%d R=%d" % (kind, M, N, R), kind, 3 if kind in ("blocks", "zeros") else 1, R, M, N)


@pytest.mark.parametrize("kind", tw.KINDS)
@pytest.mark.parametrize("M,N", WIDTHS_ABI)
def test_widths_that_are_no_multiple_of_32_through_the_c_abi(M, N, kind):
    """Columns past M / N inside lda / ldb are NaN: the kernel clamps its loads to the last column and zeroes what it
    loaded there; dW has NaN columns past N inside ldw that keep their bits."""
    for R in (33, 97, 513):
        _check("abi %s M=%d N=%d R=%d" % (kind, M, N, R), kind, 3 if kind in ("blocks", "zeros") else 1, R, M, N, how=12,
               abi=True)


@pytest.mark.parametrize("kind", tw.KINDS)
@pytest.mark.parametrize("name", sorted(tw.FORMS))
def test_every_launch_form_of_the_catalogue(name, kind):
    f = tw.FORMS[name]
    rows = ROWS_FORMS + ((rows_256(f["nprob"]),) if f["nprob"] >= 2 else ())
    for R in rows:
        _check("form %s %s R=%d" % (name, kind, R), kind, f["nprob"], R, f["M"], f["N"], db=f["db"],
               how="slice" if f["wide"] else 0, accumulate=f["accumulate"], dyn=f["dyn"])


@pytest.mark.parametrize("kind", ["main", "rising", "zeros"])
def test_three_bf16_pieces_meet_their_own_bound(kind, monkeypatch):
    """GEOSSL_ARITH_24BIT (read per call): k_wgrad_split<., ., PlainOps, 3>."""
    monkeypatch.setenv("GEOSSL_ARITH_24BIT", "1")
    for nprob, R, M, N in ((1, 33, 128, 128), (1, 513, 128, 128), (1, 97, 64, 32), (3, 22050, 128, 128),
                           (1, 32641, 128, 128)):
        _check("bf16x3 %s nprob=%d R=%d M=%d N=%d" % (kind, nprob, R, M, N), kind, nprob, R, M, N, db="mixed", pieces=3)


# ---------------------------------------------------------------------------------------------------------- accumulate
@pytest.mark.parametrize("nprob,R", [(1, 97), (3, 513), (12, 5410)])
def test_two_accumulating_rounds_into_prefilled_outputs(nprob, R):
    """Outputs prefilled with entries up to 2^10 times the product's, then two accumulating launches into them (the
    tape's rounds): each round is held to the twin with the contents it found as the prior."""
    M = N = 128
    chunk, _ = tw.plan(R, nprob)
    given = tw.db_given("mixed", nprob)
    first = tw.operands("main", nprob, R, M, N, chunk, seed=1)
    L = Launch(first, R, M, N, given, how="slice", accumulate=True, prior=tw.priors(first, M, N, given, seed=1))
    outs = L.outputs()
    before = [(w.clone(), None if b is None else b.clone()) for w, b in zip(outs[0], outs[1])]
    L.fire(outs)
    _compare("accumulate round 1 nprob=%d R=%d" % (nprob, R),
             tw.wgrad(list(zip(L.A, L.B)), R, M, N, chunk, prior=before), outs[0], outs[1], 2)
    second = tw.operands("blocks", nprob, R, M, N, chunk, seed=2)
    L2 = Launch(second, R, M, N, given, how="slice", accumulate=True)
    before = [(w.clone(), None if b is None else b.clone()) for w, b in zip(outs[0], outs[1])]
    L2.fire(outs)
    _compare("accumulate round 2 nprob=%d R=%d" % (nprob, R),
             tw.wgrad(list(zip(L2.A, L2.B)), R, M, N, chunk, prior=before), outs[0], outs[1], 2)
    _assert_guards(outs[2], "accumulate")


# ------------------------------------------------------------------------------------------------ device-side row count
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("nprob,cap", [(1, 700), (3, 22050)])
def test_device_side_row_count(nprob, cap, accumulate):
    """A launch sized for `cap` rows whose real count is device data: rows past the count are NaN on both operands.  The
    results are within the bound of the twin over the real rows and bit-equal to the by-value launch of the same plan on
    operands whose rows past the count are zero, and to the by-value launch over exactly the real rows where that one
    has the same plan (an empty trailing chunk is a zero summand of the compensated sum, which applies the pending
    compensation: not the same bits).  Count 0 with accumulate: the outputs come back bit-unchanged."""
    M = N = 128
    chunk, nblk = tw.plan(cap, nprob)
    given = tw.db_given("mixed", nprob)
    probs = tw.operands("main", nprob, cap, M, N, chunk, seed=3)
    prior = tw.priors(probs, M, N, given, seed=3) if accumulate else None
    for count in (cap - 1, cap - 33, cap - chunk, 0, cap + 5):
        n = min(count, cap)
        where = "dyn nprob=%d cap=%d count=%d acc=%s" % (nprob, cap, count, accumulate)
        poisoned, zeroed = [], []
        for A, B in probs:
            Ap, Bp, Az, Bz = A.clone(), B.clone(), A.clone(), B.clone()
            Ap[n:], Bp[n:], Az[n:], Bz[n:] = float("nan"), float("nan"), 0.0, 0.0
            poisoned.append((Ap, Bp))
            zeroed.append((Az, Bz))
        L = Launch(poisoned, cap, M, N, given, accumulate=accumulate, prior=prior, count=count)
        dWs, dbs, _ = L.fire()
        if n == 0:
            for z in range(nprob):
                w0, b0 = L.prior[z] if accumulate else (torch.zeros(M, N, device=DEV), torch.zeros(M, device=DEV))
                assert torch.equal(dWs[z].view(torch.int32), w0.view(torch.int32)), where
                if dbs[z] is not None:
                    assert torch.equal(dbs[z].view(torch.int32), b0.view(torch.int32)), where
            continue
        ref = tw.wgrad([(a[:n], b[:n]) for a, b in zip(L.A, L.B)], n, M, N, chunk, prior=L.prior)
        _compare(where, ref, dWs, dbs, 2)
        same = Launch(zeroed, cap, M, N, given, accumulate=accumulate, prior=prior).fire()
        for a, b in zip(_flat(dWs, dbs), _flat(*same[:2])):
            assert torch.equal(a, b), where
        if tw.plan(n, nprob) == (chunk, nblk):
            exact = Launch([(a[:n], b[:n]) for a, b in probs], n, M, N, given, accumulate=accumulate, prior=prior).fire()
            for a, b in zip(_flat(dWs, dbs), _flat(*exact[:2])):
                assert torch.equal(a, b), where


# ------------------------------------------------------------------------------------------------ the workspace's size
@pytest.mark.parametrize("nprob,R", [(1, 65), (1, 512), (1, 513), (3, 97), (3, 22529), (32, 3618)])
def test_nothing_is_written_past_the_workspace(nprob, R):
    """The partial sums of every (problem, chunk) fit geossl_tn_workspace_floats: a NaN-filled tail behind it keeps its
    bits (a block of a dead XCD slot that ran would leave its partial there)."""
    from geossl_amd import _lib
    M = N = 128
    chunk, nblk = tw.plan(R, nprob)
    probs = tw.operands("main", nprob, R, M, N, chunk, seed=4)
    nfl = _lib.load().geossl_tn_workspace_floats(R, M, N, nprob)
    assert nfl == nprob * nblk * (M * N + 2 * M)
    tail = 2 * M * N + 4 * M
    ws = _nan(nfl + tail)
    tb = _lib.TnBatch()
    keep = []
    for i, (A, B) in enumerate(probs):
        A, B, dW, db = A.to(DEV), B.to(DEV), _nan(M, N), _nan(M)
        keep.append((A, B, dW, db))
        tb.A[i], tb.B[i], tb.dW[i], tb.db[i] = _lib.ptr(A), _lib.ptr(B), _lib.ptr(dW), _lib.ptr(db)
    _lib.call("geossl_linear_wgrad", C.byref(tb), nprob, R, M, N, M, N, N, _lib.ptr(ws), 0, _lib.stream())
    torch.cuda.synchronize()
    assert bool((ws[nfl:].view(torch.int32) == NAN_BITS).all())
    ref = tw.wgrad([(a, b) for a, b, _, _ in keep], R, M, N, chunk)
    _compare("workspace nprob=%d R=%d" % (nprob, R), ref, [k[2] for k in keep], [k[3] for k in keep], 2)


# ----------------------------------------------------------------------------------------------------- the plain order
PLAIN_CASES = ((3, 97), (3, 22529), (18, 5666), (32, 2049), (32, 3618))


def _plain_order_outputs():
    out = []
    for nprob, R in PLAIN_CASES:
        chunk, _ = tw.plan(R, nprob)
        probs = tw.operands("blocks", nprob, R, 128, 128, chunk, seed=5)
        dWs, dbs, _ = Launch(probs, R, 128, 128, tw.db_given("mixed", nprob)).fire()
        out.append([t.cpu() for t in _flat(dWs, dbs)])
    torch.cuda.synchronize()
    return out


def test_plain_block_order_gives_the_same_bits(tmp_path):
    """GEOSSL_WGRAD_PLAIN_ORDER is read once per process: a fresh child runs the multi-problem cases with it set and
    saves its outputs; they equal this process's (XCD order) bit for bit."""
    here = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path / "plain.pt")
    code = ("import sys; sys.path[:0] = [%r, %r]; import torch; import test_gpu_wgrad_elementwise as g; "
            "torch.save(g._plain_order_outputs(), %r)" % (os.path.dirname(here), here, path))
    env = dict(os.environ, GEOSSL_WGRAD_PLAIN_ORDER="1")
    env.pop("GEOSSL_ARITH_24BIT", None)
    done = subprocess.run([sys.executable, "-c", code], env=env, timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert os.environ.get("GEOSSL_WGRAD_PLAIN_ORDER") is None
    plain, mine = torch.load(path), _plain_order_outputs()
    assert len(plain) == len(mine) == len(PLAIN_CASES)
    for case, a, b in zip(PLAIN_CASES, plain, mine):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert torch.equal(x, y), case


# -------------------------------------------------------------------------------------------- the catalogue is complete
def test_every_wgrad_form_the_models_launch_is_in_the_catalogue(monkeypatch):
    """One SchNet DDM step, one PaiNN bucket step and one eager PaiNN step, one train-on-forces tape step of each
    backbone, the InfoGraph head and the Supervised head at F = 256 with ops.linear_wgrad wrapped: every launch's
    signature must be an entry of FORMS."""
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import draw_noise, make_batch
    from helpers import product_ncsn, product_schnet, t
    import test_gpu_force_training as ft
    import test_gpu_infograph as ig
    import test_gpu_masked_painn_bucket as mp
    import test_gpu_supervised as sv
    from test_gpu_round2 import FULL
    seen = []
    wgrad0 = ops.linear_wgrad

    def wgrad1(problems, R, M, N, accumulate=False, lda=None, ldb=None, ldw=None, dyn_rows=None):
        wide = (lda or M) > M or (ldb or N) > N or (ldw or N) > N
        for lo in range(0, len(problems), tw.TN_MAX):
            part = problems[lo:lo + tw.TN_MAX]
            seen.append(tw.signature(M, N, wide, len(part), accumulate, tw.db_class([p[3] for p in part]),
                                     dyn_rows is not None))
        return wgrad0(problems, R, M, N, accumulate=accumulate, lda=lda, ldb=ldb, ldw=ldw, dyn_rows=dyn_rows)
    monkeypatch.setattr(ops, "linear_wgrad", wgrad1)
    marks = []
    b = make_batch(64, seed=5, mode="B")
    nz = draw_noise(b, seed=6)
    ncsn = lambda: (product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9))
    loss, _ = pg.do_DDM(pg.Args("schnet"), pg.Batch.from_numpy(b, DEV), product_schnet(FULL, DEV), None, 0.0, 0.3,
                        NCSN_models=ncsn(), noise={k: t(v, DEV) for k, v in nz.items()})
    loss.backward()
    marks.append(len(seen))
    B = 32
    sizes = mp._ragged(96, 31, lo=1, hi=48, mean=20.0, sd=8.0)
    ds = mp._dataset(sizes, 31)
    hb = mp._loader_handles(ds, B, 0.3)[0]
    nzp = mp._noise(hb.n_atoms, hb.n_super, B, 500)
    trainer = lambda graph: pg.DDMTrainer(mp._painn(), *ncsn(), lr=5e-4, model_3d="painn", use_graph=graph)
    trainer(True)._graph_fwd_bwd(hb, nzp)
    marks.append(len(seen))
    trainer(False)._fwd_bwd(mp._twin(ds, hb), nzp)
    marks.append(len(seen))
    ft.trainer_step("schnet_md17_B1")
    marks.append(len(seen))
    ft.trainer_step("painn_F128_R32")
    marks.append(len(seen))
    ig._check([5, 17, 1, 30, 9], 256, "mean", 3)
    marks.append(len(seen))
    sv._check([5, 17, 1, 30, 9], 256, True, "mean", "mse", 3)
    marks.append(len(seen))
    torch.cuda.synchronize()
    assert all(a < b for a, b in zip([0] + marks, marks)), marks       # every step did launch weight gradients
    print("wgrad forms launched: %s" % sorted(set(seen)))
    known = {tw.form_signature(f): name for name, f in tw.FORMS.items()}
    missing = sorted({sig for sig in seen if sig not in known})
    assert not missing, "weight-gradient forms launched by a model and absent from wgrad_twin.FORMS: %s" % (missing,)
    print("catalogue entries launched: %s" % sorted({known[sig] for sig in seen}))
