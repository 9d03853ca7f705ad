"""geossl_linear_chain (csrc/chain.hip) through ops.prepare_chain / ops.linear_chain against the fp64 twin
(tests/chain_twin.py), element by element: every form of the twin's catalogue FORMS, both weight layouts, at the row
counts where the launch changes shape, on five kinds of operands.

F = 128 (k_row_chain_cu, a block takes runs of up to three row blocks): 1, 31, 32, 33 rows; 16384 (512 row blocks, every
run 1), 16411 (513: block 0 runs 2, the last row block partial), 49152 (every run 3), 49177 (1537 row blocks on 513
blocks: runs of 3 and 2, last partial).  F = 64 / 32 (k_row_chain8, rounds of 5 x grid row blocks, the fifth shared by
four team waves): 1, 33, 128 (team waves idle), 157 (team waves on a partial row block), 192, 320, 40960 (one full
round of 256 blocks), 40983 (a second round with one live, partial, regular row block), 73824 (a second round whose team
waves are live on three blocks).
Operands: `main` (randn); `blocks` (the 32-output-column blocks of every weight scaled by 2^{0, 7, -9, 3}, permuted per
stage: the four weight exponents of a stage differ in both layouts); `rows` (row magnitudes 2^-12 .. 2^12 inside every
row block, one 32-column group of each row 2^10 above the rest); `zeros` (all-zero input rows, an all-zero weight block,
rows whose first result is exactly zero so that the next row scale sits at its floor); `slices` (every row-shaped
operand a column slice of a NaN-filled [R + 128, 3 F] tensor that must stay bit-unchanged around the slice).
Every case checks |got - ref| <= c u S on every stored result, launches elementwise.REPEATS times without a differing
element, and on `main` and `blocks` proves that one removed product term (add_prev summand, res summand, silu hand-on)
is flagged in exactly one element.  c comes from the twin's arithmetic model (tests/test_chain_twin_cpu.py), the
worst err / (u S) measured here is printed and recorded in DESIGN.md section 4."""
import pytest
import torch

import chain_twin as tw
from elementwise import assert_repeatable, assert_sees_a_dropped_term, assert_within
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC00000
GUARD = 64
ROWS_128 = (1, 31, 32, 33, 16384, 16411, 49152, 49177)
ROWS_128_SHORT = (33, 16411)
ROWS_STREAM = (1, 33, 128, 157, 192, 320, 40960, 40983, 73824)
EVERY_ROW_COUNT = tw.LONGEST + (tw.SCHNET3,)
CASES = [(F, name, transB, kind) for F in (128, 64, 32) for name in tw.FORMS[F] for transB in (True, False)
         for kind in tw.KINDS]


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The worst err / (u S) per family over the cases that ran (what DESIGN.md section 4 records)."""
    yield
    for k in sorted(WORST):
        print("worst err/(u S)  %-12s %8.3f  at %s" % ((k,) + WORST[k]))


def note(family, got, ref, S, u, where, extra=0.0):
    """err / (u S) of a tensor, recorded before it is asserted on."""
    err = ((got.double() - ref).abs() - extra).clamp_min(0.0)
    r = torch.where(S > 0, err / (u * S), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = float(r.max()) if r.numel() else 0.0
    if family not in WORST or not r <= WORST[family][0]:
        WORST[family] = (r, where)
    return r


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _wide(t, R, F, col):
    """A NaN-filled [R + 2 GUARD, 3 F] tensor and its [R, F] slice behind GUARD rows at column block `col` (holding t)."""
    base = _nan(R + 2 * GUARD, 3 * F)
    view = base[GUARD:GUARD + R, col * F:(col + 1) * F]
    if t is not None:
        view.copy_(t)
    return base, view


def _prepare(F, X, stages, sliced):
    """Operand images and the input side of the stage dicts; `sliced`: every row-shaped input is a column slice."""
    from geossl_amd import ops
    R = X.size(0)
    place = (lambda t, col: _wide(t, R, F, col)[1]) if sliced else (lambda t, col: t)
    imgs = ops.prepare_chain([st["W"] for st in stages], transB=stages[0]["transB"])
    sds = []
    for st, img in zip(stages, imgs):
        sd = dict(image=img, flags=st["flags"], same_input=st["same_input"], store=st["store"])
        for key, col in (("res", 0), ("tprev", 2), ("x", 2)):
            if st[key] is not None:
                sd[key] = place(st[key], col)
        if st["bias"] is not None:
            sd["bias"] = st["bias"]
        if st["x"] is not None:
            sd["add_prev"] = st["add_prev"]
        sds.append(sd)
    return dict(F=F, R=R, x0=place(X, 1), sds=sds, stages=stages, sliced=sliced)


def _fire(prep, dyn=None):
    """One launch into fresh NaN-filled outputs: ([(out, out_act) per stage], [(base, slice) of every sliced output])."""
    from geossl_amd import ops
    F, R = prep["F"], prep["R"]
    outs, bases, sds = [], [], []
    for st, sd in zip(prep["stages"], prep["sds"]):
        sd = dict(sd)
        pair = []
        for key, want, col in (("out", st["store"], 1), ("out_act", st["out_act"], 2)):
            o = None
            if want:
                if prep["sliced"]:
                    base, o = _wide(None, R, F, col)
                    bases.append((base, o))
                else:
                    o = _nan(R, F)
                sd[key] = o
            pair.append(o)
        outs.append(tuple(pair))
        sds.append(sd)
    ops.linear_chain(prep["x0"], sds, dyn_rows=dyn)
    return outs, bases


def _flat(outs):
    return [o for pair in outs for o in pair if o is not None]


def _check_case(F, name, transB, kind, R):
    fam, u = tw.FAMILY[F], tw.U[F]
    c = tw.C_BOUND[fam]
    form = tw.FORMS[F][name]
    where = "F=%d %s transB=%s %s R=%d" % (F, name, transB, kind, R)
    X, stages = tw.operands(F, name, R, transB, "main" if kind == "slices" else kind, device=DEV)
    ref = tw.chain(X, stages)
    prep = _prepare(F, X, stages, kind == "slices")
    outs, bases = _fire(prep)
    checks = []
    for s, (o, oa) in enumerate(outs):
        if o is not None:
            checks.append((o, ref[s]["ref"], ref[s]["S"], 0.0, "%s stage %d" % (where, s)))
        if oa is not None:
            if ref[s]["ref_act"] is None:      # out_act of a stage without EPI_SILU is a copy of the result
                checks.append((oa, ref[s]["ref"], ref[s]["S"], 0.0, "%s stage %d act" % (where, s)))
            else:
                checks.append((oa, ref[s]["ref_act"], ref[s]["S_act"], tw.ACT_FLOOR, "%s stage %d act" % (where, s)))
    print("ratio %-10s %-60s %8.3f" % (fam, where, max(note(fam, g, r, S, u, w, e) for g, r, S, e, w in checks)))
    for g, r, S, e, w in checks:
        assert_within(g, r, S, c, u, w, extra=e if e else None)
    for base, view in bases:   # guard rows and neighbouring columns keep the bits they were filled with
        bits = base.view(torch.int32)
        assert int((bits != NAN_BITS).sum()) == int((view.view(torch.int32) != NAN_BITS).sum()), where
    if kind in ("main", "blocks"):
        for s, what, act, idx, term, r in tw.proofs(ref, form, F, c, u):
            w = "%s stage %d %s%s" % (where, s, what, " act" if act else "")
            assert r >= 2.0, (w, r)
            if act:
                assert_sees_a_dropped_term(outs[s][1], ref[s]["ref_act"], ref[s]["S_act"], c, u, idx, term, w,
                                           extra=tw.ACT_FLOOR)
            else:
                assert_sees_a_dropped_term(outs[s][0], ref[s]["ref"], ref[s]["S"], c, u, idx, term, w)
    assert_repeatable(lambda: _flat(_fire(prep)[0]), _flat(outs), where)


def _rows(F, name):
    if F != 128:
        return ROWS_STREAM
    return ROWS_128 if name in EVERY_ROW_COUNT else ROWS_128_SHORT


@pytest.mark.parametrize("F,name,transB,kind", CASES)
def test_chain_form_against_fp64_per_element(F, name, transB, kind):
    for R in _rows(F, name):
        _check_case(F, name, transB, kind, R)


@pytest.mark.parametrize("dyn", [0, 1, 700, 1024])
@pytest.mark.parametrize("transB", [True, False])
@pytest.mark.parametrize("name", [tw.LONGEST[0], tw.LONGEST[1], tw.SCHNET3])
def test_device_side_row_count(name, transB, dyn):
    """A launch sized for a capacity of 1024 rows whose real count is device data (bucket.DynDims): rows below the count
    are within the bound and bit-equal to the plain launch over exactly those rows; rows past it are NaN on every
    input and keep their bits on every output."""
    F, cap = 128, 1024
    fam, u = tw.FAMILY[F], tw.U[F]
    c = tw.C_BOUND[fam]
    X, stages = tw.operands(F, name, cap, transB, "main", device=DEV)
    keys = ("res", "tprev", "x")

    def rows(lo, hi, poison):
        out = []
        for st in stages:
            st = dict(st)
            for k in keys:
                if st[k] is not None:
                    st[k] = st[k][lo:hi].clone()
                    if poison:
                        st[k][dyn:] = float("nan")
            out.append(st)
        return out
    Xp = X.clone()
    Xp[dyn:] = float("nan")
    count = torch.tensor([dyn, 0, 0, 0], dtype=torch.int32, device=DEV)
    outs, _ = _fire(_prepare(F, Xp, rows(0, cap, True), False), dyn=count.data_ptr())
    for o in _flat(outs):
        assert bool((o[dyn:].view(torch.int32) == NAN_BITS).all()), (name, dyn)
    if dyn == 0:
        return
    live = rows(0, dyn, False)
    ref = tw.chain(X[:dyn], live)
    plain, _ = _fire(_prepare(F, X[:dyn].clone(), live, False))
    where = "F=128 %s transB=%s dyn=%d" % (name, transB, dyn)
    for s, (pair, ppair) in enumerate(zip(outs, plain)):
        for o, po, act in zip(pair, ppair, (False, True)):
            if o is None:
                continue
            sil = act and ref[s]["ref_act"] is not None
            r, S = (ref[s]["ref_act"], ref[s]["S_act"]) if sil else (ref[s]["ref"], ref[s]["S"])
            note(fam, o[:dyn], r, S, u, where, tw.ACT_FLOOR if sil else 0.0)
            assert_within(o[:dyn], r, S, c, u, "%s stage %d" % (where, s), extra=tw.ACT_FLOOR if sil else None)
            assert torch.equal(o[:dyn], po), (where, s, act)


# -------------------------------------------------------------------------------------------- the catalogue is complete
def _signature(x, stages, dyn):
    F = x.size(1)
    per = []
    for sd in stages:
        stored = sd.get("out") is not None or bool(sd.get("store", True))
        per.append((int(sd.get("flags", 0)), sd.get("bias") is not None, sd.get("res") is not None,
                    sd.get("tprev") is not None, stored, sd.get("out_act") is not None, sd.get("x") is not None,
                    bool(sd.get("same_input")), bool(sd.get("add_prev"))))
    wide = any(t is not None and t.stride(0) > F for sd in stages for t in
               (sd.get("out"), sd.get("res"), sd.get("tprev"), sd.get("out_act"), sd.get("x"))) or x.stride(0) > F
    return (F, tuple(per)), wide, dyn is not None


def test_every_chain_form_the_models_launch_is_in_the_catalogue(monkeypatch):
    """One SchNet step (full configuration, a small set-B batch), one eager PaiNN step and one PaiNN bucket step with
    ops.linear_chain and ops.layer_loop (whose chain operations run the same body) wrapped: every launch's signature - F,
    per stage flags and which of bias / res / tprev / out / out_act / x are present, same_input, add_prev - must be an
    entry of FORMS.  Wide row strides and device-side row counts are recorded as well: every entry of FORMS runs on
    `slices` operands, and the row count is applied before the body of any form (k_row_chain_cu, first line), so a
    form in the catalogue covers them; the test only requires that the models did exercise both."""
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import draw_noise, make_batch
    from helpers import product_ncsn, product_schnet, t
    import test_gpu_masked_painn_bucket as mp
    from test_gpu_round2 import FULL
    seen = []
    chain0, loop0 = ops.linear_chain, ops.layer_loop

    def chain1(x, stages, dyn_rows=None):
        seen.append(_signature(x, stages, dyn_rows))
        return chain0(x, stages, dyn_rows=dyn_rows)

    def loop1(ops_list, *a, **kw):
        done = loop0(ops_list, *a, **kw)
        if done:    # (else the caller launches the operations one by one: recorded there)
            seen.extend(_signature(op[1], op[2], None) for op in ops_list if op[0] == "chain")
        return done
    monkeypatch.setattr(ops, "linear_chain", chain1)
    monkeypatch.setattr(ops, "layer_loop", loop1)
    # SchNet, forward and backward
    b = make_batch(64, seed=5, mode="B")
    nz = draw_noise(b, seed=6)
    ncsn = lambda: (product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9))
    loss, _ = pg.do_DDM(pg.Args("schnet"), pg.Batch.from_numpy(b, DEV), product_schnet(FULL, DEV), None, 0.0, 0.3,
                        NCSN_models=ncsn(), noise={k: t(v, DEV) for k, v in nz.items()})
    loss.backward()
    n_schnet = len(seen)
    assert n_schnet > 0
    # PaiNN: a bucket step (capture of the bucket graph), then the eager step on the collated batch
    B = 32
    sizes = mp._ragged(96, 31, lo=1, hi=48, mean=20.0, sd=8.0)
    ds = mp._dataset(sizes, 31)
    hb = mp._loader_handles(ds, B, 0.3)[0]
    nzp = mp._noise(hb.n_atoms, hb.n_super, B, 500)
    trainer = lambda graph: pg.DDMTrainer(mp._painn(), *ncsn(), lr=5e-4, model_3d="painn", use_graph=graph)
    trainer(True)._graph_fwd_bwd(hb, nzp)
    n_bucket = len(seen)
    trainer(False)._fwd_bwd(mp._twin(ds, hb), nzp)
    torch.cuda.synchronize()
    assert n_schnet < n_bucket < len(seen)
    assert any(dyn for _, _, dyn in seen) and any(wide for _, wide, _ in seen)
    known = {tw.form_signature(F, form): name for F in tw.FORMS for name, form in tw.FORMS[F].items()}
    missing = sorted({sig for sig, _, _ in seen if sig not in known})
    assert not missing, "chain forms launched by a model and absent from chain_twin.FORMS: %s" % (missing,)
    print("chain forms launched: %s" % sorted({known[sig] for sig, _, _ in seen}))


# ------------------------------------------------------------------------------------ rows beyond 4 GB of byte offsets
@pytest.mark.parametrize("F,R", [(64, 2 ** 24 + 96), (128, 2 ** 23 + 96)])
def test_rows_whose_byte_offsets_pass_32_bits(F, R):
    """R * ld * 4 >= 2^32 with ld = ldx = F: both default forms compute row-piece offsets in 32 bits and run such an input
    as two launches of half the rows (launch_chain).  One stage, bias + SSP, on fully allocated tensors (a wrapped offset
    would still land inside them); the first and the last 4096 rows per element against the twin.  Without the split
    the rows from 2^32 / (4 ld) on are read AND stored at wrapped offsets: they recompute the first rows of `out` from
    the first rows of X, and the tail of `out` keeps its NaN fill (F = 64 before launch_chain split the eight-wave
    form: 6144 of the tail's elements, its last 96 rows)."""
    from geossl_amd import ops
    torch.cuda.empty_cache()
    fam, u = tw.FAMILY[F], tw.U[F]
    g = torch.Generator(device=DEV).manual_seed(F)
    X = torch.randn(R, F, generator=g, device=DEV)
    W = torch.randn(F, F, generator=g, device=DEV) / F ** 0.5
    bias = 0.1 * torch.randn(F, generator=g, device=DEV)
    out = _nan(R, F)
    img = ops.prepare_chain([W], transB=True)[0]
    ops.linear_chain(X, [dict(image=img, bias=bias, flags=tw.EPI_SSP, out=out)])
    parts = []
    for name, sl in (("head", slice(0, 4096)), ("tail", slice(R - 4096, R))):
        d = tw.chain(X[sl], [dict(W=W, transB=True, bias=bias, flags=tw.EPI_SSP)])[0]
        where = "F=%d R=2^%d+96 %s" % (F, 24 if F == 64 else 23, name)
        print("ratio %-10s %-60s %8.3f" % (fam, where, note(fam, out[sl], d["ref"], d["S"], u, where)))
        parts.append((out[sl], d, where))
    for got, d, where in parts:
        assert_within(got, d["ref"], d["S"], tw.C_BOUND[fam], u, where)
