"""The fp64 twins of the embedding, readout and row-normalize kernels (tests/row_twin.py) against torch autograd in
float64, the launch regimes the shapes of tests/test_gpu_row_kernels_elementwise.py are named for (row_twin.plan /
launch restate geossl_embedding_bwd_dyn), and the validity of that test's dropped-term proofs: on its seeded inputs the
term chosen for every case stands at least twice above the bound of its element, and the checker, given the reference
itself, flags that element alone."""
import math

import pytest
import torch
import torch.nn.functional as nnf

import row_twin as tw
from elementwise import assert_sees_a_dropped_term, flagged

TINY = 1e-13      # fp64 evaluations of the same expression in another order


def _same(a, b):
    return float((a - b).abs().max()) <= TINY * max(float(b.abs().max()), 1e-300) if a.numel() else a.shape == b.shape


# ------------------------------------------------------------------------------------------------- twins vs autograd
@pytest.mark.parametrize("accumulate", [False, True])
def test_embedding_twin_is_the_gradient_of_a_table_lookup(accumulate):
    C, F, N = 7, 5, 60
    g = torch.Generator().manual_seed(1)
    z = torch.randint(0, C - 1, (N,), generator=g)            # class C - 1 never present
    z[4], z[9], z[17], z[30] = -1, C, 2 ** 32 + 1, 2 ** 32 + 1
    dh = torch.randn(N, F, generator=g)
    prior = torch.randn(C, F, generator=g) if accumulate else None
    ref, S, c = tw.embedding_bwd(z, dh, C, N - 3, prior)      # the last three rows are past the real count
    ok = [a for a in range(N - 3) if 0 <= int(z[a]) < C]
    assert len(ok) == N - 3 - 4
    table = torch.zeros(C, F, dtype=torch.float64, requires_grad=True)
    (nnf.embedding(z[ok], table) * dh[ok].double()).sum().backward()
    want = torch.zeros(C, F, dtype=torch.float64).index_add_(0, z[ok], dh[ok].double())
    assert _same(table.grad, want)
    if accumulate:
        want = want + prior.double()
    assert _same(ref, want) and bool((S >= ref.abs() * (1 - TINY)).all())
    assert bool((ref[C - 1] == (prior[C - 1].double() if accumulate else 0.0)).all())
    assert bool((ref[1] == want[1]).all())                    # 2^32 + 1 is not class 1
    ng, nchunks = tw.plan(N, C, F)
    assert c == (math.ceil(math.ceil((N - 3) / nchunks) / ng) - 1) + (ng - 1) + 2 + 3 + int(accumulate)


@pytest.mark.parametrize("mean", [False, True])
def test_readout_twins_are_a_scatter_and_its_gradient(mean):
    mp = tw.seg_mol_ptr()
    sizes = torch.tensor(tw.SEG_SIZES)
    assert tw.SEG_SIZES[0] == 0 and tw.SEG_SIZES[-1] == 0 and int(mp[-1]) == int(sizes.sum())
    N, B, F = int(mp[-1]), len(tw.SEG_SIZES), 6
    g = torch.Generator().manual_seed(2)
    h = torch.randn(N, F, generator=g, dtype=torch.float64).requires_grad_()
    dout, prior = torch.randn(B, F, generator=g, dtype=torch.float64), torch.randn(N, F, generator=g, dtype=torch.float64)
    mol = tw.row_of_molecule(mp)
    out = torch.zeros(B, F, dtype=torch.float64).index_add(0, mol, h)
    if mean:
        out = out / sizes.clamp_min(1)[:, None]
    out.backward(dout)
    ref, S, c = tw.segment_reduce_fwd(h.detach(), mp, mean)
    assert _same(ref, out.detach()) and bool((ref[0] == 0).all()) and bool((ref[-1] == 0).all()) and bool((S[0] == 0).all())
    assert [float(v) for v in c[:, 0]] == [max(n - 1, 0) + int(mean) for n in tw.SEG_SIZES]
    gref, gS, gc = tw.segment_reduce_bwd(dout, mp, mean)
    assert gref.shape == (N, F) and _same(gref, h.grad) and gc == int(mean)
    if not mean:
        assert torch.equal(gref, dout[mol])
    aref, aS, ac = tw.segment_reduce_bwd(dout, mp, mean, prior)
    assert _same(aref, h.grad + prior) and ac == int(mean) + 1 and _same(aS, h.grad.abs() + prior.abs())


def test_row_normalize_twins_are_f_normalize_and_its_gradient():
    N, F, eps = 9, 11, 2.0 ** -40                              # (an eps that fp32 holds exactly)
    g = torch.Generator().manual_seed(3)
    h = torch.randn(N, F, generator=g, dtype=torch.float64)
    h[2], h[5], h[7] = 0.0, 1e-20, 3.0 * eps / math.sqrt(F)    # all zero; clamped; just above eps
    h = h.requires_grad_()
    gy = torch.randn(N, F, generator=g, dtype=torch.float64)
    y = nnf.normalize(h, dim=-1, eps=eps)
    y.backward(gy)
    ref, S, c = tw.row_normalize_fwd(h.detach(), eps)
    nr = tw.row_norm(h.detach(), eps)
    k = math.ceil(F / 64)
    assert _same(ref, y.detach()) and _same(nr[0][:, 0], h.detach().norm(dim=1)) and nr[2] == k + 7
    assert [float(v) for v in c[:, 0]] == [1.0 if r in (2, 5) else k + 8.0 for r in range(N)]
    assert float(nr[3][2]) == 0.0 and float(nr[0][2]) == 0.0
    dref, dS, dc = tw.row_normalize_bwd(gy, ref, nr[0], eps)
    assert _same(dref, h.grad)
    assert torch.equal(dref[2], gy[2] / eps) and torch.equal(dref[5], gy[5] / eps)
    assert [float(v) for v in dc[:, 0]] == [2.0 if r in (2, 5) else k + 10.0 for r in range(N)]
    # S holds the terms of the cancellation, not its result
    assert bool((dS >= dref.abs() * (1 - TINY)).all())
    assert _same(dS[0], (gy[0].abs() + ref[0].abs() * (gy[0] * ref[0]).abs().sum()) / nr[0][0])


# ---------------------------------------------------------------------------------------------------- launch regimes
def test_plan_group_counts():
    """The five group plans of the GPU test: (ng, threads per block).  700 rows: four groups stand on the floor of 16
    chunks (6 chunks of 128 rows wanted), one group takes 22 chunks of 32 rows, rounded to 24."""
    want = {(9, 128): (4, 512), (100, 128): (1, 128), (9, 256): (4, 1024), (13, 256): (1, 256), (9, 48): (4, 256)}
    for (C, F), (ng, threads) in want.items():
        L = tw.launch(700, C, F, 700)
        assert (L["ng"], L["threads"], L["nchunks"], L["refused"]) == (ng, threads, 16 if ng == 4 else 24, False), (C, F)
        assert tw.EMB_BWD["plan C=%d F=%d" % (C, F)]["N"] == 700
    assert 4 * 100 * 128 * 4 > 48 * 1024                       # PaiNN's table: four group tables do not fit
    assert 4 * 12 * 256 * 4 <= 48 * 1024 < 4 * 13 * 256 * 4    # F = 256: one group from 13 classes on
    assert tw.plan(700, 12, 256)[0] == 4


def test_plan_row_counts():
    L = lambda N, C=9, real=None: tw.launch(N, C, 128, N if real is None else real)
    p = L(0)
    assert (p["nchunks"], p["per"], p["used"], p["empty"]) == (16, 0, 0, 16)
    p = L(1)
    assert (p["nchunks"], p["per"], p["used"], p["empty"]) == (16, 1, 1, 15)
    p = L(700)
    assert (p["nchunks"], p["per"], p["PER"]) == (16, 44, 4)                 # 6 chunks of 128 rows: the floor of 16
    assert L(2048)["nchunks"] == 16 and L(2176)["nchunks"] == 20
    p = L(2049)
    assert (p["nchunks"], p["per"], p["PER"], p["empty"]) == (20, 103, 5, 0)  # 17 chunks rounded to 20; PER below 64
    p = L(32768)
    assert (p["nchunks"], p["PER"], p["per"], p["empty"]) == (256, 64, 128, 0)  # the second ballot round: no lane
    p = L(32769)
    # one lane in the second round: chunks 64, 129, 194 hold rows, chunk 259 (slice 3's) is the one empty chunk
    assert (p["nchunks"], p["PER"], p["per"], p["used"], p["empty"]) == (260, 65, 127, 259, 1)
    assert L(65536)["nchunks"] == 512 and L(65536)["per"] == 128 and L(65536)["empty"] == 0
    p = L(65537)
    assert (p["nchunks"], p["PER"], p["per"], p["used"], p["empty"]) == (512, 128, 129, 509, 3)   # capped: 513 wanted
    # the one-group plan: 32 rows per chunk
    p = L(8192, 100)
    assert (p["ng"], p["nchunks"], p["PER"]) == (1, 256, 64)
    p = L(8193, 100)
    assert (p["ng"], p["nchunks"], p["PER"], p["per"], p["used"]) == (1, 260, 65, 32, 257)   # chunks 64, 129, 194 live
    p = L(16385, 100)
    assert (p["ng"], p["nchunks"], p["PER"], p["per"], p["used"], p["empty"]) == (1, 512, 128, 33, 497, 15)
    # a device-side count: the chunks come from the capacity, the rows per chunk from the count
    p = L(8203, real=5000)
    assert (p["nchunks"], p["per"], p["used"]) == (68, 74, 68)


def test_every_embedding_case_is_in_the_regime_its_name_claims():
    regime = {"rows 0": (16, 0), "rows 1": (16, 1), "rows 2049": (20, 103), "rows 32768": (256, 128),
              "rows 32769": (260, 127), "rows 65537": (512, 129), "one group rows 8193": (260, 32),
              "one group rows 16385": (512, 33), "dyn 5000 of 8203": (68, 74)}
    for name, s in tw.EMB_BWD.items():
        L = tw.launch(s["N"], s["C"], s["F"], s["N"] if s["dyn"] is None else s["dyn"])
        assert not L["refused"] and L["lds"] <= tw.LDS_LIMIT and L["threads"] <= 1024, name
        assert L["ng"] == (1 if "one group" in name or (s["C"], s["F"]) in ((100, 128), (13, 256)) else 4), name
        if name in regime:
            assert (L["nchunks"], L["per"]) == regime[name], name
    c = tw.emb_bwd_case("one chunk, one absent")
    per = c["launch"]["per"]
    rows = (c["z"] == tw.ONE_CHUNK_CLASS).nonzero().reshape(-1)
    assert rows.numel() == 3 and {int(r) // per for r in rows} == {tw.ONE_CHUNK} and c["absent"] == [tw.ABSENT_CLASS]
    b = c["bands"]
    assert int((b[:, 1] == tw.ONE_CHUNK_CLASS).sum()) == 1 and int(b[tw.ONE_CHUNK, 1]) == tw.ONE_CHUNK_CLASS
    c = tw.emb_bwd_case("classes 1 and 8")
    assert c["absent"] == [0, 2, 3, 4, 5, 6, 7] and bool((c["bands"] == torch.tensor([1, 8])).all())
    c = tw.emb_bwd_case("sorted")                              # hit lists differ by class: no chunk holds every class
    assert int((c["bands"][:, 1] - c["bands"][:, 0]).max()) <= 1 and int(c["bands"][0, 0]) == 0 and int(c["bands"][-1, 1]) == 8
    c = tw.emb_bwd_case("rows 65537")
    assert bool((c["bands"][509:] == torch.tensor([9, -1])).all()) and bool((c["bands"][:509, 0] == 0).all())
    c = tw.emb_bwd_case("out of range")
    assert {int(v) for v in c["z"].unique() if not 0 <= int(v) < 9} == {-1, 9, 2 ** 32 + 1}
    c = tw.emb_bwd_case("dyn 5000 of 8203")
    assert bool(c["dh"][5000:].isnan().all()) and bool((c["z"][5000:] == 99).all()) and not bool(c["ref"].isnan().any())
    assert c["z_store"].shape == (8203, 1) and tw.emb_bwd_case("z stride 2")["z_store"].shape == (2049, 2)
    for s in (-20, 20):                                        # the scaled cases are the base case times a power of two
        assert torch.equal(tw.emb_bwd_case("dh 2^%d" % s)["dh"], tw.emb_bwd_case("rows 2049")["dh"] * 2.0 ** s)
        assert tw.emb_bwd_case("dh 2^%d" % s)["pick"][0] == tw.emb_bwd_case("rows 2049")["pick"][0]


def test_refused_launches():
    """F above 256, and a table whose launch would ask for more LDS than a CU has: 160 classes at F = 256 are 160 KB of
    table plus one 8-byte band."""
    assert tw.launch(33, 9, 257)["refused"] and not tw.launch(33, 9, 256)["refused"]
    L = tw.launch(33, 160, 256)
    assert L["ng"] == 1 and L["lds"] == 163848 and L["lds"] > tw.LDS_LIMIT and L["refused"]
    assert 160 * 256 * 4 == tw.LDS_LIMIT                       # the table alone is admitted by a check on the table
    assert not tw.launch(33, 159, 256)["refused"]
    assert tw.launch(2 ** 31, 9, 128)["refused"]


# ----------------------------------------------------------------------------------------------- dropped-term proofs
def _proof(ref, S, c, pick, what):
    """The chosen term stands at least twice above its element's bound, and the checker on the reference itself flags
    that element alone."""
    index, term, ratio = pick
    assert ratio >= 2.0, (what, index, term, ratio)
    assert int(flagged(ref, ref, S, c, tw.U).sum()) == 0, what
    assert_sees_a_dropped_term(ref, ref, S, c, tw.U, index, term, what)


@pytest.mark.parametrize("name", sorted(tw.EMB_BWD))
def test_embedding_dropped_term_stands_above_its_bound(name):
    c = tw.emb_bwd_case(name)
    if c["N_real"] == 0:
        assert c["pick"] is None and bool((c["S"] == (0 if c["prior"] is None else c["prior"].double().abs())).all())
        return
    _proof(c["ref"], c["S"], c["c"], c["pick"], name)
    assert 0 <= c["pick"][0][0] < c["C"]


@pytest.mark.parametrize("F", tw.SEG_F)
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
def test_readout_dropped_term_stands_above_its_bound(F, mean, accumulate):
    c = tw.seg_case(F, mean, accumulate)
    _proof(*c["fwd"], c["pick_fwd"], "fwd F=%d mean=%d" % (F, mean))
    _proof(*c["bwd"], c["pick_bwd"], "bwd F=%d mean=%d acc=%d" % (F, mean, accumulate))


@pytest.mark.parametrize("F", tw.RN_F)
@pytest.mark.parametrize("N", tw.RN_ROWS)
def test_row_normalize_dropped_term_stands_above_its_bound(N, F):
    c = tw.rn_case(N, F)
    what = "N=%d F=%d" % (N, F)
    for key in ("fwd", "bwd"):
        ref, S, cc = c[key]
        (r, f), term, ratio = c["pick_" + key]
        assert ratio >= 2.0 and r == c["drop_row"], (what, key, ratio)
        bad = flagged(ref, c["drop_" + key], S, cc, tw.U)
        assert bool(bad[r].any()) and int(bad.sum()) == int(bad[r].sum()), (what, key)
    _proof(*c["bwd"], c["pick_g"], what + " g term")
    if N in tw.RN_ZERO:
        y, S, cc = c["fwd"]
        zero, tiny, above = tw.RN_ZERO[N], tw.RN_TINY[N], tw.RN_ABOVE_EPS[N]
        e = tw.eps32(tw.EPS)
        assert bool((y[zero] == 0).all()) and float(cc[zero]) == 1 and float(cc[tiny]) == 1 and float(cc[above]) > 1
        assert float(c["norm"][0][tiny]) < e / 1e6 and 3.9 * e < float(c["norm"][0][above]) < 4.1 * e
        assert float(c["norm"][3][zero]) == 0 and float(c["norm"][3][tiny]) > 0
        # under the clamp the backward is g / eps on its own scale
        dref, dS, dc = c["bwd"]
        for r in (zero, tiny):
            assert float(dc[r]) == 2 and torch.equal(dref[r], c["g"][r].double() / e) and torch.equal(dS[r], dref[r].abs())
