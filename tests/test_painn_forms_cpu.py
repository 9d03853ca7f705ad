"""CPU tests of what the GPU tests of PaiNN's forward forms and mixing kernels stand on (tests/test_gpu_painn_mma.py,
test_gpu_painn_atom.py, test_gpu_painn_mix.py): the mixing twin's backward is fp64 autograd of its forward, the constants
of the two forward forms and of the mixing kernels are the documented counts, the hand-made edge list has the group
layout the matrix-pipe kernel's cases need, and an fp32 emulation of that kernel's order of additions stays inside
c_fwd_mma of the fp64 twin (the bound can be met by a correct implementation)."""
import math

import numpy as np
import pytest
import torch

import painn_mix_twin as mx
import painn_mma_case as hc
import painn_tile_twin as tw
from elementwise import flagged


def _mix_inputs(N, F, seed, zero_rows=()):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c = dict(q=rnd(N, F), mu=rnd(N, 3, F), mm=rnd(N, 3, 2 * F), xx=rnd(N, 3 * F), gq=rnd(N, F), gm=rnd(N, 3, F),
             dctx=rnd(N, 2 * F))
    for r in zero_rows:
        c["mm"][r, :, :F] = 0.0                                 # mu_V = 0 exactly: |V| = sqrt(eps)
    return c


@pytest.mark.parametrize("null_forms", [False, True], ids=["general", "null"])
@pytest.mark.parametrize("eps", [1e-8, 0.25])
def test_mixing_twin_backward_is_autograd_of_its_forward(null_forms, eps):
    N, F = 7, 5
    c = _mix_inputs(N, F, 11, zero_rows=(2, 6))
    q, mu, mm, xx = (c[k].clone().requires_grad_(True) for k in ("q", "mu", "mm", "xx"))
    V, W = mm[:, :, :F], mm[:, :, F:]
    ctx = torch.cat([q, torch.sqrt((V * V).sum(1) + eps)], dim=1)                      # painn.py:101-104
    dot = (V * W).sum(1)                                                               # :110
    q_out = q + xx[:, :F] + xx[:, 2 * F:] * dot                                        # :107-112
    mu_out = mu + xx[:, None, F:2 * F] * W                                             # :113
    loss = (q_out * c["gq"]).sum() + (ctx * c["dctx"]).sum()
    if not null_forms:                                          # (NULL dmu_new: mu' is nobody's input, its gradient zero)
        loss = loss + (mu_out * c["gm"]).sum()
    loss.backward()
    pre = mx.pre_fwd(c["q"], c["mm"], eps)
    assert torch.allclose(pre["ctx_q"][0], ctx[:, :F].detach()) and torch.allclose(pre["ctx_n"][0], ctx[:, F:].detach())
    assert torch.equal(pre["ctx_n"][0][2], torch.full((F,), math.sqrt(eps), dtype=torch.float64))
    assert torch.allclose(pre["dot"][0], dot.detach(), rtol=1e-13, atol=1e-13)
    fw = mx.post_fwd(c["q"], c["mu"], c["mm"], c["xx"], pre["dot"][0], with_mu_out=not null_forms)
    assert torch.allclose(fw["q_out"][0], q_out.detach(), rtol=1e-13, atol=1e-13)
    assert ("mu_out" in fw) == (not null_forms)
    if not null_forms:
        assert torch.allclose(fw["mu_out"][0], mu_out.detach(), rtol=1e-13, atol=1e-13)
    ctx_ref = torch.cat([pre["ctx_q"][0], pre["ctx_n"][0]], dim=1)
    pb = mx.post_bwd(c["gq"], None if null_forms else c["gm"], c["mm"], c["xx"], pre["dot"][0])
    rb = mx.pre_bwd(c["gq"], c["dctx"], ctx_ref, c["mm"], pb["dmm_V_post"])
    dxx = torch.cat([pb["dxx_0"][0], pb["dxx_1"][0], pb["dxx_2"][0]], dim=1)
    dmm = mx.pack_dmm(rb["dmm_V"][0], pb["dmm_W"][0])
    assert torch.allclose(dxx, xx.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dmm, mm.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(rb["dq_in"][0], q.grad, rtol=1e-12, atol=1e-12)
    assert bool(torch.isfinite(dmm).all()) and bool((rb["term_V_norm"][2] == 0).all())   # the eps-dominated rows
    if null_forms:
        assert mu.grad is None and bool((pb["dxx_1"][0] == 0).all())
    # every magnitude sum bounds its value; the parts of dmm_W and dmm_V add up
    for part in (pre, fw, pb, rb):
        for name, v in part.items():
            if isinstance(v, tuple):
                assert bool((v[0].abs() <= v[1] * (1 + 1e-12)).all()), name
    assert torch.allclose(pb["term_W_gm"] + pb["term_W_dot"], pb["dmm_W"][0])
    assert torch.allclose(pb["dmm_V_post"][0] + rb["term_V_norm"], rb["dmm_V"][0])


def test_constants_are_the_documented_counts():
    assert tw.U == 2.0 ** -22 and tw.U24 == 2.0 ** -24 and mx.U == 2.0 ** -24
    assert tw.c_fwd_mma(17) == 16.0 and tw.c_fwd_mma(43) == 24.0
    assert tw.c_fwd_mma(0) == 9 + 1.25 + 0.25 and tw.c_fwd_mma(33) == 9 + 1.25 + (33 + 9 + 1) / 4
    assert tw.c_fwd_atom(20, 70) == 96.0 and tw.c_fwd_atom(32, 70) == 108.0 and tw.c_fwd_atom(8, 0) == 14.0
    assert mx.C == dict(ctx_q=0.0, ctx_n=7.0, dot=5.0, q_out=3.0, mu_out=2.0, dxx_0=0.0, dxx_1=6.0, dxx_2=1.0,
                        dmm_V_post=2.0, dmm_W=4.0, dq_in=1.0, dmm_V=5.0)
    assert mx.C["dmm_V"] == mx.C["dmm_V_post"] + 3


def test_build_line_has_no_fast_math():
    """Division and square root count one rounding each only while hipcc's default (correctly rounded) holds."""
    import inspect
    from geossl_amd import build
    src = inspect.getsource(build)
    assert "-O3" in src
    for flag in ("fast-math", "-Ofast", "correctly-rounded-divide-sqrt", "unsafe-math", "-ffp-model"):
        assert flag not in src, flag


def test_hand_made_edge_list_has_the_groups_the_cases_need():
    ei, batch = hc.edges()
    deg_lists = hc.degrees()
    N = sum(hc.SIZES)
    deg = np.bincount(ei[0], minlength=N)
    assert np.array_equal(deg, np.concatenate(deg_lists)) and deg.max() == hc.MAX_DEGREE
    assert set(hc.REQUIRED_DEGREES) <= set(deg[:44].tolist())
    assert np.array_equal(batch[ei[0]], batch[ei[1]]) and bool((np.diff(batch[ei[0]]) >= 0).all())   # inside, in batch order
    row_edge, code, grp_ptr, mol_grp = hc.groups_np(ei, hc.SIZES)
    per_mol = np.diff(mol_grp)
    assert 0 in (per_mol % 8).tolist() and 1 in (per_mol % 8).tolist()
    first, last = grp_ptr[:44] - mol_grp[0], grp_ptr[1:45] - 1 - mol_grp[0]                # groups inside the molecule
    assert any(f // 8 != l // 8 for f, l in zip(first, last))                               # a run crosses a tile's end
    assert any(l % 8 == 7 and f // 8 == l // 8 for f, l in zip(first, last))                # a run ends with its tile
    # every edge sits once in its target's rows, padding is -1, an atom without edges has one empty group
    assert sorted(row_edge[row_edge >= 0].tolist()) == list(range(ei.shape[1]))
    own = np.repeat(code >> 1, 4)
    assert bool((ei[0][row_edge[row_edge >= 0]] == own[row_edge >= 0]).all())
    assert int((code & 1).sum()) == N


@pytest.mark.parametrize("R", [8, 20])
def test_fp32_emulation_of_the_group_order_stays_inside_c_fwd_mma(R):
    ei, _ = hc.edges()
    E, N, F = ei.shape[1], sum(hc.SIZES), 16
    g = torch.Generator().manual_seed(R)
    rnd = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    dirv = rnd(E, 3)
    dirv = dirv / dirv.norm(dim=1, keepdim=True)
    c = dict(q=rnd(N, F), mu=rnd(N, 3, F), xc=rnd(N, 3 * F), phi=torch.rand(E, R, generator=g),
             fcut=torch.rand(E, generator=g), dirv=dirv, Wf=rnd(3 * F, R, scale=0.3), bf=rnd(3 * F, scale=0.2))
    ref = tw.forward(c["q"], c["mu"], c["xc"], torch.from_numpy(ei[0]), torch.from_numpy(ei[1]), c["phi"], c["fcut"],
                     c["dirv"], c["Wf"], c["bf"])
    n = {k: v.numpy() for k, v in c.items()}
    q_out, mu_out = hc.emulate_fwd_mma(n["q"], n["mu"], n["xc"], ei, hc.SIZES, n["phi"], n["fcut"], n["dirv"], n["Wf"], n["bf"])
    cc = tw.c_fwd_mma(hc.MAX_DEGREE)
    for name, got in (("q_out", q_out), ("mu_out", mu_out)):
        r, S = ref[name]
        got = torch.from_numpy(got)
        assert int(flagged(got, r, S, cc, tw.U).sum()) == 0, name
        worst = float(((got.double() - r).abs()[S > 0] / (tw.U * S[S > 0])).max())
        assert 0 < worst < cc
    # the two parts of terms_mu add up to it, and dropping the mu_j part of one edge is far outside the bound
    assert torch.equal(ref["terms_mu_r"] + ref["terms_mu_m"], ref["terms_mu"])
    r, S = ref["mu_out"]
    e = int(ref["terms_mu_m"].abs().sum((1, 2)).argmax())
    r2 = r.clone()
    r2[int(ei[0][e])] -= ref["terms_mu_m"][e]
    assert int(flagged(torch.from_numpy(mu_out), r2, S, cc, tw.U).sum()) > 0
