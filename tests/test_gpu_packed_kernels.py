"""Kernels that hold packed-fp32 forms with a LOW result read from a HIGH half (tests/packed_opsel_registry.py), against
fp64 at full occupancy, element by element.

Round 6: `v_pk_mul_f32 .. op_sel:[0,1]` in the mu-zero k_painn_fwd_mma dropped one term in lanes 48-63 of
5-10 atoms per launch, only with two waves on a SIMD, on the same lanes launch after launch: a bit-reproducibility test
or a norm-based comparison at a small shape does not see that.  Each test here
- launches at the registry's shape and asserts the waves per SIMD that launch reaches on the built code object;
- checks |got - ref| <= c u S per element (NaN-prefilled outputs): ref the fp64 value, S the same fp64 expression on
  absolute values (sum of |terms|), u = 2^-22 for two-piece fp16 products, 2^-24 for fp32 arithmetic, c per family;
- proves it would see one missing term: drops one term from the fp64 reference (on lanes 48-63 where the layout has
  them) and asserts the checker flags exactly that element;
- launches eight times and counts the elements that differ between launches (must be 0)."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

import packed_opsel_registry as reg  # noqa: E402
from elementwise import (REPEATS, assert_repeatable, assert_sees_a_dropped_term, assert_within, flagged,  # noqa: E402,F401
                         pick_term)
from filter_twin import _filter_ref_and_bound  # noqa: E402
from ncsn_twin import KEYS as _NCSN_KEYS, _ncsn_ref_and_bound  # noqa: E402
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U22, U24 = 2.0 ** -22, 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------- helpers
_RES = {}


def assert_occupancy(symbol, label, lds=None, grid=None):
    """The launch the test makes (`lds`, `grid` from its actual data; the registry's where not given) reaches the waves
    per SIMD the registry states for it, on this build's code object."""
    import scan_packed_opsel as sp
    block, lds0, grid0, waves = reg.launch(symbol, label)
    lds, grid = lds0 if lds is None else lds, grid0 if grid is None else grid
    if not os.path.exists(sp.READELF):
        assert (lds, grid) == (lds0, grid0), (symbol, label)
        return waves
    if not _RES:
        from geossl_amd import _lib
        _RES.update(sp.resources(_lib.LIB_PATH))
    (k,) = [k for k in _RES if re.search(symbol, k)]
    got = sp.waves_per_simd(_RES[k], block, lds, grid)
    assert got == waves, (symbol, label, got, waves)
    return waves


# ----------------------------------------------------------------------------------------------- filter backward
@pytest.fixture(scope="module")
def filter_problems():
    from test_gpu_round2 import _filter_problem
    cache = {}

    def get(F):
        if F not in cache:
            G = {128: 51, 64: 20, 32: 8}[F]
            cache[F] = _filter_problem(nmol=reg.BENCH_MOLS, seed=21, F=F, G=G, L=reg.FILTER_L, mode="B")
        return cache[F]
    return get


@pytest.mark.parametrize("form", ["saved", "recompute", "bf16x3"])
@pytest.mark.parametrize("F", [32, 64, 128])
def test_filter_backward_at_full_occupancy_vs_fp64(F, form, filter_problems, monkeypatch):
    """geossl_cfconv_filter_bwd (k_filter_bwd_h<NW, T == NULL>, k_filter_bwd<NW> under GEOSSL_FILTER_BWD_BF16X3) on 1024
    molecules of set B: every weight-gradient element within 8 u S of fp64 (u = 2^-22; 2^-24 for the three-piece
    form), one pair's product dropped from dw2 seen, eight launches bit-identical."""
    lay, daggs, run, _ = filter_problems(F)
    run.lay = lay
    nw = F // 32
    if form == "bf16x3":
        monkeypatch.setenv("GEOSSL_FILTER_BWD_BF16X3", "1")
        symbol, lds, u = r"k_filter_bwdILi%dE" % nw, reg.filter_bwd_lds(F), U24
    else:
        monkeypatch.delenv("GEOSSL_FILTER_BWD_BF16X3", raising=False)
        monkeypatch.delenv("GEOSSL_ARITH_24BIT", raising=False)
        symbol, lds, u = r"k_filter_bwd_hILi%dELb%dE" % (nw, form == "recompute"), reg.filter_bwd_h_lds(F), U22
    ntiles = (run.inputs["P"] + 31) // 32
    assert ntiles >= 256
    assert_occupancy(symbol, "F=%d %s" % (F, form), lds=lds, grid=reg.filter_bwd_grid(reg.FILTER_L, ntiles))
    saved = form != "recompute"
    c = 8.0

    def launch():
        G = run.inputs["ws"][0][0].size(1)
        outs = [[torch.full((F, G), float("nan"), device=DEV), torch.full((F,), float("nan"), device=DEV),
                 torch.full((F, F), float("nan"), device=DEV), torch.full((F,), float("nan"), device=DEV)]
                for _ in range(reg.FILTER_L)]
        return [t for o in run(daggs, saved_T=saved, outs=outs) for t in o]

    got = launch()
    refs = _filter_ref_and_bound(run, daggs)
    for l, r in enumerate(refs):
        for k, name in enumerate(("dw1", "db1", "dw2", "db2")):
            assert_within(got[4 * l + k], r["ref"][k], r["S"][k], c, u, "layer %d %s" % (l, name))
    # one pair's product dO[p, f] T[p, g] dropped from dw2[f, g]: p in the last quarter of a 32-pair tile, f on lanes
    # 48-63 of a 64-unit block of hidden units
    r = refs[0]
    P = r["dO"].size(0)
    pairs = torch.arange(P, device=DEV)
    cand = pairs[(pairs % 32) >= 24][:4096]
    fsel = torch.arange(F, device=DEV)
    fsel = fsel[(fsel % 64) >= 48] if F >= 64 else fsel[fsel >= 16]
    terms = r["dO"][cand][:, fsel, None] * r["tt"][cand][:, None, :]                    # [p, f, g]
    bound = c * u * r["S"][2][fsel][None, :, :] + (got[2].double() - r["ref"][2]).abs()[fsel][None, :, :]
    k, ratio = pick_term(terms, bound, torch.ones_like(terms, dtype=torch.bool))
    assert ratio > 2.0, ("no single product stands above the bound", ratio)
    kp, kf, kg = np.unravel_index(k, terms.shape)
    assert_sees_a_dropped_term(got[2], r["ref"][2], r["S"][2], c, u, (int(fsel[kf]), int(kg)),
                               float(terms[kp, kf, kg]), "dw2 without pair %d" % int(cand[kp]))
    assert_repeatable(launch, got, "filter bwd F=%d %s" % (F, form))


# ------------------------------------------------------------------------------------------------------ NCSN heads
def _ncsn_problem(F, seed=5, K=50):
    from helpers import ncsn_oracle_params
    from geossl_amd.synthetic import make_batch
    b = make_batch(reg.BENCH_MOLS, seed=seed, mode="A")
    sei = torch.from_numpy(np.asarray(b["super_edge_index"])).long()
    batch = torch.from_numpy(np.asarray(b["batch"])).long()
    N, S = batch.numel(), sei.size(1)
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(N, F, generator=gen) * 0.5
    pos = torch.from_numpy(np.asarray(b["positions"], dtype=np.float32))
    dist = (pos[sei[0]] - pos[sei[1]]).norm(dim=-1, keepdim=True)
    nl = torch.randint(0, K, (reg.BENCH_MOLS,), generator=gen)
    dn = torch.randn(S, 1, generator=gen)
    P = ncsn_oracle_params(F, K)
    return dict(h=h.to(DEV), dist=dist.to(DEV), nl=nl.to(DEV), dn=dn.to(DEV), batch=batch.to(DEV), sei0=sei[0].contiguous().to(DEV),
                sei1=sei[1].contiguous().to(DEV), P={k: v.detach().to(DEV) for k, v in P.items()}, S=S)


@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("F", [32, 64, 128])
def test_ncsn_head_forward_at_full_occupancy_vs_fp64(F, heads):
    """geossl_ddm_loss_fwd (k_ncsn_fwd<F/32>) and geossl_ddm_loss_fwd2 (k_ncsn_fwd2<F/32>, two heads in one launch) on
    the bench batch (1024 molecules of set A, 156 672 super-edges): every loss_e within 16 u S of fp64 (u = 2^-24), one
    term of the last layer's dot product dropped seen, eight launches bit-identical."""
    import ctypes as C
    from geossl_amd import _lib
    from geossl_amd._lib import call, ptr, stream
    p = _ncsn_problem(F)
    S, power = p["S"], 2.0
    assert S == reg.NCSN_S
    NMB = F // 32
    if heads == 1:
        assert_occupancy(r"k_ncsn_fwdILi%dE" % NMB, "F=%d" % F, grid=reg.ncsn_fwd_grid(S))
    else:
        assert_occupancy(r"k_ncsn_fwd2ILi%dE" % NMB, "F=%d two heads" % F, grid=reg.ncsn_fwd2_grid(S))
    w = _lib.NcsnWeights()
    for name, k in zip(("in_w1", "in_b1", "in_w2", "in_b2", "o1_w", "o1_b", "o2_w", "o2_b", "o3_w", "o3_b"), _NCSN_KEYS):
        setattr(w, name, ptr(p["P"][k]))
    w.sigmas = ptr(p["P"]["sigmas"])
    nws = max(int(_lib.load().geossl_ddm_loss_fwd_workspace_floats(F)), 256)
    keep = []

    def launch():
        outs = [torch.full((S,), float("nan"), device=DEV) for _ in range(heads)]
        wss = [torch.empty(nws, device=DEV) for _ in range(heads)]
        keep.append(wss)
        if heads == 1:
            call("geossl_ddm_loss_fwd", ptr(p["h"]), ptr(p["batch"]), ptr(p["sei0"]), ptr(p["sei1"]), S, ptr(p["dist"]),
                 ptr(p["nl"]), ptr(p["dn"]), C.byref(w), F, power, ptr(outs[0]), None, ptr(wss[0]), stream())
        else:
            hs = (_lib.NcsnHeadFwd * 2)()
            for k in range(2):
                hs[k].h, hs[k].distance, hs[k].noise_level = ptr(p["h"]), ptr(p["dist"]), ptr(p["nl"])
                hs[k].distance_noise, hs[k].w, hs[k].anneal_power = ptr(p["dn"]), w, power
                hs[k].loss_e, hs[k].workspace = ptr(outs[k]), ptr(wss[k])
            call("geossl_ddm_loss_fwd2", C.byref(hs), ptr(p["batch"]), ptr(p["sei0"]), ptr(p["sei1"]), S, F, stream())
        torch.cuda.synchronize()
        return outs

    got = launch()
    ref, Sb, parts = _ncsn_ref_and_bound(p, power)
    c, u = 16.0, U24
    for k in range(heads):
        assert_within(got[k], ref, Sb, c, u, "loss_e head %d" % k)
    # drop the largest last-layer term of one super-edge on lanes 48-63 (rows of a 64-row wave tile)
    e = torch.arange(S, device=DEV)
    where = ((e % 64) >= 48)[:, None].expand_as(parts["last"])
    dl = parts["last"]   # d loss / d s = (s - t) sp: the loss without that term
    s2 = parts["s"][:, None] - dl
    dloss = 0.5 * (parts["s"][:, None] - parts["t"][:, None]) ** 2 * parts["sp"][:, None] - 0.5 * (s2 - parts["t"][:, None]) ** 2 * parts["sp"][:, None]
    bound = (c * u * Sb + (got[0].double() - ref).abs())[:, None].expand_as(dloss)
    kk, ratio = pick_term(dloss, bound, where)
    assert ratio > 2.0, ("no single term stands above the bound", ratio)
    ke = kk // dl.size(1)
    assert_sees_a_dropped_term(got[0], ref, Sb, c, u, (ke,), float(dloss.reshape(-1)[kk]), "loss_e without a term")
    assert_repeatable(launch, got, "ncsn fwd F=%d heads=%d" % (F, heads))


# --------------------------------------------------------------------------------------------------- PaiNN message
@pytest.fixture(scope="module")
def painn_cases():
    from test_gpu_round3 import _painn_edge_case
    from geossl_amd.synthetic import molecule_sizes
    cache = {}

    def get(molset, R):
        if (molset, R) not in cache:
            sizes = [18] * reg.BENCH_MOLS if molset == "A" else [int(n) for n in molecule_sizes(reg.BENCH_MOLS, "B")]
            assert max(sizes) <= reg.SET_B_MAX_N
            c = _painn_edge_case(sizes, seed=7, R=R)
            c["sizes"] = sizes
            cache.clear()                      # (one case alive at a time: the fp64 tensors are large)
            cache[(molset, R)] = c
        return cache[(molset, R)]
    return get


def painn_message64(c, q, mu, xc, Wf, bf, phi, fcut, dirv):
    """painn.py:54-64 in fp64: q_out = q + sum_e x0, mu_out = mu + sum_e (x1 dir + x2 mu[j]), [x0, x1, x2] = W_e * xc[j],
    W_e = (Wf phi_e + bf) fcut_e, e over the edges into each atom."""
    el, F = c["el"], reg.PAINN_F
    i, j = el.idx_i.long(), el.idx_j.long()
    W = (phi @ Wf.t() + bf) * fcut[:, None]
    x = W * xc[j]
    x0, x1, x2 = x[:, :F], x[:, F:2 * F], x[:, 2 * F:]
    dmu = x1[:, None, :] * dirv[:, :, None] + x2[:, None, :] * mu[j]
    return q.index_add(0, i, x0), mu.index_add(0, i, dmu), dict(W=W, x0=x0, x=x)


def _painn_inputs64(c, mu_zero=False, absolute=False):
    f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    mu = torch.zeros_like(c["mu"], dtype=torch.float64) if mu_zero else f(c["mu"])
    return dict(q=f(c["q"]), mu=mu, xc=f(c["xc"]), Wf=f(c["Wf"]), bf=f(c["bf"]), phi=f(c["phi"]), fcut=f(c["fcut"]),
                dirv=f(c["dirv"]))


@pytest.mark.parametrize("molset", ["A", "B"])
@pytest.mark.parametrize("R", [8, 16, 20, 32])
def test_painn_interaction_forward_at_full_occupancy_vs_fp64(R, molset, painn_cases):
    """geossl_painn_interaction_fwd_mol (k_painn_interaction_fwd_mol<R>) on 1024 molecules: q_out and mu_out within
    8 u S of fp64 (u = 2^-24: fp32 arithmetic), one edge's contribution to one atom dropped seen (a feature on lanes 48-63),
    eight launches bit-identical."""
    from geossl_amd import _lib
    c = painn_cases(molset, R)
    lay, el, N, F = c["lay"], c["el"], c["N"], reg.PAINN_F
    lds = reg.painn_fwd_mol_lds(lay.max_n, R)
    assert_occupancy(r"k_painn_interaction_fwd_molILi%dE" % R, "R=%d set %s" % (R, molset), lds=lds,
                     grid=reg.painn_fwd_mol_grid(lay.B, lds))
    inc_ptr, inc_idx = el.inc["i"]

    def launch():
        q_out, mu_out = torch.full_like(c["q"], float("nan")), torch.full_like(c["mu"], float("nan"))
        _lib.call("geossl_painn_interaction_fwd_mol", c["q"].data_ptr(), c["mu"].data_ptr(), c["xc"].data_ptr(),
                  el.idx_j.data_ptr(), inc_ptr.data_ptr(), inc_idx.data_ptr(), c["phi"].data_ptr(), c["fcut"].data_ptr(),
                  c["dirv"].data_ptr(), c["Wf"].data_ptr(), c["bf"].data_ptr(), lay.mol_ptr.data_ptr(), lay.B, lay.max_n,
                  N, F, R, q_out.data_ptr(), mu_out.data_ptr(), _lib.stream())
        torch.cuda.synchronize()
        return q_out, mu_out

    got = launch()
    q_ref, mu_ref, parts = painn_message64(c, **_painn_inputs64(c))
    Sq, Smu, _ = painn_message64(c, **_painn_inputs64(c, absolute=True))
    cc, u = 8.0, U24
    assert_within(got[0], q_ref, Sq, cc, u, "q_out")
    assert_within(got[1], mu_ref, Smu, cc, u, "mu_out")
    # one edge's x0 dropped from q_out[i, f], f on lanes 48-63
    i = el.idx_i.long()
    fl = torch.arange(F, device=DEV)
    lanes = (fl % 64) >= 48
    bound = cc * u * Sq[i] + (got[0].double() - q_ref).abs()[i]
    k, ratio = pick_term(parts["x0"], bound, lanes[None, :].expand_as(parts["x0"]))
    assert ratio > 2.0, ("no single edge stands above the bound", ratio)
    e, f = divmod(k, F)
    assert_sees_a_dropped_term(got[0], q_ref, Sq, cc, u, (int(i[e]), f), float(parts["x0"][e, f]), "q_out without edge %d" % e)
    assert_repeatable(launch, got, "painn fwd_mol R=%d set %s" % (R, molset))


_BWD_CASES = [("mol", R, mz, s) for R in (8, 16, 20) for mz in (False, True) for s in ("A", "B")] + \
             [("atom", R, False, "A") for R in (8, 16, 20, 32)]


@pytest.mark.parametrize("path,R,mu_zero,molset", _BWD_CASES,
                         ids=["%s-R%d-%s-set%s" % (p, R, "mu0" if mz else "general", s) for p, R, mz, s in _BWD_CASES])
def test_painn_interaction_backward_at_full_occupancy_vs_fp64(path, R, mu_zero, molset, painn_cases):
    """geossl_painn_interaction_bwd_mol (k_painn_interaction_bwd_mol<R, mu0>) and geossl_painn_interaction_bwd (the
    per-atom k_painn_interaction_bwd<R>, the product's form at n_rbf = 32) on 1024 molecules: dxc, dmu_in, dWf, dbf within
    8 u S of fp64 autograd (u = 2^-24), one edge's term of a filter-weight gradient dropped seen, eight launches identical."""
    from geossl_amd import _lib
    c = painn_cases(molset, R)
    lay, el, N, F, E = c["lay"], c["el"], c["N"], reg.PAINN_F, c["E"]
    lib = _lib.load()
    if path == "mol":
        lds = reg.painn_bwd_mol_lds(lay.max_n, R)
        assert_occupancy(r"k_painn_interaction_bwd_molILi%dELb%dE" % (R, mu_zero),
                         "R=%d %s set %s" % (R, "mu0" if mu_zero else "general", molset), lds=lds, grid=min(lay.B, 256))
        nws = int(lib.geossl_painn_interaction_bwd_mol_workspace_floats(N, lay.B, F, R))
    else:
        assert_occupancy(r"k_painn_interaction_bwdILi%dE" % R, "R=%d per atom" % R, grid=reg.painn_bwd_grid(N))
        nws = int(lib.geossl_painn_interaction_bwd_workspace_floats(N, F, R))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11 + R)
    dq_out = torch.randn(N, F, device=DEV, generator=gen)
    dmu_out = torch.randn(N, 3, F, device=DEV, generator=gen)
    inc_ptr, inc_idx = el.inc["j"]
    wsp = torch.empty(max(nws, 1), device=DEV)

    def launch():
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)
        dxc, dmu, dWf, dbf = nan(N, 3 * F), nan(N, 3, F), nan(3 * F, R), nan(3 * F)
        args = (dq_out.data_ptr(), dmu_out.data_ptr(), None if mu_zero else c["mu"].data_ptr(), c["xc"].data_ptr(),
                el.idx_i.data_ptr(), inc_ptr.data_ptr(), inc_idx.data_ptr(), c["phi"].data_ptr(), c["fcut"].data_ptr(),
                c["dirv"].data_ptr(), c["Wf"].data_ptr(), c["bf"].data_ptr())
        if path == "mol":
            _lib.call("geossl_painn_interaction_bwd_mol", *args, lay.mol_ptr.data_ptr(), lay.B, lay.max_n, N, F, R,
                      dxc.data_ptr(), None if mu_zero else dmu.data_ptr(), dWf.data_ptr(), dbf.data_ptr(), wsp.data_ptr(),
                      0, _lib.stream())
        else:
            _lib.call("geossl_painn_interaction_bwd", *args, N, F, R, dxc.data_ptr(), dmu.data_ptr(), dWf.data_ptr(),
                      dbf.data_ptr(), wsp.data_ptr(), 0, _lib.stream())
        torch.cuda.synchronize()
        return (dxc, dWf, dbf) if mu_zero else (dxc, dmu, dWf, dbf)

    got = launch()

    def grads(absolute):
        x = _painn_inputs64(c, mu_zero=mu_zero, absolute=absolute)
        leaves = ["xc", "Wf", "bf"] + ([] if mu_zero else ["mu"])
        for k in leaves:
            x[k].requires_grad_(True)
        q_out, mu_out, parts = painn_message64(c, **x)
        parts["W"].retain_grad()
        gq, gm = (dq_out.double(), dmu_out.double()) if not absolute else (dq_out.double().abs(), dmu_out.double().abs())
        ((q_out * gq).sum() + (mu_out * gm).sum()).backward()
        out = [x["xc"].grad, x["Wf"].grad, x["bf"].grad] if mu_zero else [x["xc"].grad, x["mu"].grad, x["Wf"].grad, x["bf"].grad]
        return out, parts["W"].grad.detach() * x["fcut"][:, None], x["phi"]

    ref, gW, phi = grads(False)
    Sb, _, _ = grads(True)
    names = ("dxc", "dWf", "dbf") if mu_zero else ("dxc", "dmu_in", "dWf", "dbf")
    cc, u = 8.0, U24
    for g, r, s, n in zip(got, ref, Sb, names):
        assert_within(g, r.detach(), s.detach(), cc, u, n)
    # one edge's term gW[e, o] phi[e, r] dropped from dWf[o, r], o on lanes 48-63 of the dmuR third's 64-row blocks (the
    # dmumu third is zero in the mu-zero form)
    kW = names.index("dWf")
    osel = torch.arange(F, 2 * F, device=DEV)
    osel = osel[(osel % 64) >= 48]
    terms = gW[:, osel, None] * phi[:, None, :]                                              # [e, o, r]
    bound = (cc * u * Sb[kW].detach() + (got[kW].double() - ref[kW].detach()).abs())[osel][None]
    k, ratio = pick_term(terms, bound, torch.ones_like(terms, dtype=torch.bool))
    assert ratio > 2.0, ("no single edge stands above the bound", ratio)
    ke, ko, kr = np.unravel_index(k, terms.shape)
    assert_sees_a_dropped_term(got[kW], ref[kW].detach(), Sb[kW].detach(), cc, u, (int(osel[ko]), int(kr)),
                               float(terms[ke, ko, kr]), "dWf without edge %d" % ke)
    del terms, bound
    assert_repeatable(launch, got, "painn bwd %s R=%d mu0=%s set %s" % (path, R, mu_zero, molset))


@pytest.mark.parametrize("R", [8, 16, 20, 32])
def test_painn_edge_grads_at_full_occupancy_vs_fp64(R, painn_cases):
    """geossl_painn_edge_grads (k_painn_edge_grads<R>, the force path) on 1024 molecules of set A: dphi, dfcut, ddir
    within 8 u S of fp64 autograd (u = 2^-24), one feature's term of ddir dropped seen on an edge in lanes 48-63, eight
    launches bit-identical."""
    from geossl_amd import _lib
    c = painn_cases("A", R)
    el, N, F, E = c["el"], c["N"], reg.PAINN_F, c["E"]
    assert E >= reg.PAINN_EDGES_MIN
    assert_occupancy(r"k_painn_edge_gradsILi%dE" % R, "R=%d" % R, grid=reg.painn_edge_grads_grid(E))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(31 + R)
    gq, gmu = torch.randn(N, F, device=DEV, generator=gen), torch.randn(N, 3, F, device=DEV, generator=gen)

    def launch():
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)
        dphi, dfc, ddir = nan(E, R), nan(E), nan(E, 3)
        _lib.call("geossl_painn_edge_grads", gq.data_ptr(), gmu.data_ptr(), c["mu"].data_ptr(), c["xc"].data_ptr(),
                  el.idx_i.data_ptr(), el.idx_j.data_ptr(), c["phi"].data_ptr(), c["fcut"].data_ptr(), c["dirv"].data_ptr(),
                  c["Wf"].data_ptr(), c["bf"].data_ptr(), E, F, R, dphi.data_ptr(), dfc.data_ptr(), ddir.data_ptr(), 0,
                  _lib.stream())
        torch.cuda.synchronize()
        return dphi, dfc, ddir

    got = launch()

    def grads(absolute):
        x = _painn_inputs64(c, absolute=absolute)
        for k in ("phi", "fcut", "dirv"):
            x[k].requires_grad_(True)
        q_out, mu_out, parts = painn_message64(c, **x)
        a, b = gq.double(), gmu.double()
        if absolute:
            a, b = a.abs(), b.abs()
        ((q_out * a).sum() + (mu_out * b).sum()).backward()
        x1 = parts["x"][:, F:2 * F].detach()
        return [x["phi"].grad, x["fcut"].grad, x["dirv"].grad], x1

    ref, x1 = grads(False)
    Sb, _ = grads(True)
    cc, u = 8.0, U24
    for g, r, s, n in zip(got, ref, Sb, ("dphi", "dfcut", "ddir")):
        assert_within(g, r, s, cc, u, n)
    # ddir[e, d] = sum_f x1[e, f] gmu[i_e, d, f]: one f dropped for x (d = 0), on an edge in lanes 48-63
    i = el.idx_i.long()
    terms = x1 * gmu.double()[i, 0, :]
    e_ = torch.arange(E, device=DEV)
    bound = (cc * u * Sb[2][:, 0] + (got[2][:, 0].double() - ref[2][:, 0]).abs())[:, None].expand_as(terms)
    k, ratio = pick_term(terms, bound, ((e_ % 64) >= 48)[:, None].expand_as(terms))
    assert ratio > 2.0, ("no single feature stands above the bound", ratio)
    e, f = divmod(k, F)
    assert_sees_a_dropped_term(got[2], ref[2], Sb[2], cc, u, (e, 0), float(terms[e, f]), "ddir without feature %d" % f)
    assert_repeatable(launch, got, "painn edge_grads R=%d" % R)


# ------------------------------------------------------------------------------------------------- tape unary maps
def test_tape_unary_maps_at_full_occupancy_vs_fp64():
    """Every map of geossl_tape_unary (k_tape_unary) on 2^24 elements (8192 blocks, 8 waves per SIMD): y within
    2 u |alpha x + beta| S' + 8 ulp(y) of fp64 per element, where S' is the map's derivative bound (the argument's own
    fp32 rounding) and the ulp term the map's fp32 error; a term of the argument (beta) dropped seen; eight launches
    identical."""
    from geossl_amd import tape as tp
    n = reg.TAPE_N
    assert_occupancy(r"k_tape_unaryE", "n=2^24", grid=reg.tape_grid(n))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    x = torch.randn(n, device=DEV, generator=gen) * 3.0
    x[:6] = torch.tensor([0.0, 19.9, 20.0, 20.1, 25.0, -30.0], device=DEV)
    pos = x.abs() + 0.5
    xs = x.clamp(-6, 6)
    sig = torch.sigmoid
    a, b = 0.7, -0.2
    ulp = lambda y: torch.where(y == 0, torch.full_like(y, 2.0 ** -149), (y.abs() * 2.0 ** -23))

    def td_(v, a_, b_):
        return a_ * v.double() + b_

    cases = []    # (kind, input, alpha, beta, fp64 map of t, |d map / d t| bound as a function of t)
    for kind, f, df in (
            (tp.AFFINE, lambda t: t, lambda t: torch.ones_like(t)),
            (tp.EXP, torch.exp, torch.exp),
            (tp.COS, torch.cos, lambda t: torch.ones_like(t)),
            (tp.SIN, torch.sin, lambda t: torch.ones_like(t)),
            (tp.SSP, lambda t: torch.nn.functional.softplus(t) - math.log(2.0), lambda t: sig(t)),
            (tp.SIGMOID, sig, lambda t: sig(t) * (1 - sig(t))),
            (tp.DSIGMOID, lambda t: sig(t) * (1 - sig(t)), lambda t: 0.25 * torch.ones_like(t)),
            (tp.D2SIGMOID, lambda t: sig(t) * (1 - sig(t)) * (1 - 2 * sig(t)), lambda t: 0.25 * torch.ones_like(t)),
            (tp.SILU, lambda t: t * sig(t), lambda t: 1.1 * torch.ones_like(t)),
            (tp.DSILU, lambda t: sig(t) * (1 + t * (1 - sig(t))), lambda t: 0.5 * torch.ones_like(t)),
            (tp.D2SILU, lambda t: sig(t) * (1 - sig(t)) * (2 + t * (1 - 2 * sig(t))), lambda t: 0.5 * torch.ones_like(t)),
            (tp.ABS, torch.abs, lambda t: torch.ones_like(t))):
        cases.append((kind, x, a, b, f, df))
    for kind, f, df in ((tp.RECIP, lambda t: 1.0 / t, lambda t: 1.0 / t ** 2), (tp.SQRT, torch.sqrt, lambda t: 0.5 * t ** -0.5),
                        (tp.DRECIP, lambda t: -1.0 / t ** 2, lambda t: 2.0 / t ** 3), (tp.D2RECIP, lambda t: 2.0 / t ** 3, lambda t: 6.0 / t ** 4),
                        (tp.RSQRT, lambda t: t ** -0.5, lambda t: 0.5 * t ** -1.5), (tp.RSQRT3, lambda t: t ** -1.5, lambda t: 1.5 * t ** -2.5)):
        cases.append((kind, pos, 2.0, 0.1, f, df))
    cg = -0.35
    for kind, f, df in ((tp.GAUSS, lambda v: torch.exp(cg * v ** 2), lambda v: (2 * cg * v).abs() * torch.exp(cg * v ** 2)),
                        (tp.DGAUSS, lambda v: 2 * cg * v * torch.exp(cg * v ** 2), lambda v: (2 * cg + 4 * cg * cg * v ** 2).abs() * torch.exp(cg * v ** 2)),
                        (tp.D2GAUSS, lambda v: (2 * cg + 4 * cg * cg * v ** 2) * torch.exp(cg * v ** 2), lambda v: (12 * cg * cg * v.abs() + 8 * cg ** 3 * v.abs() ** 3) * torch.exp(cg * v ** 2))):
        cases.append((kind, xs, cg, None, f, df))

    # the magnitude of each map's parts (its fp32 error is a few ulp of that, not of a value that cancels)
    parts = {tp.SSP: lambda t: torch.nn.functional.softplus(t) + math.log(2.0),
             tp.D2SIGMOID: lambda t: sig(t) * (1 - sig(t)), tp.DSILU: lambda t: sig(t) * (1 + t.abs()),
             tp.D2SILU: lambda t: sig(t) * (1 - sig(t)) * (2 + t.abs()), tp.COS: lambda t: torch.ones_like(t),
             tp.SIN: lambda t: torch.ones_like(t),
             tp.DGAUSS: lambda v: (2 * cg * v).abs() * torch.exp(cg * v ** 2),
             tp.D2GAUSS: lambda v: (2 * abs(cg) + 4 * cg * cg * v ** 2) * torch.exp(cg * v ** 2)}
    for kind, inp, a_, b_, f, df in cases:
        if b_ is None:   # exp(alpha x^2) and its derivatives in x: alpha is the map's constant, the argument is x
            t, St = inp.double(), inp.double().abs()
            launch = lambda: [tp._raw_unary(kind, inp, a_)]
        else:
            t, St = td_(inp, a_, b_), abs(a_) * inp.double().abs() + abs(b_)
            launch = lambda: [tp._raw_unary(kind, inp, a_, b_)]
        got = launch()
        ref = f(t)
        extra = 8.0 * ulp(parts[kind](t) if kind in parts else ref) + 2.0 ** -126
        # S: the argument's rounding through the map (|f'(t)| S(t)); the map's own fp32 error: 8 ulp of y
        S = df(t).abs() * St
        assert_within(got[0], ref, S, 4.0, U24, "tape map %d" % kind, extra=extra)
        if kind == tp.AFFINE:
            # the affine map's beta term dropped from an element on lanes 48-63 whose |beta| stands above its bound
            k = 48
            while not abs(b_) > 2 * (4.0 * U24 * float(S[k]) + float(extra[k])):
                k += 64
            assert_sees_a_dropped_term(got[0], ref, S, 4.0, U24, (k,), b_, "affine without beta", extra=extra)
        assert_repeatable(launch, got, "tape map %d" % kind)
    assert torch.equal(tp._raw_unary(tp.SIGN, x), torch.sign(x))
    assert torch.equal(tp._raw_unary(tp.LT, x, 0.25), (x < 0.25).float())
