"""CPU tests of the atom-tile PaiNN interaction (csrc/painn_tile.hip): the fp64 twin the GPU tests check the kernels
against (tests/painn_tile_twin.py) equals a plain restatement of the reference lines and torch.autograd of it, its
magnitude sums bound its values, its constants follow their formulas, the switch reads as documented, and the C ABI."""
import os
import re

import pytest
import torch

import painn_tile_twin as tw
from conftest import REPO

NEW_SYMBOLS = ("geossl_painn_tile_ok", "geossl_painn_interaction_fwd_tile", "geossl_painn_interaction_bwd_tile")


def _case(mu_given, N=11, F=8, R=5, E=60, seed=3):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    idx_i, idx_j = torch.randint(0, N - 1, (E,), generator=g), torch.randint(0, N - 1, (E,), generator=g)   # (atom N-1: no edges)
    dirv = rnd(E, 3)
    dirv = dirv / dirv.norm(dim=1, keepdim=True)
    return dict(q=rnd(N, F), mu=rnd(N, 3, F) if mu_given else None, xc=rnd(N, 3 * F), idx_i=idx_i, idx_j=idx_j,
                phi=torch.rand(E, R, generator=g, dtype=torch.float64), fcut=torch.rand(E, generator=g, dtype=torch.float64),
                dirv=dirv, Wf=rnd(3 * F, R), bf=rnd(3 * F)), rnd


@pytest.mark.parametrize("mu_given", [True, False])
def test_twin_equals_the_plain_restatement_and_its_autograd(mu_given):
    c, rnd = _case(mu_given)
    N, F = c["q"].shape
    fw = tw.forward(**c)
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("xc", "Wf", "bf")}
    mu = (c["mu"] if mu_given else torch.zeros(N, 3, F, dtype=torch.float64)).clone().requires_grad_(True)
    q_out, mu_out = tw.plain_forward(c["q"], mu, leaves["xc"], c["idx_i"], c["idx_j"], c["phi"], c["fcut"], c["dirv"],
                                     leaves["Wf"], leaves["bf"])
    for name, got in (("q_out", q_out), ("mu_out", mu_out)):
        ref, S = fw[name]
        assert torch.allclose(ref, got.detach(), rtol=1e-13, atol=1e-13), name
        assert bool((ref.abs() <= S * (1 + 1e-12)).all()), name
    # every element is the residual plus its terms
    assert torch.allclose(fw["q_out"][0], c["q"] + torch.zeros(N, F, dtype=torch.float64).index_add_(0, c["idx_i"], fw["terms_q"]))
    assert bool((fw["terms_q"].abs() <= fw["abs_q"] * (1 + 1e-12)).all())
    assert bool((fw["terms_mu"].abs() <= fw["abs_mu"] * (1 + 1e-12)).all())
    dq_out, dmu_out = rnd(N, F), rnd(N, 3, F)
    (q_out * dq_out).sum().backward(retain_graph=True)
    (mu_out * dmu_out).sum().backward()
    bw = tw.backward(dq_out, dmu_out, c["mu"], c["xc"], c["idx_i"], c["idx_j"], c["phi"], c["fcut"], c["dirv"], c["Wf"],
                     c["bf"])
    want = dict(dxc=leaves["xc"].grad, dWf=leaves["Wf"].grad, dbf=leaves["bf"].grad)
    if mu_given:
        want["dmu_in"] = mu.grad
    else:
        assert bw["dmu_in"] is None
    for name, g_ in want.items():
        ref, S = bw[name]
        assert torch.allclose(ref, g_, rtol=1e-12, atol=1e-12), name
        assert bool((ref.abs() <= S * (1 + 1e-12)).all()), name
    assert torch.allclose(bw["terms_dWf"].sum(0), bw["dWf"][0]) and torch.allclose(bw["terms_dbf"].sum(0), bw["dbf"][0])
    # the atom with no edges: identities forward, the residual alone backward
    assert torch.equal(fw["q_out"][0][N - 1], c["q"][N - 1]) and bool((bw["dxc"][0][N - 1] == 0).all())
    # restricted to a list of source atoms, dWf is the sum over their edges
    atoms = torch.tensor([0, 3, 4])
    part = tw.backward(dq_out, dmu_out, c["mu"], c["xc"], c["idx_i"], c["idx_j"], c["phi"], c["fcut"], c["dirv"], c["Wf"],
                       c["bf"], atoms=atoms)
    keep = torch.isin(c["idx_j"], atoms)
    assert torch.allclose(part["dWf"][0], bw["terms_dWf"][keep].sum(0)) and 0 < int(keep.sum()) < keep.numel()


def test_constants_follow_their_rounding_counts():
    assert tw.U == 2.0 ** -22 and tw.MAX_DEGREE == 70
    assert tw.C_FWD == tw.c_fwd(70) == 9 + 1.25 + (32 * 3 + 2) / 4
    assert tw.C_BWD == tw.c_bwd(70) == 9 + 1.5 + (16 * 3 + 2) / 4
    assert tw.C_WGRAD == tw.c_wgrad(3) == 2 + (48 * 3 + 6) / 4
    assert tw.c_wgrad(6) > tw.c_wgrad(3) and tw.c_fwd(32) < tw.c_fwd(33)   # they grow with the edges accumulated


def test_switch_reads_as_documented(monkeypatch):
    from geossl_amd import bucket, switches
    monkeypatch.setenv("GEOSSL_PAINN_TILE", "1")
    assert switches.painn_tile(18) and switches.painn_tile(300)
    monkeypatch.setenv("GEOSSL_PAINN_TILE", "0")
    assert not switches.painn_tile(18) and not switches.painn_tile(300)
    monkeypatch.delenv("GEOSSL_PAINN_TILE")
    assert not switches.painn_tile(bucket.MAX_N)                       # 255 atoms and below: never by default
    assert switches.painn_tile(bucket.MAX_N + 1) == switches.PAINN_TILE_DEFAULT


def test_new_abi_symbols_declared_bound_and_exported():
    from geossl_amd import _lib, build
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"\bint64_t geossl_painn_interaction_bwd_tile_workspace_floats\(", h)
    assert "geossl_painn_interaction_bwd_tile_workspace_floats" in _lib.PROTOTYPES
    assert _lib.PROTOTYPES["geossl_painn_interaction_fwd_tile"] == _lib.PROTOTYPES["geossl_painn_interaction_fwd_atoms"]
    assert _lib.PROTOTYPES["geossl_painn_interaction_bwd_tile"] == _lib.PROTOTYPES["geossl_painn_interaction_bwd_atoms"]
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    served = [(F, R) for F in (32, 64, 128, 256) for R in (8, 16, 20, 32) if lib.geossl_painn_tile_ok(F, R)]
    assert served == [(128, 8), (128, 16), (128, 20)]
    per_block = 3 * 128 * 20 + 3 * 128
    assert lib.geossl_painn_interaction_bwd_tile_workspace_floats(96, 128, 20) == 96 * per_block
    big = lib.geossl_painn_interaction_bwd_tile_workspace_floats(1 << 20, 128, 20)
    assert big % per_block == 0 and 96 < big // per_block <= 1024          # a bounded number of blocks
    assert "painn_tile.hip" in build._sources() and build.SOURCE_FLAGS.get("painn_tile.hip") == ["-fno-slp-vectorize"]
