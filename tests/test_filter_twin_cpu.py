"""The fp64 twin of the filter-network kernels (tests/filter_twin.py) is right, checked without a GPU: its forward
against the oracle's filter rows on a golden SchNet fixture, its position gradient against torch.autograd in fp64, and
the (F, G) grid of tests/test_gpu_filter_classes.py against the kernel instantiations of the built library."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, max_abs_rel, rel_err

sys.path.insert(0, os.path.join(REPO, "tools"))

import filter_twin as ft  # noqa: E402
from helpers import cfg_of, schnet_oracle_params, t  # noqa: E402
from oracle import nets  # noqa: E402


def _molecules(sizes, seed, F, G, L, cutoff=5.0, spread=1.6):
    """A small pair-slot problem built on the host: lexicographic i < j slots molecule after molecule (the order of
    MolLayout), random positions, every slot within the cutoff an edge in both directions."""
    gen = torch.Generator().manual_seed(seed)
    mol_ptr = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int32)
    pair_ptr = torch.tensor([0] + list(np.cumsum([n * (n - 1) // 2 for n in sizes])), dtype=torch.int32)
    pi, pj = [], []
    for m, n in enumerate(sizes):
        a, b = np.triu_indices(n, k=1)
        pi.append(torch.from_numpy(a) + int(mol_ptr[m]))
        pj.append(torch.from_numpy(b) + int(mol_ptr[m]))
    pair_i, pair_j = torch.cat(pi).int(), torch.cat(pj).int()
    N = int(mol_ptr[-1])
    pos = torch.randn(N, 3, generator=gen, dtype=torch.float64) * spread
    offset = torch.linspace(0.0, cutoff, G)
    coeff = -0.5 / float(offset[1] - offset[0]) ** 2
    ws = [[torch.randn(F, G, generator=gen) / G ** 0.5, 0.3 * torch.randn(F, generator=gen),
           torch.randn(F, F, generator=gen) / F ** 0.5, 0.3 * torch.randn(F, generator=gen)] for _ in range(L)]
    xs = [torch.randn(N, F, generator=gen) for _ in range(L)]
    daggs = [torch.randn(N, F, generator=gen) for _ in range(L)]
    return dict(mol_ptr=mol_ptr, pair_ptr=pair_ptr, pair_i=pair_i, pair_j=pair_j, pos=pos, offset=offset, coeff=coeff,
                ws=ws, xs=xs, daggs=daggs, cutoff=cutoff, N=N)


@pytest.mark.parametrize("tag", ["reduced", "full_r5"])
def test_forward_twin_equals_the_oracles_filter_rows(tag):
    """schnet.py:186-187 as oracle.nets states it (fp32, on the fixture's graph and weights) against the twin, at the
    oracle's own pinning of 1e-6."""
    g = load_golden("g4_schnet_" + tag)
    cfg = cfg_of(g)
    P = schnet_oracle_params(cfg, requires_grad=False)
    _, tr = nets.schnet_forward(P, t(g["x"])[:, 0], t(g["positions"]), t(g["batch"]), cfg["cutoff"],
                                cfg["num_interactions"], cfg["readout"], return_trace=True)
    d, rbf = tr["edge_weight"], tr["edge_attr"]
    assert d.numel() > 0
    offset = P["distance_expansion.offset"]
    coeff = nets.smearing_constants(cfg["cutoff"], cfg["num_gaussians"])[1]
    C = 0.5 * (torch.cos(d * math.pi / cfg["cutoff"]) + 1.0)
    ws = []
    for l in range(cfg["num_interactions"]):
        p = "interactions.%d.mlp." % l
        ws.append([P[p + "0.weight"], P[p + "0.bias"], P[p + "2.weight"], P[p + "2.bias"]])
    twin = ft.filter_forward(d, C, ws, offset, coeff)
    for l, w in enumerate(ws):
        hidden = nets.shifted_softplus(torch.nn.functional.linear(rbf, w[0], w[1]))
        W = torch.nn.functional.linear(hidden, w[2], w[3]) * C.view(-1, 1)
        # (relative to the tensor's scale: T = softplus(u) - log 2 cancels near u = 0, where the fp32 oracle itself carries
        # an absolute error)
        for got, ref in ((hidden, twin[l]["T"]), (W, twin[l]["Wf"])):
            assert max_abs_rel(got, ref) < 1e-6 and rel_err(got, ref) < 1e-6, l
        # S is the expression on absolute values: never below the value
        assert bool((twin[l]["ST"] >= twin[l]["T"].abs()).all()) and bool((twin[l]["SWf"] >= twin[l]["Wf"].abs()).all())


@pytest.mark.parametrize("G", [1 + 16, 40, 64])
def test_dpos_twin_equals_autograd_of_the_forward_twin(G):
    """dd[l][p] of the twin against d/dd of sum_c g[p][c] Wf_l[p][c] through the forward twin, C a function of d, all in
    fp64: relative 1e-10 (both are analytic in fp64; the figure is slack for the order of summation)."""
    p = _molecules([1, 2, 7, 5, 9], seed=G, F=32, G=G, L=2)
    i, j = p["pair_i"].long(), p["pair_j"].long()
    d = (p["pos"][i] - p["pos"][j]).norm(dim=-1).requires_grad_(True)
    flag = torch.where(d < p["cutoff"], 3, 0).to(torch.uint8)
    flag[::5] = 1       # one direction only
    flag[1::7] = 2
    assert int((flag == 0).sum()) > 0 and int((flag == 3).sum()) > 0
    C, _, _ = ft.envelope(d, p["cutoff"])
    fwd = ft.filter_forward(d, C, p["ws"], p["offset"], p["coeff"])
    twin = ft.filter_dpos(d.detach(), C.detach(), flag, p["pair_i"], p["pair_j"], p["ws"], p["offset"], p["coeff"],
                          p["cutoff"], p["xs"], p["daggs"])
    for l in range(2):
        g, Sg = ft.upstream_rows(flag, p["pair_i"], p["pair_j"], p["xs"][l], p["daggs"][l])
        (ref,) = torch.autograd.grad((g * fwd[l]["Wf"]).sum(), d, retain_graph=True)
        err = float((twin[l]["dd"] - ref).abs().max() / ref.abs().max())
        assert err < 1e-10, (l, err)
        assert bool((twin[l]["dd"][flag == 0] == 0).all())
        assert bool((twin[l]["S"] >= twin[l]["dd"].abs()).all()) and float(twin[l]["extra"].abs().max()) == 0.0


def test_dpos_twin_gives_the_dropped_envelope_term_as_extra_only_where_c_is_zero():
    p = _molecules([6, 4], seed=3, F=32, G=20, L=1)
    i, j = p["pair_i"].long(), p["pair_j"].long()
    d = (p["pos"][i] - p["pos"][j]).norm(dim=-1).float()
    d[3] = p["cutoff"] * (1.0 - 2.0 ** -20)
    flag = torch.full_like(d, 3).to(torch.uint8)
    c32 = 0.5 * (torch.cos(d * np.float32(math.pi) / p["cutoff"]) + 1.0)
    assert float(c32[3]) == 0.0 and int((c32 == 0).sum()) == 1
    args = (flag, p["pair_i"], p["pair_j"], p["ws"], p["offset"], p["coeff"], p["cutoff"], p["xs"], p["daggs"])
    kept = ft.filter_dpos(d, c32, *args, drop_where_c_is_zero=False)[0]
    drop = ft.filter_dpos(d, c32, *args)[0]
    assert float(drop["dd"][3]) == 0.0 and float(drop["extra"][3]) > 0.0
    assert abs(float(kept["dd"][3])) == pytest.approx(float(drop["extra"][3]), rel=1e-12)
    rest = torch.arange(d.numel()) != 3
    assert torch.equal(kept["dd"][rest], drop["dd"][rest]) and float(drop["extra"][rest].abs().max()) == 0.0


def test_position_gradient_twin_equals_autograd_through_the_norm():
    """sum_l sum_p dd[l][p] |pos_i - pos_j| differentiated by autograd against the twin's dense slot formula, with 1- and
    2-atom molecules; a coincident pair (distance 0) and a slot whose layers cancel to zero are skipped."""
    p = _molecules([1, 2, 6, 1, 9, 3], seed=2, F=32, G=8, L=3)
    gen = torch.Generator().manual_seed(9)
    P = p["pair_i"].numel()
    dd = torch.randn(3, P, generator=gen, dtype=torch.float64)
    dd[:, 4] = torch.tensor([0.5, -0.25, -0.25], dtype=torch.float64)      # sums to zero: skipped
    pos = p["pos"].clone()
    i, j = p["pair_i"].long(), p["pair_j"].long()
    pos[j[7]] = pos[i[7]]                                                   # coincident atoms: distance 0, skipped
    pos.requires_grad_(True)
    delta = pos[i] - pos[j]
    keep = torch.ones(P, dtype=torch.bool)
    keep[7] = False                                                         # (the norm has no derivative at 0)
    dist = torch.zeros(P, dtype=torch.float64)
    dist[keep] = delta[keep].norm(dim=-1)
    (ref,) = torch.autograd.grad((dd.sum(0)[keep] * dist[keep]).sum(), pos)
    got, S, terms, atom = ft.pair_position_grad(pos.detach(), dist.detach(), dd, p["mol_ptr"], p["pair_ptr"])
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12
    assert bool((S >= got.abs()).all())
    assert float(got[0].abs().max()) == 0.0 and float(got[6 + 3].abs().max()) == 0.0   # the 1-atom molecules
    # the slots the twin derives are the layout's own: every (a, b) meets slot p with {i, j} = {a, b}
    a, b, slot = ft.pair_slots(p["mol_ptr"], p["pair_ptr"])
    assert torch.equal(torch.minimum(a, b), i[slot]) and torch.equal(torch.maximum(a, b), j[slot])
    assert a.numel() == 2 * P


# ------------------------------------------------------------------------------------ coverage of the built library
FAMILIES = ("k_filter_fwd", "k_filter_fwd_h", "k_filter_dpos")


def instantiations(names):
    """{(family, NMB, K1S)} among the symbol names of a code object (Itanium mangling of k_<family><NMB, K1S>)."""
    out = set()
    for n in names:
        m = re.search(r"\d+(k_filter_(?:fwd|fwd_h|dpos))ILi(\d+)ELi(\d+)EE", n)
        if m:
            out.add((m.group(1), int(m.group(2)), int(m.group(3))))
    return out


def grid_classes(Fs, Gs):
    """The launchers' rule (filter_fwd.hip, filter_dpos.hip): NMB = F / 32, K1S = ceil(G / 16)."""
    return {(fam, F // 32, (G + 15) // 16) for fam in FAMILIES for F in Fs for G in Gs}


def test_instantiation_names_are_read_from_mangled_symbols():
    names = ["_ZN12_GLOBAL__N_112k_filter_fwdILi4ELi3EEEvPKfS2_i19GeosslFilterWeightsiS2_fPfS4_PKi",
             "_ZN12_GLOBAL__N_114k_filter_fwd_hILi1ELi1EEEvPKfS2_i", "_ZN12_GLOBAL__N_113k_filter_dposILi2ELi4EEEvPKf",
             "_ZN12_GLOBAL__N_114k_filter_bwd_hILi4ELb0EEEvPKf", "_ZN12_GLOBAL__N_112k_filter_bwdILi4EEEvPKf"]
    assert instantiations(names) == {("k_filter_fwd", 4, 3), ("k_filter_fwd_h", 1, 1), ("k_filter_dpos", 2, 4)}
    # a new instantiation without a grid point is seen
    assert ("k_filter_dpos", 2, 5) not in grid_classes((32, 64, 128), (1, 64))
    assert grid_classes((64,), (40,)) == {(f, 2, 3) for f in FAMILIES}


def test_gpu_grid_reaches_every_instantiation_of_the_built_library():
    """Every k_filter_fwd / k_filter_fwd_h / k_filter_dpos instantiation of the built code object has a point of the
    (F, G) grid of tests/test_gpu_filter_classes.py, and every grid point an instantiation."""
    import scan_packed_opsel as sp
    from geossl_amd import _lib
    if not os.path.exists(sp.READELF):
        pytest.skip("llvm-readelf of the ROCm toolchain not found")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libgeossl_hip.so is not built")
    import test_gpu_filter_classes as gpu
    built = instantiations(sp.resources(_lib.LIB_PATH))
    assert {f for f, _, _ in built} == set(FAMILIES), built
    covered = grid_classes(gpu.GRID_F, gpu.GRID_G)
    assert not built - covered, "instantiations no grid point launches: %s" % sorted(built - covered)
    assert not covered - built, "grid points without an instantiation: %s" % sorted(covered - built)
    assert len(built) == 3 * 3 * 4
