"""CPU tests of LBA fine-tuning and of the sparse pair list's host side: the fp64 oracle reproduces fixture G24 (the
unmodified reference's finetune_lba.py step on pocket-sized structures), the capacity bound of the pair list holds for
every molecule of the fixture, the switch and the bound of layout.py, the numpy Spearman of eval_LBA, and the C ABI."""
import json
import os
import re

import numpy as np
import pytest
import torch

import force_twin as ft
import lba_structures as ls
from conftest import GOLDEN, REPO, load_golden, rel_err
from helpers import fill_dict, schnet_oracle_params
from oracle import nets
from oracle.graph import radius_graph_np

G24 = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("g24_lba_"))


def test_g24_cases_present():
    assert G24 == ["g24_lba_painn", "g24_lba_schnet_full", "g24_lba_schnet_reduced"]
    for case in G24:
        assert os.path.getsize(os.path.join(GOLDEN, case + ".npz")) < 400 * 1024


def _oracle_pred(g):
    meta, cfg = json.loads(str(g["meta"])), json.loads(str(g["cfg"]))
    x, pos, batch = (torch.from_numpy(g[k]) for k in ("x", "positions", "batch"))
    if meta["kind"] == "schnet":
        P = {k: v.double() for k, v in schnet_oracle_params(cfg, requires_grad=False).items()}
        ei = ft.schnet_edges(g["positions"], g["batch"], cfg["cutoff"])
        rep = nets.schnet_forward(P, x, pos.double(), batch, cfg["cutoff"], cfg["num_interactions"], cfg["readout"],
                                  edge_index=ei)
        H = {k: v.double() for k, v in fill_dict({"weight": (1, meta["emb_dim"]), "bias": (1,)}).items()}
    else:
        from geossl_amd.Geom3D.models import PaiNN
        from helpers import fill_module_
        model = fill_module_(PaiNN(**cfg))
        params, bufs = ft.module_tensors(model)
        P = {k: v.double() for k, v in list(params.items()) + list(bufs.items()) if v.is_floating_point()}
        rep = nets.painn_forward(P, x, pos.double(), torch.from_numpy(g["radius_edge_index"]).long(), batch,
                                 cfg["n_atom_basis"], cfg["n_interactions"], cfg["cutoff"], cfg["readout"])
        H = {k: v.detach().double() for k, v in fill_module_(model.create_output_layers()).state_dict().items()}
    return ft.head_forward(rep, H)


@pytest.mark.parametrize("case", G24)
def test_oracle_reproduces_g24(case):
    g = load_golden(case)
    pred = _oracle_pred(g)
    y = torch.from_numpy(g["y"]).double()
    assert rel_err(pred, g["pred"]) < 1e-5
    assert abs(float(((pred - y) ** 2).mean()) - float(g["loss"])) < 1e-5 * float(g["loss"])
    # eval()'s metrics of the stored predictions
    from geossl_amd.finetune_lba import spearman
    assert abs(float(np.sqrt(np.mean((g["pred"].astype(np.float64) - g["y"]) ** 2))) - float(g["rmse"])) < 1e-5 * float(g["rmse"])
    assert abs(np.corrcoef(g["y"], g["pred"])[0, 1] - float(g["pearson"])) < 1e-9
    assert abs(spearman(g["y"], g["pred"]) - float(g["spearman"])) < 1e-9


@pytest.mark.parametrize("case", G24)
def test_g24_structures_are_the_shared_generator_and_keep_the_margin(case):
    g = load_golden(case)
    meta = json.loads(str(g["meta"]))
    s = ls.checked(tuple(int(n) for n in g["sizes"]), meta["cutoff"])
    assert s["seed"] == meta["seed"] and np.array_equal(s["positions"], g["positions"]) and np.array_equal(s["x"], g["x"])
    assert ft.cutoff_margin(g["positions"], g["batch"], meta["cutoff"]) >= ft.CUTOFF_MARGIN


@pytest.mark.parametrize("case", G24)
def test_pair_capacity_bounds_every_molecule(case):
    from geossl_amd.layout import sparse_pair_capacity
    g = load_golden(case)
    cutoff = json.loads(str(g["meta"]))["cutoff"]
    ei = radius_graph_np(g["positions"], cutoff, g["batch"])
    lo, hi = np.minimum(ei[0], ei[1]), np.maximum(ei[0], ei[1])
    pairs = np.unique(np.stack([lo, hi]), axis=1)
    per_mol = np.bincount(g["batch"][pairs[0]], minlength=len(g["sizes"]))
    for n, real in zip(g["sizes"], per_mol):
        assert real <= sparse_pair_capacity([n]) == ls.pair_capacity([n])
    assert sparse_pair_capacity(g["sizes"]) == sum(sparse_pair_capacity([n]) for n in g["sizes"])
    # in-degree never above 33: what the bound rests on
    assert np.bincount(ei[1]).max() <= 33


def test_sparse_switch(monkeypatch):
    from geossl_amd import layout
    monkeypatch.delenv("GEOSSL_SPARSE_PAIRS", raising=False)
    assert not layout.want_sparse(255) and layout.want_sparse(256) and not layout.want_sparse(1)
    monkeypatch.setenv("GEOSSL_SPARSE_PAIRS", "1")
    assert layout.want_sparse(2) and layout.want_sparse(1024)
    monkeypatch.setenv("GEOSSL_SPARSE_PAIRS", "0")
    assert not layout.want_sparse(256)
    assert layout.sparse_pair_capacity([1, 2, 67, 68, 500]) == 0 + 1 + 67 * 33 + 68 * 33 + 500 * 33
    assert layout.SPARSE_MAX_N == 1024 and layout.DENSE_MAX_N == 255


def test_spearman_equals_scipy_on_ties():
    stats = pytest.importorskip("scipy.stats")
    from geossl_amd.finetune_lba import average_ranks, spearman
    rng = np.random.default_rng(7)
    for n in (2, 3, 10, 257):
        a = rng.integers(0, max(2, n // 3), size=n).astype(np.float64)     # many ties
        b = np.round(rng.standard_normal(n), 1)
        assert np.array_equal(average_ranks(a), stats.rankdata(a))
        if len(set(a)) > 1 and len(set(b)) > 1:
            assert abs(spearman(a, b) - stats.spearmanr(a, b)[0]) < 1e-12
    assert np.array_equal(average_ranks([3.0, 1.0, 3.0, 2.0]), [3.5, 1.0, 3.5, 2.0])


def test_sparse_entry_points_in_header_and_ctypes():
    from geossl_amd import _lib
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name in ("geossl_sparse_pairs_build", "geossl_cfconv_aggregate_sparse", "geossl_pair_position_grad_sparse"):
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in _lib.PROTOTYPES, name


def test_adjacency_rule_is_stated_once():
    """k_radius and the sparse-list kernels call one device function for the edges (csrc/radius_adj.h)."""
    src = {f: open(os.path.join(REPO, "geossl_amd", "csrc", f)).read() for f in ("graph.hip", "sparse_pairs.hip",
                                                                                  "radius_adj.h")}
    assert "radius_scan_target(" in src["graph.hip"] and "radius_scan_target(" in src["sparse_pairs.hip"]
    for f in ("graph.hip", "sparse_pairs.hip"):
        assert "rank < cap" not in src[f], f
    assert src["radius_adj.h"].count("rank < cap") == 1


def test_do_lba_falls_back_to_the_reference_lines_on_cpu():
    """Anything the kernels do not serve runs the ATen lines: a stand-in backbone on the CPU, B = 1 included."""
    import types
    from geossl_amd.finetune_lba import do_LBA, eval_LBA

    class Backbone(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(3, 4)

        def forward(self, x, positions, batch):
            B = int(batch.max()) + 1
            return torch.zeros(B, 4).index_add_(0, batch, self.lin(positions) * x[:, None])

    class B_:
        def __init__(self, n):
            g = torch.Generator().manual_seed(n)
            self.x = torch.arange(1, 4 * n + 1, dtype=torch.float32)
            self.positions = torch.randn(4 * n, 3, generator=g)
            self.batch = torch.repeat_interleave(torch.arange(n), 4)
            self.y = torch.randn(n, generator=g)
            self.num_graphs = n

        def to(self, device):
            return self

    torch.manual_seed(0)
    model, head = Backbone(), torch.nn.Linear(4, 1)
    args = types.SimpleNamespace(model_3d="schnet")
    for n in (1, 3):
        b = B_(n)
        loss = do_LBA(args, b, model, head, torch.nn.MSELoss())
        ref = torch.nn.MSELoss()(head(model(b.x, b.positions, b.batch)).squeeze(), b.y)
        assert torch.equal(loss, ref)
    loss.backward()
    assert head.weight.grad is not None
    rmse, pearson, spear, y_true, y_pred = eval_LBA(args, [B_(3), B_(2)], model, head)
    assert len(y_true) == len(y_pred) == 5 and np.isfinite([rmse, pearson, spear]).all()
    with pytest.raises(Exception, match="not included"):
        do_LBA(types.SimpleNamespace(model_3d="egnn"), B_(2), model, head)
