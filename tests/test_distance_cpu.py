"""CPU tests of Distance Prediction pretraining: the fp64 twin against fixture G18 (the reference run verbatim,
tests/golden/make_golden_distance.py), the public surface against the reference's, and the C ABI of the new kernels."""
import glob
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import distance_twin as tw
from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(REPO, "tests", "golden", "g18_distance_*.npz")))
NEW_SYMBOLS = ("geossl_distance_head_fwd", "geossl_distance_head_fwd_dyn", "geossl_distance_head_bwd",
               "geossl_distance_head_bwd_dyn")


def test_g18_cases_present():
    assert len(CASES) == 5
    gs = {c: load_golden(c) for c in CASES}
    metas = {c: json.loads(str(g["meta"])) for c, g in gs.items()}
    assert {m["kind"] for m in metas.values()} == {"schnet", "painn"}
    assert {m["option"] for m in metas.values()} == {"permutation", "combination"}
    assert any(m["ratio"] < 1 for m in metas.values())
    sizes = [set(g["sizes"].tolist()) for g in gs.values()]
    assert any({1, 2} <= s for s in sizes)                           # ragged with a 1-atom and a 2-atom molecule
    assert any(g["sizes"].tolist() == [2] for g in gs.values())      # B = 1, n = 2
    assert any(json.loads(str(g["cfg"])).get("hidden_channels") == 128 for g in gs.values())   # SchNet full


@pytest.mark.parametrize("case", CASES)
def test_twin_reproduces_g18(case):
    g = load_golden(case)
    h = torch.from_numpy(g["node_repr"]).double().requires_grad_()
    W = torch.from_numpy(g["pred_weight"]).double().requires_grad_()
    b = torch.from_numpy(g["pred_bias"]).double().requires_grad_()
    sei = torch.from_numpy(g["super_edge_index"])
    loss, pred, target = tw.distance_loss(h, W, b, torch.from_numpy(g["positions"]), sei)
    ref = float(g["loss"])
    assert abs(loss.item() - ref) <= 1e-5 * abs(ref)
    assert float((target - torch.from_numpy(g["distance_actual"]).double()).abs().max()) <= 1e-6 * max(
        float(target.abs().max()), 1.0)
    assert float((pred.detach() - torch.from_numpy(g["pred"]).double()).abs().max()) <= 1e-5 * max(float(pred.detach().abs().max()), 1.0)
    loss.backward()
    for got, key in ((h.grad, "grad_node_repr"), (W.grad, "grad_pred_weight"), (b.grad, "grad_pred_bias")):
        want = torch.from_numpy(g[key]).double().reshape(got.shape)
        assert float((got - want).abs().max()) <= 1e-5 * max(float(want.abs().max()), 1e-6), key


def test_one_view_host_plan():
    """A one-view bucket (views = 1): the aggregation work list covers the B molecules of view 0 alone; the pointer arrays
    the gather reads keep both views."""
    from geossl_amd import bucket as bk
    n = np.array([5, 18, 2, 9, 33, 1, 12])
    one, two = bk.host_plan(n, "permutation", views=1), bk.host_plan(n, "permutation")
    assert one["counts"][:3] == two["counts"][:3] == (80, 794, 1588)
    mols = one["work"][one["work"] >= 0] & 0xFFFFFF
    assert set(mols.tolist()) == set(range(len(n)))
    assert set((two["work"][two["work"] >= 0] & 0xFFFFFF).tolist()) == set(range(2 * len(n)))
    for k in ("mol_ptr2", "pair_ptr2", "se_ptr", "inc_ptr"):
        assert np.array_equal(one[k], two[k]), k
    assert bk.batch_counts(n, "permutation", 1)[3] <= bk.batch_counts(n, "permutation")[3]


def test_distance_predictor_matches_the_reference():
    from geossl_amd.pretrain_DistancePrediction import DistancePredictor, do_DistancePrediction
    for emb in (48, 128):
        torch.manual_seed(3)
        ours = DistancePredictor(emb)
        sd = ours.state_dict()
        assert list(sd) == ["predictor.weight", "predictor.bias"]
        assert tuple(sd["predictor.weight"].shape) == (1, 2 * emb) and tuple(sd["predictor.bias"].shape) == (1,)
        assert type(ours.criterion) is torch.nn.L1Loss and ours.criterion.reduction == "mean"
        torch.manual_seed(3)
        lin = torch.nn.Linear(2 * emb, 1)   # the reference's init: nn.Linear(emb_dim*2, 1) drawn first
        assert torch.equal(sd["predictor.weight"], lin.weight.detach()) and torch.equal(sd["predictor.bias"],
                                                                                        lin.bias.detach())
        u, v, d = torch.randn(5, emb), torch.randn(5, emb), torch.rand(5)
        assert torch.equal(ours(u, v, d), torch.nn.L1Loss()(lin(torch.cat([u, v], 1)).squeeze(), d))
    assert list(inspect.signature(DistancePredictor.forward).parameters) == ["self", "u_node_repr", "v_node_repr",
                                                                             "distance_actual"]
    assert list(inspect.signature(do_DistancePrediction).parameters)[:4] == ["args", "batch", "model",
                                                                             "distance_predictor"]


def test_trainer_and_op_surface():
    from geossl_amd import ops
    from geossl_amd.pretrain_DistancePrediction import DistancePredictionTrainer
    sig = inspect.signature(DistancePredictionTrainer)
    for p in ("model", "distance_predictor", "lr", "weight_decay", "model_3d", "use_graph"):
        assert p in sig.parameters, p
    assert list(inspect.signature(ops.distance_head).parameters)[:6] == ["h", "W", "b", "positions", "super_edge_index",
                                                                         "incidence"]
    assert [F for F in (32, 48, 64, 96, 128, 256, 512, 1024) if ops.distance_head_width_ok(F)] == [64, 128, 256, 512]


def test_new_abi_symbols_declared_bound_and_exported():
    from geossl_amd import _lib
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
