"""CPU tests of Charge Prediction pretraining: the fp64 twin against fixture G19 (the reference run verbatim,
tests/golden/make_golden_charge.py), the mask-size rule and the numpy draw, the public surface against the reference's,
the fallback selection, and the C ABI of the new kernels."""
import glob
import inspect
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import charge_twin as tw
from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(REPO, "tests", "golden", "g19_charge_*.npz")))
NEW_SYMBOLS = ("geossl_charge_mask", "geossl_charge_mask_dyn", "geossl_charge_head_fwd", "geossl_charge_head_fwd_dyn",
               "geossl_charge_head_bwd", "geossl_charge_head_bwd_dyn")


def test_g19_cases_present():
    assert len(CASES) == 5
    gs = {c: load_golden(c) for c in CASES}
    metas = {c: json.loads(str(g["meta"])) for c, g in gs.items()}
    assert {m["kind"] for m in metas.values()} == {"schnet", "painn"}
    assert {m["ratio"] for m in metas.values()} == {0.3, 0.5}
    assert any(g["masked_index"].size == 0 and np.isnan(g["loss"]) for g in gs.values())   # k = 0
    assert any(json.loads(str(g["cfg"])).get("hidden_channels") == 128 for g in gs.values())   # SchNet full
    # the mask token is also a real type: some label equals it
    assert any((g["charge_actual"][g["masked_index"]] == 8).any() for g in gs.values())


@pytest.mark.parametrize("case", CASES)
def test_twin_reproduces_g19(case):
    g = load_golden(case)
    idx = g["masked_index"]
    x, x_after = g["x"], g["x_after"]
    # the step's own bookkeeping: labels are the original types, the masked rows carry the token afterwards
    assert np.array_equal(g["charge_actual"], x[:, 0])
    expect = x.copy()
    expect[idx, 0] = 8
    assert np.array_equal(x_after, expect)
    assert idx.size == tw.mask_count(x.shape[0], json.loads(str(g["meta"]))["ratio"])
    h = torch.from_numpy(g["node_repr"]).double().requires_grad_()
    W = torch.from_numpy(g["pred_weight"]).double().requires_grad_()
    b = torch.from_numpy(g["pred_bias"]).double().requires_grad_()
    loss, z = tw.charge_loss(h, W, b, idx, x[idx, 0])
    if idx.size == 0:
        assert np.isnan(float(g["loss"])) and torch.isnan(loss)
        for key in ("grad_node_repr", "grad_pred_weight", "grad_pred_bias"):
            assert not np.abs(g[key]).sum(), key
        return
    ref = float(g["loss"])
    assert abs(loss.item() - ref) <= 1e-5 * abs(ref)
    assert float((z.detach() - torch.from_numpy(g["logits"]).double()).abs().max()) <= 1e-5 * float(z.detach().abs().max())
    loss.backward()
    for got, key in ((h.grad, "grad_node_repr"), (W.grad, "grad_pred_weight"), (b.grad, "grad_pred_bias")):
        want = torch.from_numpy(g[key]).double().reshape(got.shape)
        assert float((got - want).abs().max()) <= 1e-5 * max(float(want.abs().max()), 1e-6), key


@pytest.mark.parametrize("case", CASES)
def test_numpy_draw_reproduces_the_fixture(case):
    from geossl_amd.pretrain_ChargePrediction import numpy_mask
    g = load_golden(case)
    meta = json.loads(str(g["meta"]))
    np.random.seed(meta["seed"])
    got = numpy_mask(g["x"].shape[0], meta["ratio"])
    assert np.array_equal(got, g["masked_index"])


def test_k_rule_matches_python_int():
    """The library's k (the rule the device computes) is int(M * r) for every M up to 300 000 at several ratios."""
    from geossl_amd import _lib
    lib = _lib.load()
    M = np.arange(0, 300001, dtype=np.int64)
    for r in (0.0, 0.1, 0.15, 0.3, 1.0 / 3.0, 0.5, 0.7, 0.9, 0.999, 1.0):
        want = np.array([int(m * r) for m in M.tolist()], dtype=np.int64)
        assert np.array_equal((M.astype(np.float64) * r).astype(np.int64), want)   # (numpy restates it vectorised)
        for m in list(range(0, 2000)) + list(range(2000, 300001, 997)) + [261120, 300000]:
            assert lib.geossl_charge_mask_count(m, r) == want[m], (m, r)


def test_charge_predictor_matches_the_reference():
    from geossl_amd.pretrain_ChargePrediction import ChargePredictor, do_ChargePrediction, node_class
    assert node_class == 9
    for emb in (48, 128):
        torch.manual_seed(3)
        ours = ChargePredictor(emb)
        sd = ours.state_dict()
        assert list(sd) == ["predictor.weight", "predictor.bias"]
        assert tuple(sd["predictor.weight"].shape) == (9, emb) and tuple(sd["predictor.bias"].shape) == (9,)
        assert type(ours.criterion) is torch.nn.CrossEntropyLoss and ours.criterion.reduction == "mean"
        torch.manual_seed(3)
        lin = torch.nn.Linear(emb, 9)   # the reference's init: nn.Linear(emb_dim, node_class) drawn first
        assert torch.equal(sd["predictor.weight"], lin.weight.detach()) and torch.equal(sd["predictor.bias"],
                                                                                        lin.bias.detach())
        h, y = torch.randn(5, emb), torch.tensor([0, 8, 3, 8, 1])
        assert torch.equal(ours(h, y), torch.nn.CrossEntropyLoss()(lin(h), y))
    assert list(inspect.signature(ChargePredictor.forward).parameters) == ["self", "node_repr", "charge_actual"]
    assert list(inspect.signature(do_ChargePrediction).parameters)[:4] == ["args", "batch", "model", "charge_predictor"]


def test_fallback_selection():
    """fused_head_ok takes the reference predictor only: other criteria, a subclass, unserved widths and CPU parameters
    run the ATen head."""
    from geossl_amd import ops
    from geossl_amd.pretrain_ChargePrediction import (ChargePredictor, ChargePredictionTrainer, _fused_batch_ok,
                                                      fused_head_ok, mask_rng_of)
    assert [F for F in (32, 48, 64, 96, 128, 256, 512, 1024) if ops.charge_head_width_ok(F, 9)] == [64, 128, 256, 512]
    assert [C for C in (1, 2, 9, 16, 17) if ops.charge_head_width_ok(128, C)] == [2, 9, 16]
    p = ChargePredictor(128)
    assert not fused_head_ok(p)   # CPU parameters

    class Sub(ChargePredictor):
        pass
    for q in (Sub(128), ChargePredictor(48)):
        assert not fused_head_ok(q)
    for crit in (torch.nn.CrossEntropyLoss(label_smoothing=0.1), torch.nn.CrossEntropyLoss(weight=torch.ones(9)),
                 torch.nn.CrossEntropyLoss(ignore_index=8), torch.nn.CrossEntropyLoss(reduction="sum")):
        q = ChargePredictor(128)
        q.criterion = crit
        assert not fused_head_ok(q)
    cpu = types.SimpleNamespace(x=torch.zeros(4, 2, dtype=torch.long), positions=torch.zeros(4, 3))
    assert not _fused_batch_ok(cpu)
    assert mask_rng_of(types.SimpleNamespace()) == "numpy"
    with pytest.raises(ValueError):
        mask_rng_of(types.SimpleNamespace(mask_rng="torch"))
    sig = inspect.signature(ChargePredictionTrainer)
    for name in ("model", "charge_predictor", "lr", "weight_decay", "model_3d", "use_graph", "charge_masking_ratio",
                 "mask_rng", "seed"):
        assert name in sig.parameters, name
    assert sig.parameters["mask_rng"].default == "device" and sig.parameters["charge_masking_ratio"].default == 0.3


def test_new_abi_symbols_declared_bound_and_exported():
    from geossl_amd import _lib
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
