"""CPU tests of the contrastive objectives (InfoNCE, EBM-NCE): the fp64 twin against fixture G17 (the reference run
verbatim, tests/golden/make_golden_contrastive.py), the public surface, and the C ABI of the new kernels."""
import glob
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import contrastive_twin as tw
from conftest import load_golden, rel_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(REPO, "tests", "golden", "g17_contrastive_*.npz")))
NEW_SYMBOLS = ("geossl_infonce_fwd", "geossl_infonce_bwd", "geossl_ebm_nce_fwd", "geossl_ebm_nce_bwd")
# the reference's signature of both functions (examples/pretrain_GeoSSL.py:103, :141)
REF_PARAMS = ["args", "batch", "model", "criterion", "mu", "sigma", "num_neg"]


def test_g17_cases_present():
    assert len(CASES) == 9
    metas = [json.loads(str(load_golden(c)["meta"])) for c in CASES]
    assert {m["option"] for m in metas} == {"InfoNCE", "EBM_NCE"}
    assert {m["kind"] for m in metas} == {"schnet", "painn"}
    assert {m["num_neg"] for m in metas if m["option"] == "EBM_NCE"} == {1, 2}
    assert {m["T"] for m in metas if m["option"] == "InfoNCE"} == {0.1, 1.0}
    assert {m["normalize"] for m in metas} == {True, False}
    assert min(load_golden(c)["X"].shape[0] for c in CASES) == 1


@pytest.mark.parametrize("case", CASES)
def test_twin_reproduces_g17(case):
    g = load_golden(case)
    m = json.loads(str(g["meta"]))
    X = torch.from_numpy(g["X"]).double().requires_grad_()
    Y = torch.from_numpy(g["Y"]).double().requires_grad_()
    B = X.size(0)
    if m["option"] == "InfoNCE":
        loss, h0, h1 = tw.infonce(X, Y, m["T"])
        acc = tw.infonce_acc(h0, h1, B)
        assert str(g["loss_dtype"]) == "torch.float32"
    else:
        loss, h0, h1 = tw.ebm_nce(X, Y, m["num_neg"])
        acc = tw.ebm_acc(h0, h1, B, m["num_neg"])
        assert str(g["loss_dtype"]) == "torch.float64"
    assert acc == float(g["acc"])
    ref = float(g["loss"])
    assert abs(loss.item() - ref) <= 1e-5 * max(abs(ref), 1e-3), (loss.item(), ref)
    loss.backward()
    for got, key in ((X.grad, "grad_X"), (Y.grad, "grad_Y")):
        want = torch.from_numpy(g[key]).double()
        assert float((got - want).abs().max()) <= 1e-5 * max(float(want.abs().max()), 1e-6), key


def test_public_surface_matches_the_reference():
    from geossl_amd import pretrain_GeoSSL as pg
    for fn in (pg.do_InfoNCE, pg.do_EBM_NCE):
        names = list(inspect.signature(fn).parameters)
        assert names[:len(REF_PARAMS)] == REF_PARAMS, names
        assert {"noise", "device_noise", "graph"} <= set(names)
    assert type(pg.CE_criterion) is torch.nn.CrossEntropyLoss
    sig = inspect.signature(pg.ContrastiveTrainer)
    for p in ("model", "option", "lr", "weight_decay", "mu", "sigma", "T", "num_neg", "normalize", "model_3d",
              "use_graph"):
        assert p in sig.parameters, p
    from geossl_amd import ops
    assert list(inspect.signature(ops.infonce_loss).parameters)[:3] == ["X", "Y", "T"]
    assert list(inspect.signature(ops.ebm_nce_loss).parameters)[:3] == ["X", "Y", "num_neg"]


def test_stock_criteria_take_the_kernels_others_the_fallback():
    from geossl_amd import pretrain_GeoSSL as pg
    nn = torch.nn
    assert pg._stock_ce(nn.CrossEntropyLoss())
    for c in (nn.CrossEntropyLoss(label_smoothing=0.1), nn.CrossEntropyLoss(reduction="sum"),
              nn.CrossEntropyLoss(weight=torch.ones(4)), nn.CrossEntropyLoss(ignore_index=0)):
        assert not pg._stock_ce(c)
    assert pg._stock_bce(None) and pg._stock_bce(nn.BCEWithLogitsLoss())
    for c in (nn.BCEWithLogitsLoss(pos_weight=torch.ones(1)), nn.BCEWithLogitsLoss(reduction="sum"), nn.MSELoss()):
        assert not pg._stock_bce(c)


def test_acc_from_counts_matches_the_reference_arithmetic():
    from geossl_amd import pretrain_GeoSSL as pg
    for B in (1, 3, 7, 128):
        for h0 in range(0, B + 1, max(1, B // 5)):
            for h1 in range(0, B + 1, max(1, B // 3)):
                assert pg.contrastive_acc("InfoNCE", (h0, h1), B) == tw.infonce_acc(h0, h1, B)
                for K in (1, 2):
                    assert pg.contrastive_acc("EBM_NCE", (h0, h1), B, K) == tw.ebm_acc(h0, h1, B, K)


def test_new_abi_symbols_declared_bound_and_exported():
    from geossl_amd import _lib
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.geossl_abi_version() == 1
