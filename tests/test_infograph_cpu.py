"""CPU tests of 3D InfoGraph pretraining: the public surface against the reference's (Discriminator, cycle_index), the fp64
twin and the ATen do_InfoGraph against fixture G20 (the reference run verbatim, tests/golden/make_golden_infograph.py),
the fallback selection, and the C ABI of the new kernels."""
import glob
import inspect
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import infograph_twin as tw
from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(REPO, "tests", "golden", "g20_infograph_*.npz")))
NEW_SYMBOLS = ("geossl_infograph_fwd", "geossl_infograph_fwd_dyn", "geossl_infograph_bwd", "geossl_infograph_bwd_dyn")


def _close(got, want, rel, what):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double().reshape(got.shape)
    scale = max(float(want.abs().max()), 1e-6)
    assert float((got - want).abs().max()) <= rel * scale, what


def test_g20_cases_present():
    assert len(CASES) == 5
    gs = {c: load_golden(c) for c in CASES}
    metas = {c: json.loads(str(g["meta"])) for c, g in gs.items()}
    assert {m["kind"] for m in metas.values()} == {"schnet", "painn"}
    assert {m["readout"] for m in metas.values()} == {"mean", "add"}
    assert any(g["sizes"].size == 1 for g in gs.values())                  # B = 1
    assert any((g["sizes"] == 1).any() and g["sizes"].size > 1 for g in gs.values())   # a 1-atom molecule
    assert any(json.loads(str(g["cfg"])).get("hidden_channels") == 128 for g in gs.values())   # SchNet full


def test_discriminator_matches_the_reference():
    from geossl_amd.pretrain_3DInfoGraph import Discriminator
    for F in (64, 128, 300):
        torch.manual_seed(5)
        d = Discriminator(F)
        sd = d.state_dict()
        assert list(sd) == ["weight"] and tuple(sd["weight"].shape) == (F, F)
        bound = 1.0 / math.sqrt(F)
        w = sd["weight"]
        assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound   # U(-1/sqrt F, 1/sqrt F)
        assert abs(float(w.mean())) < 0.1 * bound
        torch.manual_seed(5)
        ref = torch.Tensor(F, F).uniform_(-bound, bound)   # PyG's uniform(size, w): the same draw
        assert torch.equal(w, ref)
        x, s = torch.randn(7, F), torch.rand(7, F)
        assert torch.equal(d(x, s), torch.sum(x * torch.matmul(s, w), dim=1))
    # the fixture's reference init: same bound
    for c in CASES:
        g = load_golden(c)
        F = g["disc_init_weight"].shape[0]
        assert np.abs(g["disc_init_weight"]).max() <= 1.0 / math.sqrt(F)
    assert list(inspect.signature(Discriminator.forward).parameters) == ["self", "x", "summary"]


def test_cycle_index_is_the_references():
    from geossl_amd.pretrain_3DInfoGraph import cycle_index

    def ref(num, shift):   # examples/util.py:19-22
        arr = torch.arange(num) + shift
        arr[-shift:] = torch.arange(shift)
        return arr
    for B in (1, 2, 3, 7, 128):
        assert torch.equal(cycle_index(B, 1), ref(B, 1))
        assert torch.equal(cycle_index(B, 1), tw.cycle_index(B))
    assert cycle_index(1, 1).tolist() == [0]
    assert torch.equal(cycle_index(6, 2), ref(6, 2))


@pytest.mark.parametrize("case", CASES)
def test_twin_reproduces_g20(case):
    g = load_golden(case)
    meta = json.loads(str(g["meta"]))
    batch = torch.from_numpy(g["batch"])
    B = g["sizes"].size
    x = torch.from_numpy(g["node_repr"]).double().requires_grad_()
    # the backbone's readout is the twin's readout of node_repr
    _close(tw.readout(x.detach(), batch, B, meta["readout"]), g["molecule_repr"], 1e-5, "readout")
    m = torch.from_numpy(g["molecule_repr"]).double().requires_grad_()
    W = torch.from_numpy(g["disc_weight"]).double().requires_grad_()
    loss, pos, neg = tw.infograph_loss(x, m, W, batch)
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    _close(pos.detach(), g["pos_score"], 1e-5, "pos")
    _close(neg.detach(), g["neg_score"], 1e-5, "neg")
    cp, cn = tw.counts(g["pos_score"], g["neg_score"])
    assert (cp + cn) / (2.0 * x.size(0)) == pytest.approx(float(g["acc"]), abs=1e-6)
    loss.backward()
    _close(m.grad, g["grad_molecule_repr"], 1e-5, "d molecule_repr")
    _close(W.grad, g["grad_disc_weight"], 1e-5, "d W")
    # node_repr's retained gradient holds the readout's path too: partial + the readout's backward of d molecule_repr
    total = x.grad + readout_expand(m.grad, batch, B, meta["readout"])
    _close(total, g["grad_node_repr"], 1e-5, "d node_repr")


def readout_expand(dm, batch, B, kind):
    d = dm[batch]
    if kind == "mean":
        cnt = torch.bincount(batch, minlength=B).clamp(min=1).to(torch.float64)
        d = d / cnt[batch][:, None]
    return d


@pytest.mark.parametrize("case", CASES)
def test_do_infograph_aten_on_cpu_reproduces_g20(case):
    """do_InfoGraph on CPU tensors (the reference's ATen code) gives G20's loss, acc and gradients."""
    from geossl_amd.pretrain_3DInfoGraph import Discriminator, do_InfoGraph
    g = load_golden(case)
    meta = json.loads(str(g["meta"]))
    batch = types.SimpleNamespace(batch=torch.from_numpy(g["batch"]))
    B = g["sizes"].size
    x = torch.from_numpy(g["node_repr"]).requires_grad_()
    m = torch.from_numpy(g["molecule_repr"]).requires_grad_()
    d = Discriminator(meta["emb_dim"])
    with torch.no_grad():
        d.weight.copy_(torch.from_numpy(g["disc_weight"]))
    loss, acc = do_InfoGraph(x, m, batch, torch.nn.BCEWithLogitsLoss(), d)
    assert isinstance(acc, float) and acc == float(g["acc"])
    assert loss.dtype == torch.float32 and abs(loss.item() - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))
    loss.backward()
    _close(m.grad, g["grad_molecule_repr"], 1e-5, "d molecule_repr")
    _close(d.weight.grad, g["grad_disc_weight"], 1e-5, "d W")
    total = x.grad.double() + readout_expand(m.grad.double(), batch.batch, B, meta["readout"])
    _close(total, g["grad_node_repr"], 1e-5, "d node_repr")


def test_fallback_selection():
    """The fused path takes a stock mean BCEWithLogitsLoss and the reference Discriminator at a served width on the GPU;
    everything else runs the reference's ATen code."""
    from geossl_amd import ops
    from geossl_amd.pretrain_3DInfoGraph import (Discriminator, InfoGraphTrainer, _fused_batch_ok, _fused_loss_ok,
                                                 criterion_ok, do_3DInfoGraph, do_InfoGraph, fused_head_ok, readout_of)
    assert [F for F in (32, 48, 64, 96, 128, 192, 256, 512) if ops.infograph_width_ok(F)] == [64, 128, 256]
    assert criterion_ok(torch.nn.BCEWithLogitsLoss())
    for crit in (torch.nn.BCEWithLogitsLoss(pos_weight=torch.ones(1)), torch.nn.BCEWithLogitsLoss(weight=torch.ones(1)),
                 torch.nn.BCEWithLogitsLoss(reduction="sum"), torch.nn.BCELoss()):
        assert not criterion_ok(crit)

    class SubLoss(torch.nn.BCEWithLogitsLoss):
        pass
    assert not criterion_ok(SubLoss())

    class Sub(Discriminator):
        pass
    for d in (Discriminator(128), Sub(128), Discriminator(96)):   # (CPU weights, a subclass, an unserved width)
        assert not fused_head_ok(d)
    cpu = types.SimpleNamespace(batch=torch.zeros(4, dtype=torch.long), positions=torch.zeros(4, 3))
    assert not _fused_batch_ok(cpu)
    assert not _fused_loss_ok(torch.zeros(4, 128), torch.zeros(1, 128), cpu, torch.nn.BCEWithLogitsLoss(),
                              Discriminator(128))
    # a pos_weight criterion on CPU tensors runs the reference's code and uses the weight
    torch.manual_seed(0)
    x, m = torch.randn(6, 64), torch.randn(2, 64)
    b = types.SimpleNamespace(batch=torch.tensor([0, 0, 0, 1, 1, 1]))
    d = Discriminator(64)
    l1, _ = do_InfoGraph(x, m, b, torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([3.0])), d)
    l0, _ = do_InfoGraph(x, m, b, torch.nn.BCEWithLogitsLoss(), d)
    assert abs(l1.item() - l0.item()) > 1e-6
    sch = types.SimpleNamespace(readout="mean", scale=None)
    assert readout_of(sch) == "mean" and readout_of(types.SimpleNamespace(readout="add")) == "add"
    assert readout_of(types.SimpleNamespace(readout="mean", scale=2.0)) is None
    assert readout_of(types.SimpleNamespace(readout="max")) is None
    assert list(inspect.signature(do_InfoGraph).parameters) == ["node_repr", "molecule_repr", "batch", "criterion",
                                                                "infograph_discriminator_SSL_model"]
    assert list(inspect.signature(do_3DInfoGraph).parameters)[:5] == ["args", "batch", "model", "discriminator",
                                                                       "criterion"]
    sig = inspect.signature(InfoGraphTrainer)
    for name in ("model", "discriminator", "lr", "weight_decay", "model_3d", "use_graph"):
        assert name in sig.parameters, name


def test_bucket_modules_accept_a_width_128_discriminator_only():
    from geossl_amd import bucket
    from geossl_amd.pretrain_3DInfoGraph import Discriminator
    assert not bucket.modules_ok(types.SimpleNamespace(), Discriminator(128), None)   # (not a backbone)


def test_new_abi_symbols_declared_bound_and_exported():
    from geossl_amd import _lib
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in NEW_SYMBOLS + ("geossl_infograph_width_ok",):
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"\bint64_t geossl_infograph_fwd_workspace_floats\(", h)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert [F for F in (32, 64, 128, 256, 512) if lib.geossl_infograph_width_ok(F)] == [64, 128, 256]
