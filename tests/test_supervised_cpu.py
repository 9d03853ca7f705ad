"""CPU tests of Supervised pretraining / property fine-tuning: the fp64 twin and do_Supervised's ATen fallback against
fixture G21 (the reference run verbatim, tests/golden/make_golden_supervised.py), the fallback selection, B = 1, and the C
ABI of the new kernels."""
import glob
import inspect
import json
import os
import re
import types

import pytest
import torch

import supervised_twin as tw
from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(REPO, "tests", "golden", "g21_supervised_*.npz")))
NEW_SYMBOLS = ("geossl_property_fwd", "geossl_property_fwd_dyn", "geossl_property_predict",
               "geossl_property_predict_dyn", "geossl_property_bwd", "geossl_property_bwd_dyn",
               "geossl_property_targets", "geossl_property_width_ok")


def _close(got, want, rel, what):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double().reshape(got.shape)
    scale = max(float(want.abs().max()), 1e-6)
    assert float((got - want).abs().max()) <= rel * scale, what


def _head_params(g):
    """(names, tensors) of the head's parameters in kernel order: (w, b) or (W1, b1, w2, b2)."""
    keys = ["weight", "bias"] if "head/weight" in g else ["0.weight", "0.bias", "1.weight", "1.bias"]
    return keys, [torch.from_numpy(g["head/" + k]) for k in keys]


def test_g21_cases_present():
    assert len(CASES) == 5
    gs = {c: load_golden(c) for c in CASES}
    metas = {c: json.loads(str(g["meta"])) for c, g in gs.items()}
    assert {m["kind"] for m in metas.values()} == {"schnet", "painn"}
    assert {m["readout"] for m in metas.values()} == {"mean", "add"}
    assert {m["loss"] for m in metas.values()} == {"mae", "mse"}
    assert {(m["kind"], m["loss"]) for m in metas.values()} >= {("painn", "mae"), ("painn", "mse")}
    assert any(json.loads(str(g["cfg"])).get("cutoff") == 10.0 for g in gs.values())   # SchNet full
    for c, g in gs.items():
        assert (g["sizes"] == 1).any() and g["sizes"].size > 1, c          # ragged with a 1-atom molecule
        assert metas[c]["T"] > 1 and g["y"].size == g["sizes"].size * metas[c]["T"], c
        assert os.path.getsize(os.path.join(REPO, "tests", "golden", c + ".npz")) < 320 * 1024, c


@pytest.mark.parametrize("case", CASES)
def test_twin_reproduces_g21(case):
    g = load_golden(case)
    meta = json.loads(str(g["meta"]))
    B = g["sizes"].size
    m = torch.from_numpy(g["molecule_repr"]).double().requires_grad_()
    keys, ps = _head_params(g)
    ps = [p.double().requires_grad_() for p in ps]
    pred = tw.head(m, ps)
    _close(pred.detach(), g["pred"], 1e-5, "pred")
    t = tw.target(g["y"], B, int(g["task_id"]), float(g["TRAIN_mean"]), float(g["TRAIN_std"]))
    loss = tw.loss(pred, t, meta["loss"])
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    loss.backward()
    _close(m.grad, g["grad_molecule_repr"], 1e-5, "d molecule_repr")
    for k, p in zip(keys, ps):
        _close(p.grad, g["head_grad/" + k], 1e-5, k)


class _Fixed(torch.nn.Module):
    """A stand-in backbone on CPU that returns the fixture's molecule_3D_repr (our backbones run on the GPU only)."""

    def __init__(self, rep, readout="mean"):
        super().__init__()
        self.rep = rep
        self.readout = readout
        self.calls = []

    def forward(self, *a):
        self.calls.append(a)
        return self.rep


def _cpu_head(keys, ps):
    """The fixture's head on CPU: nn.Linear(F, 1), or Linear -> SiLU -> Linear with PaiNN's output-layer weights."""
    if len(ps) == 2:
        head = torch.nn.Linear(ps[0].size(1), 1)
        mods = [head]
    else:
        head = torch.nn.Sequential(torch.nn.Linear(ps[0].size(1), ps[0].size(0)), torch.nn.SiLU(),
                                   torch.nn.Linear(ps[2].size(1), 1))
        mods = [head[0], head[2]]
    with torch.no_grad():
        for i, mod in enumerate(mods):
            mod.weight.copy_(ps[2 * i])
            mod.bias.copy_(ps[2 * i + 1])
    return head, mods


@pytest.mark.parametrize("case", CASES)
def test_do_supervised_aten_on_cpu_reproduces_g21(case):
    """do_Supervised on CPU tensors runs the reference's own lines and gives G21's loss and gradients."""
    from geossl_amd.pretrain_Supervised import do_Supervised
    g = load_golden(case)
    meta = json.loads(str(g["meta"]))
    rep = torch.from_numpy(g["molecule_repr"]).requires_grad_()
    model = _Fixed(rep)
    keys, ps = _head_params(g)
    head, mods = _cpu_head(keys, ps)
    batch = types.SimpleNamespace(x=torch.from_numpy(g["x"]), positions=torch.from_numpy(g["positions"]),
                                  batch=torch.from_numpy(g["batch"]), y=torch.from_numpy(g["y"]),
                                  radius_edge_index=torch.from_numpy(g["radius_edge_index"]) if "radius_edge_index" in g
                                  else None)
    args = types.SimpleNamespace(model_3d=meta["kind"], loss=meta["loss"])
    loss = do_Supervised(args, batch, model, head, float(g["TRAIN_mean"]), float(g["TRAIN_std"]),
                         task_id=int(g["task_id"]))
    assert loss.dtype == torch.float32 and abs(loss.item() - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))
    # the backbone call the reference makes: SchNet gets x[:, 0], PaiNN batch.x unsliced with the radius edges
    a = model.calls[0]
    if meta["kind"] == "schnet":
        assert len(a) == 3 and torch.equal(a[0], batch.x[:, 0])
    else:
        assert len(a) == 4 and a[0] is batch.x and a[2] is batch.radius_edge_index
    loss.backward()
    _close(rep.grad, g["grad_molecule_repr"], 1e-5, "d molecule_repr")
    for i, mod in enumerate(mods):
        _close(mod.weight.grad, g["head_grad/" + keys[2 * i]], 1e-5, "dW%d" % i)
        _close(mod.bias.grad, g["head_grad/" + keys[2 * i + 1]], 1e-5, "db%d" % i)


def test_b1_raises_like_the_reference():
    """pred.squeeze() is 0-d at B = 1 and the reference's pred.size()[0] raises IndexError; do_Supervised does too."""
    from geossl_amd.pretrain_Supervised import _raise_like_squeeze, do_Supervised
    model = _Fixed(torch.randn(1, 64))
    head = torch.nn.Linear(64, 1)
    batch = types.SimpleNamespace(x=torch.zeros(3, 2, dtype=torch.long), positions=torch.zeros(3, 3),
                                  batch=torch.zeros(3, dtype=torch.long), y=torch.randn(8))
    args = types.SimpleNamespace(model_3d="schnet", loss="mae")
    with pytest.raises(IndexError):
        do_Supervised(args, batch, model, head, 0.0, 1.0)
    with pytest.raises(IndexError):
        _raise_like_squeeze(1)
    _raise_like_squeeze(2)


def test_fallback_selection():
    """The fused path takes stock mean L1 / MSE criteria, Linear(F, 1) or the default two-layer output head, an unscaled
    backbone with a mean / add readout at F = 64 / 128 / 256 and CUDA batches; everything else runs the reference's
    lines."""
    from geossl_amd import ops
    from geossl_amd.Geom3D.models.painn import Dense, PaiNN
    from geossl_amd.Geom3D.models.schnet import SchNet
    from geossl_amd.pretrain_Supervised import (SupervisedTrainer, _fused_batch_ok, criterion_of, do_Supervised,
                                                fused_ok, head_params, loss_kind, predict_Supervised, readout_of)
    assert [F for F in (32, 48, 64, 96, 128, 192, 256, 512) if ops.property_width_ok(F)] == [64, 128, 256]
    assert loss_kind(torch.nn.L1Loss()) == "mae" and loss_kind(torch.nn.MSELoss()) == "mse"
    assert type(criterion_of(types.SimpleNamespace(loss="mae"))) is torch.nn.L1Loss
    assert type(criterion_of(types.SimpleNamespace(loss="mse"))) is torch.nn.MSELoss
    with pytest.raises(ValueError):
        criterion_of(types.SimpleNamespace(loss="huber"))

    class SubL1(torch.nn.L1Loss):
        pass
    for crit in (SubL1(), torch.nn.L1Loss(reduction="sum"), torch.nn.MSELoss(reduction="none"), torch.nn.HuberLoss()):
        assert loss_kind(crit) is None
    # heads: CPU parameters, num_tasks > 1, no bias, unserved widths, other layer stacks
    for head in (torch.nn.Linear(128, 1), torch.nn.Linear(128, 2), torch.nn.Linear(128, 1, bias=False),
                 torch.nn.Linear(96, 1), torch.nn.Sequential(torch.nn.Linear(128, 64), torch.nn.SiLU(),
                                                              torch.nn.Linear(64, 1))):
        assert head_params(head) is None
    painn = PaiNN(n_atom_basis=128, n_interactions=1, n_rbf=20, cutoff=5.0, n_out=1, readout="add", max_z=9)
    out = painn.create_output_layers()
    assert [type(m) for m in out] == [Dense, Dense] and out[0].out_features == 64 and out[1].in_features == 64
    assert head_params(out) is None    # (CPU parameters)
    assert readout_of(painn) == "add"
    sch = SchNet(hidden_channels=64, num_filters=64, num_interactions=1, num_gaussians=8, cutoff=5.0, node_class=9)
    assert readout_of(sch) == "mean"
    sch.mean, sch.std = 1.0, 2.0
    assert readout_of(sch) is None
    sch2 = SchNet(hidden_channels=64, num_filters=64, num_interactions=1, num_gaussians=8, cutoff=5.0, node_class=9,
                  atomref=torch.zeros(100, 1))
    assert readout_of(sch2) is None
    assert readout_of(types.SimpleNamespace(readout="mean", scale=None)) is None   # (not one of our backbones)
    assert not fused_ok(sch, torch.nn.Linear(64, 1), torch.nn.L1Loss())
    cpu = types.SimpleNamespace(batch=torch.zeros(4, dtype=torch.long), positions=torch.zeros(4, 3), y=torch.zeros(4),
                                num_graphs=1)
    assert not _fused_batch_ok(cpu, 0)
    # a criterion the kernels do not have runs the reference's lines and uses it
    torch.manual_seed(0)
    rep = torch.randn(5, 64)
    head = torch.nn.Linear(64, 1)
    b = types.SimpleNamespace(x=torch.zeros(10, 2, dtype=torch.long), positions=torch.zeros(10, 3),
                              batch=torch.arange(5).repeat_interleave(2), y=torch.randn(15))
    args = types.SimpleNamespace(model_3d="schnet", loss="mae")
    l_h = do_Supervised(args, b, _Fixed(rep), head, 0.5, 2.0, task_id=1, criterion=torch.nn.HuberLoss())
    l_1 = do_Supervised(args, b, _Fixed(rep), head, 0.5, 2.0, task_id=1)
    pred = head(rep).squeeze()
    t = (b.y.view(5, -1)[:, 1] - 0.5) / 2.0
    assert l_h.item() == torch.nn.HuberLoss()(pred, t).item()
    assert l_1.item() == torch.nn.L1Loss()(pred, t).item()
    p = predict_Supervised(args, b, _Fixed(rep), head, 0.5, 2.0)
    assert torch.equal(p, pred.detach() * 2.0 + 0.5)
    assert list(inspect.signature(do_Supervised).parameters)[:8] == [
        "args", "batch", "model", "graph_pred_linear", "TRAIN_mean", "TRAIN_std", "task_id", "criterion"]
    assert inspect.signature(do_Supervised).parameters["task_id"].default == 6
    assert list(inspect.signature(predict_Supervised).parameters) == [
        "args", "batch", "model", "graph_pred_linear", "TRAIN_mean", "TRAIN_std"]
    sig = inspect.signature(SupervisedTrainer)
    for name in ("model", "graph_pred_linear", "TRAIN_mean", "TRAIN_std", "task_id", "loss", "lr", "weight_decay",
                 "model_3d", "use_graph"):
        assert name in sig.parameters, name
    assert hasattr(SupervisedTrainer, "set_lr")


def test_bucket_modules_reject_cpu_heads():
    from geossl_amd import bucket
    assert not bucket.modules_ok(types.SimpleNamespace(), torch.nn.Linear(128, 1), None)   # (not a backbone)


def test_new_abi_symbols_declared_bound_and_exported():
    from geossl_amd import _lib
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"\bint64_t geossl_property_workspace_floats\(", h)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert [F for F in (16, 32, 64, 96, 128, 192, 256, 512) if lib.geossl_property_width_ok(F)] == [64, 128, 256]


def test_property_head_builds_without_packed_fp32():
    from geossl_amd import build
    assert build.SOURCE_FLAGS.get("property_head.hip") == ["-fno-slp-vectorize"]
