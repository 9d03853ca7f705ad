"""CPU tests of GeoSSL-RR (--GeoSSL_option RR): the fp64 twin (tests/rr_twin.py) against torch autograd, the
AutoEncoder's surface, the ATen route of the heads against fixture G27 (the reference's do_RR run verbatim on this
project's AutoEncoder, tests/golden/make_golden_rr.py), the B = 1 error and the C ABI of the new kernels."""
import copy
import glob
import inspect
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import rr_twin as tw
from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(REPO, "tests", "golden", "g27_rr_*.npz")))
NEW_SYMBOLS = ("geossl_rr_head_fwd", "geossl_rr_head_bwd", "geossl_rr_head_width_ok")
PARAM_NAMES = ["fc_layers.0.weight", "fc_layers.0.bias", "fc_layers.1.weight", "fc_layers.1.bias", "fc_layers.3.weight",
               "fc_layers.3.bias"]


def heads_of(g, meta, dtype=torch.float32, device="cpu"):
    """The two heads of a G27 case with their stored initial parameters."""
    from geossl_amd.Geom3D.models import AutoEncoder
    F = g["X"].shape[1]
    heads = []
    for k in (1, 2):
        h = AutoEncoder(emb_dim=F, loss=meta["AE_loss"], detach_target=meta["detach_target"], beta=1)
        with torch.no_grad():
            for name, p in h.named_parameters():
                p.copy_(torch.from_numpy(g["head%d/param/%s" % (k, name)]))
        heads.append(h.to(dtype).to(device))
    return heads


def test_g27_cases_present():
    assert len(CASES) == 6
    metas = [json.loads(str(load_golden(c)["meta"])) for c in CASES]
    assert {m["AE_loss"] for m in metas} == {"l1", "l2", "cosine"}
    assert {m["kind"] for m in metas} == {"schnet", "painn"}
    assert {m["detach_target"] for m in metas} == {True, False} and {m["normalize"] for m in metas} == {True, False}
    assert min(load_golden(c)["X"].shape[0] for c in CASES) == 2
    assert sorted({load_golden(c)["X"].shape[1] for c in CASES}) == [32, 128]
    for m in metas:   # the kink band of the maker: 1e-4, several times the fp32 rounding of z and p
        assert m["kink_margin"] > 1e-4 and m["z_fp32_vs_fp64"] < 5e-5 and m["p_fp32_vs_fp64"] < 5e-5


def test_models_export_the_autoencoder():
    from geossl_amd.Geom3D import models
    from geossl_amd.Geom3D.models import AutoEncoder, PaiNN, SchNet  # noqa: F401  (the reference's import line resolves)
    assert models.AutoEncoder is AutoEncoder
    sig = inspect.signature(AutoEncoder)
    assert list(sig.parameters) == ["emb_dim", "loss", "detach_target", "beta"] and sig.parameters["beta"].default == 1
    with pytest.raises(ValueError):
        AutoEncoder(8, "huber", True)


def test_autoencoder_state_dict_keys_and_shapes():
    from geossl_amd.Geom3D.models import AutoEncoder
    ae = AutoEncoder(emb_dim=128, loss="l2", detach_target=True, beta=1)
    sd = ae.state_dict()
    assert list(sd) == PARAM_NAMES[:4] + ["fc_layers.1.running_mean", "fc_layers.1.running_var",
                                          "fc_layers.1.num_batches_tracked"] + PARAM_NAMES[4:]
    assert [n for n, _ in ae.named_parameters()] == PARAM_NAMES
    assert tuple(sd["fc_layers.0.weight"].shape) == (128, 128) == tuple(sd["fc_layers.3.weight"].shape)
    for k in ("fc_layers.0.bias", "fc_layers.1.weight", "fc_layers.1.bias", "fc_layers.1.running_mean",
              "fc_layers.1.running_var", "fc_layers.3.bias"):
        assert tuple(sd[k].shape) == (128,), k
    assert sd["fc_layers.1.num_batches_tracked"].dtype == torch.long
    assert [type(m) for m in ae.fc_layers] == [torch.nn.Linear, torch.nn.BatchNorm1d, torch.nn.ReLU, torch.nn.Linear]
    x, y = torch.randn(5, 128), torch.randn(5, 128)
    out = ae(x, y)
    assert out.dim() == 0 and out.dtype == torch.float32


@pytest.mark.parametrize("kind", ["l1", "l2", "cosine"])
@pytest.mark.parametrize("detach", [True, False])
@pytest.mark.parametrize("B", [2, 3, 9])
def test_twin_matches_torch_autograd_in_fp64(kind, detach, B):
    from geossl_amd.Geom3D.models import AutoEncoder
    from geossl_amd.pretrain_GeoSSL import rr_heads_aten
    torch.manual_seed(10 * B + len(kind))
    F = 16
    heads = [AutoEncoder(F, kind, detach).double() for _ in range(2)]
    with torch.no_grad():
        for h in heads:
            h.fc_layers[1].weight.uniform_(0.5, 1.5)
            h.fc_layers[1].bias.uniform_(-0.5, 0.5)
    before = [[b.clone() for b in (h.fc_layers[1].running_mean, h.fc_layers[1].running_var,
                                   h.fc_layers[1].num_batches_tracked)] for h in heads]
    X = torch.randn(B, F, dtype=torch.float64, requires_grad=True)
    Y = torch.randn(B, F, dtype=torch.float64, requires_grad=True)
    t = tw.step(X, Y, list(heads[0].parameters()), list(heads[1].parameters()), kind, detach)
    loss = rr_heads_aten(heads[0], heads[1], X, Y)
    loss.backward()
    assert abs(loss.item() - t["loss"].item()) <= 1e-12 * max(1.0, abs(loss.item()))
    params = list(heads[0].parameters()) + list(heads[1].parameters())
    for got, want in [(t["dX"], X.grad), (t["dY"], Y.grad)] + [(g, p.grad) for g, p in zip(t["grads"], params)]:
        assert float((got - want).abs().max()) <= 1e-11 * max(float(want.abs().max()), 1e-3)
    for h, b0, th in zip(heads, before, t["heads"]):
        bn = h.fc_layers[1]
        rm, rv, nb = tw.buffers_after(b0, th["mean"], th["var"], B, bn.momentum)
        assert float((rm - bn.running_mean).abs().max()) < 1e-13 and float((rv - bn.running_var).abs().max()) < 1e-13
        assert nb == int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("case", CASES)
def test_aten_route_reproduces_g27_on_cpu(case):
    """The heads' ATen route (what do_RR runs on CPU tensors, in eval mode, for subclasses and at unserved widths) on the
    fixture's X / Y: the reference's loss, gradients and BatchNorm buffers."""
    from geossl_amd.pretrain_GeoSSL import rr_heads_loss
    g = load_golden(case)
    meta = json.loads(str(g["meta"]))
    a, b = heads_of(g, meta)
    X = torch.from_numpy(g["X"]).requires_grad_()
    Y = torch.from_numpy(g["Y"]).requires_grad_()
    loss = rr_heads_loss(a, b, X, Y)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    ref = float(g["loss"])
    assert abs(loss.item() - ref) <= 1e-5 * max(abs(ref), 1e-3)
    loss.backward()
    close = lambda got, want: float((got - torch.from_numpy(want)).abs().max()) <= 1e-5 * max(float(np.abs(want).max()), 1e-6)
    assert close(X.grad, g["grad_X"]) and close(Y.grad, g["grad_Y"])
    for k, h in ((1, a), (2, b)):
        for name, p in h.named_parameters():
            if name == "fc_layers.0.bias":
                # exactly zero in exact arithmetic (BatchNorm subtracts the column mean, so a shift of its input does not
                # reach the loss): the fixture holds the rounding noise of sum_b dZ_b.  Absolute check at 1e-5 of the
                # scale of dZ, taken from the same layer's weight gradient sum_b dZ_b x_b^T over the largest input.
                scale = float(np.abs(g["head%d/grad/fc_layers.0.weight" % k]).max()) / float(
                    max(np.abs(g["X"]).max(), np.abs(g["Y"]).max()))
                assert float(p.grad.abs().max()) <= 1e-5 * scale and float(np.abs(g["head%d/grad/%s" % (k, name)]).max()) <= 1e-5 * scale
                continue
            assert close(p.grad, g["head%d/grad/%s" % (k, name)]), (k, name)
        bn = h.fc_layers[1]
        assert close(bn.running_mean, g["head%d/running_mean" % k]) and close(bn.running_var, g["head%d/running_var" % k])
        assert int(bn.num_batches_tracked) == int(g["head%d/num_batches_tracked" % k]) == 1
    # and the fp64 twin on the same rows
    a64, b64 = heads_of(g, meta, torch.float64)
    t = tw.step(X.detach(), Y.detach(), list(a64.parameters()), list(b64.parameters()), meta["AE_loss"],
                meta["detach_target"])
    assert abs(t["loss"].item() - ref) <= 1e-5 * max(abs(ref), 1e-3)
    assert close(t["dX"].float(), g["grad_X"]) and close(t["dY"].float(), g["grad_Y"])


def test_batch_of_one_raises_torchs_own_error():
    from geossl_amd.Geom3D.models import AutoEncoder
    from geossl_amd.pretrain_GeoSSL import rr_heads_loss
    a, b = AutoEncoder(128, "l2", True), AutoEncoder(128, "l2", True)
    x = torch.randn(1, 128)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        rr_heads_loss(a, b, x, x.clone())
    a.eval(), b.eval()   # eval mode: running statistics, B = 1 is fine
    assert torch.isfinite(rr_heads_loss(a, b, x, x.clone()))


def test_fused_head_ok_refuses_what_the_kernels_do_not_serve():
    from geossl_amd import bucket
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.models import AutoEncoder

    class Sub(AutoEncoder):
        pass
    for h in (AutoEncoder(128, "l2", True), Sub(128, "l2", True), AutoEncoder(96, "l1", False),
              AutoEncoder(128, "cosine", True).eval()):   # (CPU parameters, a subclass, a width, eval mode)
        assert not pg.fused_head_ok(h)
    a = AutoEncoder(128, "l2", True)
    assert not pg.fused_heads_ok(a, a) and not pg.fused_heads_ok(a, None)
    assert not bucket.modules_ok(types.SimpleNamespace(), a, copy.deepcopy(a))   # (not a backbone)


def test_public_surface():
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    names = list(inspect.signature(pg.do_RR).parameters)
    assert names[:5] == ["args", "batch", "model", "mu", "sigma"]   # the reference's (:77), then ours
    assert {"AE_models", "noise", "device_noise", "graph", "kwargs"} <= set(names)
    assert pg.AE_model_01 is None and pg.AE_model_02 is None
    assert pg.RR.name == "RR" and pg.RR.views == 2 and not pg.RR.normalize
    assert pg.RR.noise_keys(types.SimpleNamespace()) == ("pos_noise",)
    k1 = pg.RR.graph_key(types.SimpleNamespace(model_3d="schnet", normalize=True, heads_key=("l1",)))
    k2 = pg.RR.graph_key(types.SimpleNamespace(model_3d="schnet", normalize=True, heads_key=("l2",)))
    assert k1 != k2 and k1[:3] == ("RR", "schnet", True)
    sig = inspect.signature(pg.RRTrainer)
    for p in ("model", "ae_01", "ae_02", "lr", "weight_decay", "mu", "sigma", "normalize", "model_3d", "use_graph",
              "graph_mode", "ae_lr"):
        assert p in sig.parameters, p
    assert sig.parameters["ae_lr"].default is None
    assert callable(pg.RRTrainer.set_lr) and callable(pg.rr_step_aten)
    with pytest.raises(RuntimeError):
        pg.do_RR(types.SimpleNamespace(model_3d="schnet"), None, None)
    assert ops.RR_LOSSES == {"l1": 0, "l2": 1, "cosine": 2}


def test_new_abi_symbols_declared_bound_and_exported():
    from geossl_amd import _lib
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"\bint64_t geossl_rr_head_workspace_floats\(", h)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert [F for F in (32, 64, 128, 256) if lib.geossl_rr_head_width_ok(F)] == [128]
    assert lib.geossl_rr_head_workspace_floats(257) == 4 * 257
