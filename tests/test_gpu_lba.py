"""GPU tests of LBA fine-tuning (geossl_amd/finetune_lba.py): fixture G24 - the unmodified reference's finetune_lba.py
step on pocket-sized structures - through do_LBA and through the documented trainer (eager and with use_graph=True),
eval_LBA against the stored metrics, and three steps of do_LBA + torch.optim.Adam against the reference's ATen lines on
our backbone."""
import json
import os
import types

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from helpers import fill_module_, grad_summary, t, unique_named_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G24 = sorted(f[:-4] for f in os.listdir(os.path.join(REPO, "tests", "golden")) if f.startswith("g24_lba_"))
TOL_OUT, TOL_GRAD = 1e-5, 1e-4


def _setup(case):
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    g = load_golden(case)
    meta, cfg = json.loads(str(g["meta"])), json.loads(str(g["cfg"]))
    model = fill_module_(SchNet(**cfg) if meta["kind"] == "schnet" else PaiNN(**cfg)).to(DEV)
    head = (fill_module_(torch.nn.Linear(meta["emb_dim"], 1)) if meta["kind"] == "schnet"
            else fill_module_(model.create_output_layers())).to(DEV)
    rei = t(g["radius_edge_index"], DEV).long() if "radius_edge_index" in g else None

    def batch():
        b = pg.Batch(t(g["x"], DEV), t(g["positions"], DEV), t(g["batch"], DEV), None, radius_edge_index=rei,
                     num_graphs=len(g["sizes"]), sizes=g["sizes"])
        b.y = t(g["y"], DEV)
        return b
    return g, meta, model, head, batch, types.SimpleNamespace(model_3d=meta["kind"])


def _check(g, model, head, loss, case):
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert rel_err(loss.detach().cpu(), g["loss"]) < TOL_OUT, case
    for name, p in head.named_parameters():
        assert rel_err(p.grad.cpu(), g["head_grad/" + name]) < TOL_GRAD, (case, name)
    grads = unique_named_grads(model)
    for k in g:
        if k.startswith("gsum/"):
            got = grad_summary(grads[k.split("/", 1)[1]].cpu())
            assert rel_err(got, g[k]) < TOL_GRAD or float(np.abs(g[k]).max()) < 1e-8, (case, k)


@pytest.mark.parametrize("case", G24)
def test_g24_do_lba(case):
    from geossl_amd.finetune_lba import do_LBA
    g, meta, model, head, make, args = _setup(case)
    loss = do_LBA(args, make(), model, head, torch.nn.MSELoss())
    loss.backward()
    _check(g, model, head, loss, case)


@pytest.mark.parametrize("case", G24)
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_g24_through_the_trainer(case, use_graph):
    """SupervisedTrainer(model, head, 0.0, 1.0, task_id=0, loss="mse") is the trainer of finetune_lba.py; with
    use_graph=True a structure above 255 atoms gets the same loss and gradients as the eager step (its batch is captured
    per structure on the second sighting, or runs eagerly)."""
    from geossl_amd.pretrain_Supervised import SupervisedTrainer
    g, meta, model, head, make, args = _setup(case)
    tr = SupervisedTrainer(model, head, 0.0, 1.0, task_id=0, loss="mse", lr=0.0, model_3d=meta["kind"],
                           use_graph=use_graph, graph_mode="structure" if use_graph else "auto")
    b = make()
    for _ in range(2 if use_graph else 1):
        loss = tr._graph_fwd_bwd(b) if use_graph else tr._eager(b)    # (the step without Adam: the gradients stay)
    _check(g, model, head, loss, case)


@pytest.mark.parametrize("case", G24)
def test_g24_eval_lba(case):
    from geossl_amd.finetune_lba import eval_LBA
    g, meta, model, head, make, args = _setup(case)
    rmse, pearson, spearman, y_true, y_pred = eval_LBA(args, [make()], model, head)
    assert rel_err(torch.tensor(y_pred), g["pred"]) < TOL_OUT and np.array_equal(np.float32(y_true), g["y"])
    assert abs(rmse - float(g["rmse"])) < TOL_OUT * float(g["rmse"])
    assert abs(pearson - float(g["pearson"])) < TOL_OUT and abs(spearman - float(g["spearman"])) < TOL_OUT


def test_do_lba_serves_b1():
    """train() of finetune_lba.py has no pred.size()[0] line: one structure per batch is a step like any other."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.finetune_lba import do_LBA
    g, meta, model, head, make, args = _setup("g24_lba_schnet_reduced")
    n = int(g["sizes"][0])
    b = pg.Batch(t(g["x"][:n], DEV), t(g["positions"][:n], DEV), t(g["batch"][:n], DEV), None, num_graphs=1, sizes=[n])
    b.y = t(g["y"][:1], DEV)
    loss = do_LBA(args, b, model, head)
    loss.backward()
    ref = torch.nn.MSELoss()(head(model(b.x, b.positions, b.batch)).reshape(1), b.y)
    assert rel_err(loss.detach().cpu(), ref.detach().cpu()) < TOL_OUT and torch.isfinite(head.weight.grad).all()


def test_three_adam_steps_match_the_reference_lines():
    """do_LBA + a stock torch.optim.Adam against :36-51 written in ATen on our backbone."""
    from geossl_amd.finetune_lba import do_LBA
    g, meta, _, _, make, args = _setup("g24_lba_schnet_reduced")

    def loop(fused):
        _, _, model, head, _, _ = _setup("g24_lba_schnet_reduced")
        opt = torch.optim.Adam(list(model.parameters()) + list(head.parameters()), lr=1e-4)
        criterion = torch.nn.MSELoss()
        losses = []
        for _ in range(3):
            batch = make()
            if fused:
                loss = do_LBA(args, batch, model, head, criterion)
            else:
                pred = head(model(batch.x, batch.positions, batch.batch)).squeeze()
                loss = criterion(pred, batch.y)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses, model, head
    ref, m1, h1 = loop(False)
    got, m2, h2 = loop(True)
    np.testing.assert_allclose(got, ref, rtol=1e-4)
    assert ref[2] != ref[0]
    assert rel_err(h2.weight.detach().cpu(), h1.weight.detach().cpu()) < TOL_GRAD
    assert rel_err(m2.lin2.weight.detach().cpu(), m1.lin2.weight.detach().cpu()) < TOL_GRAD
