"""GPU tests of LEP fine-tuning (geossl_amd/finetune_lep.py, csrc/pair_head.hip): the pair-head kernels alone against
the fp64 twin; fixture G25 - the unmodified reference's finetune_lep.py step on paired pocket-sized structures - through
do_LEP, through LEPTrainer (eager and replayed, the labels a static input of the graph) and through eval_LEP; the
one-pass step against the reference's two-pass lines on our backbone; three Adam steps; what takes the fallback."""
import json
import os
import types

import numpy as np
import pytest
import torch

import lep_twin as lt
from conftest import load_golden, rel_err
from helpers import fill_module_, grad_summary, unique_named_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G25 = sorted(f[:-4] for f in os.listdir(os.path.join(REPO, "tests", "golden")) if f.startswith("g25_lep_"))
TOL_OUT, TOL_GRAD = 1e-5, 1e-4
TOL_KERNEL = 2e-5   # the bound test_gpu_supervised.py holds the property head to: fp32 readout sums and F-long dots


def _setup(case):
    from geossl_amd.Geom3D.dataloaders import BatchLEP
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    g = load_golden(case)
    meta, cfg = json.loads(str(g["meta"])), json.loads(str(g["cfg"]))
    model = fill_module_(SchNet(**cfg) if meta["kind"] == "schnet" else PaiNN(**cfg)).to(DEV)
    head = torch.nn.Linear(2 * meta["emb_dim"], 1)
    with torch.no_grad():   # (the filled head times the fixture's two constants: stored as it ran)
        head.weight.copy_(torch.from_numpy(g["head/weight"]))
        head.bias.copy_(torch.from_numpy(g["head/bias"]))
    head = head.to(DEV)
    items = lt.fixture_items(g)

    def batch():
        return BatchLEP.from_data_list(items).to(DEV)
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


# ---- the kernels alone ---------------------------------------------------------------------------------------------
SIZES_ACTIVE, SIZES_INACTIVE = (1, 5, 64, 3), (2, 1, 7, 65)   # B = 4 is no multiple of the tile; a one-atom structure
#                                                               on either side


@pytest.mark.parametrize("readout", ["mean", "add"])
@pytest.mark.parametrize("F", [32, 64, 128])
def test_pair_head_kernels_against_the_twin(F, readout):
    from geossl_amd import _lib, ops
    from geossl_amd.layout import get_layout, prepare_batch
    sizes = list(SIZES_ACTIVE + SIZES_INACTIVE)
    B, N = len(SIZES_ACTIVE), sum(sizes)
    gen = torch.Generator().manual_seed(2500 + F)
    h = torch.randn(N, F, generator=gen)
    w = torch.randn(1, 2 * F, generator=gen) / (2 * F) ** 0.5
    b = torch.randn(1, generator=gen)
    y = torch.tensor([1.0, 0.0, 0.0, 1.0])
    gout = torch.tensor(1.3)
    bvec = torch.repeat_interleave(torch.arange(2 * B), torch.tensor(sizes))

    hd, wd, bd = h.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    loss_t, z_t = lt.head_on_fused(hd, bvec, B, readout, wd, bd, y)
    (loss_t * gout.double()).backward()

    bv = bvec.to(DEV)
    prepare_batch(bv, None, sizes, lazy=True)
    lay = get_layout(bv)
    assert lay.B == 2 * B and not lay.sparse
    hg, wg, bg, yg, gg = (t_.to(DEV) for t_ in (h, w, b, y, gout))
    kind = ops.PROPERTY_READOUTS[readout]
    nws = int(_lib.load().geossl_pair_head_workspace_floats(B))
    assert nws >= 2 * B

    def run():
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
        m, z, zp, loss, dh, dw, db = nan(2 * B, F), nan(B), nan(B), nan(1), nan(N, F), nan(1, 2 * F), nan(1)
        ws = nan(nws)
        _lib.call("geossl_pair_head_fwd", _lib.ptr(hg), N, F, _lib.ptr(lay.mol_ptr), B, kind, _lib.ptr(wg), _lib.ptr(bg),
                  _lib.ptr(yg), _lib.ptr(m), _lib.ptr(z), _lib.ptr(ws), _lib.ptr(loss), _lib.stream())
        _lib.call("geossl_pair_head_predict", _lib.ptr(hg), N, F, _lib.ptr(lay.mol_ptr), B, kind, _lib.ptr(wg),
                  _lib.ptr(bg), _lib.ptr(zp), _lib.stream())
        ws2 = nan(nws)
        _lib.call("geossl_pair_head_bwd", N, F, _lib.ptr(lay.mol_ptr), B, kind, _lib.ptr(wg), _lib.ptr(m), _lib.ptr(z),
                  _lib.ptr(yg), _lib.ptr(gg), _lib.ptr(dh), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws2), 0, _lib.stream())
        return [t_.cpu() for t_ in (m, z, zp, loss, dh, dw, db)]

    first, second = run(), run()
    for a_, b_ in zip(first, second):
        assert torch.equal(a_, b_)
    m, z, zp, loss, dh, dw, db = first
    assert torch.equal(z, zp)
    assert torch.isfinite(dh).all() and torch.isfinite(m).all()
    errs = dict(m=rel_err(m, lt.readout(h, bvec, 2 * B, readout)), z=rel_err(z, z_t), loss=rel_err(loss, loss_t),
                dh=rel_err(dh, hd.grad), dw=rel_err(dw, wd.grad), db=rel_err(db, bd.grad))
    print("pair head F=%d %s:" % (F, readout), " ".join("%s %.2e" % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e < TOL_KERNEL, (k, e)

    # the autograd wrapper launches the same kernels: the same bits
    hq, wq, bq = hg.clone().requires_grad_(), wg.clone().requires_grad_(), bg.clone().requires_grad_()
    loss_o, z_o = ops.pair_head(hq, wq, bq, lay, readout, yg)
    (loss_o * gg).backward()
    assert torch.equal(loss_o.detach().cpu().reshape(1), loss) and torch.equal(z_o.cpu(), z)
    assert torch.equal(hq.grad.cpu(), dh) and torch.equal(wq.grad.cpu(), dw) and torch.equal(bq.grad.cpu(), db)
    assert torch.equal(ops.pair_predict(hg, wg, bg, lay, readout).cpu(), z)


def test_pair_head_refuses_other_widths():
    from geossl_amd import ops
    from geossl_amd.layout import get_layout
    assert [F for F in (16, 32, 48, 64, 128, 256) if ops.pair_head_width_ok(F)] == [32, 64, 128]
    bv = torch.tensor([0, 0, 1, 1], device=DEV)
    with pytest.raises(ValueError, match="pair head"):
        ops.pair_head(torch.zeros(4, 48, device=DEV), torch.zeros(1, 96, device=DEV), torch.zeros(1, device=DEV),
                      get_layout(bv), "mean", torch.zeros(1, device=DEV))


# ---- fixture G25 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G25)
def test_g25_do_lep(case):
    from geossl_amd.finetune_lep import do_LEP, fused_batch
    from geossl_amd.layout import get_layout
    g, meta, model, head, make, args = _setup(case)
    b = make()
    loss = do_LEP(args, b, model, head, torch.nn.BCEWithLogitsLoss())
    loss.backward()
    _check(g, model, head, loss, case)
    fb = fused_batch(b)
    assert fused_batch(b) is fb and fb.num_graphs == 2 * len(g["sizes_active"])   # built once per batch object
    assert get_layout(fb.batch).sparse == (case != "g25_lep_schnet_dense")   # one side above 255 atoms: sparse


@pytest.mark.parametrize("case", G25)
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_g25_through_the_trainer(case, use_graph):
    """The replayed step gives the fixture's loss and gradients, and the labels are DATA of its graph: a third replay
    with the labels flipped gives the loss of an eager step on the flipped labels."""
    from geossl_amd.finetune_lep import LEPTrainer
    g, meta, model, head, make, args = _setup(case)
    tr = LEPTrainer(model, head, lr=0.0, model_3d=meta["kind"], use_graph=use_graph,
                    graph_mode="structure" if use_graph else "auto")
    b = make()
    for _ in range(2 if use_graph else 1):
        loss = tr._graph_fwd_bwd(b) if use_graph else tr._eager(b)    # (the step without Adam: the gradients stay)
    _check(g, model, head, loss, case)
    if not use_graph:
        return
    assert tr.step_graphs.captures == 1
    b.y = 1 - b.y
    flipped = tr._graph_fwd_bwd(b)
    eager = tr._eager(b)
    assert tr.step_graphs.captures == 1
    assert rel_err(flipped.cpu(), eager.cpu()) < TOL_OUT
    assert abs(float(flipped) - float(loss)) > 1e-2 * float(loss)   # (it IS another loss)
    if meta["kind"] == "schnet":
        # another batch object with the same size sequences and other labels shares the graph
        b2 = make()
        b2.y = 1 - b2.y
        again = tr._graph_fwd_bwd(b2)
        assert tr.step_graphs.captures == 1 and rel_err(again.cpu(), eager.cpu()) < TOL_OUT


@pytest.mark.parametrize("case", G25)
def test_g25_eval_lep(case):
    from geossl_amd.finetune_lep import eval_LEP
    g, meta, model, head, make, args = _setup(case)
    bce, roc, pr, y_true, y_pred = eval_LEP(args, [make()], model, head)
    assert rel_err(torch.tensor(y_pred), g["pred"]) < TOL_OUT and np.array_equal(y_true, g["batch/y"].astype(np.float64))
    assert abs(bce - float(g["bce"])) < TOL_OUT * float(g["bce"])
    assert abs(roc - float(g["roc"])) < TOL_OUT and abs(pr - float(g["pr"])) < TOL_OUT


def _aten_lines(args, batch, model, head, criterion):
    """:33-45 written out, on our backbone: two passes."""
    if args.model_3d == "schnet":
        active = model(batch.x_active, batch.positions_active, batch.batch_active)
        inactive = model(batch.x_inactive, batch.positions_inactive, batch.batch_inactive)
    else:
        active = model(batch.x_active, batch.positions_active, batch.radius_edge_index_active, batch.batch_active)
        inactive = model(batch.x_inactive, batch.positions_inactive, batch.radius_edge_index_inactive,
                         batch.batch_inactive)
    pred = head(torch.cat((active, inactive), dim=1)).squeeze()
    return criterion(pred, batch.y.float())


def test_one_pass_equals_two_passes_on_our_backbone():
    from geossl_amd.finetune_lep import do_LEP
    case = "g25_lep_schnet_reduced"
    g, meta, m1, h1, make, args = _setup(case)
    _, _, m2, h2, _, _ = _setup(case)
    crit = torch.nn.BCEWithLogitsLoss()
    ref = _aten_lines(args, make(), m1, h1, crit)
    ref.backward()
    got = do_LEP(args, make(), m2, h2, crit)
    got.backward()
    assert rel_err(got.detach().cpu(), ref.detach().cpu()) < TOL_OUT
    want = dict(unique_named_grads(m1), **{"head." + k: v for k, v in unique_named_grads(h1).items()})
    have = dict(unique_named_grads(m2), **{"head." + k: v for k, v in unique_named_grads(h2).items()})
    assert set(want) == set(have) and len(want) > 10
    for k in want:
        assert rel_err(have[k].cpu(), want[k].cpu()) < TOL_GRAD or float(want[k].abs().max()) < 1e-8, k


def test_three_adam_steps_match_the_reference_lines():
    """do_LEP + a stock torch.optim.Adam against :33-49 written in ATen on our backbone."""
    from geossl_amd.finetune_lep import do_LEP
    case = "g25_lep_schnet_reduced"
    g, meta, _, _, make, args = _setup(case)

    def loop(fused):
        _, _, model, head, _, _ = _setup(case)
        opt = torch.optim.Adam(list(model.parameters()) + list(head.parameters()), lr=1e-4)
        criterion = torch.nn.BCEWithLogitsLoss()
        losses = []
        for _ in range(3):
            batch = make()
            if fused:
                loss = do_LEP(args, batch, model, head, criterion)
            else:
                loss = _aten_lines(args, batch, model, head, criterion)
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


def test_what_the_kernels_do_not_serve_takes_the_reference_lines(monkeypatch):
    from geossl_amd import ops
    from geossl_amd.finetune_lep import do_LEP, predict_LEP
    case = "g25_lep_schnet_dense"
    g, meta, model, head, make, args = _setup(case)
    calls = []
    real_head, real_predict = ops.pair_head, ops.pair_predict
    monkeypatch.setattr(ops, "pair_head", lambda *a, **k: calls.append("head") or real_head(*a, **k))
    monkeypatch.setattr(ops, "pair_predict", lambda *a, **k: calls.append("predict") or real_predict(*a, **k))

    stock = do_LEP(args, make(), model, head)
    assert calls == ["head"] and rel_err(stock.detach().cpu(), g["loss"]) < TOL_OUT
    del calls[:]

    # a criterion that is not the stock one
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(2.5, device=DEV))
    got = do_LEP(args, make(), model, head, crit)
    ref = _aten_lines(args, make(), model, head, crit)
    assert calls == [] and rel_err(got.detach().cpu(), ref.detach().cpu()) < 1e-6
    assert abs(float(got.detach()) - float(stock.detach())) > 1e-3

    # a head with two outputs: eval()'s forward is the ATen lines, and the loss refuses the shapes as the reference does
    head2 = fill_module_(torch.nn.Linear(2 * meta["emb_dim"], 2)).to(DEV)
    b = make()
    pred = predict_LEP(args, b, model, head2)
    with torch.no_grad():
        ref = head2(torch.cat((model(b.x_active, b.positions_active, b.batch_active),
                               model(b.x_inactive, b.positions_inactive, b.batch_inactive)), dim=1))
    assert calls == [] and pred.shape == (2, 2) and rel_err(pred.cpu(), ref.cpu()) < 1e-6
    with pytest.raises(ValueError, match="[Tt]arget size"):
        do_LEP(args, b, model, head2)
    assert calls == []

    # one pair: the reference's squeeze() against a [1] target
    from geossl_amd.Geom3D.dataloaders import BatchLEP
    one = BatchLEP.from_data_list(lt.fixture_items(g)[:1]).to(DEV)
    with pytest.raises(ValueError, match="[Tt]arget size"):
        do_LEP(args, one, model, head)
    assert calls == []
