"""GPU tests of Supervised pretraining / property fine-tuning: the head kernels of csrc/property_head.hip against fp64 on
NaN-poisoned outputs (every served width, mean / add readouts, L1 / MSE, both head shapes, B = 1, 1-atom molecules, the
L1 zero subgradient, capacity launches, 1024 molecules of up to 255 atoms), determinism, fixture G21 through
do_Supervised (eager and replayed), fixture G14 through SupervisedTrainer and predict_Supervised, bucket replay against
eager on collated batches and DeviceLoader handles with targets, stock-Adam and trainer trajectories against the
reference's ATen loop, and the ATen-free head."""
import json
import os
import types

import numpy as np
import pytest
import torch

import supervised_twin as tw
from conftest import load_golden, rel_err
from helpers import fill_module_, grad_summary, t, unique_named_grads
from objective_harness import (Case, assert_one_bucket, assert_only_library_kernels, backbone, device_batch, kind_args,
                               loader_handles, ragged_batches, reference_loop_vs_trainer, replay_vs_eager,
                               with_radius_edges)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G21 = sorted(f[:-4] for f in os.listdir(os.path.join(REPO, "tests", "golden")) if f.startswith("g21_supervised_"))
NAN = float("nan")
READOUTS = {"add": 0, "mean": 1}
LOSSES = {"mae": 0, "mse": 1}


def _inputs(sizes, F, mlp, seed, T=3, task=1):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.as_tensor(sizes, dtype=torch.long)
    N, B = int(sizes.sum()), sizes.numel()
    h = torch.randn(N, F, generator=g) * 0.5
    if mlp:
        K = F // 2
        ps = [torch.randn(K, F, generator=g) / F ** 0.5, torch.randn(K, generator=g) * 0.1,
              torch.randn(1, K, generator=g) / K ** 0.5, torch.randn(1, generator=g) * 0.1]
    else:
        ps = [torch.randn(1, F, generator=g) / F ** 0.5, torch.randn(1, generator=g) * 0.1]
    y = torch.randn(B, T, generator=g) * 2.0 + 0.7
    return h, ps, y, sizes, task


def _raw(h, ps, y, task, sizes, readout, loss, stats=(0.3, 1.7), gout=1.3, N_cap=None):
    """Forward + backward + predict through the C ABI on NaN-filled outputs (head 1's dW1 / db1 through ops' weight
    gradient); with N_cap the `_dyn` forms with the real N read from the device (rows past it finite, so a row the
    kernels wrongly read would show, and NaN outputs there that a wrong write would overwrite)."""
    from geossl_amd import _lib, ops
    from geossl_amd._lib import ptr, stream
    lib = _lib.load()
    N, F = h.shape
    B = sizes.numel()
    mlp = len(ps) == 4
    Nc = N_cap or N
    hd = torch.cat([h, torch.full((Nc - N, F), 3.0)]).to(DEV)
    pd = [p.to(DEV).contiguous() for p in ps]
    W1, b1 = pd[0], pd[1]
    W2, b2 = (pd[2], pd[3]) if mlp else (None, None)
    yd = y.to(DEV).contiguous()
    ycol = yd[:, task]                                    # (a strided column, as batch.y.view(B, -1)[:, task_id] is)
    st_ = torch.tensor(stats, dtype=torch.float32, device=DEV)
    mp = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)]).to(torch.int32).to(DEV)
    dims = torch.tensor([N], dtype=torch.int32, device=DEV) if N_cap else None
    f = lambda *shape: torch.full(shape, NAN, device=DEV)
    K = F // 2
    m, z, pred = f(B, F), (f(B, K) if mlp else None), f(B)
    ws = f(int(lib.geossl_property_workspace_floats(B)))
    lo = f()
    s = stream()
    _lib.call("geossl_property_fwd_dyn", ptr(hd), Nc, F, ptr(mp), B, READOUTS[readout], 1 if mlp else 0, ptr(W1),
              ptr(b1), ptr(W2), ptr(b2), ptr(ycol), ycol.stride(0), ptr(st_), LOSSES[loss], ptr(m), ptr(z), ptr(pred),
              ptr(ws), ptr(lo), ptr(dims), s)
    dh = f(Nc, F)
    dz = f(B, K) if mlp else None
    dvw, dvb = (f(1, K), f(1)) if mlp else (f(1, F), f(1))
    go = torch.tensor([gout], device=DEV)
    ws2 = f(int(lib.geossl_property_workspace_floats(B)))
    _lib.call("geossl_property_bwd_dyn", Nc, F, ptr(mp), B, READOUTS[readout], 1 if mlp else 0, ptr(W1), ptr(W2),
              ptr(m), ptr(z), ptr(pred), ptr(ycol), ycol.stride(0), ptr(st_), LOSSES[loss], ptr(go), ptr(dh), ptr(dz),
              ptr(dvw), ptr(dvb), ptr(ws2), 0, ptr(dims), s)
    grads = {}
    if mlp:
        dW1, db1 = f(K, F), f(K)
        ops._property_w1_grad(dz, m, dW1, db1, False)
        grads = dict(W1=dW1, b1=db1, w2=dvw, b2=dvb)
    else:
        grads = dict(w=dvw, b=dvb)
    ev = f(B)
    _lib.call("geossl_property_predict_dyn", ptr(hd), Nc, F, ptr(mp), B, READOUTS[readout], 1 if mlp else 0, ptr(W1),
              ptr(b1), ptr(W2), ptr(b2), ptr(st_), ptr(ev), ptr(dims), s)
    torch.cuda.synchronize()
    return lo.cpu(), pred.cpu(), dh.cpu(), {k: v.cpu() for k, v in grads.items()}, ev.cpu(), m.cpu()


def _check(sizes, F, mlp, readout, loss, seed, N_cap=None, exact_zero=False, tol=2e-5):
    h, ps, y, sizes, task = _inputs(sizes, F, mlp, seed)
    stats = (0.0, 1.0) if exact_zero else (0.3, 1.7)
    if exact_zero:   # pred == t for molecule 0: its target is what the head predicts for it (t = y at (0, 1))
        got = _raw(h, ps, y, task, sizes, readout, loss, stats)
        y[0, task] = float(got[1][0])
    lo, pred, dh, grads, ev, m = _raw(h, ps, y, task, sizes, readout, loss, stats, N_cap=N_cap)
    B = sizes.numel()
    batch = torch.repeat_interleave(torch.arange(B), sizes)
    hh = h.double().requires_grad_()
    pp = [p.double().requires_grad_() for p in ps]
    mm = tw.readout(hh, batch, B, readout)
    pr = tw.head(mm, pp)
    tt = tw.target(y.reshape(-1), B, task, stats[0], stats[1])
    L = tw.loss(pr, tt, loss)
    (L * 1.3).backward()
    Nr = h.size(0)
    assert torch.isfinite(dh[:Nr]).all() and torch.isfinite(pred).all() and torch.isfinite(m).all()
    if N_cap:
        assert torch.isnan(dh[Nr:]).all()                # rows past the real count are not written
    assert rel_err(m, mm.detach()) < 1e-6
    assert rel_err(pred, pr.detach()) < tol
    assert abs(float(lo) - L.item()) <= tol * max(abs(L.item()), 1e-3)
    assert rel_err(ev, pr.detach() * stats[1] + stats[0]) < tol
    if not exact_zero:
        assert rel_err(dh[:Nr], hh.grad) < tol
        names = ["W1", "b1", "w2", "b2"] if mlp else ["w", "b"]
        for n, p in zip(names, pp):
            assert rel_err(grads[n].reshape(p.shape), p.grad) < tol, n
    return lo, pred, dh, grads, y, task


@pytest.mark.parametrize("F", [64, 128, 256])
@pytest.mark.parametrize("readout", ["mean", "add"])
@pytest.mark.parametrize("loss", ["mae", "mse"])
@pytest.mark.parametrize("mlp", [False, True], ids=["linear", "mlp"])
def test_head_kernels_vs_fp64(F, readout, loss, mlp):
    _check([5, 18, 2, 9, 33, 1, 12, 1, 40], F, mlp, readout, loss, 7 + F)


@pytest.mark.parametrize("mlp", [False, True], ids=["linear", "mlp"])
def test_head_kernels_b1_and_one_atom(mlp):
    _check([1], 128, mlp, "mean", "mae", 3)
    _check([7], 64, mlp, "add", "mse", 4)
    _check([1, 1, 1], 256, mlp, "mean", "mse", 5)


@pytest.mark.parametrize("mlp", [False, True], ids=["linear", "mlp"])
def test_l1_zero_subgradient(mlp):
    """pred == t exactly: torch's sign(0) = 0, so molecule 0 sends no gradient to its atoms."""
    lo, pred, dh, grads, y, task = _check([4, 6, 3], 128, mlp, "mean", "mae", 11, exact_zero=True)
    assert torch.all(dh[:4] == 0)
    assert torch.all(dh[4:] != 0)


@pytest.mark.parametrize("F", [64, 128, 256])
def test_head_kernels_dyn(F):
    _check([5, 18, 2, 9, 1, 12], F, True, "mean", "mae", 21, N_cap=64)
    _check([5, 18, 2, 9, 1, 12], F, False, "add", "mse", 22, N_cap=100)


def test_head_kernels_bs1024_up_to_255_atoms():
    rng = np.random.default_rng(9)
    sizes = rng.integers(1, 256, size=1024)
    sizes[:3] = (255, 1, 255)
    _check(sizes.tolist(), 128, True, "mean", "mae", 41, tol=5e-5)
    _check(sizes.tolist(), 128, False, "add", "mse", 42, tol=5e-5)


def test_kernels_are_deterministic():
    h, ps, y, sizes, task = _inputs([5, 18, 2, 9, 33, 1, 12] * 20, 128, True, 51)
    first = _raw(h, ps, y, task, sizes, "mean", "mae")
    for _ in range(3):
        again = _raw(h, ps, y, task, sizes, "mean", "mae")
        for a, b in zip(first[:3] + first[4:], again[:3] + again[4:]):
            assert torch.equal(a, b)
        for k in first[3]:
            assert torch.equal(first[3][k], again[3][k]), k


# ------------------------------------------------------------------------------------------------------ G21
def _g21_setup(case):
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    from geossl_amd.synthetic import combination_pairs
    g = load_golden(case)
    meta, cfg = json.loads(str(g["meta"])), json.loads(str(g["cfg"]))
    model = fill_module_(SchNet(**cfg) if meta["kind"] == "schnet" else PaiNN(**cfg)).to(DEV)
    head = (fill_module_(torch.nn.Linear(meta["emb_dim"], 1)) if meta["kind"] == "schnet"
            else fill_module_(model.create_output_layers())).to(DEV)
    rei = t(g["radius_edge_index"], DEV) if "radius_edge_index" in g else None
    sizes = g["sizes"]
    off = np.concatenate([[0], np.cumsum(sizes)])
    sei = np.concatenate([combination_pairs(int(n)) + off[m] for m, n in enumerate(sizes)], axis=1).astype(np.int64)

    def batch():
        b = pg.Batch(t(g["x"], DEV), t(g["positions"], DEV), t(g["batch"], DEV), t(sei, DEV), radius_edge_index=rei,
                     num_graphs=len(sizes), sizes=sizes, canonical="combination")
        b.y = t(g["y"], DEV)
        return b
    return g, meta, model, head, batch, types.SimpleNamespace(model_3d=meta["kind"], loss=meta["loss"])


def _check_g21(g, model, head, loss, case):
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert rel_err(loss.detach().cpu(), g["loss"]) < 1e-5, case
    for name, p in head.named_parameters():
        assert rel_err(p.grad.cpu(), g["head_grad/" + name]) < 1e-4, (case, name)
    grads = unique_named_grads(model)
    for k in g:
        if k.startswith("grad/") or k.startswith("gsum/"):
            got = grads[k.split("/", 1)[1]].cpu()
            got = grad_summary(got) if k.startswith("gsum/") else got
            assert rel_err(got, g[k]) < 1e-4 or float(np.abs(g[k]).max()) < 1e-8, (case, k)


@pytest.mark.parametrize("case", G21)
@pytest.mark.parametrize("graph", [False, True])
def test_g21_do_supervised(case, graph):
    from geossl_amd.pretrain_Supervised import do_Supervised, predict_Supervised
    g, meta, model, head, make, args = _g21_setup(case)
    b = make()
    mean, std, task = float(g["TRAIN_mean"]), float(g["TRAIN_std"]), int(g["task_id"])
    for _ in range(2 if graph else 1):
        model.zero_grad(set_to_none=True)
        head.zero_grad(set_to_none=True)
        loss = do_Supervised(args, b, model, head, mean, std, task_id=task, graph=graph)
        loss.backward()
    _check_g21(g, model, head, loss, case)
    if graph:
        eng = model.__dict__["_geossl_supervised_step"]
        assert sum(len(sg) for sg in eng.graphs.values()) >= 1
    ev = predict_Supervised(args, b, model, head, mean, std)
    assert rel_err(ev.cpu(), torch.from_numpy(g["pred"]).double() * std + mean) < 1e-5


def test_g14_finetune_qm9_through_the_trainer():
    """examples/finetune_qm9.py with the product SchNet (fixture G14: two epochs of three batches, CosineAnnealingLR per
    epoch, then eval()) through SupervisedTrainer.step / set_lr and predict_Supervised, at the tolerances of
    test_g14_finetune_qm9_on_the_hip_path."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.models import SchNet
    from geossl_amd.optim import cosine_annealing_lr
    from geossl_amd.pretrain_Supervised import SupervisedTrainer, predict_Supervised
    g = load_golden("g14_finetune_qm9_schnet")
    cfg = json.loads(str(g["cfg"]))
    model = fill_module_(SchNet(**{k: cfg[k] for k in ("hidden_channels", "num_filters", "num_interactions",
                                                        "num_gaussians", "cutoff", "readout", "node_class")
                                   if k in cfg})).to(DEV)
    head = fill_module_(torch.nn.Linear(128, 1)).to(DEV)
    tm, ts, task = float(g["TRAIN_mean"]), float(g["TRAIN_std"]), int(g["task_id"])
    tr = SupervisedTrainer(model, head, tm, ts, task_id=task, loss="mae", lr=5e-4, model_3d="schnet")

    def batch(split, i):
        b = pg.Batch(*(t(g["%s/%d/%s" % (split, i, k)], DEV) for k in ("x", "positions", "batch")), None,
                     num_graphs=int(g["%s/%d/sizes" % (split, i)].size))
        b.y = t(g["%s/%d/y" % (split, i)], DEV)
        return b
    losses = []
    for epoch in (1, 2):
        for i in range(3):
            losses.append(tr.step(batch("train", i)))
        tr.set_lr(cosine_annealing_lr(5e-4, epoch, 100))
    losses = torch.stack(losses).cpu()
    TOL_OUT, TOL_GRAD = 1e-5, 1e-4
    assert rel_err(losses, g["losses"]) < TOL_OUT and abs(tr.lr - float(g["lr_after"])) < 1e-12
    scores = torch.cat([predict_Supervised(tr.args, batch("eval", i), model, head, tm, ts) for i in range(2)]).cpu()
    assert rel_err(scores, g["y_scores"]) < 5e-5
    named = dict(model.named_parameters())
    for k in g:
        if k.startswith("psum/"):
            assert rel_err(grad_summary(named[k[5:]].detach().cpu()), g[k]) < TOL_GRAD, k
    assert rel_err(head.weight.detach().cpu(), g["head/weight"]) < TOL_GRAD
    assert rel_err(head.bias.detach().cpu(), g["head/bias"]) < TOL_GRAD


# ---------------------------------------------------------------------------------------------- graph paths
def _with_targets(collated, rng, T=4):
    b = device_batch(collated)
    b.y = torch.from_numpy(rng.standard_normal(len(collated["sizes"]) * T).astype(np.float32)).to(DEV)
    return b


def _target_batches(n, B, seed):
    return ragged_batches(n, B, seed, decorate=_with_targets)


def _head(kind, model):
    return (fill_module_(torch.nn.Linear(128, 1)) if kind == "schnet" else
            fill_module_(model.create_output_layers())).to(DEV)


def _case(mean, std, task, loss="mae"):
    from geossl_amd.pretrain_Supervised import SupervisedTrainer, do_Supervised, supervised_step_aten

    def step(args, b, model, heads, graph):
        return do_Supervised(args, b, model, heads[0], mean, std, task_id=task, graph=graph), ()

    def aten_step(args, b, model, heads):
        crit = {"mae": torch.nn.L1Loss, "mse": torch.nn.MSELoss}[loss]()
        return supervised_step_aten(args, b, model, heads[0], mean, std, task, crit), ()

    def trainer(model, heads, **kw):
        return SupervisedTrainer(model, heads[0], mean, std, task_id=task, loss=loss, **kw)

    return Case("supervised", "_geossl_supervised_step", lambda kind, model: [_head(kind, model)], kind_args(loss=loss),
                step, trainer, aten_step=aten_step, head_weight=lambda heads: heads[0].weight, batches=_target_batches)


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_bucket_replay_matches_eager_on_ragged_batches(kind):
    case = _case(0.25, 1.5, task=2, loss="mse" if kind == "painn" else "mae")
    model = backbone(kind)
    heads = case.heads(kind, model)
    batches = _target_batches(4, 24, 17)
    if kind == "painn":
        with_radius_edges(batches)
    assert_one_bucket(replay_vs_eager(case, kind, model, heads, batches), views=case.views)


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_bucket_replay_matches_eager_on_device_loader(kind):
    """DeviceLoader handles of a dataset that carries y: the target column is gathered per batch on the device, over a
    shuffled epoch; DatasetBatch.y is the reference's collation."""
    y = np.random.default_rng(4).standard_normal((200, 5)).astype(np.float32)
    hbs = loader_handles(kind, dataset_kw={"y": y})
    for hb in hbs:
        assert torch.equal(hb.y.cpu(), torch.from_numpy(y[hb.ids]).reshape(-1))
    case = _case(0.25, 1.5, task=3)
    model = backbone(kind)
    sg = replay_vs_eager(case, kind, model, case.heads(kind, model), hbs)
    assert_one_bucket(sg)
    # the static target column of the graph holds the last batch's column
    (gg,) = sg.graphs.values()
    assert torch.equal(gg["noise"]["target"].cpu(), torch.from_numpy(y[hbs[-1].ids, 3]))


def test_dataset_without_targets_has_no_y():
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    from geossl_amd.synthetic import make_molecules
    ds = DeviceDataset.from_numpy(make_molecules(10, seed=3, mode="C"), DEV)
    assert ds.y is None and ds.batch([0, 1]).y is None


def test_reference_loop_and_trainer_match_stock_adam():
    """Six steps of the reference loop with do_Supervised (graph replay, stock torch.optim.Adam over the reference's two
    groups) and of SupervisedTrainer (one bucket graph) against the reference's ATen lines on our backbone."""
    reference_loop_vs_trainer(_case(0.1, 1.2, task=1), 6, 16, 5, per_step=False)


def test_stats_change_without_recapture():
    """(mean, std) are read from device memory: new values change the replayed loss, with one capture."""
    from geossl_amd.pretrain_Supervised import do_Supervised
    model = backbone("schnet")
    head = _head("schnet", model)
    b = _target_batches(1, 16, 8)[0]
    args = types.SimpleNamespace(model_3d="schnet", loss="mse")
    out = []
    for mean, std in ((0.0, 1.0), (0.5, 2.0)):
        for graph in (True, False):
            model.zero_grad(set_to_none=True)
            head.zero_grad(set_to_none=True)
            out.append(float(do_Supervised(args, b, model, head, mean, std, task_id=0, graph=graph).detach()))
    assert out[0] == pytest.approx(out[1], rel=1e-6) and out[2] == pytest.approx(out[3], rel=1e-6)
    assert abs(out[0] - out[2]) > 1e-3
    eng = model.__dict__["_geossl_supervised_step"]
    assert sum(sg.captures for sg in eng.graphs.values()) == 1


def test_head_launches_no_aten_arithmetic():
    """The head's forward and backward (as a replayed step captures them) call no floating-point ATen operator and
    launch only the library's kernels."""
    from geossl_amd import ops
    from geossl_amd.layout import get_layout
    for mlp in (False, True):
        h, ps, y, sizes, task = _inputs([5, 18, 2, 9, 1, 12], 128, mlp, 31)
        batch = torch.repeat_interleave(torch.arange(sizes.numel()), sizes)
        lay = get_layout(batch.to(DEV))
        hd = h.to(DEV).requires_grad_()
        pd = [p.to(DEV).requires_grad_() for p in ps]
        for p in pd:
            p.grad = torch.zeros_like(p)
        yd = y.to(DEV)[:, task]
        stats = torch.tensor([0.2, 1.1], device=DEV)
        one = torch.ones((), device=DEV)
        assert_only_library_kernels(lambda: ops.property_head(hd, pd, lay, "mean", yd, stats, "mae")[0].backward(one))
        assert torch.isfinite(hd.grad).all() and all(torch.isfinite(p.grad).all() for p in pd)


def test_fallbacks_match_aten_and_checkpoints_load():
    """A Huber criterion and an unserved width (48) run the reference's lines on our backbone; a checkpoint in the
    reference's format ({"model", "graph_pred_linear"}) saved after trainer steps loads into fresh modules and predicts
    the same values."""
    import io
    from geossl_amd.Geom3D.models import SchNet
    from geossl_amd.pretrain_Supervised import (SupervisedTrainer, do_Supervised, predict_Supervised,
                                                supervised_step_aten)
    args = types.SimpleNamespace(model_3d="schnet", loss="mae")
    b = _target_batches(1, 12, 23)[0]
    for F, crit in ((48, torch.nn.L1Loss()), (64, torch.nn.HuberLoss())):
        cfg = dict(hidden_channels=F, num_filters=F, num_interactions=2, num_gaussians=8, cutoff=5.0, node_class=9)
        model = fill_module_(SchNet(**cfg)).to(DEV)
        head = fill_module_(torch.nn.Linear(F, 1)).to(DEV)
        got = do_Supervised(args, b, model, head, 0.3, 1.4, task_id=2, criterion=crit)
        ref = supervised_step_aten(args, b, model, head, 0.3, 1.4, 2, crit)
        assert torch.equal(got.detach(), ref.detach()), F
    model = backbone("schnet")
    head = _head("schnet", model)
    tr = SupervisedTrainer(model, head, 0.3, 1.4, task_id=2, lr=1e-4)
    for bb in _target_batches(3, 12, 24):
        tr.step(bb)
    buf = io.BytesIO()
    torch.save({"model": model.state_dict(), "graph_pred_linear": head.state_dict()}, buf)
    buf.seek(0)
    ck = torch.load(buf)
    m2 = backbone("schnet")
    h2 = _head("schnet", m2)
    m2.load_state_dict(ck["model"])
    h2.load_state_dict(ck["graph_pred_linear"])
    want = predict_Supervised(args, b, model, head, 0.3, 1.4)
    assert torch.equal(predict_Supervised(args, b, m2, h2, 0.3, 1.4), want)
    assert torch.equal(tr.predict(b), want)
