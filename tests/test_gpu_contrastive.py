"""GPU tests of the contrastive objectives (--GeoSSL_option InfoNCE / EBM_NCE): the loss kernels of
csrc/contrastive.hip against the fp64 twin (tests/contrastive_twin.py), their determinism, the whole step against
fixture G17 (the reference run verbatim), the graph paths against the eager step, the reference's own training loop,
independence from the allocator's free memory, and a scaled upstream gradient."""
import gc
import json
import os
import types

import numpy as np
import pytest
import torch

import contrastive_twin as tw
from conftest import load_golden, rel_err
from helpers import fill_module_, t
from objective_harness import backbone

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G17 = sorted(f[:-4] for f in os.listdir(os.path.join(REPO, "tests", "golden")) if f.startswith("g17_contrastive_"))


def _reps(B, F, seed, normalize):
    g = torch.Generator().manual_seed(seed)
    X = 0.3 * torch.randn(B, F, generator=g)
    Y = 0.6 * X + 0.3 * torch.randn(B, F, generator=g)
    if normalize:
        X, Y = torch.nn.functional.normalize(X, dim=-1), torch.nn.functional.normalize(Y, dim=-1)
    return X, Y


def _close_grad(got, want, floor=0.0):
    # 1e-5 of the largest magnitude (a gradient that is exactly zero - InfoNCE at B = 1 - must come out exactly zero);
    # `floor`: what the fp64 twin itself cannot resolve
    return float((got.double().cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max()) + floor


# ---------------------------------------------------------------------------------------------- kernels vs the twin
@pytest.mark.parametrize("B", [1, 2, 3, 31, 127, 128, 1024])
@pytest.mark.parametrize("F", [32, 64, 128, 33])
def test_infonce_kernel_vs_twin(B, F):
    from geossl_amd import ops
    for T in (0.1, 1.0):
        for normalize in (False, True):
            X, Y = _reps(B, F, 1000 * B + F, normalize)
            Xd, Yd = X.to(DEV).requires_grad_(), Y.to(DEV).requires_grad_()
            loss, counts = ops.infonce_loss(Xd, Yd, T)
            loss.backward()
            Xt, Yt = X.double().requires_grad_(), Y.double().requires_grad_()
            ref, hr, hc = tw.infonce(Xt, Yt, T)
            ref.backward()
            assert loss.dtype == torch.float32 and loss.dim() == 0
            # 1e-5 relative, plus what the fp32 rounding of S itself moves the loss by (first order: |dL/dS| times the
            # error bound of an fp32 dot product, 2e-7 sum|x y|) - the larger term only for a loss far below the logits
            # (a dominant diagonal); B = 1 gives exactly 0
            S = Xt.detach() @ Yt.detach().t() / T
            G = torch.softmax(S, 1) + torch.softmax(S, 0) - 2 * torch.eye(B, dtype=S.dtype)
            s_err = 2e-7 * (X.double().abs() @ Y.double().abs().t()) / T
            tol = 1e-5 * abs(ref.item()) + float((G.abs() * s_err).sum()) / (2 * B) + 1e-12
            assert abs(loss.item() - ref.item()) <= tol, (T, normalize, loss.item(), ref.item())
            assert counts.tolist() == [hr, hc], (T, normalize)
            # Beside 1e-5 of the largest magnitude: (a) what the fp32 rounding of S moves the gradient by, first order:
            # a softmax term moves by its own size - 1 - p at a row's maximum - times twice the largest error of S in
            # its row (the dot product's bound plus the rounding of S / T), against the rows it scales; (b) the twin's
            # own floor - it forms softmax - 1 in fp64, which rounds below one ulp of 1 (a diagonal that dominates by
            # e^36), where the kernel's expm1 does not.
            err = s_err + 6e-8 * S.abs()
            Pr, Pc = torch.softmax(S, 1), torch.softmax(S, 0)
            ar, ac = Pr.argmax(1), Pc.argmax(0)
            Pr[torch.arange(B), ar] = 1 - Pr[torch.arange(B), ar]
            Pc[ac, torch.arange(B)] = 1 - Pc[ac, torch.arange(B)]
            E = 2 * (Pr * err.max(1, keepdim=True).values + Pc * err.max(0, keepdim=True).values)
            fx = 2 * float((E @ Y.double().abs()).max()) / (2 * B * T)
            fy = 2 * float((E.t() @ X.double().abs()).max()) / (2 * B * T)
            twin = 4.4e-16 * max(float(X.abs().max()), float(Y.abs().max())) / T
            assert _close_grad(Xd.grad, Xt.grad, fx + twin) and _close_grad(Yd.grad, Yt.grad, fy + twin), (T, normalize)


def test_infonce_ties_take_the_first_maximum():
    from geossl_amd import ops
    # all rows equal: every entry of S ties, every row's and column's first maximum is index 0
    X = torch.full((40, 64), 0.25)
    _, counts = ops.infonce_loss(X.to(DEV), X.to(DEV), 0.1)
    assert counts.tolist() == [1, 1]
    # rows 2k and 2k+1 equal (a one-hot of k): the first maximum of rows / columns 2k and 2k+1 is 2k
    B = 36
    X = torch.zeros(B, 32)
    X[torch.arange(B), torch.arange(B) // 2] = 1.0
    loss, counts = ops.infonce_loss(X.to(DEV), X.to(DEV), 0.5)
    ref, hr, hc = tw.infonce(X, X, 0.5)
    assert counts.tolist() == [hr, hc] == [B // 2, B // 2]
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())


@pytest.mark.parametrize("B", [1, 2, 3, 31, 127, 128, 1024])
@pytest.mark.parametrize("F", [32, 128, 33])
def test_ebm_nce_kernel_vs_twin(B, F):
    from geossl_amd import ops
    for num_neg in (1, 2):
        if num_neg > B:
            continue
        for normalize in (False, True):
            X, Y = _reps(B, F, 7000 + 1000 * B + F, normalize)
            Xd, Yd = X.to(DEV).requires_grad_(), Y.to(DEV).requires_grad_()
            loss, counts = ops.ebm_nce_loss(Xd, Yd, num_neg)
            assert loss.dtype == torch.float64 and loss.dim() == 0
            loss.backward()
            Xt, Yt = X.double().requires_grad_(), Y.double().requires_grad_()
            ref, hp, hn = tw.ebm_nce(Xt, Yt, num_neg)
            ref.backward()
            assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), (num_neg, normalize)
            assert counts.tolist() == [hp, hn], (num_neg, normalize)
            assert _close_grad(Xd.grad, Xt.grad) and _close_grad(Yd.grad, Yt.grad), (num_neg, normalize)


def test_ebm_nce_refuses_more_negatives_than_molecules():
    from geossl_amd import ops
    X = torch.randn(2, 32, device=DEV)
    with pytest.raises(ValueError):
        ops.ebm_nce_loss(X, X, 3)


# ---------------------------------------------------------------------------------------------- determinism
def test_kernels_are_deterministic_eager_and_replayed():
    from geossl_amd import ops
    X, Y = _reps(1024, 128, 5, False)
    X, Y = X.to(DEV), Y.to(DEV)

    def both():
        out = []
        for fn in (lambda a, b: ops.infonce_loss(a, b, 0.1), lambda a, b: ops.ebm_nce_loss(a, b, 2)):
            a, b = X.clone().requires_grad_(), Y.clone().requires_grad_()
            loss, counts = fn(a, b)
            dx, dy = torch.autograd.grad(loss, (a, b))
            out += [loss.detach().clone(), counts.clone(), dx.clone(), dy.clone()]
        return out
    one, two = both(), both()
    assert all(torch.equal(p, q) for p, q in zip(one, two))
    # the same launches captured once and replayed twice
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = both()
    g.replay()
    first = [s.clone() for s in static]
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(first, static))
    assert all(torch.equal(p, q) for p, q in zip(first, one))


# ---------------------------------------------------------------------------------------------- G17 end to end
def _g17_setup(case):
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    g = load_golden(case)
    meta, cfg = json.loads(str(g["meta"])), json.loads(str(g["cfg"]))
    model = fill_module_(SchNet(**cfg) if meta["kind"] == "schnet" else PaiNN(**cfg)).to(DEV)
    rei = t(g["radius_edge_index"], DEV) if "radius_edge_index" in g else None
    batch = pg.Batch(t(g["x"], DEV), t(g["positions"], DEV), t(g["batch"], DEV), t(g["super_edge_index"], DEV),
                     radius_edge_index=rei, num_graphs=len(g["sizes"]))
    args = types.SimpleNamespace(model_3d=meta["kind"], normalize=meta["normalize"], T=meta["T"])
    fn = pg.do_InfoNCE if meta["option"] == "InfoNCE" else pg.do_EBM_NCE
    return g, meta, model, batch, args, fn, {"pos_noise": t(g["pos_noise"], DEV)}


@pytest.mark.parametrize("case", G17)
def test_g17_end_to_end(case):
    g, meta, model, batch, args, fn, noise = _g17_setup(case)
    crit = torch.nn.BCEWithLogitsLoss() if meta["option"] == "EBM_NCE" else None
    loss, acc = fn(args, batch, model, crit, 0.0, 0.3, num_neg=meta["num_neg"], noise=noise, graph=False)
    assert str(loss.dtype) == str(g["loss_dtype"])
    assert isinstance(acc, float) and acc == float(g["acc"])
    assert rel_err(loss.detach().cpu(), g["loss"]) < 1e-4 or abs(loss.item() - float(g["loss"])) < 1e-6
    loss.backward()
    from helpers import grad_summary, unique_named_grads
    grads = unique_named_grads(model)
    for k in g:
        if k.startswith("grad/") or k.startswith("gsum/"):
            name = k.split("/", 1)[1]
            got = grads[name].cpu()
            got = grad_summary(got) if k.startswith("gsum/") else got
            assert rel_err(got, g[k]) < 1e-4 or float(np.abs(g[k]).max()) < 1e-8, (case, k)


# ---------------------------------------------------------------------------------------------- graph paths
def _batch(kind, B, seed):
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import make_batch
    bt = pg.Batch.from_numpy(make_batch(B, seed=seed, mode="B"), DEV)
    if kind == "painn":
        bt.radius_edge_index = ops.radius_graph(bt.positions, 5.0, bt.batch)
    return bt


@pytest.mark.parametrize("kind", ["schnet", "painn"])
@pytest.mark.parametrize("option", ["InfoNCE", "EBM_NCE"])
def test_per_structure_graph_replay_equals_the_eager_step(kind, option):
    from geossl_amd import pretrain_GeoSSL as pg
    bt = _batch(kind, 48, 3)
    args = types.SimpleNamespace(model_3d=kind, normalize=option == "EBM_NCE", T=0.1, step_graph_mode="structure")
    fn = pg.do_InfoNCE if option == "InfoNCE" else pg.do_EBM_NCE
    out = {}
    for graph in (False, True):
        model = backbone(kind)
        eng_runs = []
        for step in range(3):   # (graph: captured at the first step, replayed at the next two)
            noise = {"pos_noise": torch.randn(bt.positions.shape, generator=torch.Generator().manual_seed(50 + step)).mul_(0.3).to(DEV)}
            loss, acc = fn(args, bt, model, None, 0.0, 0.3, num_neg=2, noise=noise, graph=graph)
            grads = torch.autograd.grad(loss, [p for p in model.parameters() if p.requires_grad], allow_unused=True)
            eng_runs.append((loss.item(), acc, [None if g_ is None else g_.clone() for g_ in grads]))
        out[graph] = eng_runs
        if graph:
            eng = model.__dict__["_geossl_contrastive_step_" + option]
            assert sum(sg.captures for sg in eng.graphs.values()) == 1
    for (le, ae, ge), (lg, ag, gg) in zip(out[False], out[True]):
        assert ae == ag
        assert abs(le - lg) <= 1e-6 * abs(le)
        for a, b in zip(ge, gg):
            assert (a is None) == (b is None)
            if a is not None:
                assert rel_err(b.cpu(), a.cpu()) < 1e-6


def _device_dataset(kind, n=512):
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    from geossl_amd.synthetic import add_bonds, make_molecules
    mols = add_bonds(make_molecules(n, seed=7, mode="C"), seed=7)
    return DeviceDataset.from_numpy(mols, DEV, **({"radius": 5.0} if kind == "painn" else {}))


def _handles(ds, ratio, seed=5):
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    np.random.seed(3)
    return list(DeviceLoader(ds, batch_size=128, shuffle=True, drop_last=True,
                             generator=torch.Generator().manual_seed(seed), mask_ratio=ratio))


def _noise(hb, k):
    return {"pos_noise": torch.randn(hb.n_atoms, 3, generator=torch.Generator().manual_seed(100 + k)).mul_(0.3).to(DEV)}


@pytest.mark.parametrize("option", ["InfoNCE", "EBM_NCE"])
@pytest.mark.parametrize("kind,ratio", [("schnet", 0.0), ("schnet", 0.3), ("painn", 0.0)])
def test_trainer_bucket_replay_on_a_shuffled_device_loader_equals_eager(option, kind, ratio):
    """ContrastiveTrainer fed by a shuffled DeviceLoader at bs = 128 (masked or not): ONE capacity-bucket graph serves
    every ragged batch (captured at the first, replayed from then on), the handles are never collated on the host, and
    losses, counts and parameters match the eager trainer's on the same draws within fp32 summation order."""
    from geossl_amd import pretrain_GeoSSL as pg
    ds = _device_dataset(kind)
    res = {}
    for use_graph in (False, True):
        torch.manual_seed(3)
        model = backbone(kind)
        tr = pg.ContrastiveTrainer(model, option=option, lr=5e-4, model_3d=kind, use_graph=use_graph, num_neg=2,
                                   normalize=option == "EBM_NCE", device_noise=True)
        hbs = _handles(ds, ratio)
        losses = []
        for k, hb in enumerate(hbs):
            loss, counts = tr.step(hb, _noise(hb, k))
            losses.append((loss.item(), counts.tolist()))
        if use_graph:
            assert [key[0] for key in tr.step_graphs.graphs] == ["bucket"] and tr.step_graphs.captures <= 2
            assert all(hb._batch is None for hb in hbs)   # gathered into the bucket: no host collation, ever
        res[use_graph] = (losses, tr.flat.flat.clone())
    (le, pe), (lg, pg_) = res[False], res[True]
    assert len(le) == 4
    for (a, ca), (b, cb) in zip(le, lg):
        assert abs(a - b) <= 1e-5 * abs(a) and ca == cb
    assert rel_err(pg_.cpu(), pe.cpu()) < 1e-5


@pytest.mark.parametrize("option", ["InfoNCE", "EBM_NCE"])
def test_reference_entry_points_replay_a_bucket_on_device_loader_handles(option):
    """do_InfoNCE / do_EBM_NCE on DeviceLoader handles (the reference's loop over our loader): the graph path replays one
    bucket graph without collating a handle, and gives the eager path's loss, acc and gradients."""
    from geossl_amd import pretrain_GeoSSL as pg
    ds = _device_dataset("schnet")
    fn = pg.do_InfoNCE if option == "InfoNCE" else pg.do_EBM_NCE
    args = types.SimpleNamespace(model_3d="schnet", normalize=True, T=0.1)
    out = {}
    for graph in (False, True):
        model = backbone("schnet")
        params = [p for p in model.parameters() if p.requires_grad]
        hbs = _handles(ds, 0.3)
        runs = []
        for k, hb in enumerate(hbs):
            loss, acc = fn(args, hb, model, None, 0.0, 0.3, num_neg=2, noise=_noise(hb, k), graph=graph)
            grads = torch.autograd.grad(loss, params, allow_unused=True)
            runs.append((loss.item(), acc, [None if g_ is None else g_.clone() for g_ in grads]))
        if graph:
            eng = model.__dict__["_geossl_contrastive_step_" + option]
            sgs = list(eng.graphs.values())
            assert len(sgs) == 1 and [key[0] for key in sgs[0].graphs] == ["bucket"] and sgs[0].captures <= 2
            assert all(hb._batch is None for hb in hbs)
        out[graph] = runs
    for (le, ae, ge), (lg, ag, gg) in zip(out[False], out[True]):
        assert ae == ag and abs(le - lg) <= 1e-5 * abs(le)
        for a, b in zip(ge, gg):
            assert (a is None) == (b is None)
            if a is not None:
                assert rel_err(b.cpu(), a.cpu()) < 1e-4


# ---------------------------------------------------------------------------------------------- the reference loop
@pytest.mark.parametrize("option", ["InfoNCE", "EBM_NCE"])
def test_reference_loop_graph_equals_eager(option):
    """do_X, optimizer.zero_grad(), loss.backward(), stock Adam, CosineAnnealingLR (pretrain_GeoSSL.py:234-260,
    :332-356) for two short epochs over pre-collated batches: the graph path ends where the eager path ends."""
    from geossl_amd import pretrain_GeoSSL as pg
    batches = [_batch("schnet", 24, 60 + i) for i in range(3)]
    fn = pg.do_InfoNCE if option == "InfoNCE" else pg.do_EBM_NCE
    crit = torch.nn.BCEWithLogitsLoss()
    final = {}
    for graph in (False, True):
        torch.manual_seed(11)
        model = backbone("schnet")
        opt = torch.optim.Adam(model.parameters(), lr=5e-4)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 2)
        args = types.SimpleNamespace(model_3d="schnet", normalize=False, T=0.1, step_graph=graph)
        accs = []
        for epoch in range(2):
            for k, bt in enumerate(batches):
                noise = {"pos_noise": torch.randn(bt.positions.shape, generator=torch.Generator().manual_seed(10 * epoch + k)).mul_(0.3).to(DEV)}
                loss, acc = fn(args, bt, model, crit, 0.0, 0.3, noise=noise)
                opt.zero_grad()
                loss.backward()
                opt.step()
                accs.append(acc)
            sched.step()
        final[graph] = (torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(), accs)
    assert final[False][1] == final[True][1]
    assert rel_err(final[True][0], final[False][0]) < 1e-5


# ---------------------------------------------------------------------------------------------- memory, scaling
@pytest.mark.parametrize("option", ["InfoNCE", "EBM_NCE"])
def test_step_reads_no_memory_it_has_not_written(option):
    from geossl_amd import pretrain_GeoSSL as pg
    bt = _batch("schnet", 96, 91)
    noise = {"pos_noise": torch.randn(bt.positions.shape, generator=torch.Generator().manual_seed(92)).mul_(0.3).to(DEV)}
    args = types.SimpleNamespace(model_3d="schnet", normalize=True, T=0.1)
    fn = pg.do_InfoNCE if option == "InfoNCE" else pg.do_EBM_NCE

    def poison(value):
        junk = [torch.full((n,), value, device=DEV) for n in (1 << 9, 1 << 12, 1 << 15, 1 << 18, 1 << 20, 1 << 22)
                for _ in range(8)]
        torch.cuda.synchronize()
        del junk

    def step(value):
        gc.collect()
        model = backbone("schnet")
        if value is not None:
            poison(value)
        loss, acc = fn(args, bt, model, None, 0.0, 0.3, num_neg=2, noise=noise, graph=False)
        loss.backward()
        return loss.item(), acc, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    ref_loss, ref_acc, ref = step(None)
    assert np.isfinite(ref_loss) and all(bool(torch.isfinite(g).all()) for g in ref.values())
    for value in (float("nan"), 1e30):
        loss, acc, grads = step(value)
        assert loss == ref_loss and acc == ref_acc, value
        for n in ref:
            assert torch.equal(grads[n], ref[n]), (value, n)


@pytest.mark.parametrize("option", ["InfoNCE", "EBM_NCE"])
def test_replayed_bucket_step_reads_no_memory_it_has_not_written(option):
    """The same for a REPLAYED step: a capacity-bucket graph captured after the allocator's free blocks were filled with
    NaN / 1e30 and replayed after a second fill gives the unpoisoned capture's loss and gradients bit for bit (padding
    rows of the capacity, gradient rows of the readout's padding atoms and the like are never read)."""
    from geossl_amd import pretrain_GeoSSL as pg
    bt = _batch("schnet", 96, 93)
    noise = {"pos_noise": torch.randn(bt.positions.shape, generator=torch.Generator().manual_seed(94)).mul_(0.3).to(DEV)}
    args = types.SimpleNamespace(model_3d="schnet", normalize=True, T=0.1)
    fn = pg.do_InfoNCE if option == "InfoNCE" else pg.do_EBM_NCE

    def poison(value):
        junk = [torch.full((n,), value, device=DEV) for n in (1 << 9, 1 << 12, 1 << 15, 1 << 18, 1 << 20, 1 << 22)
                for _ in range(8)]
        torch.cuda.synchronize()
        del junk

    def steps(value):
        gc.collect()
        model = backbone("schnet")
        params = [p for p in model.parameters() if p.requires_grad]
        res = []
        for _ in range(2):   # capture (+ replay), then a replay
            if value is not None:
                poison(value)
            loss, acc = fn(args, bt, model, None, 0.0, 0.3, num_neg=2, noise=noise, graph=True)
            grads = torch.autograd.grad(loss, params, allow_unused=True)
            res.append((loss.item(), acc, [None if g_ is None else g_.clone() for g_ in grads]))
        sgs = list(model.__dict__["_geossl_contrastive_step_" + option].graphs.values())
        assert [key[0] for key in sgs[0].graphs] == ["bucket"] and sgs[0].captures == 1
        return res

    ref = steps(None)
    assert np.isfinite(ref[0][0]) and all(bool(torch.isfinite(g_).all()) for g_ in ref[0][2] if g_ is not None)
    for value in (None, float("nan"), 1e30):
        for (l0, a0, g0), (l1, a1, g1) in zip(ref, steps(value) if value is not None else ref[1:] + ref[:1]):
            assert l0 == l1 and a0 == a1, value
            assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(g0, g1)), value


@pytest.mark.parametrize("option", ["InfoNCE", "EBM_NCE"])
@pytest.mark.parametrize("graph", [False, True])
def test_scaled_loss_scales_the_gradients(option, graph):
    from geossl_amd import pretrain_GeoSSL as pg
    bt = _batch("schnet", 32, 5)
    noise = {"pos_noise": torch.randn(bt.positions.shape, generator=torch.Generator().manual_seed(6)).mul_(0.3).to(DEV)}
    args = types.SimpleNamespace(model_3d="schnet", normalize=False, T=0.1, step_graph_mode="structure")
    fn = pg.do_InfoNCE if option == "InfoNCE" else pg.do_EBM_NCE
    model = backbone("schnet")
    params = [p for p in model.parameters() if p.requires_grad]
    loss, _ = fn(args, bt, model, None, 0.0, 0.3, noise=noise, graph=graph)
    g1 = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
    g2 = torch.autograd.grad(2 * loss, params, allow_unused=True)
    for a, b in zip(g1, g2):
        if a is not None:
            assert torch.equal(b, 2 * a)
