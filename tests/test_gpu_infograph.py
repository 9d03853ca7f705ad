"""GPU tests of 3D InfoGraph pretraining: the head kernels of csrc/infograph_head.hip against fp64 on NaN-poisoned outputs
(every served width, mean / add / external readouts, B = 1, 1-atom molecules, capacity launches, 1024 molecules of up to
255 atoms), determinism, the hit counts, fixture G20 through do_InfoGraph and do_3DInfoGraph, bucket replay against
eager, stock-Adam and trainer trajectories against the reference's ATen loop, and the ATen-free head."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import infograph_twin as tw
from conftest import load_golden, rel_err
from helpers import fill_module_, grad_summary, t, unique_named_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G20 = sorted(f[:-4] for f in os.listdir(os.path.join(REPO, "tests", "golden")) if f.startswith("g20_infograph_"))
NAN = float("nan")
MODES = {"add": 0, "mean": 1, "external": 2}


def _inputs(sizes, F, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.as_tensor(sizes, dtype=torch.long)
    N, B = int(sizes.sum()), sizes.numel()
    x = torch.randn(N, F, generator=g) * 0.5
    W = (torch.rand(F, F, generator=g) * 2 - 1) * (scale / F ** 0.5)
    m = torch.randn(B, F, generator=g)
    batch = torch.repeat_interleave(torch.arange(B), sizes)
    return x, W, m, batch, sizes


def _raw(x, W, m, sizes, mode, gout=1.3, N_cap=None):
    """Forward + backward through the C ABI on NaN-filled outputs (dW by ops' weight-gradient call); with N_cap the
    `_dyn` forms with the real N read from the device (rows past it finite, so a row the kernels wrongly read would
    show, and NaN outputs there that a wrong write would overwrite)."""
    from geossl_amd import _lib, ops
    from geossl_amd._lib import ptr, stream
    lib = _lib.load()
    N, F = x.shape
    B = sizes.numel()
    Nc = N_cap or N
    xd = torch.cat([x, torch.full((Nc - N, F), 3.0)]).to(DEV)
    Wd = W.to(DEV).contiguous()
    mp = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)]).to(torch.int32).to(DEV)
    md = m.to(DEV).contiguous() if mode == "external" else None
    dims = torch.tensor([N], dtype=torch.int32, device=DEV) if N_cap else None
    f = lambda *shape: torch.full(shape, NAN, device=DEV)
    s, h, scores = f(B, F), f(B, F), f(2, Nc)
    ws = f(int(lib.geossl_infograph_fwd_workspace_floats(B)))
    loss = f()
    counts = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    st = stream()
    _lib.call("geossl_infograph_fwd_dyn", ptr(xd), Nc, F, ptr(Wd), ptr(mp), B, MODES[mode], ptr(md), ptr(s), ptr(h),
              ptr(scores), ptr(ws), ptr(loss), ptr(counts), ptr(dims), st)
    dx, dh = f(Nc, F), f(B, F)
    dm = f(B, F) if mode == "external" else None
    g = torch.tensor(gout, dtype=torch.float32, device=DEV)
    _lib.call("geossl_infograph_bwd_dyn", ptr(xd), Nc, F, ptr(Wd), ptr(mp), B, MODES[mode], ptr(s), ptr(h),
              ptr(scores), ptr(g), ptr(dx), ptr(dm), ptr(dh), ptr(dims), st)
    dW = f(F, F)
    ops._infograph_wgrad(s, dh, dW, False)
    torch.cuda.synchronize()
    return dict(loss=loss.cpu(), counts=counts.cpu().tolist(), pos=scores[0].cpu(), neg=scores[1].cpu(), dx=dx.cpu(),
                dm=None if dm is None else dm.cpu(), dW=dW.cpu(), s=s.cpu(), h=h.cpu())


def _check(sizes, F, mode, seed, N_cap=None, gout=1.3, scale=1.0):
    x, W, m, batch, sizes = _inputs(sizes, F, seed, scale)
    N, B = x.size(0), sizes.numel()
    got = _raw(x, W, m, sizes, mode, gout, N_cap)
    if N_cap:   # rows past the real count are not written
        assert torch.isnan(got["dx"][N:]).all() and torch.isnan(got["pos"][N:]).all()
    x64 = x.double().requires_grad_()
    W64 = W.double().requires_grad_()
    if mode == "external":
        m64 = m.double().requires_grad_()
        mr = m64
    else:
        mr = tw.readout(x64, batch, B, mode)
    loss, pos, neg = tw.infograph_loss(x64, mr, W64, batch)
    (loss * gout).backward()
    # a score's rounding scale: sum_k |x_ik| |h_bk| with |h| bounded by sigmoid(m) |W| (fp32 dot products and GEMV)
    with torch.no_grad():
        hmag = torch.sigmoid(mr) @ W64.abs()
        xa = x64.abs()
        mag = {"pos": (xa * hmag[batch]).sum(1), "neg": (xa * hmag[tw.cycle_index(B)][batch]).sum(1)}
    tols = {k: 1e-6 * v + 1e-9 for k, v in mag.items()}
    lerr = abs(float(got["loss"]) - loss.item())
    assert lerr <= 1e-6 * float(mag["pos"].mean() + mag["neg"].mean()) + 1e-6 * abs(loss.item()), (F, mode)
    for key, want in (("pos", pos), ("neg", neg)):
        assert bool(((got[key][:N].double() - want.detach()).abs() <= tols[key]).all()), key
    # the hit counts: exact wherever the twin's score is not within rounding of 0
    assert got["counts"] == [int((got["pos"][:N] > 0).sum()), int((got["neg"][:N] < 0).sum())]
    for c, key, sgn in ((got["counts"][0], "pos", 1), (got["counts"][1], "neg", -1)):
        sv = (pos if key == "pos" else neg).detach()
        sure = int((sgn * sv > tols[key]).sum())
        near = int((sv.abs() <= tols[key]).sum())
        assert sure <= c <= sure + near
    # the gradients' rounding scales: the same chain on magnitudes (B = 1 or scores near 0 cancel g_pos against g_neg)
    with torch.no_grad():
        c = gout / N
        sv = torch.sigmoid(mr)
        xs = torch.zeros(B, x.size(1), dtype=torch.float64).index_add_(0, batch, xa)
        dh_mag = c * (xs + xs[torch.arange(B) - 1])
        dm_mag = (dh_mag @ W64.abs().t()) * sv * (1 - sv)
        cnt = torch.bincount(batch, minlength=B).clamp(min=1).double()[:, None]
        ro = torch.zeros_like(dm_mag) if mode == "external" else dm_mag / (cnt if mode == "mean" else 1.0)
        mags = {"dx": c * (hmag[batch] + hmag[tw.cycle_index(B)][batch]) + ro[batch],
                "dW": sv.t() @ dh_mag, "dm": dm_mag}
    for key, want in (("dx", x64.grad), ("dW", W64.grad)) + ((("dm", m64.grad),) if mode == "external" else ()):
        gv = got[key][:N] if key == "dx" else got[key]
        assert torch.isfinite(gv).all(), key
        err = (gv.double() - want).abs()
        assert bool((err <= 1e-5 * mags[key] + 1e-12).all()), (key, F, mode, float((err / mags[key]).max()))
    return got


@pytest.mark.parametrize("F", [64, 128, 256])
@pytest.mark.parametrize("mode", ["mean", "add", "external"])
def test_head_kernels_vs_fp64(F, mode):
    _check([5, 18, 2, 9, 33, 1, 12, 1, 40], F, mode, seed=F + len(mode))
    _check([11], F, mode, seed=3)          # B = 1: the negative summary is the positive one
    _check([1], F, mode, seed=4)           # one molecule of one atom
    _check([1, 1, 1], F, mode, seed=5)     # 1-atom molecules only


@pytest.mark.parametrize("F", [64, 128, 256])
def test_head_kernels_dyn(F):
    _check([5, 18, 2, 9, 33, 1, 12], F, "mean", seed=6, N_cap=200)
    _check([3, 7], F, "add", seed=7, N_cap=40, scale=8.0)   # (scores far from 0: saturated sigmoids)


def test_head_kernels_bs1024_up_to_255_atoms():
    rng = np.random.default_rng(11)
    sizes = rng.integers(1, 256, size=1024)
    sizes[:3] = (1, 255, 1)
    for mode in ("mean", "add"):
        _check(sizes.tolist(), 128, mode, seed=12)


def test_kernels_are_deterministic():
    sizes = np.random.default_rng(2).integers(1, 60, size=300).tolist()
    x, W, m, _, sz = _inputs(sizes, 128, 9)
    runs = [_raw(x, W, m, sz, "mean") for _ in range(3)]
    runs += [_raw(x, W, m, sz, "external") for _ in range(2)]
    for r in runs[1:3]:
        for k in ("loss", "pos", "neg", "dx", "dW", "s", "h"):
            assert torch.equal(r[k], runs[0][k]), k
        assert r["counts"] == runs[0]["counts"]
    for k in ("loss", "dx", "dW", "dm"):
        assert torch.equal(runs[4][k], runs[3][k]), k


def test_ops_head_and_loss_agree():
    """infograph_head (readout inside) and infograph_loss (readout outside + autograd through the backbone's
    _SegmentReduce) give the same loss, counts and node gradient."""
    from geossl_amd import ops
    from geossl_amd.Geom3D.models.schnet import _SegmentReduce
    from geossl_amd.layout import get_layout
    x, W, _, batch, _ = _inputs([5, 18, 2, 9, 1, 12], 128, 21)
    b = batch.to(DEV)
    lay = get_layout(b)
    for readout in ("mean", "add"):
        x1 = x.to(DEV).requires_grad_()
        W1 = W.to(DEV).requires_grad_()
        l1, c1 = ops.infograph_head(x1, W1, lay, readout)
        l1.backward()
        x2 = x.to(DEV).requires_grad_()
        W2 = W.to(DEV).requires_grad_()
        l2, c2 = ops.infograph_loss(x2, _SegmentReduce.apply(x2, lay, readout), W2, lay)
        l2.backward()
        assert torch.equal(l1, l2) and torch.equal(c1, c2)
        assert rel_err(x1.grad, x2.grad) < 1e-6 and torch.equal(W1.grad, W2.grad)


# ---------------------------------------------------------------------------------------------- G20
def _g20_setup(case):
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    from geossl_amd.pretrain_3DInfoGraph import Discriminator
    from geossl_amd.synthetic import combination_pairs
    g = load_golden(case)
    meta, cfg = json.loads(str(g["meta"])), json.loads(str(g["cfg"]))
    model = fill_module_(SchNet(**cfg) if meta["kind"] == "schnet" else PaiNN(**cfg)).to(DEV)
    disc = fill_module_(Discriminator(meta["emb_dim"])).to(DEV)
    rei = t(g["radius_edge_index"], DEV) if "radius_edge_index" in g else None
    sizes = g["sizes"]
    off = np.concatenate([[0], np.cumsum(sizes)])
    sei = np.concatenate([combination_pairs(int(n)) + off[m] for m, n in enumerate(sizes)], axis=1).astype(np.int64)

    def batch():
        return pg.Batch(t(g["x"], DEV), t(g["positions"], DEV), t(g["batch"], DEV), t(sei, DEV),
                        radius_edge_index=rei, num_graphs=len(sizes))
    return g, meta, model, disc, batch, types.SimpleNamespace(model_3d=meta["kind"])


def _check_g20(g, model, disc, loss, acc, case):
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert rel_err(loss.detach().cpu(), g["loss"]) < 1e-5, case
    assert acc == float(g["acc"]), case
    assert rel_err(disc.weight.grad.cpu(), g["grad_disc_weight"]) < 1e-4, case
    grads = unique_named_grads(model)
    for k in g:
        if k.startswith("grad/") or k.startswith("gsum/"):
            got = grads[k.split("/", 1)[1]].cpu()
            got = grad_summary(got) if k.startswith("gsum/") else got
            assert rel_err(got, g[k]) < 1e-4 or float(np.abs(g[k]).max()) < 1e-8, (case, k)


@pytest.mark.parametrize("case", G20)
def test_g20_do_infograph(case):
    """The reference's loop body with our backbone's readout and do_InfoGraph on the fused loss kernels."""
    from geossl_amd.pretrain_3DInfoGraph import do_InfoGraph
    g, meta, model, disc, make, _ = _g20_setup(case)
    b = make()
    if meta["kind"] == "schnet":
        molecule_repr, node_repr = model(b.x[:, 0], b.positions, b.batch, return_latent=True)
    else:
        molecule_repr, node_repr = model(b.x[:, 0], b.positions, b.radius_edge_index, b.batch, return_latent=True)
    node_repr.retain_grad()
    molecule_repr.retain_grad()
    loss, acc = do_InfoGraph(node_repr, molecule_repr, b, torch.nn.BCEWithLogitsLoss(), disc)
    loss.backward()
    assert rel_err(molecule_repr.grad.cpu(), g["grad_molecule_repr"]) < 1e-4
    assert rel_err(node_repr.grad.cpu(), g["grad_node_repr"]) < 1e-4
    _check_g20(g, model, disc, loss, acc, case)


@pytest.mark.parametrize("case", G20)
@pytest.mark.parametrize("graph", [False, True])
def test_g20_do_3dinfograph(case, graph):
    from geossl_amd.pretrain_3DInfoGraph import do_3DInfoGraph
    g, meta, model, disc, make, args = _g20_setup(case)
    b = make()
    for _ in range(2 if graph else 1):   # (a structure known by its tensors is captured at its second sighting)
        model.zero_grad(set_to_none=True)
        disc.zero_grad(set_to_none=True)
        loss, acc = do_3DInfoGraph(args, b, model, disc, graph=graph)
        loss.backward()
    _check_g20(g, model, disc, loss, acc, case)


def test_fallbacks_match_aten():
    """A pos_weight criterion and an unserved width (48) run the reference's ATen code on our backbone."""
    from geossl_amd.Geom3D.models import SchNet
    from geossl_amd.pretrain_3DInfoGraph import Discriminator, _infograph_aten, do_3DInfoGraph
    _, _, _, _, make, args = _g20_setup("g20_infograph_schnet_reduced")
    for F, crit in ((48, torch.nn.BCEWithLogitsLoss()), (64, torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(
            [2.0], device=DEV)))):
        cfg = dict(hidden_channels=F, num_filters=F, num_interactions=2, num_gaussians=8, cutoff=5.0, node_class=9)
        model = fill_module_(SchNet(**cfg)).to(DEV)
        disc = fill_module_(Discriminator(F)).to(DEV)
        b = make()
        loss, acc = do_3DInfoGraph(args, b, model, disc, criterion=crit)
        m, h = model(b.x[:, 0], b.positions, b.batch, return_latent=True)
        ref, ref_acc = _infograph_aten(h, m, b, crit, disc)
        assert rel_err(loss.detach().cpu(), ref.detach().cpu()) < 1e-6 and acc == ref_acc, F


# ---------------------------------------------------------------------------------------------- graph paths
def _ragged_batches(n, B, seed, option="permutation"):
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import collate_subset, make_batch
    pool = make_batch(4 * B, seed=seed, mode="B", option=option)
    rng = np.random.default_rng(seed)
    return [pg.Batch.from_numpy(collate_subset(pool, rng.permutation(4 * B)[:B], option=option), DEV) for _ in range(n)]


def _model(kind):
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    return (fill_module_(SchNet(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51,
                                cutoff=10.0, node_class=9)) if kind == "schnet" else
            fill_module_(PaiNN(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1,
                               readout="add"))).to(DEV)


def _disc(F=128):
    from geossl_amd.pretrain_3DInfoGraph import Discriminator
    return fill_module_(Discriminator(F)).to(DEV)


def _grads(model, disc):
    return [p.grad.clone() for p in list(model.parameters()) + list(disc.parameters()) if p.grad is not None]


def _replay_vs_eager(model, disc, kind, batches):
    from geossl_amd.pretrain_3DInfoGraph import do_3DInfoGraph
    args = types.SimpleNamespace(model_3d=kind)
    for k, b in enumerate(batches):
        out = []
        for graph in (False, True):
            model.zero_grad(set_to_none=True)
            disc.zero_grad(set_to_none=True)
            loss, acc = do_3DInfoGraph(args, b, model, disc, graph=graph)
            loss.backward()
            out.append((loss.detach().clone(), acc, _grads(model, disc)))
        assert rel_err(out[1][0].cpu(), out[0][0].cpu()) < 1e-6, (kind, k)
        assert out[1][1] == out[0][1], (kind, k)
        assert len(out[1][2]) == len(out[0][2])
        for a, c in zip(out[1][2], out[0][2]):
            assert rel_err(a, c) < 1e-5, (kind, k)
    eng = model.__dict__["_geossl_infograph_step"]
    (sg,) = eng.graphs.values()
    return sg


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_bucket_replay_matches_eager_on_ragged_batches(kind):
    model, disc = _model(kind), _disc()
    batches = _ragged_batches(4, 24, 17)
    if kind == "painn":
        from geossl_amd import ops
        for b in batches:
            b.radius_edge_index = ops.radius_graph(b.positions, 5.0, b.batch)
    sg = _replay_vs_eager(model, disc, kind, batches)
    assert len(sg) == 1 and next(iter(sg.graphs))[0] == "bucket" and sg.views == 1


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_bucket_replay_matches_eager_on_device_loader(kind):
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    from geossl_amd.synthetic import make_molecules
    ds = DeviceDataset.from_numpy(make_molecules(200, seed=3, mode="C"), DEV, option="permutation",
                                  **({"radius": 5.0} if kind == "painn" else {}))
    loader = DeviceLoader(ds, batch_size=32, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(2))
    sg = _replay_vs_eager(_model(kind), _disc(), kind, [hb for _, hb in zip(range(4), loader)])
    assert len(sg) == 1 and next(iter(sg.graphs))[0] == "bucket"


def test_reference_loop_and_trainer_match_stock_adam():
    """Six steps of the reference loop with do_3DInfoGraph (graph replay, stock torch.optim.Adam over the reference's two
    groups) and of InfoGraphTrainer (one bucket graph) against the reference's ATen loop body on our backbone."""
    from geossl_amd.pretrain_3DInfoGraph import InfoGraphTrainer, _infograph_aten, do_3DInfoGraph
    args = types.SimpleNamespace(model_3d="schnet")
    crit = torch.nn.BCEWithLogitsLoss()

    def ref_loop(fused):
        m, d = _model("schnet"), _disc()
        opt = torch.optim.Adam([{"params": m.parameters(), "lr": 1e-4}, {"params": d.parameters(), "lr": 1e-4}],
                               lr=1e-4)
        losses, accs = [], []
        for b in _ragged_batches(6, 16, 5):
            if fused:
                loss, acc = do_3DInfoGraph(args, b, m, d, graph=True)
            else:
                mr, nr = m(b.x[:, 0], b.positions, b.batch, return_latent=True)
                loss, acc = _infograph_aten(nr, mr, b, crit, d)
            losses.append(float(loss.detach()))
            accs.append(acc)
            opt.zero_grad()
            loss.backward()
            opt.step()
        return losses, accs, m, d

    ref, ref_acc, m1, d1 = ref_loop(False)
    rep, rep_acc, _, _ = ref_loop(True)
    np.testing.assert_allclose(rep, ref, rtol=1e-4)
    np.testing.assert_allclose(rep_acc, ref_acc, atol=0.02)
    m2, d2 = _model("schnet"), _disc()
    tr = InfoGraphTrainer(m2, d2, lr=1e-4, use_graph=True)
    got = [tr.step(b) for b in _ragged_batches(6, 16, 5)]
    np.testing.assert_allclose([float(l) for l, _ in got], ref, rtol=1e-4)
    assert all(c.dtype == torch.int32 and c.numel() == 2 for _, c in got)
    assert rel_err(d2.weight.detach().cpu(), d1.weight.detach().cpu()) < 1e-4
    assert rel_err(m2.lin2.weight.detach().cpu(), m1.lin2.weight.detach().cpu()) < 1e-4
    assert len(tr.step_graphs) == 1 and next(iter(tr.step_graphs.graphs))[0] == "bucket"


def test_head_launches_no_aten_arithmetic():
    """The head's forward and backward (as a replayed step captures them) call no floating-point ATen operator and
    launch only the library's kernels."""
    from torch.profiler import ProfilerActivity, profile
    from geossl_amd import _lib, ops
    from geossl_amd.layout import get_layout
    x, W, _, batch, _ = _inputs([5, 18, 2, 9, 1, 12], 128, 31)
    lay = get_layout(batch.to(DEV))
    xd = x.to(DEV).requires_grad_()
    Wd = W.to(DEV).requires_grad_()
    Wd.grad = torch.zeros_like(Wd)
    one = torch.ones((), device=DEV)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with _lib.direct_grads():
            loss, _ = ops.infograph_head(xd, Wd, lay, "mean")
            loss.backward(one)
        torch.cuda.synchronize()
    allowed = {"aten::empty", "aten::empty_like", "aten::empty_strided", "aten::to", "aten::_to_copy", "aten::detach",
               "detach", "aten::contiguous", "aten::slice", "aten::as_strided", "aten::view", "aten::lift_fresh",
               "aten::alias", "aten::resize_", "aten::copy_"}
    names = {e.name for e in prof.events() if e.name.startswith("aten::")}
    assert names <= allowed, names - allowed
    kernels = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()}
    ours = lambda n: re.match(r"(void )?(geossl::)?k_\w+", n.replace("(anonymous namespace)::", "")) is not None
    others = sorted(n for n in kernels if not ours(n) or "at::" in n)
    assert kernels and not others, others
    assert torch.isfinite(xd.grad).all() and torch.isfinite(Wd.grad).all()
