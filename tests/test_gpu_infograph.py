"""GPU tests of 3D InfoGraph pretraining: the head kernels of csrc/infograph_head.hip against fp64 on NaN-poisoned outputs
(every served width, mean / add / external readouts, B = 1, 1-atom molecules, capacity launches, 1024 molecules of up to
255 atoms), determinism, the hit counts, fixture G20 through do_InfoGraph and do_3DInfoGraph, bucket replay against
eager, stock-Adam and trainer trajectories against the reference's ATen loop, and the ATen-free head."""
import json
import os
import types

import numpy as np
import pytest
import torch

import infograph_twin as tw
from conftest import load_golden, rel_err
from helpers import fill_module_, grad_summary, t, unique_named_grads
from objective_harness import (Case, assert_one_bucket, assert_only_library_kernels, backbone, kind_args, loader_handles,
                               ragged_batches, reference_loop_vs_trainer, replay_vs_eager, with_radius_edges)

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
def _heads(kind, model):
    from geossl_amd.pretrain_3DInfoGraph import Discriminator
    return [fill_module_(Discriminator(128)).to(DEV)]


def _step(args, batch, model, heads, graph):
    from geossl_amd.pretrain_3DInfoGraph import do_3DInfoGraph
    loss, acc = do_3DInfoGraph(args, batch, model, heads[0], graph=graph)
    return loss, (acc,)


def _aten_step(args, b, model, heads):
    from geossl_amd.pretrain_3DInfoGraph import _infograph_aten
    mr, nr = model(b.x[:, 0], b.positions, b.batch, return_latent=True)
    loss, acc = _infograph_aten(nr, mr, b, torch.nn.BCEWithLogitsLoss(), heads[0])
    return loss, (acc,)


def _trainer(model, heads, **kw):
    from geossl_amd.pretrain_3DInfoGraph import InfoGraphTrainer
    return InfoGraphTrainer(model, heads[0], **kw)


CASE = Case("infograph", "_geossl_infograph_step", _heads, kind_args(), _step, _trainer, aten_step=_aten_step,
            head_weight=lambda heads: heads[0].weight, loss_of=lambda out: out[0])


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_bucket_replay_matches_eager_on_ragged_batches(kind):
    model = backbone(kind)
    heads = CASE.heads(kind, model)
    batches = ragged_batches(4, 24, 17)
    if kind == "painn":
        with_radius_edges(batches)
    assert_one_bucket(replay_vs_eager(CASE, kind, model, heads, batches), views=CASE.views)


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_bucket_replay_matches_eager_on_device_loader(kind):
    model = backbone(kind)
    assert_one_bucket(replay_vs_eager(CASE, kind, model, CASE.heads(kind, model), loader_handles(kind)))


def test_reference_loop_and_trainer_match_stock_adam():
    """Six steps of the reference loop with do_3DInfoGraph (graph replay, stock torch.optim.Adam over the reference's two
    groups) and of InfoGraphTrainer (one bucket graph) against the reference's ATen loop body on our backbone."""
    r = reference_loop_vs_trainer(CASE, 6, 16, 5, per_step=False)
    np.testing.assert_allclose([acc for acc, in r.rep_extras], [acc for acc, in r.ref_extras], atol=0.02)
    assert all(c.dtype == torch.int32 and c.numel() == 2 for _, c in r.trainer_out)


def test_head_launches_no_aten_arithmetic():
    """The head's forward and backward (as a replayed step captures them) call no floating-point ATen operator and
    launch only the library's kernels."""
    from geossl_amd import ops
    from geossl_amd.layout import get_layout
    x, W, _, batch, _ = _inputs([5, 18, 2, 9, 1, 12], 128, 31)
    lay = get_layout(batch.to(DEV))
    xd = x.to(DEV).requires_grad_()
    Wd = W.to(DEV).requires_grad_()
    Wd.grad = torch.zeros_like(Wd)
    one = torch.ones((), device=DEV)
    assert_only_library_kernels(lambda: ops.infograph_head(xd, Wd, lay, "mean")[0].backward(one))
    assert torch.isfinite(xd.grad).all() and torch.isfinite(Wd.grad).all()
