"""GPU tests of Charge Prediction pretraining: the mask and head kernels of csrc/charge_head.hip against fp64 on
NaN-poisoned outputs (every served width, k from 0 to thousands, logits of +-80), determinism, the device k rule up to
the largest bucket, the device draw (exact k, distinct, ascending, labels, token write, seeds, inclusion frequency),
fixture G19 through do_ChargePrediction with numpy masks, the fallbacks, bucket replay against eager, and the trainer
and a stock Adam against the reference loop."""
import gc
import json
import os
import types

import numpy as np
import pytest
import torch

import charge_twin as tw
from conftest import load_golden, rel_err
from helpers import fill_module_, grad_summary, t, unique_named_grads
from objective_harness import (Case, assert_one_bucket, backbone, kind_args, loader_handles, ragged_batches,
                               reference_loop_vs_trainer, replay_vs_eager, with_radius_edges)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G19 = sorted(f[:-4] for f in os.listdir(os.path.join(REPO, "tests", "golden")) if f.startswith("g19_charge_"))
NAN = float("nan")
MAX_N = 1024 * 255   # the largest batch a bucket holds: bs = 1024 molecules of 255 atoms


def _types(N, seed, C=9):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(N, 2, dtype=torch.long)
    x[:, 0] = torch.randint(0, C, (N,), generator=g)
    x[:, 1] = 7
    return x


def _mask_raw(x, ratio, seed=None, given=None, C=9, N_cap=None):
    """geossl_charge_mask_dyn on a copy of x (at capacity N_cap, the rows past N at type 5) -> (x after, idx, labels,
    k, seed after)."""
    from geossl_amd import _lib
    from geossl_amd._lib import ptr, stream
    N = x.size(0)
    Nc = N_cap or N
    xd = torch.cat([x, torch.full((Nc - N, x.size(1)), 5, dtype=torch.long)]).to(DEV).contiguous()
    idx = torch.full((max(Nc, 1),), -7, dtype=torch.long, device=DEV)
    lab = torch.full((max(Nc, 1),), -7, dtype=torch.long, device=DEV)
    k = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    sd = None if seed is None else torch.tensor([seed], dtype=torch.long, device=DEV)
    gv = None if given is None else torch.as_tensor(given, dtype=torch.long).to(DEV)
    dims = torch.tensor([N], dtype=torch.int32, device=DEV) if N_cap else None
    _lib.call("geossl_charge_mask_dyn", ptr(xd), x.size(1), Nc, float(ratio), C, ptr(sd), ptr(gv), ptr(idx), ptr(lab),
              ptr(k), ptr(dims), stream())
    kk = int(k.item())
    return xd.cpu(), idx[:kk].cpu(), lab[:kk].cpu(), kk, (None if sd is None else int(sd.item())), idx.cpu()


def _head_raw(h, W, b, idx, labels, gout=1.3, N_cap=None, K_cap=None):
    """Forward + backward through the C ABI on NaN-filled outputs; with caps, the `_dyn` forms with the real N and k
    read from the device (inputs past them finite, so a row the kernels wrongly processed would show)."""
    from geossl_amd import _lib
    from geossl_amd._lib import ptr, stream
    lib = _lib.load()
    N, F = h.shape
    C, K = W.size(0), idx.numel()
    Nc, Kc = N_cap or N, K_cap or K
    hd = torch.cat([h, torch.full((Nc - N, F), 3.0)]).to(DEV)
    idd = torch.cat([idx, torch.zeros(Kc - K, dtype=torch.long)]).to(DEV)
    lbd = torch.cat([labels, torch.zeros(Kc - K, dtype=torch.long)]).to(DEV)
    Wd, bd = W.to(DEV).contiguous(), b.to(DEV).contiguous()
    kd = torch.tensor([K], dtype=torch.int32, device=DEV)
    dims = torch.tensor([N], dtype=torch.int32, device=DEV) if N_cap else None
    prob = torch.full((max(Kc, 1), C), NAN, device=DEV)
    ws = torch.full((int(lib.geossl_charge_head_fwd_workspace_floats(Kc)),), NAN, device=DEV)
    loss = torch.full((), NAN, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = stream()
    _lib.call("geossl_charge_head_fwd_dyn", ptr(hd), Nc, F, ptr(Wd), ptr(bd), C, ptr(idd), ptr(lbd), Kc, ptr(kd),
              ptr(prob), ptr(ws), ptr(loss), ptr(status), ptr(dims), st)
    dh = torch.full((Nc, F), NAN, device=DEV)
    dW = torch.full((C, F), NAN, device=DEV)
    db = torch.full((C,), NAN, device=DEV)
    ws2 = torch.full((max(int(lib.geossl_charge_head_bwd_workspace_floats(Kc, F, C)), 1),), NAN, device=DEV)
    g = torch.tensor(gout, dtype=torch.float32, device=DEV)
    _lib.call("geossl_charge_head_bwd_dyn", ptr(hd), Nc, F, ptr(Wd), C, ptr(idd), ptr(lbd), Kc, ptr(kd), ptr(prob),
              ptr(g), ptr(dh), ptr(dW), ptr(db), ptr(ws2), 0, ptr(dims), st)
    torch.cuda.synchronize()
    return dict(loss=loss.cpu(), prob=prob.cpu(), dh=dh.cpu(), dW=dW.cpu(), db=db.cpu(), status=int(status.item()))


def _head_inputs(N, F, k, seed, scale=1.0, C=9):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(N, F, generator=g)
    W = torch.randn(C, F, generator=g) * (scale / F ** 0.5)
    b = torch.randn(C, generator=g) * 0.1
    idx = torch.randperm(N, generator=g)[:k]
    labels = torch.randint(0, C, (k,), generator=g)
    labels[:min(k, 3)] = C - 1   # (the mask token's type as a real label)
    return h, W, b, idx, labels


def _check_head(N, F, k, seed, scale=1.0, dyn=False, gout=1.3):
    h, W, b, idx, labels = _head_inputs(N, F, k, seed, scale)
    caps = dict(N_cap=N + 37, K_cap=k + 50) if dyn else {}
    got = _head_raw(h, W, b, idx, labels, gout, **caps)
    assert got["status"] == 0
    if dyn:   # rows past the real counts are not written
        assert torch.isnan(got["dh"][N:]).all() and torch.isnan(got["prob"][max(k, 1):]).all()
    dh = got["dh"][:N]
    h64 = h.double().requires_grad_()
    W64, b64 = W.double().requires_grad_(), b.double().requires_grad_()
    loss, z = tw.charge_loss(h64, W64, b64, idx, labels)
    if k == 0:
        assert torch.isnan(got["loss"]) and torch.isnan(loss)
        for key in ("dh", "dW", "db"):
            t_ = dh if key == "dh" else got[key]
            assert torch.equal(t_, torch.zeros_like(t_)), key   # exactly zero (and no NaN)
        return got
    assert abs(float(got["loss"]) - float(loss.detach())) <= 2e-6 * abs(float(loss)) + 1e-6
    p64 = torch.softmax(z.detach(), 1)
    assert float((got["prob"][:k].double() - p64).abs().max()) <= 1e-5
    (loss * gout).backward()
    rows = torch.zeros(N, dtype=torch.bool)
    rows[idx] = True
    assert torch.equal(dh[~rows], torch.zeros_like(dh[~rows]))
    assert rel_err(dh, h64.grad) < 1e-5
    assert rel_err(got["dW"], W64.grad) < 1e-5
    assert rel_err(got["db"], b64.grad) < 1e-5
    return got


@pytest.mark.parametrize("F", [64, 128, 256, 512])
@pytest.mark.parametrize("k", [0, 1, 7, 4500])
def test_head_kernels_vs_fp64(F, k):
    _check_head(max(2 * k, 20), F, k, 11 + F + k)


@pytest.mark.parametrize("F", [64, 128])
def test_head_kernels_dyn_and_large_logits(F):
    _check_head(3000, F, 900, 5, dyn=True)
    _check_head(300, F, 77, 6, dyn=True)
    got = _check_head(400, F, 120, 7, scale=80.0)   # logits of +-80: the max subtraction keeps them finite
    assert torch.isfinite(got["loss"]) and float(got["loss"]) > 10


def test_label_out_of_range_sets_the_status_word():
    h, W, b, idx, labels = _head_inputs(50, 64, 10, 3)
    labels[4] = 9
    got = _head_raw(h, W, b, idx, labels)
    assert got["status"] == 1 and torch.isnan(got["loss"])
    assert torch.isfinite(got["dh"]).all() and torch.isfinite(got["dW"]).all()


def test_kernels_are_deterministic():
    x = _types(20000, 1)
    h, W, b, _, _ = _head_inputs(20000, 128, 0, 2)
    runs = []
    for _ in range(4):
        xa, idx, lab, k, _, _ = _mask_raw(x, 0.3, seed=12345)
        runs.append((xa, idx, lab, _head_raw(h, W, b, idx, lab)))
    for r in runs[1:]:
        for a, c in zip(r[:3], runs[0][:3]):
            assert torch.equal(a, c)
        for key in ("loss", "dh", "dW", "db", "prob"):
            assert torch.equal(r[3][key].view(torch.int32), runs[0][3][key].view(torch.int32)), key


def test_device_k_rule_for_every_batch_size():
    """k written by the launch is int(N * r) for every N up to the bucket maximum (given mode: the k rule alone)."""
    from geossl_amd import _lib
    from geossl_amd._lib import ptr, stream
    x = torch.zeros(MAX_N, 1, dtype=torch.long, device=DEV)
    given = torch.zeros(MAX_N, dtype=torch.long, device=DEV)
    scratch = torch.empty(MAX_N, dtype=torch.long, device=DEV)
    dims = torch.empty(MAX_N + 1, dtype=torch.int32, device=DEV)
    dims.copy_(torch.arange(MAX_N + 1, dtype=torch.int32))
    for r, Ns in ((0.3, range(0, MAX_N + 1)), (0.15, range(0, MAX_N + 1, 7)), (1.0 / 3.0, range(0, MAX_N + 1, 11)),
                  (0.999, range(0, MAX_N + 1, 13))):
        Ns = list(Ns)
        ks = torch.full((len(Ns),), -1, dtype=torch.int32, device=DEV)
        st = stream()
        for j, N in enumerate(Ns):
            _lib.call("geossl_charge_mask_dyn", ptr(x), 1, MAX_N, r, 9, None, ptr(given), ptr(scratch), ptr(scratch),
                      ks.data_ptr() + 4 * j, dims.data_ptr() + 4 * N, st)
        want = np.array([int(N * r) for N in Ns], dtype=np.int32)
        assert np.array_equal(ks.cpu().numpy(), want), r


@pytest.mark.parametrize("N,ratio", [(1, 0.3), (3, 0.3), (10, 0.3), (1000, 0.3), (4097, 0.5), (1000, 1.0),
                                     (1000, 0.0), (MAX_N, 0.3), (50000, 0.001)])
def test_device_draw(N, ratio):
    x = _types(N, N)
    Nc = N + 100 if N < MAX_N else N
    xa, idx, lab, k, seed_after, idx_all = _mask_raw(x, ratio, seed=-987654321, N_cap=Nc)
    assert k == int(N * ratio) and idx.numel() == k
    assert seed_after == -987654320   # advanced by one
    if k:
        assert bool((idx[1:] > idx[:-1]).all()) and int(idx[0]) >= 0 and int(idx[-1]) < N   # distinct, ascending
    assert torch.equal(lab, x[idx, 0])
    want = x.clone()
    want[idx, 0] = 8
    assert torch.equal(xa[:N], want) and bool((xa[N:] == 5).all())
    assert bool((idx_all[k:] == -7).all())   # nothing past k written


def test_device_draw_seeds_and_frequency():
    from geossl_amd import _lib
    from geossl_amd._lib import ptr, stream
    N, r = 40, 0.3
    x = _types(N, 9)
    a = _mask_raw(x, r, seed=77)[1]
    assert torch.equal(a, _mask_raw(x, r, seed=77)[1])
    assert not torch.equal(a, _mask_raw(x, r, seed=78)[1])
    # successive launches on one seed buffer (what a replayed graph does): fresh masks, inclusion frequency k / N
    draws = 4000
    xd = x.to(DEV)
    sd = torch.tensor([2024], dtype=torch.long, device=DEV)
    idx = torch.empty(draws, N, dtype=torch.long, device=DEV)
    lab = torch.empty(N, dtype=torch.long, device=DEV)
    k = torch.empty(1, dtype=torch.int32, device=DEV)
    st = stream()
    for d in range(draws):
        xd.copy_(x.to(DEV))
        _lib.call("geossl_charge_mask", ptr(xd), 2, N, r, 9, ptr(sd), None, ptr(idx[d]), ptr(lab), ptr(k), st)
    kk = int(N * r)
    sel = idx[:, :kk].cpu()
    assert int(sd.item()) == 2024 + draws
    assert len({tuple(s.tolist()) for s in sel}) > draws - 5   # (C(40, 12) subsets: repeats are vanishingly rare)
    counts = torch.bincount(sel.reshape(-1), minlength=N).double()
    p = kk / N
    sd_ = (draws * p * (1 - p)) ** 0.5
    assert float((counts - draws * p).abs().max()) < 5 * sd_, counts   # 5 sigma per atom, 40 atoms


def test_given_list_used_as_is():
    x = _types(30, 4)
    given = torch.tensor([17, 3, 29, 8, 0, 11, 22, 5, 14])
    xa, idx, lab, k, _, _ = _mask_raw(x, 0.3, given=given)
    assert k == 9 and torch.equal(idx, given) and torch.equal(lab, x[given, 0])
    want = x.clone()
    want[given, 0] = 8
    assert torch.equal(xa, want)


# ---------------------------------------------------------------------------------------------- the step vs G19
def _g19_setup(case):
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    from geossl_amd.pretrain_ChargePrediction import ChargePredictor
    g = load_golden(case)
    meta, cfg = json.loads(str(g["meta"])), json.loads(str(g["cfg"]))
    model = fill_module_(SchNet(**cfg) if meta["kind"] == "schnet" else PaiNN(**cfg)).to(DEV)
    cp = fill_module_(ChargePredictor(meta["emb_dim"])).to(DEV)
    rei = t(g["radius_edge_index"], DEV) if "radius_edge_index" in g else None
    sizes = g["sizes"]
    from geossl_amd.synthetic import combination_pairs
    off = np.concatenate([[0], np.cumsum(sizes)])
    sei = np.concatenate([combination_pairs(int(n)) + off[m] for m, n in enumerate(sizes)], axis=1).astype(np.int64)

    def batch():
        return pg.Batch(t(g["x"], DEV).clone(), t(g["positions"], DEV), t(g["batch"], DEV), t(sei, DEV),
                        radius_edge_index=rei, num_graphs=len(sizes))
    args = types.SimpleNamespace(model_3d=meta["kind"], charge_masking_ratio=meta["ratio"])
    return g, meta, model, cp, batch, args


def _check_g19(g, model, cp, loss, case):
    if g["masked_index"].size == 0:
        assert torch.isnan(loss).item()
        for p in list(cp.parameters()) + list(model.parameters()):
            assert p.grad is None or not p.grad.abs().sum().item(), case
        return
    assert rel_err(loss.detach().cpu(), g["loss"]) < 1e-5, case
    assert rel_err(cp.predictor.weight.grad.cpu(), g["grad_pred_weight"]) < 1e-4, case
    assert rel_err(cp.predictor.bias.grad.cpu(), g["grad_pred_bias"]) < 1e-4, case
    grads = unique_named_grads(model)
    for k in g:
        if k.startswith("grad/") or k.startswith("gsum/"):
            got = grads[k.split("/", 1)[1]].cpu()
            got = grad_summary(got) if k.startswith("gsum/") else got
            assert rel_err(got, g[k]) < 1e-4 or float(np.abs(g[k]).max()) < 1e-8, (case, k)


@pytest.mark.parametrize("case", G19)
@pytest.mark.parametrize("graph", [False, True])
def test_g19_end_to_end(case, graph):
    from geossl_amd.pretrain_ChargePrediction import do_ChargePrediction
    g, meta, model, cp, make, args = _g19_setup(case)
    batch = make()
    x0 = batch.x.clone()
    for _ in range(2 if graph else 1):   # (a structure known by its tensors is captured at its second sighting)
        batch.x.copy_(x0)
        model.zero_grad(set_to_none=True)
        cp.zero_grad(set_to_none=True)
        np.random.seed(meta["seed"])
        loss = do_ChargePrediction(args, batch, model, cp, graph=graph)
        loss.backward()
        # the same masked atoms as the reference, written into the caller's batch.x as the reference writes them
        assert np.array_equal(batch.x.cpu().numpy(), g["x_after"]), case
    assert loss.dtype == torch.float32 and loss.dim() == 0
    _check_g19(g, model, cp, loss, case)


def test_fallbacks_match_aten():
    """label_smoothing and an unserved width (48) take the ATen head: the reference's own loss on the same mask."""
    from geossl_amd.Geom3D.models import SchNet
    from geossl_amd.pretrain_ChargePrediction import ChargePredictor, do_ChargePrediction, fused_head_ok
    _, meta, _, _, make, args = _g19_setup("g19_charge_schnet_reduced_r05")
    for F, ls in ((48, 0.0), (64, 0.1)):
        cfg = dict(hidden_channels=F, num_filters=F, num_interactions=2, num_gaussians=8, cutoff=5.0, node_class=9)
        model = fill_module_(SchNet(**cfg)).to(DEV)
        cp = fill_module_(ChargePredictor(F)).to(DEV)
        cp.criterion = torch.nn.CrossEntropyLoss(label_smoothing=ls)
        assert not fused_head_ok(cp)
        batch = make()
        x0 = batch.x.clone()
        np.random.seed(meta["seed"])
        loss = do_ChargePrediction(args, batch, model, cp)
        np.random.seed(meta["seed"])
        idx = np.random.choice(x0.size(0), int(x0.size(0) * 0.5), replace=False)
        xm = x0.clone()
        xm[idx, 0] = 8
        assert torch.equal(batch.x, xm)
        _, h = model(xm[:, 0], batch.positions, batch.batch, return_latent=True)
        ref = torch.nn.CrossEntropyLoss(label_smoothing=ls)(cp.predictor(h[idx]), x0[idx, 0])
        assert rel_err(loss.detach().cpu(), ref.detach().cpu()) < 1e-6, F


# ---------------------------------------------------------------------------------------------- graph paths
def _heads(kind, model):
    from geossl_amd.pretrain_ChargePrediction import ChargePredictor
    return [fill_module_(ChargePredictor(128)).to(DEV)]


def _step(args, b, model, heads, graph):
    from geossl_amd.pretrain_ChargePrediction import do_ChargePrediction
    return do_ChargePrediction(args, b, model, heads[0], graph=graph), ()


def _masked_types(b):
    """The caller's types (a collated batch's: not a handle's), masked alike on both paths."""
    return () if getattr(b, "_dataset", None) is not None else (b.x.clone(),)


def _same_draw(b, k):
    """numpy masks: the eager step and the replayed one see the same draw (the numpy stream is re-seeded) on the same
    unmasked types."""
    x0 = b.x.clone() if getattr(b, "_dataset", None) is None else None

    def reset():
        if x0 is not None:
            b.x.copy_(x0)
        else:   # (a handle's collated tensors, which the eager step masked in place, are gathered again)
            b._batch = None
        np.random.seed(1000 + k)
    return reset


def _trainer(model, heads, **kw):
    from geossl_amd.pretrain_ChargePrediction import ChargePredictionTrainer
    return ChargePredictionTrainer(model, heads[0], charge_masking_ratio=0.3, mask_rng="numpy", **kw)


CASE = Case("charge", "_geossl_charge_step", _heads, kind_args(charge_masking_ratio=0.3), _step, _trainer,
            aten_step=lambda args, b, model, heads: _step(args, b, model, heads, False),
            head_weight=lambda heads: heads[0].predictor.weight, prepare=_same_draw, observe=_masked_types,
            begin_loop=lambda: np.random.seed(5))


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_bucket_replay_matches_eager_on_ragged_batches(kind):
    model = backbone(kind)
    heads = CASE.heads(kind, model)
    batches = ragged_batches(4, 24, 17)
    if kind == "painn":
        with_radius_edges(batches)
    assert_one_bucket(replay_vs_eager(CASE, kind, model, heads, batches))


@pytest.mark.parametrize("kind,mask_ratio", [("schnet", 0.0), ("painn", 0.0), ("schnet", 0.2)])
def test_bucket_replay_matches_eager_on_device_loader(kind, mask_ratio):
    """DeviceLoader handles (with BFS atom masking: mask_ratio > 0) replay one one-view bucket graph per batch size."""
    from geossl_amd.synthetic import add_bonds, make_molecules
    mols = make_molecules(200, seed=3, mode="C")
    if mask_ratio:
        mols = add_bonds(mols, seed=3, cut=0.3)
    model = backbone(kind)
    handles = loader_handles(kind, dataset_kw={"mols": mols}, loader_kw={"mask_ratio": mask_ratio, "mask_rng": "device"})
    assert_one_bucket(replay_vs_eager(CASE, kind, model, CASE.heads(kind, model), handles))


def test_reference_loop_and_trainer_match_stock_adam():
    """Six steps of the reference loop (do_ChargePrediction, numpy masks, a stock torch.optim.Adam, graph replay) and of
    ChargePredictionTrainer (numpy masks, one bucket graph) against the same loop on eager launches."""
    reference_loop_vs_trainer(CASE, 6, 16, 5, per_step=False)


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_trainer_device_masks_over_a_loader_epoch(kind):
    """mask_rng "device": a shuffled DeviceLoader epoch replays ONE bucket graph; the graph's seed advances by one per
    step on the device; two trainers with one seed give the same losses."""
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    from geossl_amd.pretrain_ChargePrediction import ChargePredictionTrainer, ChargePredictor
    from geossl_amd.synthetic import make_molecules
    ds = DeviceDataset.from_numpy(make_molecules(256, seed=8, mode="C"), DEV, option="permutation",
                                  **({"radius": 5.0} if kind == "painn" else {}))
    runs = []
    for _ in range(2):
        tr = ChargePredictionTrainer(backbone(kind), fill_module_(ChargePredictor(128)).to(DEV), lr=1e-4,
                                     model_3d=kind, use_graph=True, seed=99)
        loader = DeviceLoader(ds, batch_size=32, shuffle=True, drop_last=True,
                              generator=torch.Generator().manual_seed(4))
        runs.append(torch.stack([tr.step(hb) for hb in loader]).cpu())
        assert len(tr.step_graphs) == 1 and tr.step_graphs.captures <= 2
        (g,) = tr.step_graphs.graphs.values()
        assert g["noise"]["mask_seed"].numel() == 1
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1])


def test_allocator_poison_independence():
    """A step on an allocator filled with NaN / 1e30 gives the unpoisoned loss and gradients bit for bit."""
    from geossl_amd.pretrain_ChargePrediction import ChargePredictor, do_ChargePrediction
    _, meta, _, _, make, args = _g19_setup("g19_charge_schnet_full_r03")

    def poison(value):
        junk = [torch.full((n,), value, device=DEV) for n in (1 << 9, 1 << 12, 1 << 15, 1 << 18, 1 << 20, 1 << 22)
                for _ in range(8)]
        torch.cuda.synchronize()
        del junk

    def step(value):
        gc.collect()
        model, cp = backbone("schnet"), fill_module_(ChargePredictor(128)).to(DEV)
        if value is not None:
            poison(value)
        np.random.seed(meta["seed"])
        loss = do_ChargePrediction(args, make(), model, cp, graph=False)
        loss.backward()
        return loss.item(), {n: p.grad.clone() for n, p in list(model.named_parameters()) + list(cp.named_parameters())
                             if p.grad is not None}

    ref_loss, ref = step(None)
    assert np.isfinite(ref_loss)
    for value in (float("nan"), 1e30):
        loss, grads = step(value)
        assert loss == ref_loss, value
        for n in ref:
            assert torch.equal(grads[n], ref[n]), (value, n)
