"""GPU tests of GeoSSL-RR (--GeoSSL_option RR): the fused AutoEncoder heads of csrc/rr_head.hip against the fp64 twin
(tests/rr_twin.py) with torch's own fp32 head as the yardstick of the error, the BatchNorm buffers, determinism, the
whole step against fixture G27 (the reference's do_RR run verbatim on this project's AutoEncoder), the graph paths
against the eager step, the reference's own training loop, the launch count, independence from the allocator's free
memory, and a scaled upstream gradient."""
import copy
import gc
import json
import os
import types

import numpy as np
import pytest
import torch

import rr_twin as tw
from conftest import load_golden, rel_err
from helpers import fill_module_, grad_summary, t, unique_named_grads
from objective_harness import assert_only_library_kernels, backbone, gpu_kernels, library_kernel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G27 = sorted(f[:-4] for f in os.listdir(os.path.join(REPO, "tests", "golden")) if f.startswith("g27_rr_"))
F = 128
NAMES = ["W1", "b1", "gamma", "beta", "W2", "b2"]


def _heads(kind, detach, device=DEV):
    """Two default-initialised heads with gamma ~ U(0.5, 1.5), beta ~ U(-0.5, 0.5) (the affine part is not the identity),
    drawn from torch's CPU generator where it stands."""
    from geossl_amd.Geom3D.models import AutoEncoder
    heads = [AutoEncoder(F, kind, detach) for _ in range(2)]
    with torch.no_grad():
        for h in heads:
            h.fc_layers[1].weight.uniform_(0.5, 1.5)
            h.fc_layers[1].bias.uniform_(-0.5, 0.5)
    return [h.to(device) for h in heads]


def _buffers(h):
    bn = h.fc_layers[1]
    return [bn.running_mean, bn.running_var, bn.num_batches_tracked]


def _outputs(loss, X, Y, heads):
    """loss, dX, dY and the 12 parameter gradients, named, as fp64 CPU tensors."""
    params = [p for h in heads for p in h.parameters()]
    grads = torch.autograd.grad(loss, [X, Y] + params)
    names = ["dX", "dY"] + ["head%d.%s" % (k, n) for k in (1, 2) for n in NAMES]
    out = {"loss": loss.detach().double().cpu()}
    out.update({n: g.double().cpu() for n, g in zip(names, grads)})
    return out


# ---------------------------------------------------------------------------------------------- kernels vs the twin
@pytest.mark.parametrize("detach", [True, False])
@pytest.mark.parametrize("kind", ["l1", "l2", "cosine"])
@pytest.mark.parametrize("B", [2, 3, 65, 257])
def test_kernel_vs_twin(B, kind, detach):
    """Every output within max(1e-5 of its largest magnitude, 4 x the error torch's own fp32 head makes against the same
    twin).  Elements whose twin z (for l1 also p - y) lies within 1e-4 of zero are near a kink: for exactly those the
    twin takes ReLU' / sign from the kernel's saved values; their share must stay below 0.05 % of B F per head."""
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    torch.manual_seed(1000 + B)
    X0, Y0 = torch.randn(B, F), torch.randn(B, F)
    heads = _heads(kind, detach)
    ref_heads = copy.deepcopy(heads)
    X, Y = X0.to(DEV).requires_grad_(), Y0.to(DEV).requires_grad_()
    calls = ops.RR_STATS["fwd"]
    loss = pg.rr_heads_loss(heads[0], heads[1], X, Y)
    assert ops.RR_STATS["fwd"] == calls + 1 and loss.dtype == torch.float32 and loss.dim() == 0
    saved = loss.grad_fn.saved_tensors
    act, p = saved[4].double().cpu(), saved[5].double().cpu()
    got = _outputs(loss, X, Y, heads)
    # torch's own fp32 head on the device, same inputs
    Xr, Yr = X0.to(DEV).requires_grad_(), Y0.to(DEV).requires_grad_()
    ref = _outputs(pg.rr_heads_aten(ref_heads[0], ref_heads[1], Xr, Yr), Xr, Yr, ref_heads)
    # the twin, first as it stands (to find the elements near a kink), then with the kernel's decisions at exactly those
    P1, P2 = list(heads[0].parameters()), list(heads[1].parameters())
    plain = tw.step(X0, Y0, P1, P2, kind, detach)
    masks, signs, near = [], [], []
    for k, (h, target) in enumerate(zip(plain["heads"], (Y0, X0))):
        nz = h["z"].abs() < tw.KINK
        m = torch.full_like(h["z"], float("nan"))
        m[nz] = (act[k][nz] > 0).double()
        masks.append(m)
        n_near = [int(nz.sum())]
        s = None
        if kind == "l1":
            nd = h["diff"].abs() < tw.KINK
            s = torch.full_like(h["diff"], float("nan"))
            s[nd] = torch.sign(p[k].float() - target)[nd].double()
            n_near.append(int(nd.sum()))
        signs.append(s)
        near.append(n_near)
        assert max(n_near) <= 0.0005 * B * F, "ill-posed: %s elements near a kink" % (near,)
    twin = tw.step(X0, Y0, P1, P2, kind, detach, masks=masks, signs=signs)
    want = {"loss": twin["loss"], "dX": twin["dX"], "dY": twin["dY"]}
    want.update({"head%d.%s" % (k, n): g for (k, n), g in zip([(k, n) for k in (1, 2) for n in NAMES], twin["grads"])})
    ratios, bad = {}, []
    for name, w in want.items():
        e_k = float((got[name] - w).abs().max())
        e_t = float((ref[name] - w).abs().max())
        scale = float(w.abs().max())
        ratios[name] = (e_k / scale if scale > 0 else 0.0, e_k / e_t if e_t > 0 else float("inf") if e_k > 0 else 0.0)
        if e_k > max(1e-5 * scale, 4.0 * e_t):
            bad.append((name, e_k, e_t, scale))
    print("B=%d %s detach=%s near-kink %s; per output (error / max|twin|, error / torch's error): %s"
          % (B, kind, detach, near, {n: "%.1e, %.2f" % r for n, r in ratios.items()}))
    assert not bad, bad


def test_fused_heads_refuse_and_fall_back():
    """B = 1 in training mode never reaches the kernels (torch's own ValueError); eval mode and a subclass run ATen."""
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    torch.manual_seed(5)
    a, b = _heads("l2", True)
    calls = dict(ops.RR_STATS)
    x = torch.randn(1, F, device=DEV)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        pg.rr_heads_loss(a, b, x, x.clone())
    X, Y = torch.randn(4, F, device=DEV), torch.randn(4, F, device=DEV)
    a.eval()
    assert torch.isfinite(pg.rr_heads_loss(a, b, X, Y))
    a.train()
    assert ops.RR_STATS == calls
    assert torch.isfinite(pg.rr_heads_loss(a, b, X, Y)) and ops.RR_STATS["fwd"] == calls["fwd"] + 1


# ---------------------------------------------------------------------------------------------- BatchNorm buffers
@pytest.mark.parametrize("replayed", [False, True])
def test_batchnorm_buffers_after_three_steps(replayed):
    """running_mean / running_var (1e-5 of the largest magnitude: fp32 statistics against fp64) and num_batches_tracked
    (exactly) after three steps equal the twin's, with eager launches and with one captured step replayed three times
    (the warm-up passes before the capture leave the buffers alone)."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.replay import warm_up
    B = 65
    torch.manual_seed(77)
    heads = _heads("l2", True)
    bufs = [[b.double().cpu() if b.is_floating_point() else int(b) for b in _buffers(h)] for h in heads]
    xs = [(torch.randn(B, F) + 0.1 * k, 0.5 * torch.randn(B, F) - 0.2 * k) for k in range(3)]
    X, Y = torch.empty(B, F, device=DEV), torch.empty(B, F, device=DEV)
    if replayed:
        X.copy_(xs[0][0]), Y.copy_(xs[0][1])
        warm_up(lambda: pg.rr_heads_loss(heads[0], heads[1], X, Y))
        assert [int(h.fc_layers[1].num_batches_tracked) for h in heads] == [0, 0]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            loss = pg.rr_heads_loss(heads[0], heads[1], X, Y)
        assert [int(h.fc_layers[1].num_batches_tracked) for h in heads] == [0, 0]
    for x, y in xs:
        X.copy_(x), Y.copy_(y)
        if replayed:
            g.replay()
        else:
            loss = pg.rr_heads_loss(heads[0], heads[1], X, Y)
        plain = tw.step(x, y, list(heads[0].parameters()), list(heads[1].parameters()), "l2", True)
        bufs = [tw.buffers_after(b, h["mean"], h["var"], B) for b, h in zip(bufs, plain["heads"])]
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    for h, (rm, rv, nb) in zip(heads, bufs):
        bn = h.fc_layers[1]
        assert int(bn.num_batches_tracked) == nb == 3
        for got, want in ((bn.running_mean, rm), (bn.running_var, rv)):
            assert float((got.double().cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())


# ---------------------------------------------------------------------------------------------- determinism
def test_heads_are_deterministic_eager_and_replayed():
    from geossl_amd import pretrain_GeoSSL as pg
    torch.manual_seed(9)
    B = 257
    X, Y = torch.randn(B, F, device=DEV), torch.randn(B, F, device=DEV)
    all_heads = {(kind, d): _heads(kind, d) for kind in ("l1", "l2", "cosine") for d in (True, False)}

    def both():
        out = []
        for heads in all_heads.values():
            a, b = X.clone().requires_grad_(), Y.clone().requires_grad_()
            loss = pg.rr_heads_loss(heads[0], heads[1], a, b)
            grads = torch.autograd.grad(loss, [a, b] + [p for h in heads for p in h.parameters()])
            out += [loss.detach().clone()] + [g_.clone() for g_ in grads]
        return out
    one, two = both(), both()
    assert all(torch.equal(p, q) for p, q in zip(one, two))
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


# ---------------------------------------------------------------------------------------------- G27 end to end
def _g27_setup(case):
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    from test_rr_cpu import heads_of
    g = load_golden(case)
    meta, cfg = json.loads(str(g["meta"])), json.loads(str(g["cfg"]))
    model = fill_module_(SchNet(**cfg) if meta["kind"] == "schnet" else PaiNN(**cfg)).to(DEV)
    rei = t(g["radius_edge_index"], DEV) if "radius_edge_index" in g else None
    batch = pg.Batch(t(g["x"], DEV), t(g["positions"], DEV), t(g["batch"], DEV), t(g["super_edge_index"], DEV),
                     radius_edge_index=rei, num_graphs=len(g["sizes"]))
    args = types.SimpleNamespace(model_3d=meta["kind"], normalize=meta["normalize"])
    return g, meta, model, heads_of(g, meta, device=DEV), batch, args, {"pos_noise": t(g["pos_noise"], DEV)}


@pytest.mark.parametrize("case", G27)
def test_g27_end_to_end(case):
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    g, meta, model, heads, batch, args, noise = _g27_setup(case)
    calls = dict(ops.RR_STATS)
    loss, acc = pg.do_RR(args, batch, model, 0.0, 0.3, AE_models=heads, noise=noise, graph=False, criterion=None)
    assert acc == 0 and loss.dtype == torch.float32
    assert rel_err(loss.detach().cpu(), g["loss"]) < 1e-4 or abs(loss.item() - float(g["loss"])) < 1e-6
    loss.backward()
    # the F = 128 cases took the kernels (forward and backward), the reduced widths the ATen head on the HIP backbone
    took = int(g["X"].shape[1] == 128)
    assert ops.RR_STATS == {"fwd": calls["fwd"] + took, "bwd": calls["bwd"] + took}
    grads = unique_named_grads(model)
    # With detach_target and no --normalize the gradient of SchNet's last bias is exactly zero in exact arithmetic: lin2.bias
    # adds one vector to every readout row, its gradient is sum_b dX_b + sum_b dY_b, each dX_b = dZ_b W1 with sum_b dZ_b = 0
    # behind a BatchNorm (and no target gradient).  The fixture holds the rounding noise of that sum, so a relative
    # comparison would compare two roundings: absolute, at 1e-4 of the summands' size (column sums of |grad_X| + |grad_Y|).
    zero_sum = meta["kind"] == "schnet" and meta["detach_target"] and not meta["normalize"]
    summands = float((np.abs(g["grad_X"]).sum(0) + np.abs(g["grad_Y"]).sum(0)).max())
    for k in g:
        if k.startswith("grad/") or k.startswith("gsum/"):
            name = k.split("/", 1)[1]
            got = grads[name].cpu()
            if zero_sum and name == "lin2.bias":
                assert float(got.abs().max()) <= 1e-4 * summands, (case, k)
                continue
            got = grad_summary(got) if k.startswith("gsum/") else got
            assert rel_err(got, g[k]) < 1e-4 or float(np.abs(g[k]).max()) < 1e-8, (case, k)
    for k, h in ((1, heads[0]), (2, heads[1])):
        for name, p in h.named_parameters():
            want = g["head%d/grad/%s" % (k, name)]
            if name == "fc_layers.0.bias":
                # exactly zero in exact arithmetic (BatchNorm subtracts the column mean): the fixture holds rounding noise
                # of sum_b dZ_b, so a relative comparison would compare two roundings.  Absolute, at 1e-4 of the scale of
                # dZ taken from the same layer's weight gradient over the largest input.
                scale = float(np.abs(g["head%d/grad/fc_layers.0.weight" % k]).max()) / float(
                    max(np.abs(g["X"]).max(), np.abs(g["Y"]).max()))
                assert float(p.grad.abs().max()) <= 1e-4 * scale, (case, k, name)
                continue
            assert rel_err(p.grad.cpu(), want) < 1e-4 or float(np.abs(want).max()) < 1e-8, (case, k, name)
        bn = h.fc_layers[1]
        assert rel_err(bn.running_mean.cpu(), g["head%d/running_mean" % k]) < 1e-4
        assert rel_err(bn.running_var.cpu(), g["head%d/running_var" % k]) < 1e-4
        assert int(bn.num_batches_tracked) == int(g["head%d/num_batches_tracked" % k])


# ---------------------------------------------------------------------------------------------- graph paths
def _batch(kind, B, seed):
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import make_batch
    bt = pg.Batch.from_numpy(make_batch(B, seed=seed, mode="B"), DEV)
    if kind == "painn":
        bt.radius_edge_index = ops.radius_graph(bt.positions, 5.0, bt.batch)
    return bt


def _pos_noise(shape, seed):
    return {"pos_noise": torch.randn(shape, generator=torch.Generator().manual_seed(seed)).mul_(0.3).to(DEV)}


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_per_structure_graph_replay_equals_the_eager_step(kind):
    from geossl_amd import pretrain_GeoSSL as pg
    bt = _batch(kind, 24, 3)
    args = types.SimpleNamespace(model_3d=kind, normalize=kind == "painn", step_graph_mode="structure")
    torch.manual_seed(21)
    heads0 = _heads("l1" if kind == "schnet" else "cosine", kind == "painn", "cpu")
    out = {}
    for graph in (False, True):
        model = backbone(kind)
        heads = [copy.deepcopy(h).to(DEV) for h in heads0]
        params = [p for p in model.parameters() if p.requires_grad] + [p for h in heads for p in h.parameters()]
        runs = []
        for step in range(3):   # (graph: captured at the first step, replayed at the next two)
            loss, acc = pg.do_RR(args, bt, model, 0.0, 0.3, AE_models=heads, noise=_pos_noise(bt.positions.shape, 50 + step),
                                 graph=graph)
            grads = torch.autograd.grad(loss, params, allow_unused=True)
            runs.append((loss.item(), [None if g_ is None else g_.clone() for g_ in grads]))
        if graph:
            eng = model.__dict__["_geossl_rr_step"]
            assert sum(sg.captures for sg in eng.graphs.values()) == 1
        out[graph] = (runs, [[b.clone() for b in _buffers(h)] for h in heads])
    for (le, ge), (lg, gg) in zip(out[False][0], out[True][0]):
        assert abs(le - lg) <= 1e-6 * abs(le)
        for a, b in zip(ge, gg):
            assert (a is None) == (b is None)
            if a is not None:
                assert rel_err(b.cpu(), a.cpu()) < 1e-6
    for be, bg in zip(out[False][1], out[True][1]):   # three steps moved the buffers three times on either path
        assert int(be[2]) == int(bg[2]) == 3
        assert rel_err(bg[0].cpu(), be[0].cpu()) < 1e-6 and rel_err(bg[1].cpu(), be[1].cpu()) < 1e-6


def _device_dataset(kind, n=64):
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    from geossl_amd.synthetic import add_bonds, make_molecules
    sizes = np.random.default_rng(7).permutation(np.arange(n) % 32 + 2)   # every size of 2 .. 33 as often as the others
    mols = add_bonds(make_molecules(n, seed=7, sizes=sizes), seed=7)
    return DeviceDataset.from_numpy(mols, DEV, **({"radius": 5.0} if kind == "painn" else {}))


@pytest.mark.parametrize("ratio", [0.0, 0.3])
def test_trainer_bucket_replay_over_two_shuffled_epochs_equals_eager(ratio):
    """RRTrainer fed by a shuffled DeviceLoader (64 molecules of 2 .. 33 atoms, batch size 16, masked or not) for two
    epochs: one capacity-bucket graph per batch size, no capture in the second epoch, the handles never collated, and the
    final parameters and BatchNorm buffers those of the eager trainer on the same draws.  (detach_target off: with it on,
    the gradient of the backbone's last bias is the rounding noise of a sum that is zero in exact arithmetic, Adam turns
    noise into steps of the size of lr, and the targets - hence the loss - follow them: two correct runs then part ways.)"""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    ds = _device_dataset("schnet")
    torch.manual_seed(31)
    heads0 = _heads("l2", False, "cpu")
    res = {}
    for use_graph in (False, True):
        model = backbone("schnet")
        heads = [copy.deepcopy(h).to(DEV) for h in heads0]
        tr = pg.RRTrainer(model, heads[0], heads[1], lr=5e-4, model_3d="schnet", use_graph=use_graph, ae_lr=1e-3)
        np.random.seed(3)
        loader = DeviceLoader(ds, batch_size=16, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(5),
                              mask_ratio=ratio)
        losses, k, captures = [], 0, []
        for epoch in range(2):
            for hb in loader:
                losses.append(tr.step(hb, _pos_noise((hb.n_atoms, 3), 100 + k)).item())
                assert hb._batch is None or not use_graph   # gathered into the bucket: no host collation
                k += 1
            captures.append(tr.step_graphs.captures)
        if use_graph:
            assert [key[:2] for key in tr.step_graphs.graphs] == [("bucket", 16)]
            assert captures[0] >= 1 and captures[1] == captures[0] and captures[0] <= 2
        res[use_graph] = (losses, tr.flat.flat.clone(), [[b.clone() for b in _buffers(h)] for h in heads])
    (le, pe, be), (lg, pg_, bg) = res[False], res[True]
    print("losses eager %s\nlosses graph %s\nrelative %s" % (le, lg, ["%.1e" % (abs(a - b) / abs(a)) for a, b in zip(le, lg)]))
    assert len(le) == 8 and all(np.isfinite(le)) and all(np.isfinite(lg))
    # the first step starts from the same parameters: its two losses differ by the summation order of the two routes;
    # from then on the parameters themselves differ within the bound below, and with them the losses
    assert abs(le[0] - lg[0]) <= 1e-5 * abs(le[0])
    assert rel_err(pg_.cpu(), pe.cpu()) < 1e-5
    for x, y in zip(be, bg):
        assert int(x[2]) == int(y[2]) == 8
        assert rel_err(y[0].cpu(), x[0].cpu()) < 1e-5 and rel_err(y[1].cpu(), x[1].cpu()) < 1e-5


def test_painn_trainer_replays_a_bucket():
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    ds = _device_dataset("painn")
    torch.manual_seed(32)
    heads = _heads("cosine", False)
    tr = pg.RRTrainer(backbone("painn"), heads[0], heads[1], lr=5e-4, model_3d="painn", normalize=True, use_graph=True)
    np.random.seed(3)
    loader = DeviceLoader(ds, batch_size=16, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(5))
    losses = [tr.step(hb).item() for hb in loader]
    assert all(np.isfinite(losses)) and [key[:2] for key in tr.step_graphs.graphs] == [("bucket", 16)]
    assert int(heads[0].fc_layers[1].num_batches_tracked) == 4


def test_sampled_tuple_handles_replay_a_bucket_and_match_plain_handles():
    """Handles of a DeviceLoader(tuple_ratio < 1): the tuple draw is made and never read by this step, so the replayed
    losses are those of the same molecules without sampling."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    ds = _device_dataset("schnet")
    torch.manual_seed(33)
    heads0 = _heads("l1", False, "cpu")
    out = {}
    for ratio in (1.0, 0.3):
        heads = [copy.deepcopy(h).to(DEV) for h in heads0]
        tr = pg.RRTrainer(backbone("schnet"), heads[0], heads[1], lr=5e-4, model_3d="schnet", use_graph=True)
        np.random.seed(3)
        loader = DeviceLoader(ds, batch_size=16, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(5),
                              tuple_ratio=ratio)
        out[ratio] = [tr.step(hb, _pos_noise((hb.n_atoms, 3), 200 + k)).item() for k, hb in enumerate(loader)]
        assert len(tr.step_graphs.graphs) == 1 and next(iter(tr.step_graphs.graphs))[0] == "bucket"
    assert len(out[1.0]) == 4 and all(np.isfinite(out[0.3]))
    assert abs(out[0.3][0] - out[1.0][0]) <= 1e-5 * abs(out[1.0][0])   # (same parameters at the first step)


# ---------------------------------------------------------------------------------------------- the reference loop
def test_reference_loop_graph_equals_eager():
    """do_RR, optimizer.zero_grad(), loss.backward(), stock Adam over the reference's three parameter groups
    (pretrain_GeoSSL.py:234-260, :332-343; the AE groups at their own lr) for two short epochs: the graph path ends where
    the eager path ends.  (detach_target off, for the reason given at the trainer test.)"""
    from geossl_amd import pretrain_GeoSSL as pg
    batches = [_batch("schnet", 24, 60 + i) for i in range(3)]
    torch.manual_seed(11)
    heads0 = _heads("l2", False, "cpu")
    final = {}
    for graph in (False, True):
        model = backbone("schnet")
        pg.AE_model_01, pg.AE_model_02 = [copy.deepcopy(h).to(DEV) for h in heads0]
        try:
            group = [{"params": model.parameters(), "lr": 5e-4}, {"params": pg.AE_model_01.parameters(), "lr": 1e-3},
                     {"params": pg.AE_model_02.parameters(), "lr": 1e-3}]
            opt = torch.optim.Adam(group, lr=5e-4, weight_decay=0)
            args = types.SimpleNamespace(model_3d="schnet", normalize=False, step_graph=graph)
            for epoch in range(2):
                for k, bt in enumerate(batches):
                    loss, acc = pg.do_RR(args, bt, model, criterion=None, mu=0.0, sigma=0.3,
                                         noise=_pos_noise(bt.positions.shape, 10 * epoch + k))
                    assert acc == 0
                    opt.zero_grad()
                    loss.backward()
                    opt.step()
            mods = (model, pg.AE_model_01, pg.AE_model_02)
            final[graph] = torch.cat([p.detach().reshape(-1) for m in mods for p in m.parameters()]).cpu()
        finally:
            pg.AE_model_01 = pg.AE_model_02 = None
    assert torch.isfinite(final[True]).all()
    assert rel_err(final[True], final[False]) < 1e-5


def test_trainer_with_ae_lr_matches_stock_adam_over_the_three_groups():
    """RRTrainer(ae_lr=) - one fused Adam launch over the backbone's range of the flat buffer, one over the heads' - ends
    where do_RR + loss.backward() + torch.optim.Adam over the reference's three groups ends (eager launches both)."""
    from geossl_amd import pretrain_GeoSSL as pg
    batches = [_batch("schnet", 16, 80 + i) for i in range(3)]
    torch.manual_seed(12)
    heads0 = _heads("cosine", False, "cpu")
    final = {}
    for fused in (False, True):
        model = backbone("schnet")
        heads = [copy.deepcopy(h).to(DEV) for h in heads0]
        if fused:
            tr = pg.RRTrainer(model, heads[0], heads[1], lr=5e-4, model_3d="schnet", use_graph=False, ae_lr=2e-3)
        else:
            opt = torch.optim.Adam([{"params": model.parameters(), "lr": 5e-4}, {"params": heads[0].parameters(), "lr": 2e-3},
                                    {"params": heads[1].parameters(), "lr": 2e-3}], lr=5e-4, weight_decay=0)
        args = types.SimpleNamespace(model_3d="schnet", normalize=False)
        for k, bt in enumerate(batches):
            noise = _pos_noise(bt.positions.shape, 300 + k)
            if fused:
                tr.step(bt, noise)
            else:
                loss, _ = pg.do_RR(args, bt, model, 0.0, 0.3, AE_models=heads, noise=noise, graph=False)
                opt.zero_grad()
                loss.backward()
                opt.step()
        final[fused] = [torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu() for m in [model] + heads]
    for a, b in zip(final[True], final[False]):   # backbone, head 1, head 2: each at its own learning rate
        assert rel_err(a, b) < 1e-5
    moved = float((final[True][1] - torch.cat([p.detach().reshape(-1) for p in heads0[0].parameters()])).abs().max())
    assert moved > 2e-3   # (Adam's first step alone is lr sign(g): 2e-3 at the heads' own lr, 5e-4 at the backbone's)


# ---------------------------------------------------------------------------------------------- launches
HEAD_LAUNCHES = 11   # 5 forward + 6 backward (csrc/rr_head.hip), whatever B is


def test_head_launch_count_does_not_depend_on_B():
    """Forward + backward of both heads are 11 launches of the library's kernels at every B, with no floating-point ATen
    operator between them (as a replayed step captures them: gradients added into dense .grad buffers)."""
    from geossl_amd import pretrain_GeoSSL as pg
    torch.manual_seed(41)
    heads = _heads("l1", False)
    for p in [q for h in heads for q in h.parameters()]:
        p.grad = torch.zeros_like(p)
    one = torch.ones((), device=DEV)
    more = {"aten::select", "aten::view_as", "aten::is_nonzero", "aten::item", "aten::_local_scalar_dense",
            "aten::new_empty", "aten::set_"}
    counts = {}
    for B in (2, 3, 65, 257, 4096):
        h = torch.randn(2 * B, F, device=DEV).requires_grad_()   # the 2B readout rows, split as the step splits them

        def heads_fwd_bwd():
            X, Y = pg.split_views(h, B)
            pg.rr_heads_loss(heads[0], heads[1], X, Y).backward(one)
        counts[B] = len(assert_only_library_kernels(heads_fwd_bwd, also_allowed=more))
        assert h.grad.shape == (2 * B, F) and torch.isfinite(h.grad).all()
    assert set(counts.values()) == {HEAD_LAUNCHES}, counts


def test_replayed_step_has_no_aten_kernel_the_contrastive_step_lacks(monkeypatch):
    """A replayed RRTrainer step makes the C-ABI calls of a replayed contrastive step (gather, Adam; the head is inside
    the graph) and launches no kernel from outside the library that the replayed InfoNCE step does not launch."""
    from torch.profiler import ProfilerActivity, profile
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    from test_gpu_step_engine_launches import _Recorder
    ds = _device_dataset("schnet")
    torch.manual_seed(43)
    heads = _heads("l2", True)
    trainers = {"RR": pg.RRTrainer(backbone("schnet"), heads[0], heads[1], use_graph=True),
                "InfoNCE": pg.ContrastiveTrainer(backbone("schnet"), option="InfoNCE", use_graph=True)}
    foreign, calls = {}, {}
    rec = _Recorder(monkeypatch.setattr)   # (one for both trainers: it wraps `call` where it finds the real one)
    for name, tr in trainers.items():
        np.random.seed(3)
        hbs = list(DeviceLoader(ds, batch_size=16, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(5)))
        for hb in hbs:   # the capture, and whatever growth of the bucket these four batches ask for
            tr.step(hb)
        captures = tr.step_graphs.captures
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            tr.step(hbs[2])
            torch.cuda.synchronize()
        foreign[name] = {n for n in gpu_kernels(prof) if not library_kernel(n)}
        rec.step(lambda: tr.step(hbs[3]))
        calls[name] = rec.steps[-1]
        assert tr.step_graphs.captures == captures <= 2 and len(tr.step_graphs.graphs) == 1
    assert foreign["RR"] <= foreign["InfoNCE"], foreign["RR"] - foreign["InfoNCE"]
    assert calls["RR"] == calls["InfoNCE"] == ["gather_molecules", "adam_step"], calls


# ---------------------------------------------------------------------------------------------- memory, scaling
def test_step_reads_no_memory_it_has_not_written():
    from geossl_amd import pretrain_GeoSSL as pg
    bt = _batch("schnet", 65, 91)
    noise = _pos_noise(bt.positions.shape, 92)
    args = types.SimpleNamespace(model_3d="schnet", normalize=True)
    torch.manual_seed(93)
    heads0 = _heads("l1", False, "cpu")

    def poison(value):
        junk = [torch.full((n,), value, device=DEV) for n in (1 << 9, 1 << 12, 1 << 15, 1 << 18, 1 << 20, 1 << 22)
                for _ in range(8)]
        torch.cuda.synchronize()
        del junk

    def step(value):
        gc.collect()
        model = backbone("schnet")
        heads = [copy.deepcopy(h).to(DEV) for h in heads0]
        if value is not None:
            poison(value)
        loss, _ = pg.do_RR(args, bt, model, 0.0, 0.3, AE_models=heads, noise=noise, graph=False)
        loss.backward()
        grads = {n: p.grad.clone() for m in [model] + heads for n, p in m.named_parameters() if p.grad is not None}
        return loss.item(), list(grads.values()), [b.clone() for h in heads for b in _buffers(h)]

    ref_loss, ref, ref_buf = step(None)
    assert np.isfinite(ref_loss) and all(bool(torch.isfinite(g_).all()) for g_ in ref)
    for value in (float("nan"), 1e30):
        loss, grads, bufs = step(value)
        assert loss == ref_loss, value
        assert all(torch.equal(a, b) for a, b in zip(grads, ref)), value
        assert all(torch.equal(a, b) for a, b in zip(bufs, ref_buf)), value


@pytest.mark.parametrize("graph", [False, True])
def test_scaled_loss_scales_the_gradients(graph):
    from geossl_amd import pretrain_GeoSSL as pg
    bt = _batch("schnet", 32, 5)
    noise = _pos_noise(bt.positions.shape, 6)
    args = types.SimpleNamespace(model_3d="schnet", normalize=False, step_graph_mode="structure")
    torch.manual_seed(7)
    heads = _heads("cosine", False)
    model = backbone("schnet")
    params = [p for p in model.parameters() if p.requires_grad] + [p for h in heads for p in h.parameters()]
    loss, _ = pg.do_RR(args, bt, model, 0.0, 0.3, AE_models=heads, noise=noise, graph=graph)
    g1 = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
    g2 = torch.autograd.grad(2 * loss, params, allow_unused=True)
    assert sum(g_ is not None for g_ in g1) >= 12
    for a, b in zip(g1, g2):
        if a is not None:
            assert torch.equal(b, 2 * a)
