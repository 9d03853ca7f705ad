"""MD17 fine-tuning on the GPU (geossl_amd/finetune_md17.py, csrc/force_head.hip) against the fp64 twin of
tests/force_twin.py with its BOUNDS: PaiNN's step on the interned complete pair list against the twin on the frame's own
radius list (eager, replayed, and the route before under GEOSSL_MD17_COMPLETE_EDGES=0), SchNet's step from a DeviceLoader
handle bit for bit against ForceTrainer on the collated tensors, predict_MD17 / eval_MD17 / MD17Trainer.evaluate, and the
three kernels of force_head.hip element by element against numpy in fp64."""
import numpy as np
import pytest
import torch

import force_twin as tw
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 5e-4
SCHNET_MD17 = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0,
                   readout="mean", node_class=9)
PAINN_MD17 = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")
N_ATOMS = 21
HEAD_TOL = 2e-5   # test_gpu_supervised.py::test_head_kernels_vs_fp64: the same arithmetic against fp64


# ------------------------------------------------------------------------------------------------------------ plumbing
def _far_molecule(n, cutoff):
    return (np.arange(n, dtype=np.float32)[:, None] * np.float32(1.5 * cutoff) * np.array([[1, 0.3, 0.1]], np.float32))


def _raw(sizes, seed, cutoff, far=None):
    """make_batch over `sizes`: the first seed from `seed` on whose pairs all keep the twin's cutoff margin; molecule
    `far` gets positions without any pair inside the cutoff."""
    from geossl_amd.synthetic import make_batch
    for s in range(seed, seed + 50):
        r = make_batch(0, seed=s, sizes=sizes)
        if far is not None:
            off = int(np.sum(r["sizes"][:far]))
            r["positions"][off:off + sizes[far]] = _far_molecule(sizes[far], cutoff)
        if tw.cutoff_margin(r["positions"], r["batch"], cutoff) >= tw.CUTOFF_MARGIN:
            return r
    raise AssertionError("no seed with a cutoff margin")


def _moved(raw, k, cutoff):
    """raw with positions moved by up to ~0.05 A (frame k of a trajectory), the cutoff margin kept."""
    g = np.random.default_rng(1000 + k)
    for _ in range(50):
        p = (raw["positions"] + 0.03 * g.standard_normal(raw["positions"].shape)).astype(np.float32)
        if tw.cutoff_margin(p, raw["batch"], cutoff) >= tw.CUTOFF_MARGIN:
            return dict(raw, positions=p)
    raise AssertionError("no move with a cutoff margin")


def _cfg(kind, readout=None):
    cfg = dict(SCHNET_MD17 if kind == "schnet" else PAINN_MD17)
    if readout is not None:
        cfg["readout"] = readout
    return cfg


def _modules(kind, cfg, head="default"):
    """Backbone and head with torch's own initialisation under a fixed seed (test_gpu_force_training.py: closed-form
    weights make the forces cancel)."""
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    from geossl_amd.Geom3D.models.painn import Dense
    torch.manual_seed(1234)
    model = (SchNet(**cfg) if kind == "schnet" else PaiNN(**cfg)).to(DEV)
    F = cfg["hidden_channels"] if kind == "schnet" else cfg["n_atom_basis"]
    if head == "default":
        head = "linear" if kind == "schnet" else "painn"
    hd = {"linear": lambda: torch.nn.Linear(F, 1), "dense": lambda: Dense(F, 1),
          "painn": lambda: model.create_output_layers()}[head]().to(DEV)
    return model, hd


def _twin_cfg(kind, cfg):
    if kind == "schnet":
        return dict(num_interactions=cfg["num_interactions"], cutoff=cfg["cutoff"], readout=cfg["readout"])
    return dict(n_atom_basis=cfg["n_atom_basis"], n_interactions=cfg["n_interactions"], cutoff=cfg["cutoff"],
                readout=cfg["readout"])


def _batch(kind, cfg, raw, y=None, force=None):
    """The collated batch of the reference's MD17 loaders: 1-D x, host sizes, PaiNN with the frame's own radius list."""
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    bt = pg.Batch.from_numpy(dict(raw, x=raw["x"][:, 0].copy()), DEV)
    if kind == "painn":
        bt.radius_edge_index = ops.radius_graph(bt.positions, cfg["cutoff"], bt.batch)
    if y is not None:
        bt.y, bt.force = y.to(DEV), force.to(DEV)
    return bt


def _edges(kind, cfg, raw, bt):
    if kind == "schnet":
        return tw.schnet_edges(raw["positions"], raw["batch"], cfg["cutoff"])
    return bt.radius_edge_index.detach().cpu()


def _snapshot(model, head):
    p, b = tw.module_tensors(model)
    return p, b, tw.module_tensors(head)[0]


def _twin_predict(kind, cfg, snap, raw, ei):
    p, b, h = snap
    return tw.predict(kind, _twin_cfg(kind, cfg), p, b, h, raw["x"][:, 0].copy(), raw["positions"], raw["batch"], ei,
                      device=DEV)


def _flat_grads(tr, model, head):
    out, off, seen = {}, 0, set()
    for prefix, m in (("", model), ("head.", head)):
        for n, p in m.named_parameters():
            if id(p) in seen or not p.requires_grad:
                continue
            seen.add(id(p))
            out[prefix + n] = tr.flat.grad[off:off + p.numel()].view_as(p).detach().clone()
            off += p.numel()
    assert off == tr.flat.numel
    return out


# ----------------------------------------------------------------- PaiNN: the complete pair list against the radius list
PAINN_CASES = {"painn_md17_B1": ([N_ATOMS], 41), "painn_md17_B4": ([N_ATOMS] * 4, 61)}


@pytest.mark.parametrize("mode", ["eager", "replayed", "radius_list"])
@pytest.mark.parametrize("name", sorted(PAINN_CASES))
def test_painn_step_on_the_complete_list_meets_the_twin_on_the_radius_list(name, mode, monkeypatch):
    """Three steps on three frames: loss, energy, force (through predict) and every gradient within BOUNDS["painn"] of
    the twin, which is given the frame's own 5 A radius list.  Replayed: one capture serves the three frames.
    GEOSSL_MD17_COMPLETE_EDGES=0 is the route before: the same bounds, nothing replayed."""
    from geossl_amd.finetune_md17 import MD17Trainer
    if mode == "radius_list":
        monkeypatch.setenv("GEOSSL_MD17_COMPLETE_EDGES", "0")
    else:
        monkeypatch.delenv("GEOSSL_MD17_COMPLETE_EDGES", raising=False)
    sizes, seed = PAINN_CASES[name]
    cfg = _cfg("painn")
    base = _raw(sizes, seed, 5.0)
    model, head = _modules("painn", cfg)
    tr = MD17Trainer(model, head, model_3d="painn", lr=LR, use_graph=(mode != "eager"))
    B = len(sizes)
    for k in range(3):
        raw = _moved(base, k, 5.0)
        bt = _batch("painn", cfg, raw)
        ei = _edges("painn", cfg, raw, bt)
        assert ei.size(1) < B * N_ATOMS * (N_ATOMS - 1), "a condition of the test: a pair beyond the cutoff"
        snap = _snapshot(model, head)
        e, f = _twin_predict("painn", cfg, snap, raw, ei)
        y_e, y_f = tw.targets_with_margin(e, f, 7 + k)
        bt.y, bt.force = y_e.to(DEV), y_f.to(DEV)
        ref = tw.step("painn", _twin_cfg("painn", cfg), snap[0], snap[1], snap[2], raw["x"][:, 0].copy(),
                      raw["positions"], raw["batch"], ei, y_e, y_f, device=DEV)
        pe, pf = tr.predict(bt)
        loss = tr.step(bt)
        torch.cuda.synchronize()
        got = dict(loss=loss, energy=pe, force=pf, grads=_flat_grads(tr, model, head))
        errs = tw.errors(got, ref)
        want = set(ref["grads"]) | {"head." + n for n in ref["head_grads"]}
        assert {n[5:] for n in errs if n.startswith("grad/")} == want
        print(name, mode, k, {q: "%.2e" % max(v for n, v in errs.items() if n.split("/")[0] == q)
                              for q in ("loss", "energy", "force", "grad")})
        bad = tw.flagged(errs, "painn")
        assert not bad, (name, mode, k, bad)
    assert tr.captures == {"eager": 0, "replayed": 1, "radius_list": 0}[mode]
    if mode == "replayed":
        assert len(tr.graphs) == 1 and tr.use_graph


def test_complete_edges_on_the_gpu_is_the_closed_form():
    from geossl_amd.finetune_md17 import complete_edges
    for B, n in ((1, 1), (2, 2), (3, 21), (2, 33)):
        ei, bvec = complete_edges(B, n, DEV)
        cpu = complete_edges(B, n)
        assert ei.is_cuda and torch.equal(ei.cpu(), cpu[0]) and torch.equal(bvec.cpu(), cpu[1])
        assert complete_edges(B, n, DEV)[0] is ei


# ------------------------------------------------------------------------------- SchNet: handles against collated batches
def _frames_dataset(kind, cfg, n_batches, B, seed, with_radius=False):
    """n_batches x B frames of 21 atoms as one DeviceDataset with energies and forces (random targets), and the raw
    batches in loader order."""
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset
    raws = [_raw([N_ATOMS] * B, seed + 10 * k, cfg["cutoff"]) for k in range(n_batches)]
    g = torch.Generator().manual_seed(seed)
    M = n_batches * B
    y, f = torch.randn(M, generator=g), torch.randn(M * N_ATOMS, 3, generator=g)
    ds = DeviceDataset(np.concatenate([r["x"][:, 0] for r in raws]), np.concatenate([r["positions"] for r in raws]),
                       [N_ATOMS] * M, DEV, y=y, force=f, radius=cfg["cutoff"] if with_radius else None)
    return ds, raws, y, f


@pytest.mark.parametrize("B", [1, 4])
def test_schnet_step_from_a_handle_is_force_trainer_on_the_collated_batch(B):
    from geossl_amd.finetune_md17 import MD17Trainer
    from geossl_amd.graphed import ForceTrainer
    cfg = _cfg("schnet")
    ds, raws, y, f = _frames_dataset("schnet", cfg, 3, B, 300 + B)
    out = {}
    for which in ("handle", "collated"):
        model, head = _modules("schnet", cfg)
        tr = (MD17Trainer if which == "handle" else ForceTrainer)(model, head, lr=LR, use_graph=True)
        losses = []
        for k, raw in enumerate(raws):
            ids = np.arange(k * B, (k + 1) * B)
            if which == "handle":
                losses.append(tr.step(ds.batch(ids)))
            else:
                rows = slice(k * B * N_ATOMS, (k + 1) * B * N_ATOMS)
                losses.append(tr.step(_batch("schnet", cfg, raw), y[k * B:(k + 1) * B].to(DEV), f[rows].to(DEV)))
        torch.cuda.synchronize()
        assert tr.captures == 1
        out[which] = (torch.stack(losses), tr.flat.flat.clone())
    assert torch.equal(out["handle"][0], out["collated"][0]) and torch.equal(out["handle"][1], out["collated"][1])


# ------------------------------------------------------------------------------------------------------------- do_MD17
@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_do_md17_with_loss_backward_vs_twin(kind):
    """The reference's loop on do_MD17 - zero_grad, loss.backward() through the force, stock parameters' .grad - from a
    collated batch and from a DeviceLoader handle: the loss and every gradient within BOUNDS[kind] of the twin."""
    import types
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset
    from geossl_amd.finetune_md17 import do_MD17
    cfg = _cfg(kind)
    B = 4
    raw = _raw([N_ATOMS] * B, 700, cfg["cutoff"])
    model, head = _modules(kind, cfg)
    snap = _snapshot(model, head)
    bt = _batch(kind, cfg, raw)
    ei = _edges(kind, cfg, raw, bt)
    y_e, y_f = tw.targets_with_margin(*_twin_predict(kind, cfg, snap, raw, ei), 3)
    bt.y, bt.force = y_e.to(DEV), y_f.to(DEV)
    ref = tw.step(kind, _twin_cfg(kind, cfg), snap[0], snap[1], snap[2], raw["x"][:, 0].copy(), raw["positions"],
                  raw["batch"], ei, y_e, y_f, device=DEV)
    ds = DeviceDataset(raw["x"][:, 0].copy(), raw["positions"], [N_ATOMS] * B, DEV, y=y_e, force=y_f,
                       radius=cfg["cutoff"] if kind == "painn" else None)
    args = types.SimpleNamespace(model_3d=kind, md17_energy_coeff=0.05, md17_force_coeff=0.95)
    for what, batch in (("collated", bt), ("handle", ds.batch(np.arange(B)))):
        for p in list(model.parameters()) + list(head.parameters()):
            p.grad = None
        loss = do_MD17(args, batch, model, head, criterion=torch.nn.L1Loss())
        assert loss.dtype == torch.float32 and loss.requires_grad
        loss.backward()
        torch.cuda.synchronize()
        grads = {}
        for prefix, m in (("", model), ("head.", head)):
            for n, p in m.named_parameters():
                grads.setdefault(prefix + n, p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p))
        errs = tw.errors(dict(loss=loss.detach(), grads=grads), ref)
        assert {n[5:] for n in errs if n.startswith("grad/")} == set(ref["grads"]) | {"head." + n for n in ref["head_grads"]}
        assert not tw.flagged(errs, kind), (kind, what, tw.flagged(errs, kind))


# -------------------------------------------------------------------------------------------------------- predict_MD17
@pytest.mark.parametrize("kind,head,readout", [("schnet", "linear", "mean"), ("schnet", "linear", "add"),
                                               ("schnet", "dense", "mean"), ("schnet", "dense", "add"),
                                               ("painn", "painn", "mean"), ("painn", "painn", "add")])
def test_predict_md17_vs_twin(kind, head, readout):
    """Energies and forces within BOUNDS[kind] of the twin (on the frame's own edges), eagerly and replayed, at B = 1 and
    4 of 21 atoms, and on a ragged batch with a one-atom molecule and a molecule without a pair inside the cutoff."""
    from geossl_amd.finetune_md17 import _predictor, predict_MD17
    import types
    cfg = _cfg(kind, readout)
    cutoff = cfg["cutoff"]
    model, hd = _modules(kind, cfg, head)
    args = types.SimpleNamespace(model_3d=kind)
    snap = _snapshot(model, hd)
    worst = {}

    def check(raw, use_graph, tag):
        bt = _batch(kind, cfg, raw)
        e, f = _twin_predict(kind, cfg, snap, raw, _edges(kind, cfg, raw, bt))
        pe, pf = predict_MD17(args, bt, model, hd, use_graph=use_graph)
        torch.cuda.synchronize()
        assert not pe.requires_grad and not pf.requires_grad and tuple(pf.shape) == tuple(bt.positions.shape)
        errs = dict(energy=tw.max_err(pe, e), force=tw.max_err(pf, f))
        for q, v in errs.items():
            worst[q] = max(worst.get(q, 0.0), v)
        assert not tw.flagged(errs, kind), (tag, errs)

    for B in (1, 4):
        base = _raw([N_ATOMS] * B, 400 + B, cutoff)
        check(base, False, "eager B%d" % B)
        before = _predictor(model, hd, kind).captures
        for k in range(3):   # (capture, replay, replay - on three frames)
            check(_moved(base, k, cutoff), True, "replayed B%d frame %d" % (B, k))
        assert _predictor(model, hd, kind).captures == before + 1
    ragged = _raw([1, 2, 9, N_ATOMS], 430, cutoff, far=1)
    before = _predictor(model, hd, kind).captures
    check(ragged, False, "ragged eager")
    check(ragged, True, "ragged (first sighting: eager)")
    assert _predictor(model, hd, kind).captures == before
    print(kind, head, readout, {q: "%.2e" % v for q, v in worst.items()})


# ------------------------------------------------------------------------------------- geossl_energy_head_fwd, per element
@pytest.mark.parametrize("F", [64, 128, 256])
@pytest.mark.parametrize("readout", ["mean", "add"])
@pytest.mark.parametrize("mlp", [False, True], ids=["linear", "mlp"])
def test_energy_head_kernel_vs_fp64(F, readout, mlp):
    """Energies and every seed row against a numpy restatement in fp64: 70 atoms in molecules of 1, 2, 33 and 34 (a
    partial wave of rows, a molecule above one wave's rows).  Per element, against the tensor's scale, at the tolerance
    of property_head's kernel test for the same arithmetic."""
    from geossl_amd import ops
    from geossl_amd.layout import get_layout
    sizes = [1, 2, 33, 34]
    g = torch.Generator().manual_seed(11 + F)
    N, B, K = sum(sizes), len(sizes), F // 2
    h = torch.randn(N, F, generator=g) * 0.5
    if mlp:
        ps = [torch.randn(K, F, generator=g) / F ** 0.5, torch.randn(K, generator=g) * 0.1,
              torch.randn(1, K, generator=g) / K ** 0.5, torch.randn(1, generator=g) * 0.1]
    else:
        ps = [torch.randn(1, F, generator=g) / F ** 0.5, torch.randn(1, generator=g) * 0.1]
    bvec = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)).to(DEV)
    bvec._geossl_sizes = (sizes, bvec._version)
    energy, seed = ops.energy_head(h.to(DEV), [p.to(DEV) for p in ps], get_layout(bvec), readout)
    torch.cuda.synchronize()
    energy, seed = energy.cpu().double().numpy(), seed.cpu().double().numpy()
    hh, pp = h.double().numpy(), [p.double().numpy() for p in ps]
    off = np.concatenate([[0], np.cumsum(sizes)])
    e_ref, s_ref = np.zeros(B), np.zeros((N, F))
    for b in range(B):
        rows = hh[off[b]:off[b + 1]]
        m = rows.sum(0) / (sizes[b] if readout == "mean" else 1)
        if mlp:
            z = pp[0] @ m + pp[1]
            sig = 1.0 / (1.0 + np.exp(-z))
            e_ref[b] = pp[2][0] @ (z * sig) + pp[3][0]
            dm = (pp[2][0] * sig * (1.0 + z * (1.0 - sig))) @ pp[0]
        else:
            e_ref[b] = pp[0][0] @ m + pp[1][0]
            dm = pp[0][0]
        s_ref[off[b]:off[b + 1]] = dm / (sizes[b] if readout == "mean" else 1)
    assert np.isfinite(energy).all() and np.isfinite(seed).all()
    assert np.abs(energy - e_ref).max() <= HEAD_TOL * np.abs(e_ref).max()
    for a in range(N):
        assert np.abs(seed[a] - s_ref[a]).max() <= HEAD_TOL * np.abs(s_ref[a]).max(), a


# ----------------------------------------------------------------------------------- geossl_force_metrics_accumulate
def test_force_metrics_accumulate_vs_numpy():
    """Two calls into one accumulator, NaN whole rows and a single NaN element in dE_dpos: the counts exact, the sums
    within 1e-12 relative of numpy on the same fp32 differences (an fp64 sum of fewer than 1e4 non-negative terms: each
    addition rounds by 2^-53 relative, so any two orders agree to about n 2^-53 < 1e-12)."""
    from geossl_amd import ops
    g = torch.Generator().manual_seed(5)
    acc = ops.force_metrics_buffer(DEV)
    se = sf = 0.0
    ne = nf = 0
    for B, N, nan_rows, nan_el in ((4, 84, (3, 40), (17, 1)), (7, 300, (), (0, 2))):
        pe, y = torch.randn(B, generator=g), torch.randn(B, generator=g)
        dE, ft = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)
        for r in nan_rows:
            dE[r] = float("nan")
        dE[nan_el[0], nan_el[1]] = float("nan")
        ops.force_metrics_accumulate(pe.to(DEV), y.to(DEV), dE.to(DEV), ft.to(DEV), acc)
        keep = ~np.isnan(dE.numpy())
        de32 = np.abs(pe.numpy() - y.numpy())                       # fp32 differences, as the reference's tensors
        df32 = np.abs((-dE.numpy()) - ft.numpy())[keep]
        se, sf = se + de32.astype(np.float64).sum(), sf + df32.astype(np.float64).sum()
        ne, nf = ne + B, nf + int(keep.sum())
    got = ops.force_metrics_read(acc)
    assert got[2] == ne and got[3] == nf and nf == 3 * (84 + 300) - 3 * 2 - 2
    assert abs(got[0] - se) <= 1e-12 * se and abs(got[1] - sf) <= 1e-12 * sf


# ----------------------------------------------------------------------------------------------- geossl_gather_atom_rows
def test_handle_force_is_the_dataset_rows_in_batch_order():
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset
    sizes = [1, 21, 2]
    g = torch.Generator().manual_seed(9)
    n = sum(sizes)
    f = torch.randn(n, 3, generator=g)
    ds = DeviceDataset(torch.ones(n, dtype=torch.long), torch.randn(n, 3, generator=g), sizes, DEV,
                       y=torch.randn(3, generator=g), force=f)
    ids = [1, 2, 0]
    hb = ds.batch(ids)
    off = np.concatenate([[0], np.cumsum(sizes)])
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in ids])
    got = hb.force
    assert got is hb.force and tuple(got.shape) == (n, 3)        # (gathered once)
    assert torch.equal(got.cpu(), f[rows])
    assert torch.equal(hb.y.cpu(), ds.y.cpu()[ids].reshape(-1))
    assert DeviceDataset(torch.ones(n, dtype=torch.long), torch.randn(n, 3, generator=g), sizes, DEV).batch(ids).force is None


# -------------------------------------------------------------------------------------- eval_MD17 / MD17Trainer.evaluate
@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_eval_md17_vs_twin(kind):
    """Three batches of 4 frames, as handles (MD17Trainer.evaluate) and collated (eval_MD17), against the two MAEs
    computed in numpy from the twin's predictions: a mean absolute error moves by at most the largest prediction error,
    BOUNDS[kind] x max|E| / max|F|.  The second and third batch replay the first one's graph."""
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceLoader
    from geossl_amd.finetune_md17 import MD17Trainer, _predictor, eval_MD17
    cfg = _cfg(kind)
    B = 4
    ds, raws, y, f = _frames_dataset(kind, cfg, 3, B, 500, with_radius=(kind == "painn"))
    model, head = _modules(kind, cfg)
    tr = MD17Trainer(model, head, model_3d=kind, lr=LR)
    snap = _snapshot(model, head)
    es, fs = [], []
    collated = []
    for k, raw in enumerate(raws):
        rows = slice(k * B * N_ATOMS, (k + 1) * B * N_ATOMS)
        bt = _batch(kind, cfg, raw, y[k * B:(k + 1) * B], f[rows])
        e, fo = _twin_predict(kind, cfg, snap, raw, _edges(kind, cfg, raw, bt))
        if kind == "painn":
            assert bt.radius_edge_index.size(1) < B * N_ATOMS * (N_ATOMS - 1)
        es.append(e.numpy())
        fs.append(fo.numpy())
        collated.append(bt)
    es, fs = np.concatenate(es), np.concatenate(fs)
    e_ref = np.abs(es - y.double().numpy()).mean()
    f_ref = np.abs(fs - f.double().numpy()).mean()
    tol_e = tw.BOUNDS[kind]["energy"] * np.abs(es).max()
    tol_f = tw.BOUNDS[kind]["force"] * np.abs(fs).max()
    got_h = tr.evaluate(DeviceLoader(ds, batch_size=B, shuffle=False))
    assert _predictor(model, head, kind).captures == 1
    model.__dict__.pop("_geossl_md17_predict")
    got_c = eval_MD17(tr.args, collated, model, head)
    assert _predictor(model, head, kind).captures == 1
    for got in (got_h, got_c):
        print(kind, "energy_mae %.8g (twin %.8g, tol %.1e)  force_mae %.8g (twin %.8g, tol %.1e)"
              % (got[0], e_ref, tol_e, got[1], f_ref, tol_f))
        assert isinstance(got[0], float) and abs(got[0] - e_ref) <= tol_e
        assert isinstance(got[1], float) and abs(got[1] - f_ref) <= tol_f
