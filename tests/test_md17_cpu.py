"""CPU tests of MD17 fine-tuning (geossl_amd/finetune_md17.py): the module's surface and the C ABI of its kernels,
do_MD17's ATen lines against fixture G22 and eval_MD17 against fixture G26 (the reference's eval() run verbatim,
tests/golden/make_golden_md17_eval.py) on the oracle's CPU backbones, the NaN rule, the interned complete pair list with
its superset property, and the argument checks of per-atom targets in a DeviceDataset."""
import inspect
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import force_twin as tw
from conftest import load_golden, rel_err
from helpers import fill_module_
from oracle import nets
from oracle.graph import radius_graph_np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("geossl_energy_head_fwd", "geossl_force_metrics_accumulate", "geossl_gather_atom_rows")
TOL = 5e-5   # test_force_cpu.py's G22 tolerance (the loss: 2e-5)


# ------------------------------------------------------------------------------------------------------------ surface
def test_module_surface_and_abi():
    import geossl_amd
    from geossl_amd import _lib, build, finetune_md17 as fm, switches
    from geossl_amd.graphed import ForceTrainer
    assert "finetune_md17" in geossl_amd.__doc__
    assert set(fm.__all__) >= {"do_MD17", "predict_MD17", "eval_MD17", "MD17Trainer", "complete_edges"}
    assert list(inspect.signature(fm.do_MD17).parameters) == ["args", "batch", "model", "graph_pred_linear", "criterion"]
    assert list(inspect.signature(fm.predict_MD17).parameters)[:4] == ["args", "batch", "model", "graph_pred_linear"]
    assert inspect.signature(fm.predict_MD17).parameters["use_graph"].default is True
    assert list(inspect.signature(fm.eval_MD17).parameters)[:4] == ["args", "loader", "model", "graph_pred_linear"]
    sig = inspect.signature(fm.MD17Trainer).parameters
    want = dict(model_3d="schnet", lr=5e-4, weight_decay=0.0, energy_coeff=0.05, force_coeff=0.95, loss="l1",
                use_graph=True)
    assert list(sig)[:2] == ["model", "head"] and {k: sig[k].default for k in want} == want
    assert issubclass(fm.MD17Trainer, ForceTrainer)
    for name in ("step", "predict", "evaluate", "set_lr"):
        assert callable(getattr(fm.MD17Trainer, name))
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert build.SOURCE_FLAGS.get("force_head.hip") == ["-fno-slp-vectorize"]
    assert callable(switches.md17_complete_edges)


def test_complete_edges_switch(monkeypatch):
    from geossl_amd import switches
    monkeypatch.delenv("GEOSSL_MD17_COMPLETE_EDGES", raising=False)
    assert switches.md17_complete_edges(True) == switches.MD17_COMPLETE_EDGES_DEFAULT
    assert not switches.md17_complete_edges(False)
    monkeypatch.setenv("GEOSSL_MD17_COMPLETE_EDGES", "1")
    assert switches.md17_complete_edges(True) and not switches.md17_complete_edges(False)
    monkeypatch.setenv("GEOSSL_MD17_COMPLETE_EDGES", "0")
    assert not switches.md17_complete_edges(True)


# ------------------------------------------------------------------------------------- the oracle's backbones on CPU
class _OracleBackbone(torch.nn.Module):
    """oracle.nets on the parameters of the library's module (which itself runs on the GPU only): fp32 torch CPU kernels,
    the reference's arithmetic."""

    def __init__(self, kind, cfg):
        super().__init__()
        from geossl_amd.Geom3D.models import PaiNN, SchNet
        self.kind, self.cfg = kind, cfg
        self.net = fill_module_(SchNet(**cfg) if kind == "schnet" else PaiNN(**cfg))
        self.readout = cfg["readout"]

    def forward(self, x, positions, *rest):
        cfg = self.cfg
        P = dict(self.net.named_parameters())
        P.update({k: v for k, v in self.net.named_buffers() if v.is_floating_point()})
        if self.kind == "schnet":
            (batch,) = rest
            ei = tw.schnet_edges(positions.detach().numpy(), batch.numpy(), cfg["cutoff"])
            return nets.schnet_forward(P, x, positions, batch, cfg["cutoff"], cfg["num_interactions"], cfg["readout"],
                                       edge_index=ei)
        rei, batch = rest
        return nets.painn_forward(P, x, positions, rei, batch, cfg["n_atom_basis"], cfg["n_interactions"], cfg["cutoff"],
                                  cfg["readout"])


def _cpu_head(kind, model):
    """The fixture's head with torch's own CPU layers (the library's Dense runs on the GPU): (module, {fixture name:
    parameter})."""
    F = model.cfg["hidden_channels"] if kind == "schnet" else model.cfg["n_atom_basis"]
    if kind == "schnet":
        head = fill_module_(torch.nn.Linear(F, 1))
        return head, {"weight": head.weight, "bias": head.bias}
    src = fill_module_(model.net.create_output_layers())
    head = torch.nn.Sequential(torch.nn.Linear(F, F // 2), torch.nn.SiLU(), torch.nn.Linear(F // 2, 1))
    with torch.no_grad():
        for dst, s in ((head[0], src[0]), (head[2], src[1])):
            dst.weight.copy_(s.weight)
            dst.bias.copy_(s.bias)
    return head, {"0.weight": head[0].weight, "0.bias": head[0].bias, "1.weight": head[2].weight, "1.bias": head[2].bias}


def _ns(**kw):
    return types.SimpleNamespace(**kw)


@pytest.mark.parametrize("case", ["schnet_B1", "painn_B4"])
def test_do_md17_aten_on_cpu_reproduces_g22(case):
    """do_MD17 on CPU tensors runs the reference's lines: G22's loss, energies, forces and head gradients."""
    from geossl_amd.finetune_md17 import do_MD17
    g = load_golden("g22_md17_" + case)
    cfg, meta = json.loads(str(g["cfg"])), json.loads(str(g["meta"]))
    kind = meta["kind"]
    model = _OracleBackbone(kind, cfg)
    head, named = _cpu_head(kind, model)
    batch = _ns(x=torch.from_numpy(g["x"]), positions=torch.from_numpy(g["positions"]).clone(),
                batch=torch.from_numpy(g["batch"]), y=torch.from_numpy(g["actual_energy"]),
                force=torch.from_numpy(g["actual_force"]),
                radius_edge_index=torch.from_numpy(g["radius_edge_index"]) if "radius_edge_index" in g else None)
    args = _ns(model_3d=kind, md17_energy_coeff=meta["energy_coeff"], md17_force_coeff=meta["force_coeff"])
    loss = do_MD17(args, batch, model, head)
    assert loss.dtype == torch.float32 and rel_err(loss, g["loss"]) < 2e-5
    loss.backward()
    assert rel_err(batch.positions.grad, g["grad_pos"]) < TOL
    for k, p in named.items():
        assert rel_err(p.grad, g["head_grad/" + k]) < TOL, k
    # a stock criterion is the same lines; one the kernels do not have is used as it is
    l1 = do_MD17(args, batch, model, head, criterion=torch.nn.L1Loss())
    assert l1.item() == loss.item()
    hub = do_MD17(args, batch, model, head, criterion=torch.nn.HuberLoss())
    assert hub.item() != loss.item() and torch.isfinite(hub)
    with pytest.raises(Exception, match="not included"):
        do_MD17(_ns(model_3d="egnn", md17_energy_coeff=1.0, md17_force_coeff=1.0), batch, model, head)


def _g26_loader(g, kind):
    out = []
    for k in range(g["x"].shape[0]):
        out.append(_ns(x=torch.from_numpy(g["x"][k]), positions=torch.from_numpy(g["positions"][k]).clone(),
                       batch=torch.from_numpy(g["batch"][k]), y=torch.from_numpy(g["y"][k]),
                       force=torch.from_numpy(g["force"][k]),
                       radius_edge_index=torch.from_numpy(g["radius_edge_index_%d" % k]) if kind == "painn" else None))
    return out


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_eval_md17_on_cpu_reproduces_g26(kind):
    from geossl_amd.finetune_md17 import eval_MD17, predict_MD17
    path = os.path.join(REPO, "tests", "golden", "g26_md17_eval_%s.npz" % kind)
    assert os.path.getsize(path) < 64 * 1024
    g = load_golden("g26_md17_eval_" + kind)
    cfg, meta = json.loads(str(g["cfg"])), json.loads(str(g["meta"]))
    assert (meta["B"], meta["n"], meta["batches"]) == (4, 21, 3) and g["positions"].shape == (3, 84, 3)
    model = _OracleBackbone(kind, cfg)
    head, _ = _cpu_head(kind, model)
    args = _ns(model_3d=kind)
    e_mae, f_mae = eval_MD17(args, _g26_loader(g, kind), model, head)
    print("G26 %s: energy_mae %.9g (ref %.9g)  force_mae %.9g (ref %.9g)"
          % (kind, e_mae, float(g["energy_mae"]), f_mae, float(g["force_mae"])))
    assert isinstance(e_mae, float) and isinstance(f_mae, float)
    assert abs(e_mae - float(g["energy_mae"])) <= 1e-6 * abs(float(g["energy_mae"]))
    assert abs(f_mae - float(g["force_mae"])) <= 1e-6 * abs(float(g["force_mae"]))
    b0 = _g26_loader(g, kind)[0]
    e, f = predict_MD17(args, b0, model, head)
    assert not e.requires_grad and not f.requires_grad
    assert rel_err(e, g["pred_energy"][0]) < TOL and rel_err(f, g["pred_force"][0]) < TOL


# ----------------------------------------------------------------------------------------------------- the NaN rule
class _SqrtBackbone(torch.nn.Module):
    """Energy of a molecule = the sum of its atoms' distances to its own first atom: the gradient of sqrt at 0 makes the
    force row of every molecule's first atom NaN (0 * inf), every other row finite."""

    def forward(self, x, positions, batch):
        B = int(batch.max()) + 1
        first = torch.zeros(B, dtype=torch.long).scatter_reduce(0, batch, torch.arange(batch.numel()), "amin",
                                                                include_self=False)
        d = torch.sqrt(((positions - positions[first[batch]]) ** 2).sum(1))
        return torch.zeros(B, 1).index_add(0, batch, d[:, None])


def _reference_eval_lines(model, loader):
    """finetune_md17.py:74-117 restated for graph_pred_linear = None and a SchNet-style call."""
    pred_energy_list, actual_energy_list = [], []
    pred_force_list, actual_force_list = torch.Tensor([]), torch.Tensor([])
    for b in loader:
        positions = b.positions
        positions.requires_grad_()
        pred_energy = model(b.x, positions, b.batch).squeeze(1)
        force = -torch.autograd.grad(pred_energy, positions, torch.ones_like(pred_energy), create_graph=True,
                                     retain_graph=True)[0].detach_()
        actual = b.force
        if torch.sum(torch.isnan(force)) != 0:
            mask = torch.isnan(force)
            force = force[~mask].reshape((-1, 3))
            actual = actual[~mask].reshape((-1, 3))
        pred_energy_list.append(pred_energy.detach())
        actual_energy_list.append(b.y)
        pred_force_list = torch.cat([pred_force_list, force], dim=0)
        actual_force_list = torch.cat([actual_force_list, actual], dim=0)
    e = torch.mean(torch.abs(torch.cat(pred_energy_list) - torch.cat(actual_energy_list))).item()
    f = torch.mean(torch.abs(pred_force_list - actual_force_list)).item()
    return e, f, pred_force_list.size(0)


def test_eval_md17_keeps_the_nan_rule():
    from geossl_amd.finetune_md17 import eval_MD17
    gen = torch.Generator().manual_seed(3)

    def loader():
        out = []
        for sizes in ([5, 7], [3, 6, 4]):
            n = sum(sizes)
            g2 = torch.Generator().manual_seed(n)
            out.append(_ns(x=torch.ones(n, dtype=torch.long), positions=torch.randn(n, 3, generator=g2),
                           batch=torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)),
                           y=torch.randn(len(sizes), generator=g2), force=torch.randn(n, 3, generator=g2)))
        return out

    assert gen is not None
    model = _SqrtBackbone()
    e_ref, f_ref, rows = _reference_eval_lines(model, loader())
    assert rows == 25 - 5   # one NaN row per molecule dropped, on both sides
    e, f = eval_MD17(_ns(model_3d="schnet"), loader(), model, None)
    assert np.isfinite(e) and np.isfinite(f)
    assert abs(e - e_ref) <= 1e-6 * abs(e_ref) and abs(f - f_ref) <= 1e-6 * abs(f_ref)


# ------------------------------------------------------------------------------------------ the complete pair list
@pytest.mark.parametrize("n", [1, 2, 21, 33])
def test_complete_edges_is_the_radius_graph_at_a_large_radius(n):
    from geossl_amd.finetune_md17 import complete_edges
    B = 3
    ei, bvec = complete_edges(B, n)
    assert ei.dtype == torch.int64 and tuple(ei.shape) == (2, B * n * (n - 1)) and tuple(bvec.shape) == (B * n,)
    pos = np.random.default_rng(n).standard_normal((B * n, 3)).astype(np.float32)
    assert np.array_equal(ei.numpy(), radius_graph_np(pos, 1e3, bvec.numpy()))
    again = complete_edges(B, n)
    assert again[0] is ei and again[1] is bvec
    assert complete_edges(B + 1, n)[0] is not ei


def test_complete_edges_refuses_34_atoms():
    from geossl_amd.finetune_md17 import COMPLETE_MAX_N, complete_edges
    assert COMPLETE_MAX_N == 33
    with pytest.raises(ValueError, match="33"):
        complete_edges(1, 34)
    with pytest.raises(ValueError):
        complete_edges(0, 5)


def _frames(sizes, seed, cutoff=5.0):
    from geossl_amd.synthetic import make_batch
    for s in range(seed, seed + 50):
        r = make_batch(0, seed=s, sizes=sizes)
        if tw.cutoff_margin(r["positions"], r["batch"], cutoff) >= tw.CUTOFF_MARGIN:
            return r
    raise AssertionError("no seed with a cutoff margin")


def _is_subsequence(sub, full):
    """The columns of sub [2, e] appear in full [2, E] in the same relative order."""
    it = iter(map(tuple, full.T.tolist()))
    return all(any(c == d for d in it) for c in map(tuple, sub.T.tolist()))


@pytest.mark.parametrize("sizes,seed", [([21], 41), ([21] * 4, 61)])
def test_radius_list_is_a_subsequence_of_the_complete_list(sizes, seed):
    from geossl_amd.finetune_md17 import complete_edges
    raw = _frames(sizes, seed)
    assert tw.cutoff_margin(raw["positions"], raw["batch"], 5.0) >= tw.CUTOFF_MARGIN
    B, n = len(sizes), sizes[0]
    full = complete_edges(B, n)[0].numpy()
    rad = radius_graph_np(raw["positions"], 5.0, raw["batch"])
    per_mol = [int(((rad[1] >= m * n) & (rad[1] < (m + 1) * n)).sum()) for m in range(B)]
    print("live pairs per molecule:", per_mol, "of", n * (n - 1))
    assert min(per_mol) < n * (n - 1), "a condition of the test: a pair beyond the cutoff"
    assert rad.shape[1] < full.shape[1] and _is_subsequence(rad, full)
    for m in range(B):   # ... and molecule by molecule
        sel_r = (rad[1] >= m * n) & (rad[1] < (m + 1) * n)
        sel_f = (full[1] >= m * n) & (full[1] < (m + 1) * n)
        assert _is_subsequence(rad[:, sel_r], full[:, sel_f])


def test_complete_list_applies_to_uniform_stock_painn_only():
    from geossl_amd.finetune_md17 import complete_applies
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    painn = PaiNN(n_atom_basis=64, n_interactions=1, n_rbf=20, cutoff=5.0, n_out=1, readout="add", max_z=9)

    class Sub(PaiNN):
        pass
    sub = Sub(n_atom_basis=64, n_interactions=1, n_rbf=20, cutoff=5.0, n_out=1, readout="add", max_z=9)
    sch = SchNet(hidden_channels=64, num_filters=64, num_interactions=1, num_gaussians=8, cutoff=5.0, node_class=9)
    assert complete_applies(_ns(_sizes=[21] * 4), painn) and complete_applies(_ns(_sizes=[33]), painn)
    assert not complete_applies(_ns(_sizes=[34]), painn)
    assert not complete_applies(_ns(_sizes=[21, 20]), painn)
    assert not complete_applies(_ns(_sizes=None), painn)
    assert not complete_applies(_ns(_sizes=[21]), sub) and not complete_applies(_ns(_sizes=[21]), sch)


# ------------------------------------------------------------------------------------- per-atom targets in a dataset
def test_device_dataset_force_argument_checks():
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset, DeviceLoader, check_force
    assert "force" in inspect.signature(DeviceDataset.__init__).parameters
    f = check_force(np.zeros((9, 3), dtype=np.float64), 9)
    assert f.dtype == torch.float32 and tuple(f.shape) == (9, 3)
    with pytest.raises(ValueError, match="one row per atom"):
        check_force(np.zeros((9, 2), dtype=np.float32), 9)
    with pytest.raises(ValueError, match="one row per atom"):
        check_force(np.zeros(27, dtype=np.float32), 9)
    with pytest.raises(ValueError, match="force has 8 rows"):
        check_force(torch.zeros(8, 3), 9)
    sizes = np.array([4, 6, 3], dtype=np.int64)
    ns = _ns(sizes=sizes, off=np.concatenate([[0], np.cumsum(sizes)]), pairs=sizes * (sizes - 1) // 2,
             option="combination", x_cols=1, device=torch.device("cpu"), edges=None, edge_cnt=None,
             bonds=np.zeros((2, 0), np.int64), force=torch.zeros(13, 3))
    stub = type("Stub", (), dict(vars(ns), __len__=lambda self: 3, check_masking=DeviceDataset.check_masking))()
    with pytest.raises(ValueError, match="forces"):
        DeviceLoader(stub, batch_size=2, mask_ratio=0.3)
    DeviceLoader(stub, batch_size=2)
    stub.force = None
    DeviceLoader(stub, batch_size=2, mask_ratio=0.3)
