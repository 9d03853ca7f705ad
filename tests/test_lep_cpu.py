"""CPU tests of LEP fine-tuning (geossl_amd/finetune_lep.py): our collation against the reference's (fixture G25), the
two rank metrics against the fixture and against sklearn, the fp64 twin of the pair head against the fixture, the
conditions the fixture was made under, the C ABI, and the fallback of do_LEP on CPU tensors."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import force_twin as ft
import lep_twin as lt
from lep_twin import fixture_items
from conftest import GOLDEN, REPO, load_golden, rel_err
from helpers import schnet_oracle_params
from oracle import nets

G25 = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("g25_lep_"))
NEW_SYMBOLS = ("geossl_pair_head_fwd", "geossl_pair_head_predict", "geossl_pair_head_bwd")


def test_g25_cases_present():
    assert G25 == ["g25_lep_painn", "g25_lep_schnet_dense", "g25_lep_schnet_full", "g25_lep_schnet_reduced"]
    for case in G25:
        assert os.path.getsize(os.path.join(GOLDEN, case + ".npz")) < 400 * 1024


@pytest.mark.parametrize("case", G25)
def test_our_collation_equals_the_reference_batch(case):
    from geossl_amd.Geom3D.dataloaders import BatchLEP
    g = load_golden(case)
    batch = BatchLEP.from_data_list(fixture_items(g))
    stored = [k[len("batch/"):] for k in g if k.startswith("batch/")]
    assert sorted(batch.keys) == sorted(stored) and "batch_active" in stored and "batch_inactive" in stored
    for k in stored:
        want = torch.from_numpy(g["batch/" + k])
        if "edge_index" in k:
            want = want.long()   # (int32 on disk)
        assert batch[k].dtype == want.dtype and torch.equal(batch[k], want), (case, k)
    assert np.array_equal(batch._sizes_active, g["sizes_active"]) and batch._sizes_active.dtype == np.int64
    assert np.array_equal(batch._sizes_inactive, g["sizes_inactive"]) and batch._sizes_inactive.dtype == np.int64
    assert batch.num_graphs == len(g["sizes_active"])
    assert batch.to("cpu") is batch


def test_the_loader_collates_with_batchlep():
    from geossl_amd.Geom3D.dataloaders import BatchLEP, DataLoaderLEP
    g = load_golden("g25_lep_schnet_dense")
    items = fixture_items(g)
    batches = list(DataLoaderLEP(items, batch_size=2, shuffle=False))
    assert len(batches) == 1 and isinstance(batches[0], BatchLEP)
    assert torch.equal(batches[0].batch_inactive, torch.from_numpy(g["batch/batch_inactive"]))


@pytest.mark.parametrize("side", ["active", "inactive"])
def test_a_position_row_that_sums_to_zero_is_rejected(side):
    from geossl_amd.Geom3D.dataloaders import BatchLEP
    items = fixture_items(load_golden("g25_lep_schnet_dense"))
    pos = items[1]["positions_" + side].clone()
    pos[2] = torch.tensor([1.5, -2.0, 0.5])
    items[1]["positions_" + side] = pos
    with pytest.raises(AssertionError):
        BatchLEP.from_data_list(items)


@pytest.mark.parametrize("case", G25)
def test_metrics_equal_the_fixture(case):
    from geossl_amd.finetune_lep import average_precision, roc_auc
    g = load_golden(case)
    y, pred = g["batch/y"], g["pred"]
    assert abs(roc_auc(y, pred) - float(g["roc"])) < 1e-12
    assert abs(average_precision(y, pred) - float(g["pr"])) < 1e-12
    z, yd = torch.from_numpy(pred).double(), torch.from_numpy(y).double()
    bce = torch.nn.functional.binary_cross_entropy_with_logits(z, yd)
    assert abs(float(bce.sqrt()) - float(g["bce"])) < 1e-5 * float(g["bce"])   # eval()'s first number at one batch


def test_metrics_equal_sklearn_on_ties():
    metrics = pytest.importorskip("sklearn.metrics")
    from geossl_amd.finetune_lep import average_precision, roc_auc
    rng = np.random.default_rng(25)
    hand = [([0, 1], [0.5, 0.5]), ([1, 0, 1, 0], [0.3, 0.3, 0.3, 0.1]), ([0, 0, 1, 1], [0.1, 0.4, 0.35, 0.8]),
            ([1, 1, 0], [2.0, -1.0, -1.0])]
    drawn = []
    for n in (5, 40, 257):
        y = rng.integers(0, 2, size=n)
        y[:2] = (0, 1)
        drawn.append((y, np.round(rng.standard_normal(n), 1)))   # many ties
    for y, s in hand + drawn:
        assert abs(roc_auc(y, s) - metrics.roc_auc_score(y, s)) < 1e-12
        assert abs(average_precision(y, s) - metrics.average_precision_score(y, s)) < 1e-12


def test_metrics_on_hand_made_vectors():
    from geossl_amd.finetune_lep import average_precision, roc_auc
    assert roc_auc([0, 0, 1, 1], [0.1, 0.4, 0.35, 0.8]) == 0.75
    assert abs(average_precision([0, 0, 1, 1], [0.1, 0.4, 0.35, 0.8]) - (0.5 * 1.0 + 0.5 * 2.0 / 3.0)) < 1e-15
    assert roc_auc([0, 1], [0.5, 0.5]) == 0.5 and average_precision([0, 1], [0.5, 0.5]) == 0.5   # one threshold
    assert roc_auc([1, 0, 1, 0], [0.3, 0.3, 0.3, 0.1]) == 0.75


def test_roc_auc_with_one_class_raises():
    from geossl_amd.finetune_lep import roc_auc
    for y in ([1, 1, 1], [0, 0]):
        with pytest.raises(ValueError, match="[Oo]nly one class"):
            roc_auc(y, np.linspace(0.0, 1.0, len(y)))


@pytest.mark.parametrize("case", G25)
def test_twin_reproduces_the_fixture_from_the_reference_readouts(case):
    g = load_golden(case)
    w = torch.from_numpy(g["head/weight"]).double().requires_grad_()
    b = torch.from_numpy(g["head/bias"]).double().requires_grad_()
    z = lt.logits(torch.from_numpy(g["repr_active"]), torch.from_numpy(g["repr_inactive"]), w, b)
    loss = lt.bce(z, g["batch/y"])
    loss.backward()
    assert rel_err(z, g["pred"]) < 1e-6
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-6 * float(g["loss"])
    assert rel_err(w.grad, g["head_grad/weight"]) < 1e-6 and rel_err(b.grad, g["head_grad/bias"]) < 1e-6


@pytest.mark.parametrize("case", G25)
def test_fixture_conditions(case):
    """What the maker asserted on the reference's results: no saturated sigmoid, no near-equal logits."""
    g = load_golden(case)
    z, y = g["pred"].astype(np.float64), g["batch/y"].astype(np.float64)
    assert np.abs(z).max() <= 3.0
    assert np.abs(1.0 / (1.0 + np.exp(-z)) - y).min() >= 0.05
    assert set(y.tolist()) == {0.0, 1.0}
    assert np.diff(np.sort(z)).min() >= 1e-3
    meta = json.loads(str(g["meta"]))
    assert meta["head_weight_scale"] > 0 and "head_bias_scale" in meta
    pos = np.concatenate([g["batch/positions_active"], g["batch/positions_inactive"]])
    bvec = np.concatenate([g["batch/batch_active"], g["batch/batch_inactive"] + len(g["sizes_active"])])
    assert ft.cutoff_margin(pos, bvec, meta["cutoff"]) >= ft.CUTOFF_MARGIN
    big = max(g["sizes_active"].max(), g["sizes_inactive"].max())
    assert (big > 255) == (case != "g25_lep_schnet_dense")   # both layouts of the fused batch are in the fixture


def test_new_abi_symbols_declared_bound_and_exported():
    from geossl_amd import _lib, build
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in NEW_SYMBOLS + ("geossl_pair_head_width_ok",):
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    assert re.search(r"\bint64_t geossl_pair_head_workspace_floats\(", h)
    assert "geossl_pair_head_workspace_floats" in _lib.PROTOTYPES
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    assert [F for F in (16, 32, 64, 96, 128, 256) if lib.geossl_pair_head_width_ok(F)] == [32, 64, 128]
    assert lib.geossl_pair_head_workspace_floats(5) == 10
    assert "pair_head.hip" in build._sources() and build.SOURCE_FLAGS.get("pair_head.hip") == ["-fno-slp-vectorize"]


class OracleSchNet(torch.nn.Module):
    """The fp64 oracle of SchNet behind the backbone's call, with filler.py's weights: a backbone for CPU tensors."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.P = {k: v.double() for k, v in schnet_oracle_params(cfg, requires_grad=False).items()}

    def forward(self, x, positions, batch):
        cfg = self.cfg
        ei = ft.schnet_edges(positions.numpy(), batch.numpy(), cfg["cutoff"])
        rep = nets.schnet_forward(self.P, x, positions.double(), batch, cfg["cutoff"], cfg["num_interactions"],
                                  cfg["readout"], edge_index=ei)
        return rep.float()


def _cpu_setup():
    from geossl_amd.Geom3D.dataloaders import BatchLEP
    g = load_golden("g25_lep_schnet_dense")
    model = OracleSchNet(json.loads(str(g["cfg"])))
    head = torch.nn.Linear(g["head/weight"].shape[1], 1)
    with torch.no_grad():
        head.weight.copy_(torch.from_numpy(g["head/weight"]))
        head.bias.copy_(torch.from_numpy(g["head/bias"]))
    return g, model, head, fixture_items(g), BatchLEP, types.SimpleNamespace(model_3d="schnet")


def test_do_lep_on_cpu_tensors_runs_the_reference_lines():
    from geossl_amd.finetune_lep import do_LEP, predict_LEP
    g, model, head, items, BatchLEP, args = _cpu_setup()
    batch = BatchLEP.from_data_list(items)
    assert batch.y.dtype == torch.long   # (:43: the script's .float())
    loss = do_LEP(args, batch, model, head)
    loss.backward()
    assert loss.dtype == torch.float32 and rel_err(loss, g["loss"]) < 1e-5
    assert rel_err(head.weight.grad, g["head_grad/weight"]) < 1e-5
    assert rel_err(head.bias.grad, g["head_grad/bias"]) < 1e-5
    assert rel_err(predict_LEP(args, batch, model, head), g["pred"]) < 1e-5
    with pytest.raises(Exception, match="not included"):
        do_LEP(types.SimpleNamespace(model_3d="egnn"), batch, model, head)


def test_do_lep_at_one_pair_raises_like_the_reference():
    """pred.squeeze() is 0-d against a [1] target: BCEWithLogitsLoss refuses the sizes."""
    from geossl_amd.finetune_lep import do_LEP
    g, model, head, items, BatchLEP, args = _cpu_setup()
    with pytest.raises(ValueError, match="[Tt]arget size"):
        do_LEP(args, BatchLEP.from_data_list(items[:1]), model, head)
