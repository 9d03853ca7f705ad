"""CPU tests of angle prediction on atom triples: the fp64 twin against fixture G23 (the reference run verbatim,
tests/golden/make_golden_torsion.py), the loader surface against the reference's own (g23_triple_loader), the public
surface against the reference's, and the C ABI of the new kernels."""
import glob
import inspect
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

import torsion_twin as tw
from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(REPO, "tests", "golden", "g23_torsion_*.npz")))
NEW_SYMBOLS = ("geossl_torsion_head_fwd", "geossl_torsion_head_fwd_dyn", "geossl_torsion_head_bwd",
               "geossl_torsion_head_bwd_dyn", "geossl_triple_angles", "geossl_gather_triples")
# the reference's fp32 losses as the issue lists them (regenerated fixtures must agree but for the last digit)
LOSSES = {"schnet_reduced_full": 0.8941931, "schnet_full_r03": 1.7879466, "painn_r01": 17.3272133,
          "schnet_reduced_r001": 0.7950999, "schnet_reduced_B1_n3": 0.4194543, "schnet_reduced_T1": 0.9303299}


def test_g23_cases_present():
    assert len(CASES) == 6
    gs = {c: load_golden(c) for c in CASES}
    metas = {c: json.loads(str(g["meta"])) for c, g in gs.items()}
    assert {m["kind"] for m in metas.values()} == {"schnet", "painn"}
    assert any(m["ratio"] == 1 for m in metas.values())
    assert any(m["ratio"] == 1e-3 for m in metas.values())                      # the script's own ratio
    assert any(g["super_edge_index"].shape[1] == 1 for g in gs.values())        # T = 1
    assert any(g["sizes"].tolist() == [3] for g in gs.values())                 # B = 1
    assert any(json.loads(str(g["cfg"])).get("hidden_channels") == 128 for g in gs.values())   # SchNet full
    # a batch with molecules that contribute no triple (1 and 2 atoms at ratio 1)
    g = gs["g23_torsion_schnet_reduced_full"]
    assert {1, 2} <= set(g["sizes"].tolist()) and g["super_edge_index"].shape == (3, 6786)
    from geossl_amd.Geom3D.dataloaders.dataloaders_AtomTriple import triple_count
    for c, g in gs.items():
        T = g["super_edge_index"].shape[1]
        r = metas[c]["ratio"]
        assert T == sum(triple_count(n) if r >= 1 else int(triple_count(n) * r) for n in g["sizes"].tolist())
        assert g["super_edge_index"].shape[0] == 3 and g["super_edge_index"].dtype == np.int64
        assert g["super_edge_angle"].shape == (T,) and g["super_edge_angle"].dtype == np.float32
        assert abs(float(g["loss"]) - LOSSES[c[len("g23_torsion_"):]]) <= 2e-7 * max(1.0, LOSSES[c[len("g23_torsion_"):]])
        assert os.path.getsize(os.path.join(REPO, "tests", "golden", c + ".npz")) < 312 * 1024


@pytest.mark.parametrize("case", CASES)
def test_twin_reproduces_g23(case):
    g = load_golden(case)
    h = torch.from_numpy(g["node_repr"]).double().requires_grad_()
    W = torch.from_numpy(g["pred_weight"]).double().requires_grad_()
    b = torch.from_numpy(g["pred_bias"]).double().requires_grad_()
    sei = torch.from_numpy(g["super_edge_index"])
    loss, pred = tw.torsion_loss(h, W, b, sei, torch.from_numpy(g["super_edge_angle"]))
    ref = float(g["loss"])
    assert abs(loss.item() - ref) <= 1e-5 * abs(ref)
    assert float((pred.detach() - torch.from_numpy(g["pred"]).double()).abs().max()) <= 1e-5 * max(
        float(pred.detach().abs().max()), 1.0)
    loss.backward()
    for got, key in ((h.grad, "grad_node_repr"), (W.grad, "grad_pred_weight"), (b.grad, "grad_pred_bias")):
        want = torch.from_numpy(g[key]).double().reshape(got.shape)
        assert float((got - want).abs().max()) <= 1e-5 * max(float(want.abs().max()), 1e-6), key
    # the fixture's angles are the twin's definition rounded to float32
    ang = tw.triple_angles(torch.from_numpy(g["positions"]), sei)
    assert float((ang - torch.from_numpy(g["super_edge_angle"]).double()).abs().max()) <= 2.0 ** -22


@pytest.mark.parametrize("case", CASES)
def test_extractor_reproduces_g23_triples(case):
    """The fixture's triples came from the reference's AtomTripleExtractor under np.random.seed(seed): the library's
    extractor draws the same ones, molecule after molecule."""
    from geossl_amd.Geom3D.dataloaders import AtomTripleExtractor
    g = load_golden(case)
    meta = json.loads(str(g["meta"]))
    np.random.seed(meta["seed"])
    ext = AtomTripleExtractor(meta["ratio"])
    parts, off = [], 0
    for n in g["sizes"].tolist():
        parts.append(ext.triples(n) + off)
        off += n
    assert np.array_equal(np.concatenate(parts, axis=1), g["super_edge_index"])


def test_unranking_equals_itertools():
    from geossl_amd.Geom3D.dataloaders.dataloaders_AtomTriple import triple_count, unrank_triples
    for n in range(0, 13):
        want = np.array(list(itertools.permutations(np.arange(n), 3)), dtype=np.int64).reshape(-1, 3).T
        assert triple_count(n) == want.shape[1]
        got = unrank_triples(n, np.arange(want.shape[1]))
        assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), n
    rng = np.random.RandomState(0)
    for n in (18, 33):
        want = np.array(list(itertools.permutations(np.arange(n), 3)), dtype=np.int64).T
        pick = rng.choice(want.shape[1], 500, replace=False)
        assert np.array_equal(unrank_triples(n, pick), want[:, pick])


def test_extractor_and_collation_equal_the_reference_loader():
    """AtomTripleExtractor as a per-molecule transform and BatchAtomTriple.from_data_list against fixture
    g23_triple_loader = the unmodified reference's own classes on the same molecules under the same np.random seed."""
    from geossl_amd.Geom3D.dataloaders import AtomTripleExtractor, BatchAtomTriple, Data, DataLoaderAtomTriple
    g = load_golden("g23_triple_loader")
    sizes = g["sizes"].tolist()
    assert {1, 2, 3} <= set(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for ratio in (1, 0.3, 1e-3):
        tag = "%g" % ratio
        np.random.seed(int(g["seed"]))
        ext = AtomTripleExtractor(ratio=ratio)
        mols, a0 = [], 0
        for m, n in enumerate(sizes):
            d = ext(Data(x=torch.from_numpy(g["x"][off[m]:off[m + 1]]),
                         positions=torch.from_numpy(g["positions"][off[m]:off[m + 1]])))
            want = g["mol%d/%s" % (m, tag)]
            assert d.super_edge_index.dtype == torch.long and tuple(d.super_edge_index.shape) == want.shape
            assert want.shape[0] == 3 and np.array_equal(d.super_edge_index.numpy(), want)
            T = d.super_edge_index.size(1)
            d.super_edge_angle = torch.from_numpy(g["angle/" + tag][a0:a0 + T].copy())
            a0 += T
            lo, hi = (g["rei/" + tag][0] >= off[m]), (g["rei/" + tag][0] < off[m + 1])
            d.radius_edge_index = torch.from_numpy(g["rei/" + tag][:, lo & hi] - off[m])
            mols.append(d)
        bt = BatchAtomTriple.from_data_list(mols)
        assert np.array_equal(bt.super_edge_index.numpy(), g["sei/" + tag]) and bt.super_edge_index.dtype == torch.long
        assert np.array_equal(bt.super_edge_angle.numpy(), g["angle/" + tag])
        assert np.array_equal(bt.batch.numpy(), g["batch/" + tag])
        assert np.array_equal(bt.radius_edge_index.numpy(), g["rei/" + tag])
        assert bt.num_graphs == int(g["num_graphs/" + tag])
        assert np.array_equal(bt.x.numpy(), g["x"]) and np.array_equal(bt.positions.numpy(), g["positions"])
        assert bt.super_edge_index.is_contiguous() and bt._sizes == sizes and bt._triples
    loader = DataLoaderAtomTriple(mols, batch_size=3, shuffle=False)
    first = next(iter(loader))
    assert isinstance(first, BatchAtomTriple) and first.num_graphs == 3
    assert list(inspect.signature(AtomTripleExtractor.__init__).parameters) == ["self", "ratio"]
    assert list(inspect.signature(DataLoaderAtomTriple.__init__).parameters)[:4] == ["self", "dataset", "batch_size",
                                                                                     "shuffle"]


def test_torsion_predictor_matches_the_reference():
    from geossl_amd.pretrain_TorsionAnglePrediction import TorsionAnglePredictor, do_TorsionAnglePrediction
    for emb in (48, 128):
        torch.manual_seed(3)
        ours = TorsionAnglePredictor(emb)
        sd = ours.state_dict()
        assert list(sd) == ["predictor.weight", "predictor.bias"]
        assert tuple(sd["predictor.weight"].shape) == (1, 3 * emb) and tuple(sd["predictor.bias"].shape) == (1,)
        assert type(ours.criterion) is torch.nn.MSELoss and ours.criterion.reduction == "mean"
        torch.manual_seed(3)
        lin = torch.nn.Linear(3 * emb, 1)   # the reference's init: nn.Linear(emb_dim*3, 1) drawn first
        assert torch.equal(sd["predictor.weight"], lin.weight.detach()) and torch.equal(sd["predictor.bias"],
                                                                                        lin.bias.detach())
        u, v, w, a = torch.randn(5, emb), torch.randn(5, emb), torch.randn(5, emb), torch.rand(5)
        assert torch.equal(ours(u, v, w, a), torch.nn.MSELoss()(lin(torch.cat([u, v, w], 1)).squeeze(), a))
    assert list(inspect.signature(TorsionAnglePredictor.forward).parameters) == [
        "self", "u_node_repr", "v_node_repr", "w_node_repr", "torsion_angle_actual"]
    assert list(inspect.signature(do_TorsionAnglePrediction).parameters)[:4] == ["args", "batch", "model",
                                                                                 "torsion_angle_predictor"]


def test_trainer_op_and_bucket_surface():
    from geossl_amd import bucket as bk, build, ops
    from geossl_amd.pretrain_TorsionAnglePrediction import TorsionAnglePredictionTrainer
    sig = inspect.signature(TorsionAnglePredictionTrainer)
    for p in ("model", "torsion_angle_predictor", "lr", "weight_decay", "model_3d", "use_graph", "max_graphs",
              "graph_mode"):
        assert p in sig.parameters, p
    assert list(inspect.signature(ops.torsion_head).parameters)[:5] == ["h", "W", "b", "triples", "angle"]
    assert "dyn" in inspect.signature(ops.torsion_head).parameters
    assert list(inspect.signature(ops.triple_angles).parameters) == ["positions", "super_edge_index"]
    assert [F for F in (32, 48, 64, 96, 128, 256, 512, 1024) if ops.torsion_head_width_ok(F)] == [64, 128, 256, 512]
    assert build.SOURCE_FLAGS["torsion_head.hip"] == ["-fno-slp-vectorize"]
    # a "triples" bucket enumerates no pair tuples: no super-edges, empty incidence lists; the rest as for the pair options
    n = np.array([5, 18, 2, 9, 33, 1, 12])
    tri, perm = bk.host_plan(n, "triples", views=1), bk.host_plan(n, "permutation", views=1)
    assert tri["counts"][:3] == (80, 794, 0) and perm["counts"][:3] == (80, 794, 1588)
    assert not tri["se_ptr"].any() and not tri["inc_ptr"].any()
    for k in ("mol_ptr2", "pair_ptr2", "work"):
        assert np.array_equal(tri[k], perm[k]), k
    assert bk.triple_capacity(301, 5) >= 301 and bk.triple_capacity(5000, 5, prev=2048) >= 5000


def test_new_abi_symbols_declared_bound_and_exported():
    from geossl_amd import _lib
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in NEW_SYMBOLS + ("geossl_torsion_head_width_ok",):
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    for name in ("geossl_torsion_head_fwd_workspace_floats", "geossl_torsion_head_bwd_workspace_floats"):
        assert re.search(r"\bint64_t %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
