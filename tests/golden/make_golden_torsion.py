#!/usr/bin/env python3
"""Generate fixture G23 (angle prediction on atom triples) by running the UNMODIFIED reference on CPU.

Run in the build container only:  python tests/golden/make_golden_torsion.py
`TorsionAnglePredictor` (examples/pretrain_TorsionAnglePrediction.py:16-27) and the statements of the training loop from
`batch = batch.to(device)` to `torsion_angle_loss = torsion_angle_predictor(...)` (:64-78) are AST-extracted and executed
verbatim with the names they read injected (`molecule_model_3D`, `torsion_angle_predictor`, `args`, `device` = cpu,
`batch`).  The backbones are the reference's own SchNet / PaiNN and the predictor the reference class, all with the
closed-form weights of filler.py.  Triples: the reference's AtomTripleExtractor applied per molecule under
np.random.seed(seed), collated with node offsets.  The reference tree has no code that fills `super_edge_angle`; the maker
computes it in float64 numpy as the angle at the middle atom, atan2(|a x b|, a . b) with a = pos_u - pos_v,
b = pos_w - pos_v, and stores it as float32: an INPUT of the fixture, independent of the library.

Stored per case: the batch, the triples, the angles, the prediction, the loss, node_repr and its gradient, the
predictor's weights and gradients, and the backbone's gradients (full tensors for the reduced SchNet, grad_summary
otherwise).  Output: tests/golden/g23_torsion_<case>.npz and g23_triple_loader.npz (the reference's AtomTripleExtractor
and BatchAtomTriple.from_data_list on their own).
"""
import ast
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path[:0] = [os.path.join(HERE, "ref_shims"), REF, os.path.join(REF, "examples"), REPO, HERE]

from Geom3D.dataloaders.dataloaders_AtomTriple import AtomTripleExtractor, BatchAtomTriple  # noqa: E402  (the reference's)
from Geom3D.models import PaiNN, SchNet  # noqa: E402
from torch_geometric.data import Data  # noqa: E402  (shim)
from torch_geometric.nn import radius_graph  # noqa: E402  (shim)

from filler import fill_module_, grad_summary  # noqa: E402
from geossl_amd.synthetic import make_batch  # noqa: E402

torch.set_num_threads(4)

SCHNET_REDUCED = dict(hidden_channels=64, num_filters=64, num_interactions=2, num_gaussians=8, cutoff=5.0, node_class=9,
                      readout="mean")
SCHNET_FULL = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0, node_class=9,
                   readout="mean")
PAINN = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")

# name: (backbone, cfg, emb_dim, sizes, ratio, seed)
CASES = {
    "schnet_reduced_full": ("schnet", SCHNET_REDUCED, 64, [5, 18, 2, 9, 12, 1, 3], 1, 61),
    "schnet_full_r03": ("schnet", SCHNET_FULL, 128, [18, 18, 18, 12, 25, 1], 0.03, 62),
    "painn_r01": ("painn", PAINN, 128, [18, 9, 27, 2, 14], 0.01, 63),
    "schnet_reduced_r001": ("schnet", SCHNET_REDUCED, 64, [33, 40, 60, 12, 18], 1e-3, 64),
    "schnet_reduced_B1_n3": ("schnet", SCHNET_REDUCED, 64, [3], 1, 65),
    "schnet_reduced_T1": ("schnet", SCHNET_REDUCED, 64, [12], 1e-3, 66),
}


class Batch:
    """Duck-typed BatchAtomTriple (dataloaders_AtomTriple.py:34-72)."""

    def __init__(self, d):
        for k, v in d.items():
            if k != "sizes":
                setattr(self, k, torch.from_numpy(np.ascontiguousarray(v)))

    def to(self, device):
        return self

    @property
    def num_graphs(self):
        return self.batch[-1].item() + 1


def extract():
    """TorsionAnglePredictor and the loop statements :64-78 (ending with the `torsion_angle_loss = ...` assignment)."""
    tree = ast.parse(open(os.path.join(REF, "examples/pretrain_TorsionAnglePrediction.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "TorsionAnglePredictor"]
    train = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "train"]
    assert len(cls) == 1 and len(train) == 1
    loop = [n for n in ast.walk(train[0]) if isinstance(n, ast.For)]
    assert len(loop) == 1
    body = []
    for st in loop[0].body:
        body.append(st)
        if isinstance(st, ast.Assign) and getattr(st.targets[0], "id", None) == "torsion_angle_loss":
            break
    assert getattr(body[-1].targets[0], "id", None) == "torsion_angle_loss"
    ns = {"torch": torch, "nn": torch.nn}
    exec(compile(ast.Module(body=cls, type_ignores=[]), "pretrain_TorsionAnglePrediction.py[class]", "exec"), ns)
    step = compile(ast.Module(body=body, type_ignores=[]), "pretrain_TorsionAnglePrediction.py[loop]", "exec")
    return ns, step


def triples(sizes, ratio, seed):
    """The reference extractor per molecule (np.random.choice stream seeded once), collated with node offsets
    (dataloaders_AtomTriple.py:58-59)."""
    np.random.seed(seed)
    ext = AtomTripleExtractor(ratio=ratio)
    se, off = [], 0
    for n in sizes:
        d = ext(types.SimpleNamespace(x=np.zeros((n, 1))))
        se.append(d.super_edge_index.numpy().reshape(3, -1) + off)
        off += n
    return np.concatenate(se, axis=1).astype(np.int64)


def angles(positions, tri):
    """The angle at the middle atom of every triple in float64, stored as float32 ([0, pi]; 0 for a zero arm)."""
    p = np.asarray(positions, dtype=np.float64)
    a, b = p[tri[0]] - p[tri[1]], p[tri[2]] - p[tri[1]]
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1)).astype(np.float32).reshape(-1)


def make_case(name, kind, cfg, emb_dim, sizes, ratio, seed):
    cls_ns, step = extract()
    b = make_batch(0, seed=seed, sizes=sizes, option="combination")
    b["super_edge_index"] = triples(sizes, ratio, seed)
    b["super_edge_angle"] = angles(b["positions"], b["super_edge_index"])
    if kind == "painn":
        b["x"][:3, 0] = 0   # hydrogens: padding_idx row (painn.py:174)
    batch = Batch(b)
    if kind == "painn":
        rei = []
        for m in range(len(sizes)):
            sel = b["batch"] == m
            off = int(np.nonzero(sel)[0][0])
            rei.append(radius_graph(torch.from_numpy(b["positions"][sel]), r=cfg["cutoff"], loop=False) + off)
        batch.radius_edge_index = torch.cat(rei, dim=1)
    model = fill_module_(SchNet(**cfg) if kind == "schnet" else PaiNN(**cfg))
    predictor = fill_module_(cls_ns["TorsionAnglePredictor"](emb_dim))
    ns = dict(cls_ns, batch=batch, molecule_model_3D=model, torsion_angle_predictor=predictor, device=torch.device("cpu"),
              args=types.SimpleNamespace(model_3d=kind), torsion_angle_loss_accum=0)
    exec(step, ns)
    node_repr, loss = ns["node_repr"], ns["torsion_angle_loss"]
    node_repr.retain_grad()
    T = b["super_edge_index"].shape[1]
    with torch.no_grad():
        feats = torch.cat([ns["u_node_repr"], ns["v_node_repr"], ns["w_node_repr"]], dim=1)
        pred = predictor.predictor(feats).squeeze()
        # the same head in float64 on the reference's node_repr: how far the fp32 reference sits from exact arithmetic
        p64 = feats.double() @ predictor.predictor.weight.double().reshape(-1) + predictor.predictor.bias.double()
        loss64 = float(((p64 - batch.super_edge_angle.double()) ** 2).mean())
    loss.backward()
    meta = dict(kind=kind, ratio=ratio, emb_dim=emb_dim, seed=seed)
    arrs = dict(x=batch.x, positions=batch.positions, batch=batch.batch, super_edge_index=batch.super_edge_index,
                super_edge_angle=batch.super_edge_angle, sizes=np.asarray(sizes, dtype=np.int64), cfg=json.dumps(cfg),
                meta=json.dumps(meta), loss=loss.detach(), pred=pred.reshape(T), node_repr=node_repr.detach(),
                grad_node_repr=node_repr.grad, pred_weight=predictor.predictor.weight.detach(),
                pred_bias=predictor.predictor.bias.detach(), grad_pred_weight=predictor.predictor.weight.grad,
                grad_pred_bias=predictor.predictor.bias.grad)
    if kind == "painn":
        arrs["radius_edge_index"] = batch.radius_edge_index
    full = kind == "schnet" and cfg["hidden_channels"] == 64
    seen = set()
    for pname, p in model.named_parameters():
        if p.grad is None or id(p) in seen:
            continue
        seen.add(id(p))
        arrs["gsum/" + pname] = grad_summary(p.grad)
        if full:
            arrs["grad/" + pname] = p.grad
    out = {}
    for k, v in arrs.items():
        out[k] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    path = os.path.join(HERE, "g23_torsion_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote %-40s %7.1f KB  T %5d  loss %.7f  rel. diff to fp64 %.0e" % (
        os.path.basename(path), os.path.getsize(path) / 1024, T, float(loss.detach()),
        abs(float(loss.detach()) - loss64) / abs(loss64)))


def make_loader():
    """The reference's AtomTripleExtractor as a per-molecule transform (ratios 1, 0.3, 1e-3; np.random seeded per ratio)
    and BatchAtomTriple.from_data_list over molecules that carry positions, radius_edge_index and super_edge_angle."""
    sizes = [1, 2, 3, 5, 12, 18, 7]
    seed = 123
    b = make_batch(0, seed=67, sizes=sizes, option="combination")
    off = np.concatenate([[0], np.cumsum(sizes)])
    out = dict(x=b["x"], positions=b["positions"], sizes=np.asarray(sizes), seed=np.asarray(seed))
    for ratio in (1, 0.3, 1e-3):
        np.random.seed(seed)
        ext = AtomTripleExtractor(ratio=ratio)
        mols = []
        for m in range(len(sizes)):
            d = Data(x=torch.from_numpy(b["x"][off[m]:off[m + 1]]),
                     positions=torch.from_numpy(b["positions"][off[m]:off[m + 1]]))
            d.radius_edge_index = radius_graph(d.positions, r=5.0, loop=False)
            d = ext(d)
            assert d.super_edge_index.dtype == torch.long and d.super_edge_index.shape[0] == 3
            d.super_edge_angle = torch.from_numpy(angles(d.positions.numpy(), d.super_edge_index.numpy().reshape(3, -1)))
            out["mol%d/%g" % (m, ratio)] = d.super_edge_index
            mols.append(d)
        bt = BatchAtomTriple.from_data_list(mols)
        tag = "%g" % ratio
        out["sei/" + tag] = bt.super_edge_index
        out["angle/" + tag] = bt.super_edge_angle
        out["batch/" + tag] = bt.batch
        out["rei/" + tag] = bt.radius_edge_index
        out["num_graphs/" + tag] = bt.num_graphs
        assert torch.equal(bt.x, torch.from_numpy(b["x"])) and torch.equal(bt.positions, torch.from_numpy(b["positions"]))
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, "g23_triple_loader.npz")
    np.savez_compressed(path, **out)
    print("wrote %-40s %7.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    make_loader()
    for name, case in CASES.items():
        make_case(name, *case)
