#!/usr/bin/env python3
"""Generate fixture G18 (Distance Prediction pretraining) by running the UNMODIFIED reference on CPU.

Run in the build container only:  python tests/golden/make_golden_distance.py
`DistancePredictor` (examples/pretrain_DistancePrediction.py:15-25) and the statements of the training loop from
`batch = batch.to(device)` to `distance_loss = distance_predictor(...)` (:66-79) are AST-extracted and executed verbatim
with the names they read injected (`molecule_model_3D`, `distance_predictor`, `args`, `device` = cpu, `batch`).  The
backbones are the reference's own SchNet / PaiNN and the predictor the reference class, all with the closed-form weights
of filler.py.  Super-edges: the reference's AtomTupleExtractor applied per molecule; for ratio < 1 its np.random.choice
stream is seeded and the sampled tuples are stored.

Stored per case: the batch, distance_actual, the prediction, the loss, the gradient of node_repr, the predictor's
gradients, and the backbone's gradients (full tensors for the reduced SchNet, grad_summary otherwise).
Output: tests/golden/g18_distance_<case>.npz.
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

from Geom3D.dataloaders.dataloaders_AtomTuple import AtomTupleExtractor  # noqa: E402  (the reference's own classes)
from Geom3D.models import PaiNN, SchNet  # noqa: E402
from torch_geometric.nn import radius_graph  # noqa: E402  (shim)

from filler import fill_module_, grad_summary  # noqa: E402
from geossl_amd.synthetic import make_batch  # noqa: E402

torch.set_num_threads(4)

SCHNET_REDUCED = dict(hidden_channels=64, num_filters=64, num_interactions=2, num_gaussians=8, cutoff=5.0, node_class=9,
                      readout="mean")
SCHNET_FULL = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0, node_class=9,
                   readout="mean")
PAINN = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")

RAGGED = [5, 18, 2, 9, 33, 1, 12]
# name: (backbone, cfg, emb_dim, sizes, option, ratio, seed)
CASES = {
    "schnet_reduced_perm": ("schnet", SCHNET_REDUCED, 64, RAGGED, "permutation", 1, 51),
    "schnet_full_comb": ("schnet", SCHNET_FULL, 128, [18, 18, 18, 12, 25, 1], "combination", 1, 52),
    "painn_perm": ("painn", PAINN, 128, [18, 9, 27, 2, 14], "permutation", 1, 53),
    "schnet_reduced_ratio": ("schnet", SCHNET_REDUCED, 64, RAGGED, "permutation", 0.3, 54),
    "schnet_reduced_B1_n2": ("schnet", SCHNET_REDUCED, 64, [2], "combination", 1, 55),
}


class Batch:
    """Duck-typed BatchAtomTuple (dataloaders_AtomTuple.py:40-78)."""

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
    """DistancePredictor and the loop statements :66-79 (ending with the `distance_loss = ...` assignment)."""
    tree = ast.parse(open(os.path.join(REF, "examples/pretrain_DistancePrediction.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "DistancePredictor"]
    train = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "train"]
    assert len(cls) == 1 and len(train) == 1
    loop = [n for n in ast.walk(train[0]) if isinstance(n, ast.For)]
    assert len(loop) == 1
    body = []
    for st in loop[0].body:
        body.append(st)
        if isinstance(st, ast.Assign) and getattr(st.targets[0], "id", None) == "distance_loss":
            break
    assert getattr(body[-1].targets[0], "id", None) == "distance_loss"
    ns = {"torch": torch, "nn": torch.nn}
    exec(compile(ast.Module(body=cls, type_ignores=[]), "pretrain_DistancePrediction.py[class]", "exec"), ns)
    step = compile(ast.Module(body=body, type_ignores=[]), "pretrain_DistancePrediction.py[loop]", "exec")
    return ns, step


def super_edges(sizes, option, ratio, seed):
    """The reference extractor per molecule (np.random.choice stream seeded once), collated with node offsets
    (dataloaders_AtomTuple.py:64-65)."""
    np.random.seed(seed)
    ext = AtomTupleExtractor(ratio=ratio, option=option)
    se, off = [], 0
    for n in sizes:
        d = ext(types.SimpleNamespace(x=np.zeros((n, 1))))
        se.append(d.super_edge_index.numpy() + off)
        off += n
    return np.concatenate(se, axis=1).astype(np.int64)


def make_case(name, kind, cfg, emb_dim, sizes, option, ratio, seed):
    cls_ns, step = extract()
    b = make_batch(0, seed=seed, sizes=sizes, option=option)
    b["super_edge_index"] = super_edges(sizes, option, ratio, seed)
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
    predictor = fill_module_(cls_ns["DistancePredictor"](emb_dim))
    ns = dict(cls_ns, batch=batch, molecule_model_3D=model, distance_predictor=predictor, device=torch.device("cpu"),
              args=types.SimpleNamespace(model_3d=kind), distance_loss_accum=0)
    exec(step, ns)
    node_repr, loss = ns["node_repr"], ns["distance_loss"]
    node_repr.retain_grad()
    with torch.no_grad():
        pred = predictor.predictor(torch.cat([ns["u_node_repr"], ns["v_node_repr"]], dim=1)).squeeze()
    loss.backward()
    meta = dict(kind=kind, option=option, ratio=ratio, emb_dim=emb_dim)
    S = b["super_edge_index"].shape[1]
    arrs = dict(x=batch.x, positions=batch.positions, batch=batch.batch, super_edge_index=batch.super_edge_index,
                sizes=np.asarray(sizes, dtype=np.int64), cfg=json.dumps(cfg), meta=json.dumps(meta), loss=loss.detach(),
                distance_actual=ns["distance_actual"], pred=pred.reshape(S), node_repr=node_repr.detach(),
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
    path = os.path.join(HERE, "g18_distance_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote %-40s %7.1f KB  S %5d  loss %.6f" % (os.path.basename(path), os.path.getsize(path) / 1024, S,
                                                    float(loss.detach())))


if __name__ == "__main__":
    for name, case in CASES.items():
        make_case(name, *case)
