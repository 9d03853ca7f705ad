#!/usr/bin/env python3
"""Generate fixture G19 (Charge Prediction pretraining) by running the UNMODIFIED reference on CPU.

Run in the build container only:  python tests/golden/make_golden_charge.py
`ChargePredictor` (examples/pretrain_ChargePrediction.py:15-25) and the statements of the training loop from
`batch = batch.to(device)` to `charge_loss = charge_predictor(...)` (:62-81) are AST-extracted and executed verbatim with
the names they read injected (`molecule_model_3D`, `charge_predictor`, `args`, `device` = cpu, `batch`, `node_class`).
The backbones are the reference's own SchNet / PaiNN and the predictor the reference class, all with the closed-form
weights of filler.py; np.random is seeded before the step, so its np.random.choice draws the stored masked_index.

Stored per case: the batch (x before the step, and after it: the loop writes the mask token into batch.x[:, 0]), the
seed, masked_index, charge_actual, the logits of the masked rows, the loss, the gradient of node_repr, the predictor's
gradients, and the backbone's gradients (full tensors for the reduced SchNet, grad_summary otherwise).
Output: tests/golden/g19_charge_<case>.npz.
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

from Geom3D.models import PaiNN, SchNet  # noqa: E402  (the reference's own classes)
from torch_geometric.nn import radius_graph  # noqa: E402  (shim)

from filler import fill_module_, grad_summary  # noqa: E402
from geossl_amd.synthetic import make_batch  # noqa: E402

torch.set_num_threads(4)

NODE_CLASS = 9   # :106
SCHNET_REDUCED = dict(hidden_channels=64, num_filters=64, num_interactions=2, num_gaussians=8, cutoff=5.0, node_class=9,
                      readout="mean")
SCHNET_FULL = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0, node_class=9,
                   readout="mean")
PAINN = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")

RAGGED = [5, 18, 2, 9, 33, 1, 12]
# name: (backbone, cfg, emb_dim, sizes, ratio, seed)
CASES = {
    "schnet_reduced_r03": ("schnet", SCHNET_REDUCED, 64, RAGGED, 0.3, 61),
    "schnet_full_r03": ("schnet", SCHNET_FULL, 128, [18, 18, 18, 12, 25, 1], 0.3, 62),
    "painn_r03": ("painn", PAINN, 128, [18, 9, 27, 2, 14], 0.3, 63),
    "schnet_reduced_r05": ("schnet", SCHNET_REDUCED, 64, RAGGED, 0.5, 64),
    "schnet_reduced_B1_n3": ("schnet", SCHNET_REDUCED, 64, [3], 0.3, 65),
}


class Batch:
    """Duck-typed torch_geometric Batch of Molecule3DDataset / MoleculeDataset3DRadius (x, positions, batch)."""

    def __init__(self, d):
        for k, v in d.items():
            if k in ("x", "positions", "batch"):
                setattr(self, k, torch.from_numpy(np.ascontiguousarray(v)))

    def to(self, device):
        return self


def extract():
    """ChargePredictor and the loop statements :62-81 (ending with the `charge_loss = ...` assignment)."""
    tree = ast.parse(open(os.path.join(REF, "examples/pretrain_ChargePrediction.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ChargePredictor"]
    train = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "train"]
    assert len(cls) == 1 and len(train) == 1
    loop = [n for n in ast.walk(train[0]) if isinstance(n, ast.For)]
    assert len(loop) == 1
    body = []
    for st in loop[0].body:
        body.append(st)
        if isinstance(st, ast.Assign) and getattr(st.targets[0], "id", None) == "charge_loss":
            break
    assert getattr(body[-1].targets[0], "id", None) == "charge_loss"
    ns = {"torch": torch, "nn": torch.nn, "np": np, "node_class": NODE_CLASS}
    exec(compile(ast.Module(body=cls, type_ignores=[]), "pretrain_ChargePrediction.py[class]", "exec"), ns)
    step = compile(ast.Module(body=body, type_ignores=[]), "pretrain_ChargePrediction.py[loop]", "exec")
    return ns, step


def make_case(name, kind, cfg, emb_dim, sizes, ratio, seed):
    cls_ns, step = extract()
    b = make_batch(0, seed=seed, sizes=sizes, option="combination")
    if kind == "painn":
        b["x"][:3, 0] = 0   # hydrogens: padding_idx row (painn.py:174)
    b["x"][-1, 0] = NODE_CLASS - 1   # a real atom of the mask token's type
    x_before = b["x"].copy()
    batch = Batch(b)
    if kind == "painn":
        rei = []
        for m in range(len(sizes)):
            sel = b["batch"] == m
            off = int(np.nonzero(sel)[0][0])
            rei.append(radius_graph(torch.from_numpy(b["positions"][sel]), r=cfg["cutoff"], loop=False) + off)
        batch.radius_edge_index = torch.cat(rei, dim=1)
    model = fill_module_(SchNet(**cfg) if kind == "schnet" else PaiNN(**cfg))
    predictor = fill_module_(cls_ns["ChargePredictor"](emb_dim))
    ns = dict(cls_ns, batch=batch, molecule_model_3D=model, charge_predictor=predictor, device=torch.device("cpu"),
              args=types.SimpleNamespace(model_3d=kind, charge_masking_ratio=ratio), charge_loss_accum=0)
    np.random.seed(seed)
    exec(step, ns)
    node_repr, loss, masked_index = ns["node_repr"], ns["charge_loss"], ns["masked_index"]
    node_repr.retain_grad()
    with torch.no_grad():
        logits = predictor.predictor(node_repr[masked_index])
    loss.backward()
    meta = dict(kind=kind, ratio=ratio, emb_dim=emb_dim, seed=seed, node_class=NODE_CLASS)
    lin = predictor.predictor
    grad = lambda p: p.grad if p.grad is not None else torch.zeros_like(p)   # (k = 0: no gradient reaches them)
    arrs = dict(x=x_before, x_after=batch.x, positions=batch.positions, batch=batch.batch,
                sizes=np.asarray(sizes, dtype=np.int64), cfg=json.dumps(cfg), meta=json.dumps(meta), loss=loss.detach(),
                masked_index=np.asarray(masked_index, dtype=np.int64), charge_actual=ns["charge_actual"],
                logits=logits, node_repr=node_repr.detach(), grad_node_repr=grad(node_repr),
                pred_weight=lin.weight.detach(), pred_bias=lin.bias.detach(), grad_pred_weight=grad(lin.weight),
                grad_pred_bias=grad(lin.bias))
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
    path = os.path.join(HERE, "g19_charge_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote %-40s %7.1f KB  k %4d  loss %.6f" % (os.path.basename(path), os.path.getsize(path) / 1024,
                                                   len(masked_index), float(loss.detach())))


if __name__ == "__main__":
    for name, case in CASES.items():
        make_case(name, *case)
