#!/usr/bin/env python3
"""Generate fixture G21 (Supervised pretraining / property fine-tuning) by running the UNMODIFIED reference on CPU.

Run in the build container only:  python tests/golden/make_golden_supervised.py
`model_setup` (examples/pretrain_Supervised.py:19-65) and the statements of the training loop from
`batch = batch.to(device)` to `loss = criterion(pred, y)` (:80-101) are AST-extracted and executed verbatim with the names
they read injected (`args`, `node_class` = 9, `intermediate_dim` = emb_dim, `num_tasks` = 1, `model`,
`graph_pred_linear`, `TRAIN_mean`, `TRAIN_std`, `task_id`, `criterion` from args.loss as :199-204 picks it, `device` =
cpu, `batch`).  The backbones are the reference's own SchNet / PaiNN and the heads the ones model_setup builds
(Linear(emb_dim, 1) / PaiNN.create_output_layers()), all with the closed-form weights of filler.py.

Stored per case: the batch (ragged, with a 1-atom molecule), y with T > 1 columns, task_id, TRAIN_mean / TRAIN_std (the
column's mean and std over the batch, as :185-188 computes them over the dataset), the backbone's molecule_3D_repr and
its gradient, pred (normalised), the loss, the head's parameters and full gradients, and the backbone's gradients
(grad_summary; full tensors for the reduced SchNet).
Output: tests/golden/g21_supervised_<case>.npz.
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

BASE = dict(model_3d="schnet", emb_dim=64, num_filters=64, num_interactions=2, num_gaussians=8, cutoff=5.0,
            readout="mean", painn_n_interactions=3, painn_n_rbf=20, painn_radius_cutoff=5.0, painn_readout="add",
            loss="mae")
RAGGED = [5, 18, 2, 9, 33, 1, 12]
# name: (args overrides, sizes, T, task_id, seed)
CASES = {
    "schnet_reduced_mean_mae": (dict(), RAGGED, 8, 6, 81),
    "schnet_reduced_add_mse": (dict(readout="add", loss="mse"), RAGGED, 8, 3, 82),
    "schnet_full_mae": (dict(emb_dim=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0),
                        [18, 18, 1, 12, 25, 7], 12, 6, 83),
    "painn_mae": (dict(model_3d="painn", emb_dim=128), [18, 9, 1, 27, 2, 14], 8, 6, 84),
    "painn_mse": (dict(model_3d="painn", emb_dim=128, loss="mse"), [7, 1, 20, 3, 11], 8, 2, 85),
}


class Batch:
    """Duck-typed torch_geometric Batch of Molecule3DDataset / MoleculeDataset3DRadius (x, positions, batch, y)."""

    def __init__(self, d):
        for k, v in d.items():
            if k in ("x", "positions", "batch"):
                setattr(self, k, torch.from_numpy(np.ascontiguousarray(v)))

    def to(self, device):
        return self


def extract():
    """model_setup and the loop statements :80-101 (ending with `loss = criterion(pred, y)`)."""
    tree = ast.parse(open(os.path.join(REF, "examples/pretrain_Supervised.py")).read())
    setup = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "model_setup"]
    train = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "train"]
    assert len(setup) == 1 and len(train) == 1
    loop = [n for n in ast.walk(train[0]) if isinstance(n, ast.For)]
    assert len(loop) == 1
    body, started = [], False
    for st in loop[0].body:
        if isinstance(st, ast.Assign) and ast.unparse(st) == "batch = batch.to(device)":
            started = True
        if started:
            body.append(st)
        if started and isinstance(st, ast.Assign) and ast.unparse(st) == "loss = criterion(pred, y)":
            break
    assert started and ast.unparse(body[-1]) == "loss = criterion(pred, y)"
    setup_code = compile(ast.Module(body=setup, type_ignores=[]), "pretrain_Supervised.py[model_setup]", "exec")
    step = compile(ast.Module(body=body, type_ignores=[]), "pretrain_Supervised.py[loop]", "exec")
    return setup_code, step


def criterion_of(loss):
    """:199-204."""
    if loss == "mse":
        return torch.nn.MSELoss()
    if loss == "mae":
        return torch.nn.L1Loss()
    raise ValueError(loss)


def make_case(name, over, sizes, T, task_id, seed):
    setup_code, step = extract()
    args = types.SimpleNamespace(**dict(BASE, **over))
    b = make_batch(0, seed=seed, sizes=sizes, option="combination")
    if args.model_3d == "painn":
        b["x"][:3, 0] = 0   # hydrogens: padding_idx row (painn.py:174)
    batch = Batch(b)
    if args.model_3d == "painn":
        rei = []
        for m in range(len(sizes)):
            sel = b["batch"] == m
            off = int(np.nonzero(sel)[0][0])
            rei.append(radius_graph(torch.from_numpy(b["positions"][sel]), r=args.painn_radius_cutoff, loop=False) + off)
        batch.radius_edge_index = torch.cat(rei, dim=1)
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((len(sizes), T)) * np.linspace(0.5, 3.0, T) + np.linspace(-4.0, 4.0, T)).astype(np.float32)
    batch.y = torch.from_numpy(y.reshape(-1))   # (PyG collation of 1-D per-molecule rows: concatenated)
    col = torch.from_numpy(y[:, task_id])
    TRAIN_mean, TRAIN_std = col.mean().item(), col.std().item()
    ns = {"torch": torch, "SchNet": SchNet, "PaiNN": PaiNN, "DimeNetPlusPlus": None, "args": args, "node_class": 9,
          "intermediate_dim": args.emb_dim, "num_tasks": 1}
    exec(setup_code, ns)
    model, graph_pred_linear = ns["model_setup"]()
    fill_module_(model)
    fill_module_(graph_pred_linear)
    captured = {}
    orig_forward = type(model).forward

    def forward(self, *a, **k):   # (the backbone's output, for its retained gradient)
        out = orig_forward(self, *a, **k)
        out.retain_grad()
        captured["repr"] = out
        return out
    model.forward = types.MethodType(forward, model)
    ns = dict(batch=batch, model=model, graph_pred_linear=graph_pred_linear, TRAIN_mean=TRAIN_mean,
              TRAIN_std=TRAIN_std, task_id=task_id, criterion=criterion_of(args.loss), device=torch.device("cpu"),
              args=args, torch=torch)
    exec(step, ns)
    loss, pred = ns["loss"], ns["pred"]
    loss.backward()
    rep = captured["repr"]
    meta = dict(kind=args.model_3d, emb_dim=args.emb_dim, seed=seed, loss=args.loss, T=T,
                readout=args.readout if args.model_3d == "schnet" else args.painn_readout)
    if args.model_3d == "schnet":
        cfg = dict(hidden_channels=args.emb_dim, num_filters=args.num_filters, num_interactions=args.num_interactions,
                   num_gaussians=args.num_gaussians, cutoff=args.cutoff, readout=args.readout, node_class=9)
    else:
        cfg = dict(n_atom_basis=args.emb_dim, n_interactions=args.painn_n_interactions, n_rbf=args.painn_n_rbf,
                   cutoff=args.painn_radius_cutoff, max_z=9, n_out=1, readout=args.painn_readout)
    arrs = dict(x=batch.x, positions=batch.positions, batch=batch.batch, sizes=np.asarray(sizes, dtype=np.int64),
                y=batch.y, task_id=np.int64(task_id), TRAIN_mean=np.float64(TRAIN_mean),
                TRAIN_std=np.float64(TRAIN_std), cfg=json.dumps(cfg), meta=json.dumps(meta), loss=loss.detach(),
                pred=pred.detach(), molecule_repr=rep.detach(), grad_molecule_repr=rep.grad)
    if args.model_3d == "painn":
        arrs["radius_edge_index"] = batch.radius_edge_index
    for pname, p in graph_pred_linear.named_parameters():
        arrs["head/" + pname] = p.detach()
        arrs["head_grad/" + pname] = p.grad
    full = args.model_3d == "schnet" and args.emb_dim == 64
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
    path = os.path.join(HERE, "g21_supervised_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote %-44s %7.1f KB  loss %.6f" % (os.path.basename(path), os.path.getsize(path) / 1024, float(loss.detach())))


if __name__ == "__main__":
    for name, case in CASES.items():
        make_case(name, *case)
