#!/usr/bin/env python3
"""Generate fixture G20 (3D InfoGraph pretraining) by running the UNMODIFIED reference on CPU.

Run in the build container only:  python tests/golden/make_golden_infograph.py
`Discriminator` and `do_InfoGraph` (examples/pretrain_3DInfoGraph.py:19-31,56-76), `cycle_index` (examples/util.py:19-22)
and the statements of the training loop from `batch = batch.to(device)` to `loss = CL_loss` (:92-108) are AST-extracted
and executed verbatim with the names they read injected (`molecule_model_3D`, `infograph_discriminator_SSL_model`,
`criterion` = nn.BCEWithLogitsLoss(), `args`, `device` = cpu, `batch`, and PyG's `uniform` restated: the import of
torch_geometric.nn.inits is not executed).  The backbones are the reference's own SchNet / PaiNN and the discriminator
the reference class, all with the closed-form weights of filler.py.

Stored per case: the batch, the loss and acc, the positive / negative scores, node_repr and molecule_repr with their
gradients (node_repr's through the readout as well: its retained .grad), the discriminator's weight and gradient, and the
backbone's gradients (full tensors for the reduced SchNet, grad_summary otherwise).
Output: tests/golden/g20_infograph_<case>.npz.
"""
import ast
import json
import math
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

SCHNET_REDUCED = dict(hidden_channels=64, num_filters=64, num_interactions=2, num_gaussians=8, cutoff=5.0, node_class=9,
                      readout="mean")
SCHNET_REDUCED_ADD = dict(SCHNET_REDUCED, readout="add")
SCHNET_FULL = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0, node_class=9,
                   readout="mean")
PAINN = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")

RAGGED = [5, 18, 2, 9, 33, 1, 12]
# name: (backbone, cfg, emb_dim, sizes, seed)
CASES = {
    "schnet_reduced": ("schnet", SCHNET_REDUCED, 64, RAGGED, 71),
    "schnet_full": ("schnet", SCHNET_FULL, 128, [18, 18, 18, 12, 25, 1], 72),
    "painn": ("painn", PAINN, 128, [18, 9, 27, 2, 14], 73),
    "schnet_reduced_add": ("schnet", SCHNET_REDUCED_ADD, 64, RAGGED, 74),
    "schnet_reduced_B1": ("schnet", SCHNET_REDUCED, 64, [7], 75),
}


def uniform(size, value):
    """torch_geometric.nn.inits.uniform restated."""
    if value is not None:
        bound = 1.0 / math.sqrt(size)
        value.data.uniform_(-bound, bound)


class Batch:
    """Duck-typed torch_geometric Batch of Molecule3DDataset / MoleculeDataset3DRadius (x, positions, batch)."""

    def __init__(self, d):
        for k, v in d.items():
            if k in ("x", "positions", "batch"):
                setattr(self, k, torch.from_numpy(np.ascontiguousarray(v)))

    def to(self, device):
        return self


def _defs(path, names):
    tree = ast.parse(open(os.path.join(REF, path)).read())
    got = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert sorted(n.name for n in got) == sorted(names), path
    return got, tree


def extract():
    """Discriminator, do_InfoGraph, cycle_index and the loop statements :92-108 (ending with `loss = CL_loss`)."""
    defs, tree = _defs("examples/pretrain_3DInfoGraph.py", ("Discriminator", "do_InfoGraph"))
    util, _ = _defs("examples/util.py", ("cycle_index",))
    train = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "train"]
    assert len(train) == 1
    loop = [n for n in ast.walk(train[0]) if isinstance(n, ast.For)]
    assert len(loop) == 1
    body, started = [], False
    for st in loop[0].body:
        if isinstance(st, ast.Assign) and ast.unparse(st) == "batch = batch.to(device)":
            started = True
        if started:
            body.append(st)
        if started and isinstance(st, ast.Assign) and ast.unparse(st) == "loss = CL_loss":
            break
    assert started and ast.unparse(body[-1]) == "loss = CL_loss"
    ns = {"torch": torch, "nn": torch.nn, "np": np, "uniform": uniform}
    exec(compile(ast.Module(body=util, type_ignores=[]), "util.py[cycle_index]", "exec"), ns)
    exec(compile(ast.Module(body=defs, type_ignores=[]), "pretrain_3DInfoGraph.py[defs]", "exec"), ns)
    step = compile(ast.Module(body=body, type_ignores=[]), "pretrain_3DInfoGraph.py[loop]", "exec")
    return ns, step


def make_case(name, kind, cfg, emb_dim, sizes, seed):
    defs_ns, step = extract()
    b = make_batch(0, seed=seed, sizes=sizes, option="combination")
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
    torch.manual_seed(seed)
    disc = defs_ns["Discriminator"](emb_dim)
    init_weight = disc.weight.detach().clone()   # (the reference's init draw, for the bound check)
    fill_module_(disc)
    ns = dict(defs_ns, batch=batch, molecule_model_3D=model, infograph_discriminator_SSL_model=disc,
              criterion=torch.nn.BCEWithLogitsLoss(), device=torch.device("cpu"),
              args=types.SimpleNamespace(model_3d=kind), CL_loss_accum=0, CL_acc_accum=0)
    exec(step, ns)
    node_repr, molecule_repr, loss = ns["node_repr"], ns["molecule_repr"], ns["loss"]
    node_repr.retain_grad()
    molecule_repr.retain_grad()
    with torch.no_grad():
        summary = torch.sigmoid(molecule_repr)
        pos = disc(node_repr, summary[batch.batch])
        neg = disc(node_repr, summary[defs_ns["cycle_index"](len(summary), 1)][batch.batch])
    loss.backward()
    meta = dict(kind=kind, emb_dim=emb_dim, seed=seed, readout=cfg["readout"])
    arrs = dict(x=batch.x, positions=batch.positions, batch=batch.batch, sizes=np.asarray(sizes, dtype=np.int64),
                cfg=json.dumps(cfg), meta=json.dumps(meta), loss=loss.detach(), acc=np.float64(ns["CL_acc"]),
                pos_score=pos, neg_score=neg, node_repr=node_repr.detach(), molecule_repr=molecule_repr.detach(),
                grad_node_repr=node_repr.grad, grad_molecule_repr=molecule_repr.grad, disc_weight=disc.weight.detach(),
                grad_disc_weight=disc.weight.grad, disc_init_weight=init_weight)
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
    path = os.path.join(HERE, "g20_infograph_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote %-40s %7.1f KB  loss %.6f  acc %.6f" % (os.path.basename(path), os.path.getsize(path) / 1024,
                                                       float(loss.detach()), ns["CL_acc"]))


if __name__ == "__main__":
    for name, case in CASES.items():
        make_case(name, *case)
