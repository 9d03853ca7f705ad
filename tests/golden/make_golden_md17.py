#!/usr/bin/env python3
"""Generate fixture G22 (training on forces at the reference's own MD17 configuration) by running the UNMODIFIED
reference on CPU.

Run in the build container only:  python tests/golden/make_golden_md17.py
The statements of train()'s loop from `batch_data = batch_data.to(device)` to `loss.backward()`
(examples/finetune_md17.py:31-53; `optimizer.step()` and what follows are left out) are AST-extracted and executed
verbatim with the names they read injected (`args` with the config.py defaults, `model`, `graph_pred_linear`,
`criterion` = L1Loss as :232 builds it, `optimizer` = the stock Adam of :233-238, `grad`, `device` = cpu, `batch_data`).
The backbones are the reference's own SchNet (the MD17 defaults of config.py:111-115: 128 / 128 / 6 / 51, 10 A, mean,
node_class 9, head Linear(128, 1) as :211) and PaiNN (128, 3 interactions, n_rbf 20, 5 A, add, head
create_output_layers() as :223), all with the closed-form weights of filler.py.  x is 1-D, as DatasetMD17 stores it
(datasets_MD17.py:61).

The L1 targets are drawn around the reference's own predictions (a forward pass before the loop) so that no residual
lies near zero, and the seeds are chosen so that no pair lies within 1e-4 A of the cutoff: an fp64 twin then takes the
same graph and the same signs.
Stored per case: inputs and targets, energy, force, loss, positions.grad, the head's parameters and full gradients, the
backbone's gradients as grad_summary.  Output: tests/golden/g22_md17_<case>.npz.
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
sys.path[:0] = [os.path.join(HERE, "ref_shims"), REF, os.path.join(REF, "examples"), REPO, HERE,
                os.path.join(REPO, "tests")]

from Geom3D.models import PaiNN, SchNet  # noqa: E402  (the reference's own classes)
from torch_geometric.nn import radius_graph  # noqa: E402  (shim)

from filler import fill_module_, grad_summary  # noqa: E402
from force_twin import cutoff_margin, targets_with_margin  # noqa: E402
from geossl_amd.synthetic import make_batch  # noqa: E402

torch.set_num_threads(1)   # (bit-for-bit regeneration: a multi-threaded CPU scatter sums in varying order)

ARGS = dict(model_3d="schnet", emb_dim=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0,
            readout="mean", painn_radius_cutoff=5.0, painn_n_interactions=3, painn_n_rbf=20, painn_readout="add",
            md17_energy_coeff=0.05, md17_force_coeff=0.95, lr=5e-4)
# name: (backbone, molecules, atoms per molecule, seed)
CASES = {"schnet_B1": ("schnet", 1, 21, 221), "schnet_B4": ("schnet", 4, 21, 222),
         "painn_B1": ("painn", 1, 21, 223), "painn_B4": ("painn", 4, 21, 224)}


class BatchData:
    """Duck-typed torch_geometric Batch of DatasetMD17 / DatasetMD17Radius: x (1-D), positions, batch, y, force
    [, radius_edge_index]."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to(self, device):
        return self


def extract():
    """The loop statements :31-53 of train() (from `batch_data = batch_data.to(device)` to `loss.backward()`)."""
    tree = ast.parse(open(os.path.join(REF, "examples/finetune_md17.py")).read())
    train = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "train"]
    assert len(train) == 1
    loop = [n for n in ast.walk(train[0]) if isinstance(n, ast.For)]
    assert len(loop) == 1
    body, started = [], False
    for st in loop[0].body:
        if ast.unparse(st) == "batch_data = batch_data.to(device)":
            started = True
        if started:
            body.append(st)
        if started and ast.unparse(st) == "loss.backward()":
            break
    assert started and ast.unparse(body[-1]) == "loss.backward()"
    assert not any("optimizer.step" in ast.unparse(st) for st in body)
    return compile(ast.Module(body=body, type_ignores=[]), "finetune_md17.py[train loop]", "exec")


def make_case(name, backbone, B, n, seed):
    step = extract()
    args = types.SimpleNamespace(**dict(ARGS, model_3d=backbone))
    cutoff = args.cutoff if backbone == "schnet" else args.painn_radius_cutoff
    b = make_batch(0, seed=seed, sizes=[n] * B)
    assert cutoff_margin(b["positions"], b["batch"], cutoff) >= 1e-4, name
    x = b["x"][:, 0].copy()
    if backbone == "painn":
        x[:2] = 0   # hydrogens: padding_idx row (painn.py:174)
    pos = torch.from_numpy(b["positions"])
    bvec = torch.from_numpy(b["batch"])
    if backbone == "schnet":   # :203-212
        model = SchNet(hidden_channels=args.emb_dim, num_filters=args.num_filters, num_interactions=args.num_interactions,
                       num_gaussians=args.num_gaussians, cutoff=args.cutoff, readout=args.readout, node_class=9)
        graph_pred_linear = torch.nn.Linear(args.emb_dim, 1)
        rei = None
    else:                      # :214-223
        model = PaiNN(n_atom_basis=args.emb_dim, n_interactions=args.painn_n_interactions, n_rbf=args.painn_n_rbf,
                      cutoff=args.painn_radius_cutoff, max_z=9, n_out=1, readout=args.painn_readout)
        graph_pred_linear = model.create_output_layers()
        parts = []
        for m in range(B):   # datasets_MD17.py (DatasetMD17Radius): radius_graph per molecule, then collation offsets
            sel = b["batch"] == m
            off = int(np.nonzero(sel)[0][0])
            parts.append(radius_graph(pos[sel], r=cutoff, loop=False) + off)
        rei = torch.cat(parts, dim=1)
    fill_module_(model)
    fill_module_(graph_pred_linear)
    # the targets: around the reference's own predictions (same code path, before the loop)
    p0 = pos.clone().requires_grad_(True)
    rep0 = model(torch.from_numpy(x), p0, bvec) if rei is None else model(torch.from_numpy(x), p0, rei, bvec)
    e0 = graph_pred_linear(rep0).squeeze(1)
    f0 = -torch.autograd.grad(e0, p0, torch.ones_like(e0))[0]
    y_e, y_f = targets_with_margin(e0.detach(), f0.detach(), seed)
    batch_data = BatchData(x=torch.from_numpy(x), positions=pos.clone(), batch=bvec, y=y_e, force=y_f)
    if rei is not None:
        batch_data.radius_edge_index = rei
    optimizer = torch.optim.Adam([{"params": model.parameters(), "lr": args.lr},
                                  {"params": graph_pred_linear.parameters(), "lr": args.lr}], lr=args.lr, weight_decay=0)
    ns = dict(batch_data=batch_data, model=model, graph_pred_linear=graph_pred_linear, args=args,
              criterion=torch.nn.L1Loss(), optimizer=optimizer, grad=torch.autograd.grad, device=torch.device("cpu"),
              torch=torch)
    exec(step, ns)
    loss, pred_energy, pred_force = ns["loss"], ns["pred_energy"], ns["pred_force"]
    if backbone == "schnet":
        cfg = dict(hidden_channels=args.emb_dim, num_filters=args.num_filters, num_interactions=args.num_interactions,
                   num_gaussians=args.num_gaussians, cutoff=args.cutoff, readout=args.readout, node_class=9)
    else:
        cfg = dict(n_atom_basis=args.emb_dim, n_interactions=args.painn_n_interactions, n_rbf=args.painn_n_rbf,
                   cutoff=args.painn_radius_cutoff, max_z=9, n_out=1, readout=args.painn_readout)
    meta = dict(kind=backbone, B=B, n=n, seed=seed, loss="l1", energy_coeff=args.md17_energy_coeff,
                force_coeff=args.md17_force_coeff)
    arrs = dict(x=batch_data.x, positions=pos, batch=bvec, actual_energy=y_e, actual_force=y_f, cfg=json.dumps(cfg),
                meta=json.dumps(meta), energy=pred_energy.detach(), force=pred_force.detach(), loss=loss.detach(),
                grad_pos=batch_data.positions.grad)
    if rei is not None:
        arrs["radius_edge_index"] = rei
    for pname, p in graph_pred_linear.named_parameters():
        arrs["head_grad/" + pname] = p.grad
    seen = set()
    for pname, p in model.named_parameters():
        if p.grad is None or id(p) in seen:
            continue
        seen.add(id(p))
        arrs["gsum/" + pname] = grad_summary(p.grad)
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(HERE, "g22_md17_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote %-28s %7.1f KB  loss %.6f" % (os.path.basename(path), os.path.getsize(path) / 1024, float(loss.detach())))


if __name__ == "__main__":
    for name, case in CASES.items():
        make_case(name, *case)
