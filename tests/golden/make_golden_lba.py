#!/usr/bin/env python3
"""Generate fixture G24 (LBA fine-tuning on pocket-sized structures) by running the UNMODIFIED reference on CPU.

Run in the build container only:  python tests/golden/make_golden_lba.py
The statements of `train()`'s loop in examples/finetune_lba.py from `batch = batch.to(device)` to
`loss = criterion(pred, actual)` (:34-47) are AST-extracted and executed verbatim with the names they read injected
(`args`, `model`, `graph_pred_linear`, `criterion` = nn.MSELoss() as :263 sets it, `device` = cpu, `batch`); `eval()`
(:67-101, with its metric lines: the RMSE, np.corrcoef and scipy's spearmanr) is extracted whole and called on a loader
of that one batch.  The backbones are the reference's own SchNet / PaiNN built as :203-224 build them (node_class = 9,
num_tasks = 1), the heads Linear(emb_dim, 1) / PaiNN.create_output_layers(), all with the closed-form weights of
filler.py.

The structures are those of tests/lba_structures.py (rejection sampling at pocket density; the first seed that keeps
every pair 1e-4 A away from the cutoff - asserted here); batch.x is the 1-D atomic number, as DatasetLBA's is.

Stored per case: the batch and y, pred and the loss, the head's parameters and full gradients, the backbone's gradients
(grad_summary), and eval()'s RMSE, Pearson and Spearman of pred against y.
Output: tests/golden/g24_lba_<case>.npz.
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
sys.path[:0] = [os.path.join(HERE, "ref_shims"), REF, os.path.join(REF, "examples"), REPO, HERE, os.path.join(REPO, "tests")]

import torch.nn.functional as F  # noqa: E402
from Geom3D.models import PaiNN, SchNet  # noqa: E402  (the reference's own classes)
from scipy.stats import spearmanr  # noqa: E402
from torch_geometric.nn import radius_graph  # noqa: E402  (shim)

import lba_structures as ls  # noqa: E402
from filler import fill_module_, grad_summary  # noqa: E402

torch.set_num_threads(4)

BASE = dict(model_3d="schnet", emb_dim=64, num_filters=64, num_interactions=2, num_gaussians=8, cutoff=5.0,
            readout="mean", painn_n_interactions=3, painn_n_rbf=20, painn_radius_cutoff=5.0, painn_readout="add")
# name: (args overrides, sizes).  schnet_reduced reads out with "add": with the filler's weights the MEAN readout of three
# pockets of one density gives three predictions within 1.3e-3 of each other, and the Pearson correlation of such a column
# moves by 4e-3 for a relative error of 1e-6 in the predictions - a metric no fp32 path could be held to.  The sum over
# 300 / 7 / 257 atoms spreads them; schnet_full keeps the script's default readout (two structures: Pearson is +-1).
CASES = {
    "schnet_reduced": (dict(readout="add"), (300, 7, 257)),
    "schnet_full": (dict(emb_dim=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0), (260, 40)),
    "painn": (dict(model_3d="painn", emb_dim=128), (300, 7, 257)),
}


class Batch:
    """Duck-typed torch_geometric Batch of DatasetLBA / DatasetLBARadius (x, positions, batch, y)."""

    def __init__(self, d):
        for k in ("x", "positions", "batch"):
            setattr(self, k, torch.from_numpy(np.ascontiguousarray(d[k])))

    def to(self, device):
        return self


def extract():
    """The loop statements :34-47 (ending with `loss = criterion(pred, actual)`) and eval() whole."""
    tree = ast.parse(open(os.path.join(REF, "examples/finetune_lba.py")).read())
    train = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "train"]
    ev = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "eval"]
    assert len(train) == 1 and len(ev) == 1
    loop = [n for n in ast.walk(train[0]) if isinstance(n, ast.For)]
    assert len(loop) == 1
    body, started = [], False
    for st in loop[0].body:
        if isinstance(st, ast.Assign) and ast.unparse(st) == "batch = batch.to(device)":
            started = True
        if started:
            body.append(st)
        if started and isinstance(st, ast.Assign) and ast.unparse(st) == "loss = criterion(pred, actual)":
            break
    assert started and ast.unparse(body[-1]) == "loss = criterion(pred, actual)"
    metrics = [ast.unparse(n) for n in ast.walk(ev[0]) if isinstance(n, ast.Assign)]
    assert "pearson_corr = np.corrcoef(y_true, y_pred)[0, 1]" in metrics
    assert "spearman_corr = spearmanr(y_true, y_pred)[0]" in metrics
    step = compile(ast.Module(body=body, type_ignores=[]), "finetune_lba.py[loop]", "exec")
    ev_code = compile(ast.Module(body=ev, type_ignores=[]), "finetune_lba.py[eval]", "exec")
    return step, ev_code


def make_case(name, over, sizes):
    step, ev_code = extract()
    args = types.SimpleNamespace(**dict(BASE, **over))
    cutoff = args.cutoff if args.model_3d == "schnet" else args.painn_radius_cutoff
    s = ls.checked(sizes, cutoff)
    assert s["margin"] >= ls.MARGIN, (name, s["margin"])
    batch = Batch(s)
    if args.model_3d == "painn":
        off = np.concatenate([[0], np.cumsum(sizes)])
        rei = [radius_graph(torch.from_numpy(s["positions"][off[m]:off[m + 1]]), r=cutoff, loop=False) + int(off[m])
               for m in range(len(sizes))]
        batch.radius_edge_index = torch.cat(rei, dim=1)
    rng = np.random.default_rng(2400 + len(name))
    batch.y = torch.from_numpy((rng.standard_normal(len(sizes)) * 1.5 + 6.0).astype(np.float32))
    node_class, num_tasks = 9, 1
    if args.model_3d == "schnet":      # :203-213
        cfg = dict(hidden_channels=args.emb_dim, num_filters=args.num_filters, num_interactions=args.num_interactions,
                   num_gaussians=args.num_gaussians, cutoff=args.cutoff, readout=args.readout, node_class=node_class)
        model = SchNet(**cfg)
        graph_pred_linear = torch.nn.Linear(args.emb_dim, num_tasks)
    else:                              # :214-224
        cfg = dict(n_atom_basis=args.emb_dim, n_interactions=args.painn_n_interactions, n_rbf=args.painn_n_rbf,
                   cutoff=args.painn_radius_cutoff, max_z=node_class, n_out=num_tasks, readout=args.painn_readout)
        model = PaiNN(**cfg)
        graph_pred_linear = model.create_output_layers()
    fill_module_(model)
    fill_module_(graph_pred_linear)
    ns = dict(batch=batch, model=model, graph_pred_linear=graph_pred_linear, criterion=torch.nn.MSELoss(),
              device=torch.device("cpu"), args=args, torch=torch)
    exec(step, ns)
    loss, pred = ns["loss"], ns["pred"]
    loss.backward()
    ens = dict(model=model, graph_pred_linear=graph_pred_linear, args=args, torch=torch, np=np, F=F, spearmanr=spearmanr)
    exec(ev_code, ens)
    rmse, pearson, spearman, y_true, y_pred = ens["eval"](torch.device("cpu"), [batch])
    assert np.allclose(y_pred, pred.detach().numpy(), rtol=0, atol=0)
    meta = dict(kind=args.model_3d, emb_dim=args.emb_dim, seed=s["seed"], margin=s["margin"], cutoff=cutoff)
    arrs = dict(x=batch.x, positions=batch.positions, batch=batch.batch, sizes=np.asarray(sizes, dtype=np.int64),
                y=batch.y, cfg=json.dumps(cfg), meta=json.dumps(meta), loss=loss.detach(), pred=pred.detach(),
                rmse=np.float64(rmse), pearson=np.float64(pearson), spearman=np.float64(spearman))
    if args.model_3d == "painn":
        arrs["radius_edge_index"] = batch.radius_edge_index.to(torch.int32)   # (int32 on disk: half the bytes)
    for pname, p in graph_pred_linear.named_parameters():
        arrs["head/" + pname] = p.detach()
        arrs["head_grad/" + pname] = p.grad
    seen = set()
    for pname, p in model.named_parameters():
        if p.grad is None or id(p) in seen:
            continue
        seen.add(id(p))
        arrs["gsum/" + pname] = grad_summary(p.grad)
    out = {}
    for k, v in arrs.items():
        out[k] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    path = os.path.join(HERE, "g24_lba_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote %-28s %7.1f KB  seed %d margin %.2e  loss %.6f  rmse %.6f pearson %.6f spearman %.6f"
          % (os.path.basename(path), os.path.getsize(path) / 1024, s["seed"], s["margin"], float(loss.detach()), rmse,
             pearson, spearman))


if __name__ == "__main__":
    for name, case in CASES.items():
        make_case(name, *case)
