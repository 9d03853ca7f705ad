#!/usr/bin/env python3
"""Generate fixture G26 (MD17 evaluation at the reference's own MD17 configuration) by running the UNMODIFIED reference
on CPU.

Run in the build container only:  python tests/golden/make_golden_md17_eval.py
eval() of examples/finetune_md17.py (:70-123) is AST-extracted as a whole and executed verbatim in a namespace that
holds the globals it reads (`args` with verbose off, `model`, `graph_pred_linear`, `torch`, `grad`, `tqdm`), on a loader of
three batches of 4 frames of 21 atoms.  Backbones, heads, weights and the 1-D x are those of make_golden_md17.py (G22):
the reference's SchNet at the MD17 defaults of config.py with Linear(128, 1), and PaiNN with create_output_layers(),
closed-form weights of filler.py.  The targets are drawn around the reference's own predictions (a forward pass per batch
before eval(), the same lines), so the two errors are of the predictions' own scale; those per-batch predictions are
stored beside eval()'s two results.
Output: tests/golden/g26_md17_eval_<backbone>.npz - x, positions, batch [3, 84(, 3)], y [3, 4], force [3, 84, 3],
pred_energy [3, 4], pred_force [3, 84, 3], energy_mae, force_mae, cfg / meta as JSON (PaiNN: radius_edge_index_<k>).
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

from filler import fill_module_  # noqa: E402
from force_twin import cutoff_margin, targets_with_margin  # noqa: E402
from geossl_amd.synthetic import make_batch  # noqa: E402
from make_golden_md17 import ARGS, BatchData  # noqa: E402

torch.set_num_threads(1)   # (bit-for-bit regeneration: a multi-threaded CPU scatter sums in varying order)

B, N_ATOMS, BATCHES = 4, 21, 3
SEEDS = {"schnet": 261, "painn": 271}   # the first seeds from here on whose pairs all keep the cutoff margin


def extract():
    """eval() of finetune_md17.py, whole and unmodified, as a code object that defines it."""
    tree = ast.parse(open(os.path.join(REF, "examples/finetune_md17.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "eval"]
    assert len(fn) == 1
    src = ast.unparse(fn[0])
    assert "torch.isnan(force)" in src and "force_mae" in src
    return compile(ast.Module(body=fn, type_ignores=[]), "finetune_md17.py[eval]", "exec")


def frames(backbone, cutoff):
    out, s = [], SEEDS[backbone]
    while len(out) < BATCHES:
        b = make_batch(0, seed=s, sizes=[N_ATOMS] * B)
        s += 1
        if cutoff_margin(b["positions"], b["batch"], cutoff) >= 1e-4:
            out.append(b)
    return out


def make_case(backbone):
    args = types.SimpleNamespace(**dict(ARGS, model_3d=backbone, verbose=False))
    cutoff = args.cutoff if backbone == "schnet" else args.painn_radius_cutoff
    if backbone == "schnet":   # finetune_md17.py:203-212
        model = SchNet(hidden_channels=args.emb_dim, num_filters=args.num_filters, num_interactions=args.num_interactions,
                       num_gaussians=args.num_gaussians, cutoff=args.cutoff, readout=args.readout, node_class=9)
        graph_pred_linear = torch.nn.Linear(args.emb_dim, 1)
        cfg = dict(hidden_channels=args.emb_dim, num_filters=args.num_filters, num_interactions=args.num_interactions,
                   num_gaussians=args.num_gaussians, cutoff=args.cutoff, readout=args.readout, node_class=9)
    else:                      # :214-223
        model = PaiNN(n_atom_basis=args.emb_dim, n_interactions=args.painn_n_interactions, n_rbf=args.painn_n_rbf,
                      cutoff=args.painn_radius_cutoff, max_z=9, n_out=1, readout=args.painn_readout)
        graph_pred_linear = model.create_output_layers()
        cfg = dict(n_atom_basis=args.emb_dim, n_interactions=args.painn_n_interactions, n_rbf=args.painn_n_rbf,
                   cutoff=args.painn_radius_cutoff, max_z=9, n_out=1, readout=args.painn_readout)
    fill_module_(model)
    fill_module_(graph_pred_linear)
    loader, arrs = [], {k: [] for k in ("x", "positions", "batch", "y", "force", "pred_energy", "pred_force")}
    for k, b in enumerate(frames(backbone, cutoff)):
        x = b["x"][:, 0].copy()
        if backbone == "painn":
            x[:2] = 0   # hydrogens: padding_idx row (painn.py:174)
        pos, bvec = torch.from_numpy(b["positions"]), torch.from_numpy(b["batch"])
        rei = None
        if backbone == "painn":   # DatasetMD17Radius: radius_graph per molecule, then collation offsets
            parts = []
            for m in range(B):
                sel = b["batch"] == m
                parts.append(radius_graph(pos[sel], r=cutoff, loop=False) + int(np.nonzero(sel)[0][0]))
            rei = torch.cat(parts, dim=1)
        p0 = pos.clone().requires_grad_(True)
        rep0 = model(torch.from_numpy(x), p0, bvec) if rei is None else model(torch.from_numpy(x), p0, rei, bvec)
        e0 = graph_pred_linear(rep0).squeeze(1)
        f0 = -torch.autograd.grad(e0, p0, torch.ones_like(e0))[0]
        y_e, y_f = targets_with_margin(e0.detach(), f0.detach(), SEEDS[backbone] + k)
        bd = BatchData(x=torch.from_numpy(x), positions=pos.clone(), batch=bvec, y=y_e, force=y_f)
        if rei is not None:
            bd.radius_edge_index = rei
            arrs["radius_edge_index_%d" % k] = rei
        loader.append(bd)
        for name, v in (("x", x), ("positions", pos), ("batch", bvec), ("y", y_e), ("force", y_f),
                        ("pred_energy", e0.detach()), ("pred_force", f0.detach())):
            arrs[name].append(np.asarray(v))
    ns = dict(args=args, model=model, graph_pred_linear=graph_pred_linear, torch=torch, grad=torch.autograd.grad,
              tqdm=lambda it: it)
    exec(extract(), ns)
    energy_mae, force_mae = ns["eval"](torch.device("cpu"), loader)
    out = {k: (np.stack(v) if isinstance(v, list) else v.numpy()) for k, v in arrs.items()}
    out.update(energy_mae=np.float64(energy_mae), force_mae=np.float64(force_mae), cfg=json.dumps(cfg),
               meta=json.dumps(dict(kind=backbone, B=B, n=N_ATOMS, batches=BATCHES, seed=SEEDS[backbone])))
    path = os.path.join(HERE, "g26_md17_eval_%s.npz" % backbone)
    np.savez_compressed(path, **out)
    print("wrote %-28s %7.1f KB  energy_mae %.6f  force_mae %.6f"
          % (os.path.basename(path), os.path.getsize(path) / 1024, energy_mae, force_mae))


if __name__ == "__main__":
    for backbone in ("schnet", "painn"):
        make_case(backbone)
