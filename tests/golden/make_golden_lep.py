#!/usr/bin/env python3
"""Generate fixture G25 (LEP fine-tuning: a binary label per protein-ligand pair seen in its active and its inactive
conformation) by running the UNMODIFIED reference on CPU.

Run in the build container only:  python tests/golden/make_golden_lep.py
The statements of `train()`'s loop in examples/finetune_lep.py from `batch = batch.to(device)` to
`loss = criterion(pred, actual)` (:31-45) are AST-extracted and executed verbatim with the names they read injected
(`args`, `model`, `graph_pred_linear`, `criterion` = nn.BCEWithLogitsLoss() as :226 sets it, `device` = cpu, `batch`);
`eval()` (:65-101, with its metric lines: sklearn's roc_auc_score and average_precision_score - imported here from
sklearn, and the maker stops if that import fails) is extracted whole and called on a loader of that one batch.  The
batch is collated by the reference's own `BatchLEP.from_data_list` from `Data` items of the ref_shims; it is stored
beside the items, which is what pins our loader.  The backbones are the reference's own SchNet / PaiNN built as :184-206
build them (node_class = 9, num_tasks = 1), the head Linear(2 * emb_dim, 1) for both, with the closed-form weights of
filler.py.

The structures are those of tests/lba_structures.py, all 2B of a case drawn in one call (active 0 .. B-1, then inactive
0 .. B-1: no two structures share a generator), with its 1e-4 A cutoff margin asserted; x_* is the 1-D atomic number and
y an int64 label per pair, as DatasetLEP's are.

With filler.py's weights a readout over hundreds of atoms gives logits in the tens ("add") or logits that agree to four
digits ("mean"): the first saturates the sigmoid, the second makes a rank metric a coin toss.  So the head's filled
weight and bias are multiplied by two constants per case, chosen below from the unscaled reference's own logits and
recorded in `meta` (`head_weight_scale`, `head_bias_scale`): parameters of the fixture, the reference code is untouched.
The maker asserts, on the reference's results alone: every |z_b| <= 3, every |sigmoid(z_b) - y_b| >= 0.05, both labels
present, neighbouring sorted logits >= 1e-3 apart.

Stored per case: the uncollated items (concatenated, with the per-item counts to split them), the collated batch (every
tensor, batch_active / batch_inactive included), y, the backbone's two readouts, pred and the loss, the head's parameters
and full gradients, the backbone's gradients (grad_summary), and eval()'s three numbers.
Output: tests/golden/g25_lep_<case>.npz.
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

from sklearn.metrics import average_precision_score, roc_auc_score  # noqa: E402  (no substitute: fail if absent)
from Geom3D.dataloaders.dataloaders_LEP import BatchLEP  # noqa: E402  (the reference's own collation)
from Geom3D.models import PaiNN, SchNet  # noqa: E402  (the reference's own classes)
from torch_geometric.data import Data  # noqa: E402  (shim)
from torch_geometric.nn import radius_graph  # noqa: E402  (shim)

import lba_structures as ls  # noqa: E402
from filler import fill_module_, grad_summary  # noqa: E402

torch.set_num_threads(4)

BASE = dict(model_3d="schnet", emb_dim=64, num_filters=64, num_interactions=2, num_gaussians=8, cutoff=5.0,
            readout="add", painn_n_interactions=3, painn_n_rbf=20, painn_radius_cutoff=5.0, painn_readout="add")
# name: (args overrides, active sizes, inactive sizes).  The smallest cases that reach every branch: a side above 255
# atoms (the fused batch is sparse) in either order of big / small within a pair and a pair of equal sizes; a batch with
# no such side (dense) at B = 2; the script's defaults (readout "mean"); PaiNN with its per-structure edge lists.
# The reduced cases read out with "add": the sums over 7 ... 260 atoms spread the logits, which the "mean" of pockets of
# one density does not (schnet_full keeps it: the script's default).
BIG = ((260, 7, 40), (9, 257, 40))
CASES = {
    "schnet_reduced": (dict(), *BIG),
    "schnet_dense": (dict(), (20, 7), (9, 30)),
    "schnet_full": (dict(emb_dim=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0,
                         readout="mean"), (260, 40), (40, 33)),
    "painn": (dict(model_3d="painn", emb_dim=128), *BIG),
}
Z_MAX, P_MARGIN, GAP = 3.0, 0.05, 1e-3   # the conditions on the reference's logits
# The logits of a case span SPREAD around MIDDLE (not around 0: logits +a / -a with the labels 1 / 0 make the bias
# gradient sum_b (sigmoid(z_b) - y_b) vanish identically, and the stored value would be rounding noise) ...
SPREAD, MIDDLE = 4.0, 0.5
AMPLIFY_MAX = 8.0  # ... unless that takes |weight scale * (pred - bias)| above this: then they sit around CENTRE
CENTRE = 1.0


def extract():
    """The loop statements :31-45 (ending with `loss = criterion(pred, actual)`) and eval() whole."""
    tree = ast.parse(open(os.path.join(REF, "examples/finetune_lep.py")).read())
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
    assert "roc = roc_auc_score(y_true, y_pred)" in metrics
    assert "pr = average_precision_score(y_true, y_pred)" in metrics
    step = compile(ast.Module(body=body, type_ignores=[]), "finetune_lep.py[loop]", "exec")
    ev_code = compile(ast.Module(body=ev, type_ignores=[]), "finetune_lep.py[eval]", "exec")
    return step, ev_code


def make_items(args, cutoff, sizes_a, sizes_i):
    B = len(sizes_a)
    sizes = tuple(sizes_a) + tuple(sizes_i)
    s = ls.checked(sizes, cutoff)
    assert s["margin"] >= ls.MARGIN, s["margin"]
    off = np.concatenate([[0], np.cumsum(sizes)])
    part = lambda k, m: torch.from_numpy(np.ascontiguousarray(s[k][off[m]:off[m + 1]]))
    items = []
    for b in range(B):
        d = dict(x_active=part("x", b), positions_active=part("positions", b), x_inactive=part("x", B + b),
                 positions_inactive=part("positions", B + b), y=torch.tensor([(b + 1) % 2], dtype=torch.long))
        if args.model_3d == "painn":   # DatasetLEPRadius: per structure, local indices
            d["radius_edge_index_active"] = radius_graph(d["positions_active"], r=cutoff, loop=False)
            d["radius_edge_index_inactive"] = radius_graph(d["positions_inactive"], r=cutoff, loop=False)
        items.append(Data(**d))
    return items, s


def head_scales(u, b0):
    """(weight scale, bias scale) from the unscaled head's u_b = pred_b - bias: z_b = alpha u_b + beta b0."""
    u = np.asarray(u, dtype=np.float64)
    alpha = SPREAD / (u.max() - u.min())
    centre = MIDDLE
    if alpha * np.abs(u).max() > AMPLIFY_MAX:
        alpha, centre = AMPLIFY_MAX / np.abs(u).max(), CENTRE
    alpha = float(np.float32(alpha))
    beta = float(np.float32((centre - alpha * 0.5 * (u.max() + u.min())) / b0))
    return alpha, beta


def make_case(name, over, sizes_a, sizes_i):
    step, ev_code = extract()
    args = types.SimpleNamespace(**dict(BASE, **over))
    cutoff = args.cutoff if args.model_3d == "schnet" else args.painn_radius_cutoff
    items, s = make_items(args, cutoff, sizes_a, sizes_i)
    batch = BatchLEP.from_data_list(items)
    batch.to = lambda device: batch
    node_class, num_tasks = 9, 1
    intermediate_dim = args.emb_dim * 2
    if args.model_3d == "schnet":      # :184-194
        cfg = dict(hidden_channels=args.emb_dim, num_filters=args.num_filters, num_interactions=args.num_interactions,
                   num_gaussians=args.num_gaussians, cutoff=args.cutoff, readout=args.readout, node_class=node_class)
        model = SchNet(**cfg)
    else:                              # :195-206
        cfg = dict(n_atom_basis=args.emb_dim, n_interactions=args.painn_n_interactions, n_rbf=args.painn_n_rbf,
                   cutoff=args.painn_radius_cutoff, max_z=node_class, n_out=num_tasks, readout=args.painn_readout)
        model = PaiNN(**cfg)
    graph_pred_linear = torch.nn.Linear(intermediate_dim, num_tasks)
    fill_module_(model)
    fill_module_(graph_pred_linear)
    ns = dict(batch=batch, model=model, graph_pred_linear=graph_pred_linear, criterion=torch.nn.BCEWithLogitsLoss(),
              device=torch.device("cpu"), args=args, torch=torch)
    with torch.no_grad():              # the unscaled head's logits, to choose the two constants from
        exec(step, ns)
        b0 = float(graph_pred_linear.bias)
        alpha, beta = head_scales(ns["pred"].double().numpy() - b0, b0)
        graph_pred_linear.weight.mul_(alpha)
        graph_pred_linear.bias.mul_(beta)
    exec(step, ns)
    loss, pred = ns["loss"], ns["pred"]
    loss.backward()
    ens = dict(model=model, graph_pred_linear=graph_pred_linear, args=args, torch=torch, np=np,
               criterion=torch.nn.BCEWithLogitsLoss(), roc_auc_score=roc_auc_score,
               average_precision_score=average_precision_score)
    exec(ev_code, ens)
    bce, roc, pr, y_true, y_pred = ens["eval"](torch.device("cpu"), [batch])
    assert np.array_equal(y_pred, pred.detach().double().numpy())

    # the conditions of the fixture, on the reference's results alone
    z, y = pred.detach().double().numpy(), batch.y.double().numpy()
    zs = np.sort(z)
    assert np.abs(z).max() <= Z_MAX, (name, z)
    assert np.abs(1.0 / (1.0 + np.exp(-z)) - y).min() >= P_MARGIN, (name, z, y)
    assert set(y.tolist()) == {0.0, 1.0}, (name, y)
    assert np.diff(zs).min() >= GAP, (name, zs)

    meta = dict(kind=args.model_3d, emb_dim=args.emb_dim, seed=s["seed"], margin=s["margin"], cutoff=cutoff,
                head_weight_scale=alpha, head_bias_scale=beta)
    arrs = dict(cfg=json.dumps(cfg), meta=json.dumps(meta), loss=loss.detach(), pred=pred.detach(),
                bce=np.float64(bce), roc=np.float64(roc), pr=np.float64(pr),
                sizes_active=np.asarray(sizes_a, dtype=np.int64), sizes_inactive=np.asarray(sizes_i, dtype=np.int64),
                # the two readouts the loop's own variables hold (:34-38): what the fp64 twin of the head starts from
                repr_active=ns["active_mol_repr"].detach(), repr_inactive=ns["inactive_mol_repr"].detach())
    on_disk = lambda k, v: v.to(torch.int32) if "edge_index" in k else v   # (int32 on disk: half the bytes)
    for k in items[0].keys:
        arrs["items/" + k] = on_disk(k, torch.cat([it[k] for it in items], dim=items[0].__cat_dim__(k, items[0][k])))
        if "edge_index" in k:
            arrs["items_edges/" + k] = np.asarray([it[k].size(1) for it in items], dtype=np.int64)
    for k in batch.keys:
        if torch.is_tensor(batch[k]):
            arrs["batch/" + k] = on_disk(k, batch[k])
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
    path = os.path.join(HERE, "g25_lep_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote %-28s %7.1f KB  seed %d margin %.2e  scales %.6g %.6g  z %s  loss %.6f  bce %.6f roc %.6f pr %.6f"
          % (os.path.basename(path), os.path.getsize(path) / 1024, s["seed"], s["margin"], alpha, beta,
             np.array2string(z, precision=4), float(loss.detach()), bce, roc, pr))


if __name__ == "__main__":
    for name, case in CASES.items():
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        make_case(name, *case)
