#!/usr/bin/env python3
"""Generate fixture G27 (GeoSSL-RR, --GeoSSL_option RR) by running the UNMODIFIED reference step on CPU.

Run in the build container only:  python tests/golden/make_golden_rr.py
`perturb` and `do_RR` (examples/pretrain_GeoSSL.py:68-100) are AST-extracted and executed verbatim with the names they
read from their module injected: `F`, whose `normalize` is wrapped only to keep the gradient of its output, and
`AE_model_01` / `AE_model_02`.  The reference tree has no AutoEncoder class: the two heads are instances of THIS
PROJECT'S `geossl_amd.Geom3D.models.AutoEncoder` (torch's default initialisation under a seed, then gamma ~ U(0.5, 1.5)
and beta ~ U(-0.5, 0.5) so that the affine part is not the identity); their initial parameters are stored.  The backbones
are the reference's own SchNet / PaiNN with the closed-form weights of filler.py; the one normal draw of perturb is
captured.

ReLU and the l1 loss have kinks.  Every case is computed in fp64 beside fp32; no pre-ReLU z and, for l1, no p - y may lie
within 1e-4 of zero in the fp64 run - otherwise the next head seed is taken.  The seed, the smallest margin and the
fp32-vs-fp64 difference of z and p are recorded.

Stored per case (arrays only): the batch, the noise, the loss, X / Y after --normalize with their gradients, the initial
parameters and the gradient of every head parameter, the backbone gradients (full for the reduced SchNet, grad_summary
otherwise) and the three BatchNorm buffers of both heads after the step.  Output: tests/golden/g27_rr_<case>.npz.
"""
import ast
import copy
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
from geossl_amd.Geom3D.models.autoencoder import AutoEncoder  # noqa: E402  (this project's definition)
from geossl_amd.synthetic import make_batch  # noqa: E402

torch.set_num_threads(4)

SCHNET_REDUCED = dict(hidden_channels=32, num_filters=32, num_interactions=2, num_gaussians=8, cutoff=5.0, node_class=9,
                      readout="mean")
SCHNET_FULL = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0, node_class=9,
                   readout="mean")
PAINN = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")

RAGGED = [5, 18, 2, 9, 33, 1, 12]
KINK = 1e-4
# name: (backbone, cfg, sizes, AE_loss, detach_target, normalize, seed)
CASES = {
    "schnet_reduced_l2_detach": ("schnet", SCHNET_REDUCED, RAGGED, "l2", True, False, 71),
    "schnet_reduced_l1_nodetach_norm": ("schnet", SCHNET_REDUCED, RAGGED, "l1", False, True, 72),
    "schnet_reduced_cosine_detach_B2": ("schnet", SCHNET_REDUCED, [18, 7], "cosine", True, False, 73),
    "schnet_full_l2_detach": ("schnet", SCHNET_FULL, [18, 3, 18, 12, 25, 1], "l2", True, False, 74),
    "schnet_full_l1_nodetach": ("schnet", SCHNET_FULL, [18, 9, 2, 27, 14], "l1", False, False, 75),
    "painn_cosine_detach_norm": ("painn", PAINN, [18, 9, 27, 2, 14], "cosine", True, True, 76),
}


class Batch:
    """Duck-typed BatchAtomTuple (dataloaders_AtomTuple.py:40-78)."""

    def __init__(self, d, dtype=torch.float32):
        for k, v in d.items():
            if k != "sizes":
                v = torch.from_numpy(np.ascontiguousarray(v))
                setattr(self, k, v.to(dtype) if v.is_floating_point() else v)

    @property
    def num_graphs(self):
        return self.batch[-1].item() + 1


def extract():
    tree = ast.parse(open(os.path.join(REF, "examples/pretrain_GeoSSL.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("perturb", "do_RR")]
    assert len(keep) == 2
    ns = {"torch": torch}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "pretrain_GeoSSL.py[RR]", "exec"), ns)
    return ns


class Recorder:
    """The representations that enter the heads, with their gradients kept: the model's outputs, replaced by the
    outputs of F.normalize when --normalize is on."""

    def __init__(self, model):
        self.model, self.reps = model, []

    def __call__(self, *a, **kw):
        out = self.model(*a, **kw)
        out.retain_grad()
        self.reps.append(out)
        return out

    def normalize(self, x, dim=-1):
        out = torch.nn.functional.normalize(x, dim=dim)
        out.retain_grad()
        self.reps[[r is x for r in self.reps].index(True)] = out
        return out


def make_heads(emb_dim, loss, detach_target, seed):
    torch.manual_seed(seed)
    heads = [AutoEncoder(emb_dim=emb_dim, loss=loss, detach_target=detach_target, beta=1) for _ in range(2)]
    with torch.no_grad():
        for h in heads:
            h.fc_layers[1].weight.uniform_(0.5, 1.5)
            h.fc_layers[1].bias.uniform_(-0.5, 0.5)
    return heads


def run(ns, kind, cfg, b, heads, normalize, noise, dtype):
    """do_RR verbatim in `dtype` -> (loss, X, Y, model, heads, z [2], p [2]) after loss.backward()."""
    batch = Batch(b, dtype)
    if kind == "painn":
        rei = []
        for m in range(len(b["sizes"])):
            sel = b["batch"] == m
            off = int(np.nonzero(sel)[0][0])
            rei.append(radius_graph(torch.from_numpy(b["positions"][sel]), r=cfg["cutoff"], loop=False) + off)
        batch.radius_edge_index = torch.cat(rei, dim=1)
    model = fill_module_(SchNet(**cfg) if kind == "schnet" else PaiNN(**cfg)).to(dtype)
    heads = [copy.deepcopy(h).to(dtype).train() for h in heads]
    rec = Recorder(model)
    zs, ps = [], []
    for h in heads:
        h.fc_layers[1].register_forward_hook(lambda m, i, o: zs.append(o.detach()))
        h.fc_layers.register_forward_hook(lambda m, i, o: ps.append(o.detach()))
    ns.update(F=types.SimpleNamespace(normalize=rec.normalize), AE_model_01=heads[0], AE_model_02=heads[1])
    args = types.SimpleNamespace(model_3d=kind, normalize=normalize)
    normal = torch.normal
    drawn = []

    def given_normal(mu, sigma, size):
        out = normal(mu, sigma, size=size) if noise is None else noise.clone()
        drawn.append(out.clone())
        return out.to(dtype)
    torch.normal = given_normal
    try:
        loss, acc = ns["do_RR"](args, batch, rec, 0.0, 0.3, criterion=None)
    finally:
        torch.normal = normal
    assert acc == 0 and len(drawn) == 1 and len(rec.reps) == 2 and len(zs) == 2 and len(ps) == 2
    loss.backward()
    return loss, rec.reps[0], rec.reps[1], model, heads, zs, ps, drawn[0], batch


def make_case(name, kind, cfg, sizes, ae_loss, detach, normalize, seed):
    ns = extract()
    b = make_batch(0, seed=seed, sizes=sizes)
    if kind == "painn":
        b["x"][:3, 0] = 0   # hydrogens: padding_idx row (painn.py:174)
    emb = cfg.get("hidden_channels", cfg.get("n_atom_basis"))
    torch.manual_seed(seed)
    noise = torch.normal(0.0, 0.3, size=tuple(b["positions"].shape))
    head_seed = 1000 + seed
    while True:
        heads = make_heads(emb, ae_loss, detach, head_seed)
        l64, X64, Y64, _, _, z64, p64, _, _ = run(ns, kind, cfg, b, heads, normalize, noise, torch.float64)
        margin = min(float(z.abs().min()) for z in z64)
        if ae_loss == "l1":
            margin = min(margin, float((p64[0] - Y64.detach()).abs().min()), float((p64[1] - X64.detach()).abs().min()))
        if margin > KINK:
            break
        head_seed += 1
    loss, X, Y, model, hs, z32, p32, drawn, batch = run(ns, kind, cfg, b, heads, normalize, noise, torch.float32)
    dz = max(float((a.double() - c).abs().max()) for a, c in zip(z32, z64))
    dp = max(float((a.double() - c).abs().max()) for a, c in zip(p32, p64))
    meta = dict(kind=kind, AE_loss=ae_loss, detach_target=detach, normalize=normalize, head_seed=head_seed,
                kink_margin=margin, z_fp32_vs_fp64=dz, p_fp32_vs_fp64=dp, loss_fp64=float(l64.detach()))
    arrs = dict(x=batch.x, positions=batch.positions, batch=batch.batch, super_edge_index=batch.super_edge_index,
                sizes=np.asarray(sizes, dtype=np.int64), pos_noise=drawn, cfg=json.dumps(cfg), meta=json.dumps(meta),
                loss=loss.detach(), X=X.detach(), Y=Y.detach(), grad_X=X.grad, grad_Y=Y.grad)
    if kind == "painn":
        arrs["radius_edge_index"] = batch.radius_edge_index
    for k, (h0, h) in enumerate(zip(heads, hs)):
        for pname, p in h0.named_parameters():
            arrs["head%d/param/%s" % (k + 1, pname)] = p.detach()
        for pname, p in h.named_parameters():
            arrs["head%d/grad/%s" % (k + 1, pname)] = p.grad
        bn = h.fc_layers[1]
        arrs["head%d/running_mean" % (k + 1)] = bn.running_mean
        arrs["head%d/running_var" % (k + 1)] = bn.running_var
        arrs["head%d/num_batches_tracked" % (k + 1)] = bn.num_batches_tracked
    full = kind == "schnet" and cfg["hidden_channels"] == 32
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
    path = os.path.join(HERE, "g27_rr_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote %-44s %7.1f KB  loss %.6f  seed %d margin %.2e  dz %.1e dp %.1e"
          % (os.path.basename(path), os.path.getsize(path) / 1024, float(loss.detach()), head_seed, margin, dz, dp))


if __name__ == "__main__":
    for name, case in CASES.items():
        make_case(name, *case)
