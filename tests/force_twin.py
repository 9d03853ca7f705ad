"""float64 torch twin of the train-on-forces step (examples/finetune_md17.py:31-54), written from its definition, for the
force-training tests: the backbone of oracle.nets in fp64, the energy head, pred_force = -grad(E, pos, create_graph=True),
the L1 or MSE loss on energy and force with its two coefficients, then backward - torch autograd differentiates twice.

The graph is an input, decided once from the fp32 positions the kernels see (SchNet: oracle.graph.radius_graph_np with
its 32-neighbour cap; PaiNN: the batch's radius_edge_index).  `check_inputs` refuses inputs on which fp32 and fp64 could
legitimately disagree: a pair within 1e-4 A of the cutoff (in or out of the graph, and - the cap keeps the first 32 hits
in index order - of the capped neighbour lists), or, for L1, a residual within 1e-3 of its tensor's scale of zero (the
sign of the loss's derivative).

The comparison (`errors`, `BOUNDS`) is the one the GPU tests and the CPU teeth test share: per tensor
max|got - ref| / max|ref| (a max, not a norm: a term lost for a few atoms shows), the loss by its relative error."""
import numpy as np
import torch

from oracle import nets
from oracle.graph import pair_dist2_f32, radius_graph_np

CUTOFF_MARGIN = 1e-4   # A: no same-molecule pair this close to the cutoff
L1_MARGIN = 1e-3       # no L1 residual within this fraction of its tensor's max |residual| of zero

# bounds of the GPU tests on max|got - ref| / max|ref| against the twin (the loss: relative error), per backbone: about
# 4x the worst error measured on the MI355X over every case and entry point of tests/test_gpu_force_training.py, within
# the suite's 1e-5 (outputs, loss) and 1e-4 (gradients).  Worst measured - SchNet: loss 5.2e-7, energy 3.0e-6, force
# 1.2e-6, gradients 3.5e-6; PaiNN: loss 2.3e-7, energy 4.7e-7, force 1.2e-6, gradients 7.9e-5 (mixing.0.mu_channel_mix
# .weight of a ragged batch with mean readout: a sum over atoms and xyz of products of vector features that cancels by
# the molecules' rotational spread; every other PaiNN gradient <= 5.0e-5).  DESIGN.md section 4 has the table.
BOUNDS = dict(schnet=dict(loss=2e-6, energy=1e-5, force=4e-6, grad=1.4e-5),
              painn=dict(loss=1e-6, energy=2e-6, force=5e-6, grad=1e-4))


def module_tensors(module):
    """(parameters, buffers) of a module as {state_dict name: fp32 CPU tensor} (shared parameters once)."""
    seen, params = set(), {}
    for name, p in module.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            params[name] = p.detach().float().cpu().clone()
    bufs = {name: b.detach().cpu().clone() for name, b in module.named_buffers()}
    return params, bufs


def schnet_edges(pos, batch, cutoff):
    """radius_graph(pos, r=cutoff, batch) of schnet.py:91 on the fp32 positions, cap included -> int64 [2, E]."""
    return torch.from_numpy(radius_graph_np(np.asarray(pos, dtype=np.float32), cutoff, np.asarray(batch)))


def cutoff_margin(pos, batch, cutoff):
    """min over same-molecule pairs of |fp32 distance - cutoff| (inf for a batch without pairs)."""
    pos, batch = np.asarray(pos, dtype=np.float32), np.asarray(batch)
    best = np.inf
    for m in np.unique(batch):
        p = pos[batch == m]
        if len(p) < 2:
            continue
        d = np.sqrt(pair_dist2_f32(p[:, None, :], p[None, :, :]).astype(np.float64))
        d = d[~np.eye(len(p), dtype=bool)]
        best = min(best, float(np.abs(d - cutoff).min()))
    return best


def check_inputs(pos, batch, cutoff):
    m = cutoff_margin(pos, batch, cutoff)
    if not m >= CUTOFF_MARGIN:
        raise ValueError("a pair lies %.2e A from the cutoff: fp32 and fp64 may build different graphs" % m)


def _margin(res):
    a = res.detach().abs()
    return float(a.min() / a.max().clamp_min(1e-300))


def head_forward(rep, head):
    """Linear(F, 1) / Dense(F, 1) for {weight, bias}; create_output_layers() (Dense(F, F/2, silu), Dense(F/2, 1)) for
    {0.weight, 0.bias, 1.weight, 1.bias} -> [B]."""
    if "weight" in head:
        return (rep @ head["weight"].t() + head["bias"]).reshape(-1)
    a = torch.nn.functional.silu(rep @ head["0.weight"].t() + head["0.bias"])
    return (a @ head["1.weight"].t() + head["1.bias"]).reshape(-1)


def _energy(kind, cfg, P, H, z, x, batch, ei):
    if kind == "schnet":
        rep = nets.schnet_forward(P, z, x, batch, cfg["cutoff"], cfg["num_interactions"], cfg["readout"], edge_index=ei)
    else:
        rep = nets.painn_forward(P, z, x, ei, batch, cfg["n_atom_basis"], cfg["n_interactions"], cfg["cutoff"],
                                 cfg["readout"])
    return head_forward(rep, H)


def predict(kind, cfg, params, buffers, head, z, pos, batch, edge_index, device="cpu"):
    """(energy, force) of the twin in fp64 (returned on the CPU), first order only: what targets are drawn around."""
    dd = dict(dtype=torch.float64, device=device)
    P = {k: v.detach().to(**dd) for k, v in list(params.items()) + list(buffers.items()) if v.is_floating_point()}
    H = {k: v.detach().to(**dd) for k, v in head.items()}
    z = torch.as_tensor(z).to(device)
    x = torch.as_tensor(pos, dtype=torch.float32).to(**dd).requires_grad_(True)
    energy = _energy(kind, cfg, P, H, z if z.dim() == 1 else z[:, 0], x, torch.as_tensor(batch).to(device),
                     torch.as_tensor(edge_index).to(device))
    force = -torch.autograd.grad(energy, x, torch.ones_like(energy))[0]
    return energy.detach().cpu(), force.detach().cpu()


def step(kind, cfg, params, buffers, head, z, pos, batch, edge_index, y_e, y_f, coeff=(0.05, 0.95), loss="l1",
         device="cpu", drop_force_atom=None, check=True):
    """One finetune_md17.py:33-53 step in fp64.  kind "schnet": cfg = (hidden_channels, num_interactions, cutoff, readout)
    keys; "painn": (n_atom_basis, n_interactions, cutoff, readout).  params / buffers / head: {state_dict name: tensor}.
    drop_force_atom: leave that atom's force residual out of the loss (the teeth of the comparison).
    -> dict(loss, energy, force, pos_grad, grads {backbone name: grad}, head_grads {head name: grad}), all fp64 CPU."""
    dd = dict(dtype=torch.float64, device=device)
    P = {k: v.detach().to(**dd).requires_grad_(True) for k, v in params.items()}
    H = {k: v.detach().to(**dd).requires_grad_(True) for k, v in head.items()}
    C = {k: v.detach().to(**dd) for k, v in buffers.items() if v.is_floating_point()}
    z = torch.as_tensor(z).to(device)
    z = z if z.dim() == 1 else z[:, 0]
    batch = torch.as_tensor(batch).to(device)
    ei = torch.as_tensor(edge_index).to(device)
    B = int(batch.max()) + 1
    pos32 = torch.as_tensor(pos, dtype=torch.float32)
    if check:
        check_inputs(pos32.cpu().numpy(), batch.cpu().numpy(), cfg["cutoff"])
    x = pos32.to(**dd).requires_grad_(True)                                                        # :32-33
    energy = _energy(kind, cfg, dict(P, **C), H, z, x, batch, ei)                                  # :36-41
    force = -torch.autograd.grad(energy, x, torch.ones_like(energy), create_graph=True, retain_graph=True)[0]   # :46
    ye = torch.as_tensor(y_e).reshape(-1).to(**dd)
    yf = torch.as_tensor(y_f).reshape(-1, 3).to(**dd)
    re, rf = energy - ye, force - yf
    if loss == "l1" and check:
        for what, r in (("energy", re), ("force", rf)):
            if _margin(r) < L1_MARGIN:
                raise ValueError("an L1 %s residual lies within %.0e of zero: fp32 and fp64 may disagree on its sign"
                                 % (what, L1_MARGIN))
    if drop_force_atom is not None:
        keep = torch.ones(rf.size(0), 1, **dd)
        keep[drop_force_atom] = 0.0
        rf = rf * keep
    crit = (lambda r: r.abs().mean()) if loss == "l1" else (lambda r: (r * r).mean())
    L = coeff[0] * crit(re) + coeff[1] * crit(rf)                                                   # :48-51
    L.backward()                                                                                    # :53
    cpu = lambda t_: t_.detach().cpu()
    return dict(loss=cpu(L), energy=cpu(energy), force=cpu(force), pos_grad=cpu(x.grad), B=B,
                grads={k: cpu(v.grad) if v.grad is not None else torch.zeros(v.shape, dtype=torch.float64)
                       for k, v in P.items()},
                head_grads={k: cpu(v.grad) for k, v in H.items()})


def targets_with_margin(energy, force, seed, scale=0.5):
    """L1 targets whose residuals lie between 0.3 and 1 times `scale` x (the tensor's max |value|, at least 1) from zero:
    y = pred - residual (energy, force: a twin's predictions, fp64) -> fp32 (y_e [B], y_f [N, 3]).  The force residuals
    have random signs; the energy residuals one sign, so that the head bias's gradient (their mean) does not cancel."""
    g = torch.Generator().manual_seed(seed)

    def draw(v, signed):
        v = v.double()
        s = scale * float(v.abs().max().clamp_min(1.0))
        mag = 0.3 + 0.7 * torch.rand(v.shape, generator=g, dtype=torch.float64)
        sign = torch.where(torch.rand(v.shape, generator=g) < 0.5, -1.0, 1.0).double() if signed else 1.0
        return (v - sign * mag * s).float()
    return draw(energy, False), draw(force, True)


def max_err(got, ref):
    """max|got - ref| / max|ref| of one tensor."""
    got = torch.as_tensor(got).detach().double().reshape(-1).cpu()
    ref = torch.as_tensor(ref).detach().double().reshape(-1).cpu()
    if ref.numel() == 0:
        return 0.0
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def errors(got, ref):
    """Per-quantity errors of a step against the twin: got = dict(loss, energy, force, grads {name: grad}) with the
    grads keyed like the twin's (backbone names, head names prefixed "head.") - only what `got` has is compared."""
    out = {}
    if got.get("loss") is not None:
        out["loss"] = abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    for k in ("energy", "force"):
        if got.get(k) is not None:
            out[k] = max_err(got[k], ref[k])
    refg = dict(ref["grads"], **{"head." + k: v for k, v in ref["head_grads"].items()})
    for k, v in got.get("grads", {}).items():
        out["grad/" + k] = max_err(v, refg[k])
    return out


def flagged(errs, kind, bounds=None):
    """The entries of `errs` above their bound for backbone `kind` (grad/<name> entries: the "grad" bound)."""
    bounds = BOUNDS[kind] if bounds is None else bounds
    return {k: e for k, e in errs.items() if not e <= bounds[k.split("/")[0]]}
