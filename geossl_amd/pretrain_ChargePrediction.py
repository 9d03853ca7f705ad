"""Step API of ``examples/pretrain_ChargePrediction.py`` (the Charge Prediction - "type prediction" - baseline of GeoSSL)
on the HIP path.

``ChargePredictor`` is the reference module (same state_dict keys, shapes and init; its ``forward`` is the reference's
ATen code).  ``do_ChargePrediction(args, batch, model, charge_predictor)`` is the loop body :62-81 as one call and returns
the loss: the masked-atom draw and its write into the atom types (csrc/charge_head.hip, one launch), the backbone's
latent on the masked types, then the fused head (masked-row Linear + cross-entropy, forward and backward), replayed from
HIP graphs by ``autograd_step._AutogradStep`` when gradients are wanted.  The returned loss supports the reference's
own ``optimizer.zero_grad(); loss.backward(); optimizer.step()`` with a stock ``torch.optim.Adam``.
``ChargePredictionTrainer`` is the ``train()`` body with all parameters in one flat buffer (one fused Adam launch, one
all-reduce per step) and the mask drawn on the device by default.

Masks (``args.mask_rng``, as ``DeviceLoader(mask_rng=...)``): "numpy" (the default of ``do_ChargePrediction``) is the
reference's own ``np.random.choice(M, int(M * ratio), replace=False)`` on the host, so a seeded run masks the atoms the
reference masks; "device" draws a uniform k-subset on the GPU from Philox under a 64-bit seed that the launch advances
itself (include/geossl_hip.h, geossl_charge_mask).
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from .pretrain_GeoSSL import _next_noise_key
from .replay import StepGraphs
from .step import Objective, StepTrainer, backbone_forward, backbone_latent, run_graphed

node_class = 9   # examples/pretrain_ChargePrediction.py:106 (the mask token is node_class - 1)
MASK_RNGS = ("numpy", "device")


class ChargePredictor(nn.Module):
    """examples/pretrain_ChargePrediction.py:15-25 (the class count, the reference's module global, as an argument)."""

    def __init__(self, emb_dim, node_class=node_class):
        super(ChargePredictor, self).__init__()
        self.predictor = nn.Linear(emb_dim, node_class)
        self.criterion = nn.CrossEntropyLoss()
        return

    def forward(self, node_repr, charge_actual):
        charge_pred = self.predictor(node_repr)
        loss = self.criterion(charge_pred, charge_actual)
        return loss


def fused_head_ok(charge_predictor):
    """The predictor is what the fused head computes: the reference's class (not a subclass) with a Linear(F, C) that
    has a bias and a stock mean CrossEntropyLoss (no class weights, no label smoothing, the default ignore_index), F and
    C widths of the fused kernels, fp32 parameters on the GPU."""
    lin = getattr(charge_predictor, "predictor", None)
    crit = getattr(charge_predictor, "criterion", None)
    return (type(charge_predictor) is ChargePredictor and type(lin) is nn.Linear and lin.bias is not None
            and type(crit) is nn.CrossEntropyLoss and crit.reduction == "mean" and crit.weight is None
            and crit.ignore_index == -100 and crit.label_smoothing == 0.0 and lin.weight.is_cuda
            and lin.weight.dtype == torch.float32 and lin.bias.dtype == torch.float32
            and ops.charge_head_width_ok(lin.in_features, lin.out_features))


def mask_token(charge_predictor):
    """node_class - 1 of the reference (:66), with node_class the predictor's class count."""
    lin = getattr(charge_predictor, "predictor", None)
    return (lin.out_features if isinstance(lin, nn.Linear) else node_class) - 1


def mask_rng_of(args):
    rng = getattr(args, "mask_rng", "numpy")
    if rng not in MASK_RNGS:
        raise ValueError("mask_rng is 'numpy' or 'device'")
    return rng


def mask_count(M, ratio):
    """sampled_M = int(M * args.charge_masking_ratio) (:64)."""
    return int(M * ratio)


def numpy_mask(M, ratio):
    """masked_index of :65: the reference's own call on the global numpy stream (drawn even when k = 0)."""
    return np.random.choice(M, mask_count(M, ratio), replace=False)


def device_seed(dev):
    """A fresh 64-bit seed of the device draw as an int64 [1] tensor, derived from torch's CUDA generator on the host
    (torch.cuda.manual_seed governs it)."""
    s = _next_noise_key(dev)
    return torch.tensor([s - (1 << 64) if s >= 1 << 63 else s], dtype=torch.long).to(dev, non_blocking=True)


def n_atoms(batch):
    return batch.n_atoms if getattr(batch, "_dataset", None) is not None else int(batch.x.size(0))


def batch_device(batch):
    return batch.device if getattr(batch, "_dataset", None) is not None else batch.x.device


def draw_mask(rng, batch, ratio):
    """The step's mask input: {"mask_idx": the numpy draw on the device} or {"mask_seed": a fresh device seed}."""
    dev = batch_device(batch)
    if rng == "numpy":
        idx = numpy_mask(n_atoms(batch), ratio).astype(np.int64)
        return {"mask_idx": torch.from_numpy(idx).to(dev)}
    return {"mask_seed": device_seed(dev)}


def _status(model, h):
    """The backbone's deferred status word (_lib.StatusWord, made by its first forward), which a label out of range
    flags too."""
    return _lib.module_status(model, h.device, "atom type out of range (node_class=%d)" % node_class).word


def charge_step_fused(args, batch, model, charge_predictor, mask):
    """The step as eager launches: the mask draw / apply on batch.x (in place), the backbone on the masked types, the
    fused head -> (loss fp32 scalar, (idx, k): the masked atoms as the head read them and their count on the device).
    mask: {"mask_seed": int64 [1]} or {"mask_idx": int64 [>= k]} (draw_mask)."""
    lin = charge_predictor.predictor
    C = lin.out_features
    ratio = float(args.charge_masking_ratio)
    seed, given = mask.get("mask_seed"), mask.get("mask_idx")
    # (a one-view capacity bucket: the real atom count in bucket.dyn; its fill has written x before this launch)
    dyn = getattr(getattr(batch, "_bucket", None), "dyn", None)
    idx, labels, k = ops.charge_mask(batch.x, ratio, C, seed=seed, given=given, dyn=dyn)
    h, _, dyn = backbone_latent(args.model_3d, batch, model, x=batch.x[:, 0], what="Charge Prediction")
    return ops.charge_head(h, lin.weight, lin.bias, idx, labels, k, _status(model, h), dyn=dyn), (idx, k)


def charge_step_aten(args, batch, model, charge_predictor):
    """:62-81 restated in ATen on our backbone: the fallback for predictors, widths and batches the fused head does not
    take.  The mask is the reference's numpy draw, or (mask_rng "device", GPU tensors) the device draw."""
    charge = batch.x[:, 0]
    charge_actual = torch.clone(charge)
    M = charge.shape[0]
    ratio = float(args.charge_masking_ratio)
    if mask_rng_of(args) == "device" and batch.x.is_cuda:
        masked_index, charge_actual_masked, _ = ops.charge_mask(batch.x, ratio, mask_token(charge_predictor) + 1,
                                                                seed=device_seed(batch.x.device))
    else:
        masked_index = np.random.choice(M, mask_count(M, ratio), replace=False)
        charge[masked_index] = mask_token(charge_predictor)
        charge_actual_masked = charge_actual[masked_index]
    _, node_repr = backbone_forward(args, batch, model, True, x=charge)
    return charge_predictor(node_repr[masked_index], charge_actual_masked)


def _fused_batch_ok(batch):
    if getattr(batch, "_dataset", None) is not None:   # a DeviceLoader handle: int64 / float32 tensors on its device
        return batch.device.type == "cuda"
    x, pos = getattr(batch, "x", None), getattr(batch, "positions", None)
    return (x is not None and pos is not None and x.is_cuda and x.dtype == torch.long and x.dim() == 2
            and x.is_contiguous() and pos.is_cuda and not pos.requires_grad and pos.dtype == torch.float32)


class ChargeArgs:
    """The fields of the reference's argparse namespace the step reads."""

    def __init__(self, model_3d="schnet", charge_masking_ratio=0.3, mask_rng="numpy"):
        self.model_3d = model_3d
        self.charge_masking_ratio = float(charge_masking_ratio)
        self.mask_rng = mask_rng
        self.normalize = False


def _write_mask(owner, args, g, batch, mask):
    if args.mask_rng == "numpy":   # (this step's host draw into the graph's static list; a device graph advances its seed)
        StepGraphs.copy_noise(g, mask if mask is not None else draw_mask("numpy", batch, args.charge_masking_ratio))


def _keep_extra(eng, out, g):
    eng.extra = g["extra"]   # (masked atoms, k) of the step just replayed: do_ChargePrediction takes them at once
    return out


# the mask is the one draw: `noise` = {"mask_seed"} (device draw) or {"mask_idx"} (host draw); a graph binds the ratio, a
# by-value argument of its mask launch; forward -> (loss, (masked atoms, k)): static outputs of the forward graph
CHARGE = Objective(
    "ChargePrediction",
    lambda owner, args, batch, mask: charge_step_fused(args, batch, owner.model, owner.n1, mask),
    graph_key=lambda args: ("ChargePrediction", args.model_3d, float(args.charge_masking_ratio), args.mask_rng),
    noise_keys=lambda args: ("mask_idx" if args.mask_rng == "numpy" else "mask_seed",),
    capture_inputs=lambda owner, args, batch, mask: mask,
    write_inputs=_write_mask, result=_keep_extra)


def do_ChargePrediction(args, batch, model, charge_predictor, graph=None):
    """examples/pretrain_ChargePrediction.py:62-81 -> charge_loss (fp32 scalar tensor; the masked index is not returned:
    the reference's step has only the loss, and in numpy mode it is the np.random.choice draw a seeded caller can
    repeat).  args.model_3d picks the backbone call ("schnet" / "painn"), args.charge_masking_ratio the mask size,
    args.mask_rng (default "numpy") the draw.

    Like the reference, the step writes the mask token into the caller's ``batch.x[:, 0]`` (a DeviceLoader handle has no
    caller tensor: its molecules are gathered per step, and the write lands in the step's own copy).  The fused path runs
    whenever the predictor and the batch allow it (fused_head_ok; CUDA tensors, positions without a gradient); anything
    else - another criterion, label smoothing, a subclass, an unserved width, CPU tensors, positions that require a
    gradient - runs the reference's ATen head.  graph: replay HIP graphs of forward + backward (default:
    ``args.step_graph`` if present, else on unless GEOSSL_NO_STEP_GRAPH is set)."""
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    rng = mask_rng_of(args)
    ratio = float(args.charge_masking_ratio)
    if not 0.0 <= ratio <= 1.0:
        raise ValueError("charge_masking_ratio must lie in [0, 1]")
    if not (fused_head_ok(charge_predictor) and _fused_batch_ok(batch)):
        return charge_step_aten(args, batch, model, charge_predictor)
    mask = draw_mask(rng, batch, ratio)
    handle = getattr(batch, "_dataset", None) is not None
    if handle or hasattr(batch, "super_edge_index"):
        slot = "_geossl_charge_step"
        loss = run_graphed(args, graph, model, slot, CHARGE, ChargeArgs(args.model_3d, ratio, rng), batch, mask,
                           charge_predictor)
        if loss is not None:
            # (the graph's static outputs live in its memory pool: no reference to them may outlive this call, or a
            # later recapture that frees the graph would leave them behind)
            eng = model.__dict__[slot]
            idx, eng.extra = eng.extra[0], None
            if not handle:
                # the reference's write into the caller's types (:66): the graph masked its own copy of x
                ops.charge_mask(batch.x, ratio, mask_token(charge_predictor) + 1, given=idx)
            return loss
    return charge_step_fused(args, batch, model, charge_predictor, mask)[0]


class ChargePredictionTrainer(StepTrainer):
    """The body of ``train()`` (examples/pretrain_ChargePrediction.py:49-86): mask, backbone latent, fused charge head,
    backward, gradient all-reduce, Adam - backbone and predictor in one flat buffer (one fused Adam launch at one
    learning rate: the reference's gnn_3d_lr_scale is 1 by default), no host sync inside ``step``.
    mask_rng "device" (default): the masks are drawn on the GPU - a replayed graph advances its own seed, so the step
    does no host work for the draw; seed (int) fixes the first seed (else torch's CUDA generator gives it).  "numpy":
    the reference's np.random.choice per step, uploaded into the graph's static index list.
    ``use_graph=True``: forward + backward are captured into HIP graphs and replayed (StepGraphs: ragged SchNet / PaiNN
    batches and DeviceLoader handles share one ONE-view capacity-bucket graph per batch size, for a predictor of width
    128; anything else one graph per structure)."""

    def __init__(self, model, charge_predictor, lr=5e-4, weight_decay=0.0, model_3d="schnet", use_graph=False,
                 charge_masking_ratio=0.3, mask_rng="device", seed=None, max_graphs=256, graph_mode="auto"):
        if not fused_head_ok(charge_predictor):
            raise ValueError("ChargePredictionTrainer needs the reference predictor at a width of the fused head "
                             "(F in 64, 128, 256, 512; 2 <= C <= 16) on the GPU; use do_ChargePrediction for anything "
                             "else")
        if mask_rng not in MASK_RNGS:
            raise ValueError("mask_rng is 'numpy' or 'device'")
        self.predictor = charge_predictor
        self._seeds = None
        if mask_rng == "device" and seed is not None:
            # successive seeds of this trainer: splitmix64 of (seed, n) - one for the eager buffer, one per capture
            self._seeds = [int(seed), 0]
        self.key = "mask_seed" if mask_rng == "device" else "mask_idx"
        super().__init__([model, charge_predictor], CHARGE, ChargeArgs(model_3d, charge_masking_ratio, mask_rng), lr,
                         weight_decay, use_graph, max_graphs, graph_mode)
        # the eager steps' seed, advanced per draw
        self.seed = self._new_seed(self.flat.grad.device) if mask_rng == "device" else None

    def _new_seed(self, dev):
        if self._seeds is None:
            return device_seed(dev)
        m64 = (1 << 64) - 1
        self._seeds[1] += 1
        x = (self._seeds[0] + 0x9E3779B97F4A7C15 * self._seeds[1]) & m64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m64
        x ^= x >> 31
        return torch.tensor([x - (1 << 64) if x >= 1 << 63 else x], dtype=torch.long).to(dev)

    # the trainer's own: its seed sequence - one seed for the eager steps, a fresh one per capture (the engine's mask
    # comes from do_ChargePrediction, drawn per call)
    def _mask(self, batch, fresh=False):
        if self.key == "mask_idx":
            return draw_mask("numpy", batch, self.args.charge_masking_ratio)
        return {"mask_seed": self._new_seed(batch_device(batch)) if fresh else self.seed}

    def _eager(self, batch, noise=None):
        return self._fwd_bwd(batch, self._mask(batch))[0]

    def _capture_inputs(self, batch, noise):
        return self._mask(batch, fresh=True)

    def _write_inputs(self, g, batch, mask):
        # the trainer's own: a capture's fresh seed goes into its graph once; from then on device masks upload nothing
        # (the graph's seed advances on the device) and numpy masks are the objective's write, this step's draw
        if mask is not None and self.key == "mask_seed":
            StepGraphs.copy_noise(g, mask)
        else:
            super()._write_inputs(g, batch, mask)
