"""Step API of ``examples/pretrain_DistancePrediction.py`` (the Distance Prediction baseline of GeoSSL) on the HIP path.

``DistancePredictor`` is the reference module (same state_dict keys, shapes and init; its ``forward`` is the reference's
ATen code).  ``do_DistancePrediction(args, batch, model, distance_predictor)`` is the loop body :66-79 as one call and
returns the loss: the backbone's latent, then the fused distance head (csrc/distance_head.hip: two per-atom projections
instead of the [S, 2F] edge features, no index_add scatters), with forward + backward replayed from HIP graphs by
``autograd_step._AutogradStep`` when gradients are wanted.  The returned loss supports the reference's own
``optimizer.zero_grad(); loss.backward(); optimizer.step()`` with a stock ``torch.optim.Adam``.
``DistancePredictionTrainer`` is the ``train()`` body with all parameters in one flat buffer (one fused Adam launch, one
all-reduce per step).
"""
import torch
import torch.nn as nn

from . import ops
from .layout import UngroupedSuperEdges
from .step import Args, Objective, StepTrainer, backbone_forward, backbone_latent, run_graphed


class DistancePredictor(nn.Module):
    """examples/pretrain_DistancePrediction.py:15-25."""

    def __init__(self, emb_dim):
        super(DistancePredictor, self).__init__()
        self.predictor = nn.Linear(emb_dim * 2, 1)
        self.criterion = nn.L1Loss()
        return

    def forward(self, u_node_repr, v_node_repr, distance_actual):
        edge_repr = torch.cat([u_node_repr, v_node_repr], dim=1)
        distance_pred = self.predictor(edge_repr).squeeze()
        loss = self.criterion(distance_pred, distance_actual)
        return loss


def fused_head_ok(distance_predictor):
    """The predictor is what the fused head computes: the reference's Linear(2F, 1) with a bias, a stock mean L1Loss,
    F a width of the fused kernels."""
    lin = getattr(distance_predictor, "predictor", None)
    crit = getattr(distance_predictor, "criterion", None)
    return (isinstance(distance_predictor, DistancePredictor) and type(lin) is nn.Linear and lin.bias is not None
            and lin.out_features == 1 and lin.in_features % 2 == 0 and type(crit) is nn.L1Loss
            and crit.reduction == "mean" and lin.weight.is_cuda and lin.weight.dtype == torch.float32
            and ops.distance_head_width_ok(lin.in_features // 2))


def distance_step_fused(args, batch, model, distance_predictor):
    """The step as eager launches: the backbone, then the fused head -> loss (fp32 scalar)."""
    lin = distance_predictor.predictor
    bucket = getattr(batch, "_bucket", None)
    if bucket is not None:   # (capacity-sized tensors, the real atom and super-edge counts in bucket.dyn)
        sel = bucket.sel
    else:
        from .layout import get_super_edge_layout
        sel = get_super_edge_layout(batch.batch, batch.super_edge_index, batch.num_graphs)
    h, _, dyn = backbone_latent(args.model_3d, batch, model, what="Distance Prediction")
    loss, _ = ops.distance_head(h, lin.weight, lin.bias, batch.positions, batch.super_edge_index,
                                (sel.inc_ptr, sel.inc_idx), dyn=dyn)
    return loss


# (no random draws: the positions as they are; the tuple option is part of each StepGraphs key - bucket key / fingerprint)
DISTANCE = Objective("DistancePrediction",
                     lambda owner, args, batch, noise: distance_step_fused(args, batch, owner.model, owner.n1))


def distance_step_aten(args, batch, model, distance_predictor):
    """:66-77 restated in ATen on our backbone: the fallback for predictors and batches the fused head does not take."""
    _, node_repr = backbone_forward(args, batch, model, True)
    super_edge_index = batch.super_edge_index
    positions = batch.positions
    u_node_repr = torch.index_select(node_repr, dim=0, index=super_edge_index[0])
    v_node_repr = torch.index_select(node_repr, dim=0, index=super_edge_index[1])
    u_pos = torch.index_select(positions, dim=0, index=super_edge_index[0])
    v_pos = torch.index_select(positions, dim=0, index=super_edge_index[1])
    distance_actual = torch.sqrt(torch.sum((u_pos - v_pos) ** 2, dim=1))
    return distance_predictor(u_node_repr, v_node_repr, distance_actual)


def _fused_batch_ok(batch):
    if getattr(batch, "_dataset", None) is not None:   # a DeviceLoader handle: float32 / int64 tensors on its device
        return batch.device.type == "cuda"              # (checked without collating it: a bucket gathers it itself)
    pos, sei = batch.positions, batch.super_edge_index
    return (pos.is_cuda and not pos.requires_grad and pos.dtype == torch.float32 and sei.is_cuda
            and sei.dtype == torch.long and sei.dim() == 2 and sei.size(0) == 2)


def do_DistancePrediction(args, batch, model, distance_predictor, graph=None):
    """examples/pretrain_DistancePrediction.py:66-79 -> distance_loss (fp32 scalar tensor).  args.model_3d picks the
    backbone call ("schnet" / "painn").  The fused head runs whenever the predictor and the batch allow it
    (fused_head_ok; CUDA positions without a gradient, super-edges grouped by molecule as collated batches are);
    anything else - another criterion or width, CPU tensors, positions that require a gradient - runs the reference's
    ATen head.  graph: replay HIP graphs of forward + backward (default: ``args.step_graph`` if present, else on unless
    GEOSSL_NO_STEP_GRAPH is set)."""
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    if not (fused_head_ok(distance_predictor) and _fused_batch_ok(batch)):
        return distance_step_aten(args, batch, model, distance_predictor)
    try:
        loss = run_graphed(args, graph, model, "_geossl_distance_step", DISTANCE, Args(args.model_3d), batch,
                           n1=distance_predictor)
        if loss is not None:
            return loss
        return distance_step_fused(args, batch, model, distance_predictor)
    except UngroupedSuperEdges:
        # (super-edges that are not grouped by molecule in batch order: no incidence lists for the fused backward)
        return distance_step_aten(args, batch, model, distance_predictor)


class DistancePredictionTrainer(StepTrainer):
    """The body of ``train()`` (examples/pretrain_DistancePrediction.py:49-85): backbone latent, fused distance head,
    backward, gradient all-reduce, Adam - backbone and predictor in one flat buffer (one fused Adam launch at one
    learning rate: the reference's gnn_3d_lr_scale is 1 by default), no host sync inside ``step``.
    ``use_graph=True``: forward + backward are captured into HIP graphs and replayed (StepGraphs: ragged SchNet / PaiNN
    batches and DeviceLoader handles share one ONE-view capacity-bucket graph per batch size, for a predictor of width
    2 * 128; anything else one graph per structure).  There are no random draws in this step."""

    def __init__(self, model, distance_predictor, lr=5e-4, weight_decay=0.0, model_3d="schnet", use_graph=False,
                 max_graphs=256, graph_mode="auto"):
        if not fused_head_ok(distance_predictor):
            raise ValueError("DistancePredictionTrainer needs the reference predictor at a width of the fused head "
                             "(64, 128, 256 or 512) on the GPU; use do_DistancePrediction for anything else")
        self.predictor = distance_predictor
        super().__init__([model, distance_predictor], DISTANCE, Args(model_3d), lr, weight_decay, use_graph, max_graphs,
                         graph_mode)
