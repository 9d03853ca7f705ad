"""Step API of ``examples/pretrain_TorsionAnglePrediction.py`` (the angle-prediction baseline of GeoSSL on atom triples)
on the HIP path.

``TorsionAnglePredictor`` is the reference module (same state_dict keys, shapes and init; its ``forward`` is the
reference's ATen code).  ``do_TorsionAnglePrediction(args, batch, model, torsion_angle_predictor)`` is the loop body
:64-78 as one call and returns the loss: the backbone's latent, then the fused triple head (csrc/torsion_head.hip: three
per-atom projections instead of the [T, 3F] triple features, no index_add scatters), with forward + backward replayed
from HIP graphs by ``autograd_step._AutogradStep`` when gradients are wanted.  The returned loss supports the
reference's own ``optimizer.zero_grad(); loss.backward(); optimizer.step()`` with a stock ``torch.optim.Adam``.
``TorsionAnglePredictionTrainer`` is the ``train()`` body with all parameters in one flat buffer (one fused Adam launch,
one all-reduce per step).

The target ``batch.super_edge_angle`` is taken from the batch and never computed here, as in the reference loop: the
reference tree does not contain the dataset class that fills it (``MoleculeDataset3DTorsionAngle``).  To run the
objective at all, ``ops.triple_angles`` / ``DeviceDataset(triples=...)`` produce one - the angle at the middle atom of the
triple - which is THIS LIBRARY'S definition, not the reference's.
"""
import torch
import torch.nn as nn

from . import _lib, ops
from .layout import UngroupedSuperEdges
from .batch import TripleBatch  # (the device batch type of collated triple batches)
from .step import Args, Objective, StepTrainer, backbone_forward, backbone_latent, run_graphed


class TorsionAnglePredictor(nn.Module):
    """examples/pretrain_TorsionAnglePrediction.py:16-27."""

    def __init__(self, emb_dim):
        super(TorsionAnglePredictor, self).__init__()
        self.predictor = nn.Linear(emb_dim * 3, 1)
        self.criterion = nn.MSELoss()
        return

    def forward(self, u_node_repr, v_node_repr, w_node_repr, torsion_angle_actual):
        edge_repr = torch.cat([u_node_repr, v_node_repr, w_node_repr], dim=1)
        torsion_angle_pred = self.predictor(edge_repr).squeeze()
        loss = self.criterion(torsion_angle_pred, torsion_angle_actual)
        return loss


def fused_head_ok(torsion_angle_predictor):
    """The predictor is what the fused head computes: the reference's Linear(3F, 1) with a bias, a stock mean MSELoss,
    F a width of the fused kernels."""
    lin = getattr(torsion_angle_predictor, "predictor", None)
    crit = getattr(torsion_angle_predictor, "criterion", None)
    return (type(torsion_angle_predictor) is TorsionAnglePredictor and type(lin) is nn.Linear and lin.bias is not None
            and lin.out_features == 1 and lin.in_features % 3 == 0 and type(crit) is nn.MSELoss
            and crit.reduction == "mean" and lin.weight.is_cuda and lin.weight.dtype == torch.float32
            and ops.torsion_head_width_ok(lin.in_features // 3))


def _check_grouped(batch_vec, triples):
    """The fused backward finds a molecule's triples as ONE run of the list: the triples must be grouped by molecule in
    batch order with their three atoms in one molecule.  Collated AtomTripleExtractor output is (marked by the collation:
    no check); anything else is checked once per (batch vector, triples) version - one read-back."""
    tag = (batch_vec._version, triples._version)
    if getattr(triples, "_geossl_grouped", None) == tag:
        return
    if triples.size(1):
        if int(triples.min()) < 0 or int(triples.max()) >= batch_vec.numel():
            raise UngroupedSuperEdges("super_edge_index names atoms outside the batch")
        m = batch_vec[triples]
        ok = bool(((m[0] == m[1]) & (m[0] == m[2])).all()) and bool((m[0, 1:] >= m[0, :-1]).all())
        if not ok:
            raise UngroupedSuperEdges("super_edge_index must be grouped by molecule in batch order with its three atoms in "
                                      "the same molecule (collated AtomTripleExtractor output is)")
    triples._geossl_grouped = tag


def torsion_step_fused(args, batch, model, torsion_angle_predictor):
    """The step as eager launches: the backbone, then the fused head -> loss (fp32 scalar)."""
    lin = torsion_angle_predictor.predictor
    bucket = getattr(batch, "_bucket", None)
    if bucket is not None:
        # the static batch of a one-view "triples" capacity bucket (geossl_amd/bucket.py): capacity-sized tensors, the real
        # atom and triple counts in bucket.dyn
        if args.model_3d != bucket.kind or bucket.views != 1 or bucket.T_cap < 1:
            raise _lib.GeosslHipError("the angle-prediction step needs a one-view triples bucket of its own backbone")
    else:
        _check_grouped(batch.batch, batch.super_edge_index)
    h, lay, dyn = backbone_latent(args.model_3d, batch, model, what="angle-prediction", layout=True)
    loss, _ = ops.torsion_head(h, lin.weight, lin.bias, batch.super_edge_index, batch.super_edge_angle, lay.mol_ptr,
                               dyn=dyn)
    return loss


# (no random draws; triples and targets are the batch's own: static inputs of a "triples" bucket that its fill refreshes)
TORSION = Objective("TorsionAnglePrediction",
                    lambda owner, args, batch, noise: torsion_step_fused(args, batch, owner.model, owner.n1))


def torsion_step_aten(args, batch, model, torsion_angle_predictor):
    """:64-78 restated in ATen on our backbone: the fallback for predictors and batches the fused head does not take."""
    _, node_repr = backbone_forward(args, batch, model, True)
    super_edge_index = batch.super_edge_index
    u_node_repr = torch.index_select(node_repr, dim=0, index=super_edge_index[0])
    v_node_repr = torch.index_select(node_repr, dim=0, index=super_edge_index[1])
    w_node_repr = torch.index_select(node_repr, dim=0, index=super_edge_index[2])
    torsion_angle_actual = batch.super_edge_angle
    return torsion_angle_predictor(u_node_repr, v_node_repr, w_node_repr, torsion_angle_actual)


def _fused_batch_ok(batch):
    if getattr(batch, "_dataset", None) is not None:   # a DeviceLoader handle: float32 / int64 tensors on its device
        return batch.device.type == "cuda" and bool(getattr(batch, "_triples", False))
    pos, sei, ang = batch.positions, batch.super_edge_index, getattr(batch, "super_edge_angle", None)
    return (pos.is_cuda and not pos.requires_grad and pos.dtype == torch.float32 and sei.is_cuda
            and sei.dtype == torch.long and sei.dim() == 2 and sei.size(0) == 3 and torch.is_tensor(ang) and ang.is_cuda
            and ang.dtype == torch.float32 and not ang.requires_grad and ang.dim() == 1 and ang.numel() == sei.size(1))


def _as_triple_batch(batch):
    """A collated batch of another type with the reference's attributes (BatchAtomTriple.to(device), a namespace built by
    hand) as the TripleBatch the graph engine keys and captures; a TripleBatch or a DeviceLoader handle as it is."""
    if getattr(batch, "_dataset", None) is not None or isinstance(batch, TripleBatch):
        return batch
    tb = batch.__dict__.get("_geossl_triple_batch") if hasattr(batch, "__dict__") else None
    tags = tuple(id(t_) for t_ in (batch.x, batch.positions, batch.batch, batch.super_edge_index, batch.super_edge_angle))
    if tb is None or tb[0] != tags:
        out = TripleBatch(batch.x, batch.positions, batch.batch, batch.super_edge_index, batch.super_edge_angle,
                          getattr(batch, "radius_edge_index", None), getattr(batch, "_num_graphs", None) or batch.num_graphs,
                          getattr(batch, "_sizes", None))
        tb = (tags, out)
        if hasattr(batch, "__dict__"):
            batch.__dict__["_geossl_triple_batch"] = tb
    return tb[1]


def do_TorsionAnglePrediction(args, batch, model, torsion_angle_predictor, graph=None):
    """examples/pretrain_TorsionAnglePrediction.py:64-78 -> torsion_angle_loss (fp32 scalar tensor).  args.model_3d picks
    the backbone call ("schnet" / "painn").  The fused head runs whenever the predictor and the batch allow it
    (fused_head_ok; CUDA positions and float32 angles without a gradient, triples grouped by molecule as collated batches
    are); anything else - another criterion or reduction, a subclass, another width, CPU tensors, positions or angles
    that require a gradient, float64 angles, ungrouped triples - runs the reference's ATen head.  graph: replay HIP
    graphs of forward + backward (default: ``args.step_graph`` if present, else on unless GEOSSL_NO_STEP_GRAPH is set)."""
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    if not (fused_head_ok(torsion_angle_predictor) and _fused_batch_ok(batch)):
        return torsion_step_aten(args, batch, model, torsion_angle_predictor)
    try:
        tb = _as_triple_batch(batch)
        if getattr(tb, "_dataset", None) is None:
            _check_grouped(tb.batch, tb.super_edge_index)   # (before a graph binds or a bucket copies the list)
        loss = run_graphed(args, graph, model, "_geossl_torsion_step", TORSION, Args(args.model_3d), tb,
                           n1=torsion_angle_predictor)
        if loss is not None:
            return loss
        return torsion_step_fused(args, tb, model, torsion_angle_predictor)
    except UngroupedSuperEdges:
        # (triples that are not grouped by molecule in batch order: no per-molecule runs for the fused backward)
        return torsion_step_aten(args, batch, model, torsion_angle_predictor)


class TorsionAnglePredictionTrainer(StepTrainer):
    """The body of ``train()`` (examples/pretrain_TorsionAnglePrediction.py:51-83): backbone latent, fused triple head,
    backward, gradient all-reduce, Adam - backbone and predictor in one flat buffer (one fused Adam launch at one
    learning rate: the reference's gnn_3d_lr_scale is 1 by default), no host sync inside ``step``.
    ``use_graph=True``: forward + backward are captured into HIP graphs and replayed (StepGraphs: ragged SchNet / PaiNN
    batches and DeviceLoader handles of a triple dataset share one ONE-view capacity-bucket graph per batch size, for a
    predictor of width 3 * 128 - the triples, their angles and their count are static inputs of the graph at a capacity,
    refreshed per step; anything else one graph per structure).  There are no random draws in this step."""

    def __init__(self, model, torsion_angle_predictor, lr=5e-4, weight_decay=0.0, model_3d="schnet", use_graph=False,
                 max_graphs=256, graph_mode="auto"):
        if not fused_head_ok(torsion_angle_predictor):
            raise ValueError("TorsionAnglePredictionTrainer needs the reference predictor at a width of the fused head "
                             "(64, 128, 256 or 512) on the GPU; use do_TorsionAnglePrediction for anything else")
        self.predictor = torsion_angle_predictor
        super().__init__([model, torsion_angle_predictor], TORSION, Args(model_3d), lr, weight_decay, use_graph,
                         max_graphs, graph_mode)

    def step(self, batch):
        """One training step -> the loss on the device.  batch: a TripleBatch, a collated BatchAtomTriple on the device, or
        a DeviceLoader handle of a triple dataset."""
        batch = _as_triple_batch(batch)
        if getattr(batch, "_dataset", None) is None:
            _check_grouped(batch.batch, batch.super_edge_index)
        return super().step(batch)
