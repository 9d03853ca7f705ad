"""Step API of ``examples/pretrain_DistancePrediction.py`` (the Distance Prediction baseline of GeoSSL) on the HIP path.

``DistancePredictor`` is the reference module (same state_dict keys, shapes and init; its ``forward`` is the reference's
ATen code).  ``do_DistancePrediction(args, batch, model, distance_predictor)`` is the loop body :66-79 as one call and
returns the loss: the backbone's latent, then the fused distance head (csrc/distance_head.hip: two per-atom projections
instead of the [S, 2F] edge features, no index_add scatters), with forward + backward replayed from HIP graphs by
``pretrain_GeoSSL._AutogradStep`` when gradients are wanted.  The returned loss supports the reference's own
``optimizer.zero_grad(); loss.backward(); optimizer.step()`` with a stock ``torch.optim.Adam``.
``DistancePredictionTrainer`` is the ``train()`` body with all parameters in one flat buffer (one fused Adam launch, one
all-reduce per step).
"""
import torch
import torch.nn as nn

from . import _lib, ops
from .layout import UngroupedSuperEdges
from .switches import env as _env


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


def _node_repr(args, batch, model):
    """:68-73 -> node_repr [N, F] (the readout is not evaluated: the step never reads it)."""
    x = batch.x[:, 0]
    if args.model_3d == "schnet":
        _, h = model(x, batch.positions, batch.batch, return_latent=True, latent_only=True)
    elif args.model_3d == "painn":
        _, h = model(x, batch.positions, batch.radius_edge_index, batch.batch, return_latent=True, latent_only=True)
    else:
        raise Exception("3D model {} not included.".format(args.model_3d))
    return h


def distance_step_fused(args, batch, model, distance_predictor):
    """The step as eager launches: the backbone, then the fused head -> loss (fp32 scalar)."""
    lin = distance_predictor.predictor
    bucket = getattr(batch, "_bucket", None)
    if bucket is not None:
        # the static batch of a one-view capacity bucket (geossl_amd/bucket.py): capacity-sized tensors, the real atom and
        # super-edge counts in bucket.dyn
        if args.model_3d != bucket.kind or bucket.views != 1:
            raise _lib.GeosslHipError("the Distance Prediction step needs a one-view bucket of its own backbone")
        x = batch.x[:, 0]
        if bucket.kind == "schnet":
            _, h = model(x, batch.positions, bucket.b2, return_latent=True, latent_only=True, layout=bucket.lay2)
        else:
            _, h = model(x, batch.positions, bucket.e2, bucket.b2, return_latent=True, latent_only=True,
                         layout=bucket.lay2, edge_layout=bucket.el)
        sel = bucket.sel
        loss, _ = ops.distance_head(h, lin.weight, lin.bias, batch.positions, batch.super_edge_index,
                                    (sel.inc_ptr, sel.inc_idx), dyn=bucket.dyn)
        return loss
    from .layout import get_super_edge_layout
    sel = get_super_edge_layout(batch.batch, batch.super_edge_index, batch.num_graphs)
    h = _node_repr(args, batch, model)
    loss, _ = ops.distance_head(h, lin.weight, lin.bias, batch.positions, batch.super_edge_index,
                                (sel.inc_ptr, sel.inc_idx))
    return loss


def distance_step_aten(args, batch, model, distance_predictor):
    """:66-77 restated in ATen on our backbone: the fallback for predictors and batches the fused head does not take."""
    if args.model_3d == "schnet":
        _, node_repr = model(batch.x[:, 0], batch.positions, batch.batch, return_latent=True)
    elif args.model_3d == "painn":
        _, node_repr = model(batch.x[:, 0], batch.positions, batch.radius_edge_index, batch.batch, return_latent=True)
    else:
        raise Exception("3D model {} not included.".format(args.model_3d))
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


def _distance_step(model, distance_predictor):
    """The _AutogradStep of (backbone, predictor), kept on the backbone module; rebuilt when a parameter was replaced,
    moved or frozen since (the graphs bind parameter addresses)."""
    from .pretrain_GeoSSL import _AutogradStep
    eng = model.__dict__.get("_geossl_distance_step")
    if eng is None or eng.n1 is not distance_predictor or not eng.unchanged():
        eng = _AutogradStep(model, distance_predictor, None, objective="DistancePrediction")
        model.__dict__["_geossl_distance_step"] = eng
    return eng


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
    if graph is None:
        graph = getattr(args, "step_graph", _env("GEOSSL_NO_STEP_GRAPH") is None)
    try:
        if graph and torch.is_grad_enabled() and not torch.cuda.is_current_stream_capturing():
            from .pretrain_GeoSSL import Args
            a = Args(args.model_3d)
            a.step_graph_mode = getattr(args, "step_graph_mode", "auto")
            loss = _distance_step(model, distance_predictor).run(a, batch, 0.0, 0.0, None, False)
            if loss is not None:
                return loss
        return distance_step_fused(args, batch, model, distance_predictor)
    except UngroupedSuperEdges:
        # (super-edges that are not grouped by molecule in batch order: no incidence lists for the fused backward)
        return distance_step_aten(args, batch, model, distance_predictor)


class DistancePredictionTrainer:
    """The body of ``train()`` (examples/pretrain_DistancePrediction.py:49-85): backbone latent, fused distance head,
    backward, gradient all-reduce, Adam - backbone and predictor in one flat buffer (one fused Adam launch at one
    learning rate: the reference's gnn_3d_lr_scale is 1 by default), no host sync inside ``step``.
    ``use_graph=True``: forward + backward are captured into HIP graphs and replayed (StepGraphs: ragged SchNet / PaiNN
    batches and DeviceLoader handles share one ONE-view capacity-bucket graph per batch size, for a predictor of width
    2 * 128; anything else one graph per structure).  There are no random draws in this step."""

    def __init__(self, model, distance_predictor, lr=5e-4, weight_decay=0.0, model_3d="schnet", use_graph=False,
                 max_graphs=256, graph_mode="auto"):
        from .optim import FlatParams, FusedAdam
        from .parallel import GradAllReduce
        from .pretrain_GeoSSL import Args, StepGraphs
        if not fused_head_ok(distance_predictor):
            raise ValueError("DistancePredictionTrainer needs the reference predictor at a width of the fused head "
                             "(64, 128, 256 or 512) on the GPU; use do_DistancePrediction for anything else")
        self.model, self.predictor = model, distance_predictor
        self.args = Args(model_3d)
        self.flat = FlatParams([model, distance_predictor])
        self.opt = FusedAdam(self.flat, lr=lr, weight_decay=weight_decay)
        self.reduce = GradAllReduce(self.flat.grad)
        self.use_graph = use_graph
        self.step_graphs = StepGraphs(self._fwd_bwd, model_3d, max_graphs, mode=graph_mode,
                                      modules=(model, distance_predictor, None), noise_keys=(), views=1)
        self.step_graphs.zero_with_refresh = self.flat.grad
        self._one = torch.ones((), dtype=torch.float32, device=self.flat.grad.device)

    def _fwd_bwd(self, batch, noise=None):
        from .pretrain_GeoSSL import own_capture_open
        if not own_capture_open():
            self.flat.zero_grad()  # (a replayed step: cleared with the refresh of the graph's inputs, StepGraphs.refresh)
        loss = distance_step_fused(self.args, batch, self.model, self.predictor)
        with _lib.direct_grads():  # every p.grad is a view of self.flat.grad: kernels accumulate into it directly
            loss.backward(self._one)
        self.flat.rebind_grads()
        return loss.detach()

    def _graph_fwd_bwd(self, batch):
        sg = self.step_graphs
        g = sg.lookup(batch)
        if g is None:
            if not sg.capture_now(batch):  # a structure seen for the first time: eager
                return self._fwd_bwd(batch)
            g = sg.capture(batch, {})
            if g is None:  # capture failed: eager from now on
                self.use_graph = False
                return self._fwd_bwd(batch)
        if not sg.refresh(g, batch):
            return self._fwd_bwd(batch)
        g["graph"].replay()
        return g["loss"].clone()

    def step(self, batch):
        """One training step -> the loss on the device."""
        loss = self._graph_fwd_bwd(batch) if self.use_graph else self._fwd_bwd(batch)
        st = self.model.__dict__.get("_geossl_status")
        if st is not None:  # deferred index check of the backbone (a replayed graph cannot queue the host copy itself)
            st.poll()
            st.arm(every=8)
        scale = self.reduce()
        self.opt.step(grad_scale=scale)
        return loss
