"""Step API of ``examples/pretrain_Supervised.py`` (the Supervised baseline of GeoSSL) and of property fine-tuning
(``examples/finetune_qm9.py`` train() / eval()) on the HIP path.

``do_Supervised(args, batch, model, graph_pred_linear, TRAIN_mean, TRAIN_std, task_id)`` is the loop body :79-104 as one
call: the backbone's latent, then the fused head of csrc/property_head.hip with the readout inside it (graph_pred_linear,
the normalised target, the L1 / MSE mean), forward + backward replayed from HIP graphs by
``autograd_step._AutogradStep`` when gradients are wanted.  Its loss supports the reference's own
``optimizer.zero_grad(); loss.backward(); optimizer.step()`` with a stock ``torch.optim.Adam``.  ``predict_Supervised``
is eval()'s forward (finetune_qm9.py:290-374): the de-normalised predictions; ``eval_Supervised`` is eval() over a loader
(:278-384), replayed from the forward-only graphs of geossl_amd/evaluate.py.  ``SupervisedTrainer`` is the ``train()``
body with backbone and head in one flat buffer (one fused Adam launch, one all-reduce per step) and no host sync in
``step``.  Anything the kernels do not serve runs the reference's own ATen lines on our backbone.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .step import Objective, StepTrainer, backbone_forward, backbone_latent, run_graphed


# ---------------------------------------------------------------------------------------------------- what is served
def criterion_of(args):
    """pretrain_Supervised.py:199-204: args.loss "mse" -> nn.MSELoss(), "mae" -> nn.L1Loss()."""
    if args.loss == "mse":
        return nn.MSELoss()
    if args.loss == "mae":
        return nn.L1Loss()
    raise ValueError("Loss {} not included.".format(args.loss))


def loss_kind(criterion):
    """"mae" / "mse" for a stock mean nn.L1Loss / nn.MSELoss (not a subclass), else None."""
    if type(criterion) is nn.L1Loss and criterion.reduction == "mean":
        return "mae"
    if type(criterion) is nn.MSELoss and criterion.reduction == "mean":
        return "mse"
    return None


def head_params(head):
    """The parameters of a head the kernels serve, in kernel order, or None: nn.Linear(F, 1) with a bias (SchNet's
    graph_pred_linear), or PaiNN's create_output_layers() at its defaults - Dense(F, F/2, silu) then Dense(F/2, 1) -
    with fp32 CUDA parameters at a served width."""
    from .Geom3D.models.painn import Dense
    if type(head) is nn.Linear:
        ps = (head.weight, head.bias)
        ok = head.out_features == 1 and head.bias is not None
        width = head.in_features
    elif type(head) is nn.Sequential and len(head) == 2 and all(type(m) is Dense for m in head):
        l0, l1 = head[0], head[1]
        ps = (l0.weight, l0.bias, l1.weight, l1.bias)
        ok = (l0.bias is not None and l1.bias is not None and l0.activation is F.silu
              and type(l1.activation) is nn.Identity and l0.out_features * 2 == l0.in_features
              and l1.in_features == l0.out_features and l1.out_features == 1)
        width = l0.in_features
    else:
        return None
    if not ok or not ops.property_width_ok(width):
        return None
    if not all(isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float32 for p in ps):
        return None
    return ps


def head_width(head):
    ps = head_params(head)
    return None if ps is None else ps[0].size(1)


def readout_of(model):
    """The backbone's readout as the fused head computes it ("mean" / "add" / "sum"), or None: a SchNet with a scale,
    mean / std, atomref or dipole head, or a readout the kernels do not have."""
    from .Geom3D.models.painn import PaiNN
    from .Geom3D.models.schnet import SchNet
    r = getattr(model, "readout", None)
    if r not in ops.PROPERTY_READOUTS:
        return None
    if isinstance(model, SchNet):
        if (model.scale is not None or model.mean is not None or model.std is not None or model.atomref is not None
                or model.dipole):
            return None
        return r
    if isinstance(model, PaiNN):
        return r
    return None


def model_width(model):
    return getattr(model, "hidden_channels", None) or getattr(model, "n_atom_basis", None)


def fused_ok(model, graph_pred_linear, criterion):
    """The step of these modules and this criterion runs on the fused head."""
    w = head_width(graph_pred_linear)
    return (loss_kind(criterion) is not None and w is not None and readout_of(model) is not None
            and model_width(model) == w)


def _n_mols(batch):
    return int(batch.num_graphs)


def _fused_batch_ok(batch, task_id):
    ds = getattr(batch, "_dataset", None)
    if ds is not None:   # a DeviceLoader handle: float32 / int64 tensors on its device
        return batch.device.type == "cuda" and ds.y is not None and 0 <= task_id < ds.y.size(1)
    pos, b, y = getattr(batch, "positions", None), getattr(batch, "batch", None), getattr(batch, "y", None)
    if not (pos is not None and b is not None and isinstance(y, torch.Tensor) and pos.is_cuda and not pos.requires_grad
            and pos.dtype == torch.float32 and b.is_cuda and b.dtype == torch.long and b.numel() > 0 and y.is_cuda
            and y.dtype == torch.float32 and not y.requires_grad):
        return False
    B = _n_mols(batch)
    return y.numel() % B == 0 and 0 <= task_id < y.numel() // B


# ------------------------------------------------------------------------------------------------------- targets
def target_column(batch, task_id):
    """batch.y.view(B, -1)[:, task_id] (pretrain_Supervised.py:96): a strided view of the collated targets."""
    B = _n_mols(batch)
    return batch.y.view(B, -1)[:, task_id]


def write_targets(g, batch, task_id):
    """The batch's target column into the static [B] target buffer of a step graph: for a DeviceLoader handle one
    launch over the dataset's targets, from the molecule offsets the step's gather already uploaded (the bucket's blob,
    or the dataset's staging buffer of a per-structure graph); for a collated batch one copy of its column."""
    dst = g["noise"]["target"]
    ds = getattr(batch, "_dataset", None)
    if ds is None:
        dst.copy_(target_column(batch, task_id))
        return
    bkt = g.get("bucket")
    if bkt is not None:
        src = bkt.blob.data_ptr() + 4 * bkt.off["src_off"]
    else:
        src = ds.__dict__["_src_off_dev"].data_ptr()
    ops.property_targets(ds.y, task_id, ds.mol_off(), src, batch.num_graphs, dst)


def _stats_tensor(device, mean, std):
    return torch.tensor([float(mean), float(std)], dtype=torch.float32).to(device)


class _Stats:
    """(mean, std) as a float32 [2] device tensor that a captured graph reads; written again only when they change."""

    def __init__(self, device):
        self.t = torch.zeros(2, dtype=torch.float32, device=device)
        self.host = None

    def set(self, mean, std):
        v = (float(mean), float(std))
        if v != self.host:
            self.t.copy_(torch.tensor(v, dtype=torch.float32))
            self.host = v
        return self.t


# --------------------------------------------------------------------------------------------------------- steps
def _x_of(args, batch):
    """The backbone's first argument in :86-90: SchNet gets the atom-type column, PaiNN batch.x unsliced.  (A 1-D
    batch.x - DatasetLBA's atomic numbers, which finetune_lba.py hands to the backbone as they are - is that column.)"""
    return batch.x if args.model_3d == "painn" or batch.x.dim() == 1 else batch.x[:, 0]


def supervised_step_fused(args, batch, model, graph_pred_linear, target, stats, loss):
    """The step as eager launches: the backbone's latent, then the fused head with the backbone's readout in it ->
    (loss fp32 scalar, normalised pred [B]).  target [B]: the task column; stats: float32 [2] (mean, std) on the
    device."""
    h, lay, dyn = backbone_latent(args.model_3d, batch, model, x=_x_of(args, batch), what="Supervised", layout=True)
    return ops.property_head(h, head_params(graph_pred_linear), lay, readout_of(model), target, stats, loss, dyn=dyn)


def supervised_step_aten(args, batch, model, graph_pred_linear, TRAIN_mean, TRAIN_std, task_id, criterion):
    """:84-101 as the reference writes them, on our backbone."""
    molecule_3D_repr = backbone_forward(args, batch, model, False, x=_x_of(args, batch))

    if graph_pred_linear is not None:
        pred = graph_pred_linear(molecule_3D_repr).squeeze()
    else:
        pred = molecule_3D_repr.squeeze()

    B = pred.size()[0]
    y = batch.y.view(B, -1)[:, task_id]
    y = (y - TRAIN_mean) / TRAIN_std

    loss = criterion(pred, y)
    return loss


class _StepArgs:
    """What the replayed step reads: the backbone kind, the loss kind, the task column and the (mean, std) tensor."""

    def __init__(self, model_3d, loss, task_id, stats, mode="auto"):
        self.model_3d, self.loss, self.task_id, self.stats = model_3d, loss, int(task_id), stats
        self.step_graph_mode = mode


# (no draws: the batch's target column, the graph's static input "target", is the one per-step input beside the
# molecules; a graph binds the loss kind, the task column is chosen when the targets are written)
def _supervised_forward(owner, args, batch, noise):
    target = noise["target"] if noise is not None else target_column(batch, args.task_id)   # (None: an eager step)
    return supervised_step_fused(args, batch, owner.model, owner.n1, target, args.stats, args.loss)[0]


SUPERVISED = Objective(
    "Supervised", _supervised_forward,
    graph_key=lambda args: ("Supervised", args.model_3d, args.loss, args.task_id),
    noise_keys=lambda args: ("target",),
    capture_inputs=lambda owner, args, batch, noise: {"target": target_column(batch, args.task_id)},
    write_inputs=lambda owner, args, g, batch, noise: write_targets(g, batch, args.task_id),
    pair_tuples=False)


def _raise_like_squeeze(B):
    # the reference's pred.squeeze() turns a [1, 1] prediction into a 0-d tensor, and pred.size()[0] then raises
    if B == 1:
        raise IndexError("tuple index out of range")


def do_Supervised(args, batch, model, graph_pred_linear, TRAIN_mean, TRAIN_std, task_id=6, criterion=None, graph=None):
    """examples/pretrain_Supervised.py:79-104 (and finetune_qm9.py:177-259) -> the fp32 loss.  args.model_3d picks the
    backbone call ("schnet" / "painn"; PaiNN gets batch.x unsliced, like the reference); criterion None means
    args.loss ("mae": nn.L1Loss(), "mse": nn.MSELoss()).  The fused step runs for a stock mean L1 / MSE criterion,
    graph_pred_linear = Linear(F, 1) or PaiNN's default create_output_layers(), an unscaled backbone with a mean / add
    readout at F = 64 / 128 / 256, and CUDA batches with float32 targets; anything else (another criterion or a subclass,
    another head, num_tasks > 1, SchNet with mean / std / atomref, other widths, CPU tensors) runs the reference's ATen
    lines.  At B = 1 it raises IndexError, as the reference does (pred.squeeze() is 0-d there).  graph: replay HIP graphs
    of forward + backward (default: ``args.step_graph`` if present, else on unless GEOSSL_NO_STEP_GRAPH is set)."""
    if criterion is None:
        criterion = criterion_of(args)
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    if not (fused_ok(model, graph_pred_linear, criterion) and _fused_batch_ok(batch, task_id)):
        return supervised_step_aten(args, batch, model, graph_pred_linear, TRAIN_mean, TRAIN_std, task_id, criterion)
    _raise_like_squeeze(_n_mols(batch))
    kind = loss_kind(criterion)
    a = _StepArgs(args.model_3d, kind, task_id, None)

    def stats_on(eng):   # the (mean, std) tensor the engine's graphs read lives on the engine
        if "stats" not in eng.__dict__:
            eng.stats = _Stats(eng.gflat.device)
        a.stats = eng.stats.set(TRAIN_mean, TRAIN_std)
    loss = run_graphed(args, graph, model, "_geossl_supervised_step", SUPERVISED, a, batch, n1=graph_pred_linear,
                       prepare=stats_on)
    if loss is not None:
        return loss
    dev = head_params(graph_pred_linear)[0].device
    loss, _ = supervised_step_fused(args, batch, model, graph_pred_linear, target_column(batch, task_id),
                                    _stats_tensor(dev, TRAIN_mean, TRAIN_std), kind)
    return loss


@torch.no_grad()
def predict_Supervised(args, batch, model, graph_pred_linear, TRAIN_mean, TRAIN_std):
    """eval() of finetune_qm9.py:290-374 for one batch -> pred * TRAIN_std + TRAIN_mean [B] under no_grad.  The fused
    forward serves what do_Supervised's fused step serves; anything else runs the reference's lines.  B = 1 raises
    IndexError, as the reference's pred.size()[0] does."""
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    ps = head_params(graph_pred_linear)
    pos = getattr(batch, "positions", None) if getattr(batch, "_dataset", None) is None else None
    cuda = getattr(batch, "_dataset", None) is not None or (pos is not None and pos.is_cuda)
    if (ps is None or readout_of(model) is None or model_width(model) != ps[0].size(1) or not cuda):
        molecule_3D_repr = backbone_forward(args, batch, model, False, x=_x_of(args, batch))
        if graph_pred_linear is not None:
            pred = graph_pred_linear(molecule_3D_repr).squeeze()
        else:
            pred = molecule_3D_repr.squeeze()
        B = pred.size()[0]  # noqa: F841  (the reference's, :370: raises at B = 1)
        return pred * TRAIN_std + TRAIN_mean
    _raise_like_squeeze(_n_mols(batch))
    h, lay, dyn = backbone_latent(args.model_3d, batch, model, x=_x_of(args, batch), what="Supervised", layout=True)
    return ops.property_predict(h, ps, lay, readout_of(model), _stats_tensor(h.device, TRAIN_mean, TRAIN_std), dyn=dyn)


@torch.no_grad()
def eval_Supervised(args, loader, model, graph_pred_linear, TRAIN_mean, TRAIN_std, task_id=6, use_graph=None,
                    arrays=True, stats=None):
    """examples/finetune_qm9.py eval(), :278-384 -> (mae, y_true, y_scores): float32 numpy arrays in loader order, y_true
    the raw target column, y_scores = pred * TRAIN_std + TRAIN_mean, mae = np.mean(np.abs(y_scores - y_true)) of the two
    arrays on the host.  Batches are moved to the backbone's device.  ``use_graph`` (None:
    ``evaluate.USE_GRAPH_DEFAULT["property"]``, set from the measurement in DESIGN 5): the loop is ``evaluate.Evaluator.run`` - one forward-only graph per batch size
    of a ragged loader, the rows collected on the device by one launch per batch, one read of each array behind the loop;
    a batch the fused head refuses gets ``predict_Supervised`` as it is, and CPU modules take the reference's loop whole.
    ``arrays=False`` -> the MAE alone, from the fp64 sum of |y_scores - y_true| kept on the device (graph route; else
    from the arrays).  stats: a ``_Stats`` the graphs read instead of the evaluator's own (the trainer's)."""
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    model.eval()
    if graph_pred_linear is not None:
        graph_pred_linear.eval()
    params = list(model.parameters())
    device = params[0].device if params else torch.device("cpu")
    from . import evaluate
    if use_graph is None:
        use_graph = evaluate.USE_GRAPH_DEFAULT["property"]
    if use_graph and device.type == "cuda":
        ev = evaluate.evaluator_for(model, graph_pred_linear, args.model_3d, "property", task_id, stats=stats)
        ev.stats.set(TRAIN_mean, TRAIN_std)
        sum_a, _, rows, y_true, y_scores = ev.run(
            loader, arrays, eager=lambda b: predict_Supervised(args, b, model, graph_pred_linear, TRAIN_mean, TRAIN_std))
        if not arrays:
            return sum_a / rows if rows else float("nan")
        mae = np.mean(np.abs(y_scores - y_true))
        return mae, y_true, y_scores

    y_true = []
    y_scores = []
    for batch in loader:
        if hasattr(batch, "to"):
            batch = batch.to(device)
        pred = predict_Supervised(args, batch, model, graph_pred_linear, TRAIN_mean, TRAIN_std)
        B = pred.size()[0]
        y = batch.y.view(B, -1)[:, task_id]

        y_true.append(y)
        y_scores.append(pred)

    y_true = torch.cat(y_true, dim=0).cpu().numpy()
    y_scores = torch.cat(y_scores, dim=0).cpu().numpy()

    mae = np.mean(np.abs(y_scores - y_true))
    if not arrays:
        return float(mae)
    return mae, y_true, y_scores


# -------------------------------------------------------------------------------------------------------- trainer
class SupervisedTrainer(StepTrainer):
    """The body of ``train()`` (pretrain_Supervised.py:66-119, finetune_qm9.py:163-275): backbone latent, fused property
    head with the readout in it, backward, gradient all-reduce, Adam - backbone and graph_pred_linear in one flat buffer
    (one fused Adam launch: both of the reference's groups run at args.lr), no host sync inside ``step``.
    ``step(batch) -> loss`` on the device.  ``set_lr(lr)`` between epochs is how a schedule is applied
    (``optim.cosine_annealing_lr`` is CosineAnnealingLR's), ``set_stats(mean, std)`` changes the target normalisation
    without a recapture.  ``use_graph=True``: forward + backward are captured into HIP graphs and replayed (ragged SchNet /
    PaiNN batches and DeviceLoader handles share one ONE-view capacity-bucket graph per batch size at width 128 - SchNet
    handles with structures of 256 to 1024 atoms, LBA's pockets, through the sparse bucket of geossl_amd/bucket.py, and
    collated batches of such structures with GEOSSL_SPARSE_BUCKETS=1; PaiNN handles of a dataset built with ``radius=``
    likewise, collated PaiNN batches with GEOSSL_PAINN_SPARSE_BUCKETS=1; anything else one graph per structure); the
    target column is a static input of the graph."""

    def __init__(self, model, graph_pred_linear, TRAIN_mean, TRAIN_std, task_id=6, loss="mae", lr=5e-4,
                 weight_decay=0.0, model_3d="schnet", use_graph=False, max_graphs=256, graph_mode="auto"):
        if loss not in ops.PROPERTY_LOSSES:
            raise ValueError("loss is 'mae' or 'mse', got %r" % (loss,))
        ps = head_params(graph_pred_linear)
        if ps is None or readout_of(model) is None or model_width(model) != ps[0].size(1):
            raise ValueError("SupervisedTrainer needs graph_pred_linear = Linear(F, 1) or PaiNN's default "
                             "create_output_layers() at F = 64, 128 or 256 on the GPU and a backbone of that width with an "
                             "unscaled mean / add readout; use do_Supervised for anything else")
        self.head = graph_pred_linear
        self.model_3d, self.loss_kind, self.task_id = model_3d, loss, int(task_id)
        self.stats = _Stats(ps[0].device)
        self.stats.set(TRAIN_mean, TRAIN_std)
        super().__init__([model, graph_pred_linear], SUPERVISED, _StepArgs(model_3d, loss, task_id, self.stats.t), lr,
                         weight_decay, use_graph, max_graphs, graph_mode)

    def set_stats(self, mean, std):
        """TRAIN_mean / TRAIN_std of the following steps (read on the device: no recapture)."""
        self.stats.set(mean, std)

    def step(self, batch):
        """One training step -> the loss on the device.  (The trainer's own: the reference's IndexError at B = 1.)"""
        _raise_like_squeeze(_n_mols(batch))
        return super().step(batch)

    def predict(self, batch):
        """eval()'s predictions of one batch with the trainer's parameters and (mean, std); with ``use_graph`` through
        the forward-only graphs of ``evaluate.Evaluator`` (which read the trainer's (mean, std) tensor)."""
        mean, std = self.stats.host
        eager = lambda b: predict_Supervised(self.args, b, self.model, self.head, mean, std)
        if self.use_graph:
            from .evaluate import evaluator_for
            return evaluator_for(self.model, self.head, self.model_3d, "property", self.task_id,
                                 stats=self.stats).predict(batch, eager)
        return eager(batch)

    def evaluate(self, loader, arrays=True, use_graph=None):
        """eval() over a loader with the trainer's parameters and (mean, std) -> what ``eval_Supervised`` returns:
        (mae, y_true, y_scores), or the MAE alone with ``arrays=False``.  use_graph None: replayed when the trainer's
        ``use_graph`` is on, else ``eval_Supervised``'s measured default."""
        mean, std = self.stats.host
        if use_graph is None:
            use_graph = True if self.use_graph else None
        return eval_Supervised(self.args, loader, self.model, self.head, mean, std, self.task_id, use_graph=use_graph,
                               arrays=arrays, stats=self.stats)
