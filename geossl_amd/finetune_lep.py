"""Step API of ``examples/finetune_lep.py`` (ligand efficacy prediction: a binary label per protein-ligand pair seen in
its active and its inactive conformation) on the HIP path.

``do_LEP(args, batch, model, graph_pred_linear, criterion)`` is the body of ``train()``, :31-45, as one call -> the fp32
loss.  The reference runs the backbone twice per step, once per conformation; here both go through it ONCE, as one batch
of 2B structures ``[active 0 .. B-1 | inactive 0 .. B-1]`` (``fused_batch``: built once per batch object from the sizes
the collation keeps on the host), and the fused head of csrc/pair_head.hip forms the two readouts, the logit of
``Linear(2F, 1)`` and the mean BCE-with-logits.  Every backbone weight is thus used once on 2B structures where the
reference uses it twice and lets autograd add: the gradients agree to rounding, not bit for bit.  A side above 255 atoms
puts the whole fused batch on the sparse pair list (geossl_amd/layout.py), as for LBA.  The loss supports the
reference's own ``optimizer.zero_grad(); loss.backward(); optimizer.step()`` with a stock ``torch.optim.Adam``.

Anything the kernels do not serve runs the reference's own ATen lines on our backbone, two passes - B = 1 included, where
the reference's ``.squeeze()`` makes ``pred`` 0-d against a ``[1]`` target and ``BCEWithLogitsLoss`` raises ValueError.
``predict_LEP`` / ``eval_LEP`` mirror ``eval()``, :66-101, with the two rank metrics in numpy (sklearn's definitions).
``LEPTrainer`` is the ``train()`` body on the fused step with backbone and head in one flat buffer.

On shuffled pairs no two batches share both size sequences, so a graph keyed by them is never replayed.  The step reads
no pair tuples (``LEP.pair_tuples`` is False): a SchNet batch whose layout is sparse - a structure of either side above
255 atoms, or GEOSSL_SPARSE_PAIRS=1 - goes through ONE sparse capacity bucket (``bucket.SPARSE``) of 2B structures per
batch size, with the pair head's ``_dyn`` forms reading the real atom count on the device.  The switch is
GEOSSL_SPARSE_BUCKETS (switches.sparse_buckets): unset, the pair handles of a ``DeviceLoader`` over a
``PairedDeviceDataset`` take the bucket and collated ``BatchLEP`` batches keep their routing; 1: both; 0: neither.
A handle's fill is one pinned upload, one gather launch over the 2B structures and one launch that writes the labels
from the dataset's ``y`` on the device; nothing is read back and nothing is concatenated per step.  A batch whose
structures are all <= 255 atoms, a structure above 1024 atoms and PaiNN keep the per-structure graph or eager launches.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .batch import Batch
from .pretrain_Supervised import model_width, readout_of
from .step import Objective, StepTrainer, backbone_latent, run_graphed, stock_bce


# ---------------------------------------------------------------------------------------------------- what is served
def head_params(head):
    """(weight, bias) of a head the kernels serve - nn.Linear(2F, 1) with a bias, fp32 CUDA parameters, F a served
    width - or None."""
    if type(head) is not nn.Linear or head.out_features != 1 or head.bias is None or head.in_features % 2:
        return None
    ps = (head.weight, head.bias)
    if not all(p.is_cuda and p.dtype == torch.float32 for p in ps):
        return None
    return ps if ops.pair_head_width_ok(head.in_features // 2) else None


def modules_ok(model, graph_pred_linear):
    """Backbone and head run on the fused pair head: an unscaled mean / add readout at a width F the kernels take and
    Linear(2F, 1)."""
    ps = head_params(graph_pred_linear)
    return ps is not None and readout_of(model) is not None and model_width(model) * 2 == ps[0].size(1)


def _is_handle(batch):
    """A PairedBatch of a DeviceLoader over a PairedDeviceDataset (or its fused 2B-structure handle)."""
    return getattr(batch, "_dataset", None) is not None


def _check_handle(batch, model_3d):
    if model_3d == "painn" and _is_handle(batch):
        ds = getattr(batch._dataset, "structures", batch._dataset)
        if ds.edges is None:
            raise ValueError("this PairedDeviceDataset holds no radius edges: build it with radius=..., or collate "
                             "PaiNN pairs with DataLoaderLEP")


def _fused_batch_ok(batch):
    if _is_handle(batch):   # float32 / int64 tensors on its device, one label per pair, by construction
        return batch.device.type == "cuda" and _n_pairs(batch) >= 2
    need = ("x_active", "positions_active", "batch_active", "x_inactive", "positions_inactive", "batch_inactive", "y")
    ts = [getattr(batch, k, None) for k in need]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        return False
    xa, pa, ba, xi, pi, bi, y = ts
    if not (pa.dtype == torch.float32 and pi.dtype == torch.float32 and not pa.requires_grad and not pi.requires_grad
            and ba.dtype == torch.long and bi.dtype == torch.long and ba.numel() > 0 and bi.numel() > 0
            and xa.dim() == xi.dim() and not y.requires_grad):
        return False
    B = _n_pairs(batch)
    return B >= 2 and y.dim() == 1 and y.numel() == B


def _n_pairs(batch):
    sizes = getattr(batch, "_sizes_active", None)
    return len(sizes) if sizes is not None else int(batch.num_graphs)


# ------------------------------------------------------------------------------------------------- the one-pass batch
_BATCH_VECTORS = OrderedDict()   # (device, both size sequences) -> the fused batch vector


def _fused_batch_vector(batch, sizes):
    """cat(batch_active, batch_inactive + B).  It is a function of the two size sequences, so batches that agree in them
    get the SAME tensor object: the layout cached on it is built once, and a step graph - which identifies such a batch
    by its index tensors (batch.structure_fingerprint) - serves them all."""
    key = (batch.batch_active.device, sizes.tobytes())
    vec = _BATCH_VECTORS.get(key)
    if vec is None:
        B = len(sizes) // 2
        vec = _BATCH_VECTORS[key] = torch.cat([batch.batch_active, batch.batch_inactive + B])
        from .layout import prepare_batch
        prepare_batch(vec, None, sizes.tolist(), lazy=True)   # (the host sizes: a layout without a device read-back)
        while len(_BATCH_VECTORS) > 64:
            _BATCH_VECTORS.popitem(last=False)
    else:
        _BATCH_VECTORS.move_to_end(key)
    return vec


def _host_sizes(batch, side):
    sizes = getattr(batch, "_sizes_" + side, None)
    if sizes is None:   # (a batch built by hand: one read-back, then kept)
        sizes = torch.bincount(getattr(batch, "batch_" + side), minlength=int(batch.num_graphs)).cpu().numpy()
        setattr(batch, "_sizes_" + side, sizes)
    return np.asarray(sizes, dtype=np.int64)


def fused_batch(batch):
    """The two conformations as ONE batch of 2B structures [active 0 .. B-1 | inactive 0 .. B-1] - a plain
    ``batch.Batch`` without tuples - built once per batch object and kept on it.  PaiNN: the inactive side's
    edges are shifted by the TOTAL active atom count (the loader has already applied the per-side running counts).
    ``y`` is the batch's label tensor as float32, taken anew at every call."""
    if isinstance(batch, Batch) or hasattr(batch, "pairs"):
        return batch
    if _is_handle(batch):   # a PairedBatch: the 2B structures are a handle on the dataset's structures - no host cat
        return batch.fused()
    fb = batch.__dict__.get("_geossl_fused")
    if fb is None:
        sizes = np.concatenate([_host_sizes(batch, "active"), _host_sizes(batch, "inactive")])
        rei = None
        if getattr(batch, "radius_edge_index_active", None) is not None:
            n_active = int(batch.batch_active.numel())
            rei = torch.cat([batch.radius_edge_index_active, batch.radius_edge_index_inactive + n_active], dim=1)
        fb = Batch(torch.cat([batch.x_active, batch.x_inactive]),
                   torch.cat([batch.positions_active, batch.positions_inactive]), _fused_batch_vector(batch, sizes),
                   None, radius_edge_index=rei, num_graphs=len(sizes), sizes=sizes)
        batch.__dict__["_geossl_fused"] = fb
    y = batch.y
    fb.y = y if y.dtype == torch.float32 else y.float()   # (:43)
    return fb


# --------------------------------------------------------------------------------------------------------- steps
def _forward_aten(args, batch, model, graph_pred_linear):
    """:33-42 as the reference writes them, on our backbone."""
    if args.model_3d == "schnet":
        active_mol_repr = model(batch.x_active, batch.positions_active, batch.batch_active)
        inactive_mol_repr = model(batch.x_inactive, batch.positions_inactive, batch.batch_inactive)
    elif args.model_3d == "painn":
        active_mol_repr = model(batch.x_active, batch.positions_active, batch.radius_edge_index_active,
                                batch.batch_active)
        inactive_mol_repr = model(batch.x_inactive, batch.positions_inactive, batch.radius_edge_index_inactive,
                                  batch.batch_inactive)
    else:
        raise Exception("3D model {} not included.".format(args.model_3d))

    molecule_3D_repr = torch.cat((active_mol_repr, inactive_mol_repr), dim=1)

    pred = graph_pred_linear(molecule_3D_repr).squeeze()
    return pred


def lep_step_aten(args, batch, model, graph_pred_linear, criterion):
    """:33-45 as the reference writes them, on our backbone (two passes)."""
    pred = _forward_aten(args, batch, model, graph_pred_linear)
    actual = batch.y.float()

    loss = criterion(pred, actual)
    return loss


def lep_step_fused(model_3d, fb, model, graph_pred_linear, y):
    """The step as eager launches on the one-pass batch ``fb``: the backbone's latent of the 2B structures, then the
    fused pair head with the readout in it -> (loss fp32 scalar, logits [B]).  y: the labels as float32 - the leading B
    entries are read (the static "target" of a bucket graph has one row per structure).  ``fb`` may be the static batch
    of a sparse bucket of 2B structures: the head then reads the real atom count on the device (``dims``)."""
    h, lay, dyn = backbone_latent(model_3d, fb, model, x=_x_of(model_3d, fb), what="LEP", layout=True)
    w, b = head_params(graph_pred_linear)
    return ops.pair_head(h, w, b, lay, readout_of(model), y[:int(lay.B) // 2], dyn=dyn)


def _x_of(model_3d, fb):
    """The backbone's first argument: the atom types as the records hold them (1-D), which a DeviceDataset and a bucket
    keep as one column."""
    return fb.x[:, 0] if model_3d == "schnet" and fb.x.dim() == 2 else fb.x


def write_labels(g, fb):
    """The batch's labels into the leading B entries of the graph's static "target": a collated batch's by one copy;
    a handle's by one launch over the dataset's labels, from the structure offsets the step's gather has just uploaded
    (the bucket's blob, or the dataset's staging buffer of a per-structure graph) - the active structure of pair m is
    structure m of the dataset.  Nothing is read back."""
    dst, B = g["noise"]["target"], int(fb.num_graphs) // 2
    pairs = getattr(fb, "pairs", None)
    if pairs is None:
        dst[:B].copy_(fb.y)
        return
    pds, bkt = pairs._dataset, g.get("bucket")
    if bkt is not None:
        src = bkt.blob.data_ptr() + 4 * bkt.off["src_off"]
    else:
        src = pds.structures.__dict__["_src_off_dev"].data_ptr()
    ops.property_targets(pds.y.view(-1, 1), 0, pds.structures.mol_off(), src, B, dst)


class _StepArgs:
    """What the replayed step reads: the backbone kind (and the graph mode of its StepGraphs)."""

    def __init__(self, model_3d, mode="auto"):
        self.model_3d, self.step_graph_mode = model_3d, mode


# (no draws: the labels, the graph's static input "target", are the one per-step input beside the structures - data of a
# graph, not structure: batches that agree in their index tensors share a graph whatever their labels; no pair tuples
# are read, so a batch with a sparse layout - a structure above 255 atoms - may go through a sparse bucket of 2B structures)
LEP = Objective(
    "LEP",
    lambda owner, args, fb, noise:   # (noise None: an eager step, the batch's own labels)
        lep_step_fused(args.model_3d, fb, owner.model, owner.n1, noise["target"] if noise is not None else fb.y)[0],
    noise_keys=lambda args: ("target",),
    capture_inputs=lambda owner, args, fb, noise: {"target": fb.y},
    write_inputs=lambda owner, args, g, fb, noise: write_labels(g, fb),
    pair_tuples=False)


def do_LEP(args, batch, model, graph_pred_linear, criterion=None, graph=None):
    """examples/finetune_lep.py:31-45 -> the fp32 loss.  args.model_3d picks the backbone call ("schnet" / "painn");
    criterion None means the script's nn.BCEWithLogitsLoss(); batch.y may be integer (:43).  The fused one-pass step runs
    for a stock mean BCEWithLogitsLoss, graph_pred_linear = Linear(2F, 1) with a bias, an unscaled backbone with a
    mean / add readout at F = 32 / 64 / 128, and CUDA batches of B >= 2 pairs with one label per pair; anything else runs
    the reference's ATen lines (two passes) - at B = 1 they raise ValueError, as the reference does.  batch: a collated
    ``BatchLEP`` or a ``DeviceLoader`` pair handle (``PairedBatch``; PaiNN: of a dataset built with ``radius=``).  graph: replay HIP graphs of forward +
    backward (default: ``args.step_graph`` if present, else on unless GEOSSL_NO_STEP_GRAPH is set): the sparse bucket
    graph of ``LEPTrainer``'s routing where that serves the batch, else a graph of its own at the second sighting of its
    index tensors."""
    if criterion is None:
        criterion = nn.BCEWithLogitsLoss()
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    _check_handle(batch, args.model_3d)
    if not (stock_bce(criterion) and modules_ok(model, graph_pred_linear) and _fused_batch_ok(batch)):
        return lep_step_aten(args, batch, model, graph_pred_linear, criterion)
    fb = fused_batch(batch)
    loss = run_graphed(args, graph, model, "_geossl_lep_step", LEP, _StepArgs(args.model_3d), fb, n1=graph_pred_linear)
    if loss is not None:
        return loss
    return lep_step_fused(args.model_3d, fb, model, graph_pred_linear, fb.y)[0]


@torch.no_grad()
def predict_LEP(args, batch, model, graph_pred_linear):
    """eval()'s forward for one batch, :77-85 -> the logits [B] (a 0-d tensor at B = 1, on the ATen lines)."""
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    _check_handle(batch, args.model_3d)
    if not (modules_ok(model, graph_pred_linear) and _fused_batch_ok(batch)):
        return _forward_aten(args, batch, model, graph_pred_linear)
    fb = fused_batch(batch)
    h, lay, dyn = backbone_latent(args.model_3d, fb, model, x=_x_of(args.model_3d, fb), what="LEP", layout=True)
    w, b = head_params(graph_pred_linear)
    return ops.pair_predict(h, w, b, lay, readout_of(model), dyn=dyn)


# ------------------------------------------------------------------------------------------------------- metrics
def _binary(y_true):
    y = np.asarray(y_true).reshape(-1)
    classes = np.unique(y)
    if classes.size > 2:
        raise ValueError("binary labels expected, got %d classes" % classes.size)
    return y == classes[-1] if classes.size == 2 else y == 1, classes.size


def _threshold_counts(y_true, y_score):
    """Cumulative true / false positives at every DISTINCT score, scores descending (tied scores form one threshold)."""
    pos, n_classes = _binary(y_true)
    score = np.asarray(y_score, dtype=np.float64).reshape(-1)
    if score.size != pos.size:
        raise ValueError("y_true and y_score differ in length")
    order = np.argsort(-score, kind="mergesort")
    score, pos = score[order], pos[order]
    last = np.r_[np.nonzero(np.diff(score))[0], score.size - 1] if score.size else np.zeros(0, dtype=np.int64)
    tps = np.cumsum(pos, dtype=np.float64)[last]
    fps = (1.0 + last) - tps
    return tps, fps, n_classes


def roc_auc(y_true, y_score):
    """sklearn.metrics.roc_auc_score for binary labels: the trapezoidal area under (FPR, TPR) over the distinct
    thresholds.  One class present: ValueError, as sklearn raises."""
    tps, fps, n_classes = _threshold_counts(y_true, y_score)
    if n_classes != 2:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    tpr, fpr = np.r_[0.0, tps] / tps[-1], np.r_[0.0, fps] / fps[-1]
    return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))


def average_precision(y_true, y_score):
    """sklearn.metrics.average_precision_score for binary labels: the step-wise sum over the distinct thresholds of
    (R_k - R_{k-1}) P_k."""
    tps, fps, _ = _threshold_counts(y_true, y_score)
    if tps.size == 0 or tps[-1] == 0:
        return 0.0   # (no positive label: sklearn warns and returns 0)
    precision, recall = tps / (tps + fps), tps / tps[-1]
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


@torch.no_grad()
def eval_LEP(args, loader, model, graph_pred_linear, use_graph=False):
    """examples/finetune_lep.py eval(), :66-101 -> (sqrt(sum_b loss_b B_b / total), roc, pr, y_true, y_pred) with the
    script's nn.BCEWithLogitsLoss().  Batches are moved to the backbone's device.  ``use_graph=True`` (GPU modules; CPU
    modules take the loop below whole): the loop is ``evaluate.Evaluator.run`` - forward-only graphs of the one-pass batch
    on the training step's routing, no read inside the loop - and y_true / y_pred are float32 numpy arrays read once.
    The one known difference: the loss figure is sqrt(sum of the fp32 BCE terms in fp64 over all rows / rows) instead of
    the sum of per-batch fp32 means times B."""
    model.eval()
    if graph_pred_linear is not None:
        graph_pred_linear.eval()
    device = next(model.parameters()).device
    if use_graph and device.type == "cuda":
        if args.model_3d not in ("schnet", "painn"):
            raise Exception("3D model {} not included.".format(args.model_3d))
        from .evaluate import evaluator_for
        ev = evaluator_for(model, graph_pred_linear, args.model_3d, "pair")
        sum_a, _, rows, y_true, y_pred = ev.run(loader, eager=lambda b: predict_LEP(args, b, model, graph_pred_linear))
        return np.sqrt(sum_a / rows), roc_auc(y_true, y_pred), average_precision(y_true, y_pred), y_true, y_pred
    criterion = nn.BCEWithLogitsLoss()

    loss_all, total = 0, 0
    y_true, y_pred = [], []

    for batch in loader:
        batch = batch.to(device)
        output = predict_LEP(args, batch, model, graph_pred_linear)
        y = batch.y.float()

        B = y.size()[0]

        loss = criterion(output, y)
        loss_all += loss.item() * B
        total += B
        y_true.extend(y.detach().cpu().tolist())
        y_pred.extend(output.detach().cpu().tolist())

    y_true = np.array(y_true)
    y_pred = np.array(y_pred)
    roc = roc_auc(y_true, y_pred)
    pr = average_precision(y_true, y_pred)

    return np.sqrt(loss_all / total), roc, pr, y_true, y_pred


# -------------------------------------------------------------------------------------------------------- trainer
class LEPTrainer(StepTrainer):
    """The body of ``train()`` (finetune_lep.py:17-62) on the one-pass step: backbone latent of the 2B structures, fused
    pair head with the readout in it, backward, gradient all-reduce, Adam - backbone and graph_pred_linear in one flat
    buffer (one fused Adam launch: both of the reference's groups run at args.lr), no host sync inside ``step``.
    ``step(batch) -> loss`` on the device; ``set_lr(lr)`` between epochs is how a schedule is applied.
    ``use_graph=True``: forward + backward are captured into HIP graphs and replayed; the labels are a static input of
    the graph.  ``graph_mode="auto"``: SchNet batches with a sparse layout (a structure of either side above 255 atoms, up
    to 1024; or GEOSSL_SPARSE_PAIRS=1) at width 128 share ONE sparse capacity-bucket graph of 2B structures per batch
    size - the pair handles of a ``DeviceLoader`` over a ``PairedDeviceDataset`` by default, collated ``BatchLEP``
    batches with GEOSSL_SPARSE_BUCKETS=1 (``=0``: neither); PaiNN batches the same way under
    GEOSSL_PAINN_SPARSE_BUCKETS (pair handles of a ``PairedDeviceDataset(..., radius=r)``, collated batches with their
    ``radius_edge_index_*``); anything else - all structures <= 255 atoms, other widths - one graph per structure of the
    fused batch, from its second sighting on.  ``step`` takes a collated ``BatchLEP`` or a pair handle (PaiNN: of a
    dataset built with ``radius=``)."""

    def __init__(self, model, graph_pred_linear, lr=5e-4, weight_decay=0.0, model_3d="schnet", use_graph=False,
                 max_graphs=256, graph_mode="auto"):
        if not modules_ok(model, graph_pred_linear):
            raise ValueError("LEPTrainer needs graph_pred_linear = Linear(2F, 1) with a bias at F = 32, 64 or 128 on the "
                             "GPU and a backbone of width F with an unscaled mean / add readout; use do_LEP for "
                             "anything else")
        if model_3d not in ("schnet", "painn"):
            raise Exception("3D model {} not included.".format(model_3d))
        self.head, self.model_3d = graph_pred_linear, model_3d
        super().__init__([model, graph_pred_linear], LEP, _StepArgs(model_3d), lr, weight_decay, use_graph, max_graphs,
                         graph_mode)

    # the trainer's own: a collated pair batch or a pair handle becomes the one-pass batch before either route
    def _one_pass(self, batch):
        _check_handle(batch, self.model_3d)
        if not isinstance(batch, Batch) and not hasattr(batch, "pairs") and not _fused_batch_ok(batch):
            raise ValueError("LEPTrainer needs CUDA batches of B >= 2 pairs with one label per pair; use do_LEP for "
                             "anything else")
        return fused_batch(batch)

    def _eager(self, batch, noise=None):
        return super()._eager(self._one_pass(batch), noise)

    def _graph_fwd_bwd(self, batch, noise=None):
        return super()._graph_fwd_bwd(self._one_pass(batch), noise)

    def predict(self, batch):
        """eval()'s logits of one batch with the trainer's parameters; with ``use_graph`` through the forward-only graphs
        of ``evaluate.Evaluator``."""
        eager = lambda b: predict_LEP(_StepArgs(self.model_3d), b, self.model, self.head)
        if self.use_graph:
            from .evaluate import evaluator_for
            _check_handle(batch, self.model_3d)
            return evaluator_for(self.model, self.head, self.model_3d, "pair").predict(batch, eager)
        return eager(batch)

    def evaluate(self, loader, use_graph=None):
        """eval() over a loader with the trainer's parameters -> what ``eval_LEP`` returns.  use_graph None: replayed
        when the trainer's ``use_graph`` is on, else the measured default ``evaluate.USE_GRAPH_DEFAULT["pair"]``."""
        if use_graph is None:
            from .evaluate import USE_GRAPH_DEFAULT
            use_graph = self.use_graph or USE_GRAPH_DEFAULT["pair"]
        return eval_LEP(_StepArgs(self.model_3d), loader, self.model, self.head, use_graph=use_graph)
