"""Step API of ``examples/finetune_md17.py`` (train() :17-67 and eval() :70-123: energies and forces of MD17 trajectories)
on the HIP path.

``do_MD17(args, batch, model, graph_pred_linear)`` is the loop body :31-51 as one call: the backbone, the energy head,
``pred_force = -grad(pred_energy, positions, create_graph=True)`` and the loss on energy and force
(``ops.energy_force_loss``); its autograd graph goes through the force, so the reference's own ``loss.backward()`` and a
stock Adam work.  ``predict_MD17`` is eval()'s forward (:83-99) -> (energies, forces), detached: on the fused route the
backbone's latent goes through ``geossl_energy_head_fwd`` (csrc/force_head.hip), which returns the energies and the seed
d(sum E)/dh, and the seed goes through the backbone's first-order position gradient - no autograd engine, and with
``use_graph`` one captured graph per batch structure.  ``eval_MD17`` is eval() over a loader -> (energy MAE, force MAE)
with one device read at its end.  ``MD17Trainer`` is train()'s body on ``graphed.ForceTrainer``.

The complete pair list.  All frames of an MD17 trajectory have the same atoms, so the index structure of a batch of B
frames of n atoms depends on (B, n) alone - except PaiNN's ``radius_edge_index``, which ``DatasetMD17Radius`` builds per
frame (datasets_MD17Radius.py:35).  For n <= 33 the directed complete pair list (n (n - 1) edges per molecule, target
-major, sources ascending) is ``radius_graph(pos, r=inf)`` under the 32-neighbour cap and a superset of every frame's
radius list in the same relative order.  PaiNN multiplies every filter row by ``0.5 (cos(d pi / r) + 1) [d < r]``
(painn_utils.py:152-154), so an edge at d >= r contributes exact zeros to the energy, the force and every first- and
second-order gradient (the mask has no derivative), and adding +0.0 terms in an otherwise unchanged order changes no sum:
the step on the complete list is the reference's step on the frame's own list, up to the rounding of the edge-batched
GEMMs and pairs within rounding of the cutoff (where the envelope is ~0 anyway).  Its index tensors are interned per
(B, n) (``complete_edges``), so ``ForceTrainer``'s tensor-identity keying replays ONE graph for a whole trajectory.
``GEOSSL_MD17_COMPLETE_EDGES`` = 0 / 1 forces the choice (switches.md17_complete_edges).
"""
import types

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import grad

from . import _lib, bucket as bk, ops, switches
from .batch import Batch
from .graphed import ForceTrainer
from .layout import get_layout
from .pretrain_Supervised import model_width, readout_of
from .replay import StructureGraphs, capture, copy_static, owned_batch_vector, parameter_addresses, sizes_key, warm_up
from .step import latent

__all__ = ["do_MD17", "predict_MD17", "eval_MD17", "MD17Trainer", "complete_edges", "COMPLETE_MAX_N"]

COMPLETE_MAX_N = 33   # radius_graph keeps 32 neighbours per atom (max_num_neighbors): the complete list of n <= 33 atoms


# ------------------------------------------------------------------------------------------- the complete pair list
_COMPLETE = {}


def _complete_np(B, n):
    """[source ; target] of the directed complete graph of B molecules of n atoms: target-major, sources ascending."""
    i = np.repeat(np.arange(n, dtype=np.int64), n - 1) if n > 1 else np.empty(0, np.int64)
    j = (np.concatenate([np.delete(np.arange(n, dtype=np.int64), t) for t in range(n)]) if n > 1
         else np.empty(0, np.int64))
    off = np.repeat(np.arange(B, dtype=np.int64) * n, n * (n - 1))
    return np.stack([np.tile(j, B) + off, np.tile(i, B) + off])


def complete_edges(B, n, device="cpu"):
    """The interned complete pair list of B molecules of n atoms on `device` -> (edge_index int64 [2, B n (n - 1)],
    batch vector int64 [B n]): the same two tensor OBJECTS on every call, so a graph keyed by tensor identity replays.
    On the GPU it is built once by ``ops.radius_graph`` at an infinite radius (no geometry enters); n > 33 is refused -
    the radius graph would drop neighbours there."""
    B, n = int(B), int(n)
    if B < 1 or n < 1:
        raise ValueError("complete_edges: at least one molecule of at least one atom")
    if n > COMPLETE_MAX_N:
        raise ValueError("complete_edges: molecules of at most %d atoms (radius_graph keeps 32 neighbours per atom), "
                         "got %d" % (COMPLETE_MAX_N, n))
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (B, n, dev.type, dev.index)
    got = _COMPLETE.get(key)
    if got is None:
        bvec = torch.arange(B, dtype=torch.int64).repeat_interleave(n).to(dev)
        if dev.type == "cuda":
            bvec._geossl_sizes = ([n] * B, bvec._version)   # (host sizes: the layout is built without a read-back)
            ei = ops.radius_graph(torch.zeros(B * n, 3, dtype=torch.float32, device=dev), float("inf"), bvec)
            if ei.size(1) != B * n * (n - 1):
                raise _lib.GeosslHipError("the radius graph at an infinite radius is not the complete pair list")
        else:
            ei = torch.from_numpy(_complete_np(B, n))
        got = _COMPLETE[key] = (ei, bvec)
    return got


def _uniform_size(batch):
    """n when the host knows that every molecule of the batch has n atoms, else None."""
    return bk.size_range(batch)[0] if bk.is_uniform(batch) else None


def complete_applies(batch, model):
    """The complete pair list can stand in for the batch's radius edges: host sizes, all equal, n <= 33, stock PaiNN."""
    from .Geom3D.models.painn import PaiNN
    n = _uniform_size(batch)
    return n is not None and n <= COMPLETE_MAX_N and type(model) is PaiNN


def with_complete_edges(batch, model):
    """`batch` (collated, with host sizes) on the interned complete pair list where the switch and the batch allow it,
    else `batch` itself."""
    if not switches.md17_complete_edges(complete_applies(batch, model)) or not batch.positions.is_cuda:
        return batch
    B, n = len(batch._sizes), _uniform_size(batch)
    ei, bvec = complete_edges(B, n, batch.positions.device)
    out = Batch(batch.x, batch.positions, bvec, None, ei, B, batch._sizes)
    out._complete = True   # (its index tensors are the interned ones: a function of (B, n))
    return out


def _collated(batch):
    """A DeviceLoader handle as its collated batch (gathered on the device, cached on the handle); anything else as is."""
    return batch.materialize() if getattr(batch, "_dataset", None) is not None else batch


# ------------------------------------------------------------------------------------------------- what is served
def loss_kind(criterion):
    """"l1" / "mse" for None (finetune_md17.py:232 builds nn.L1Loss()) or a stock mean nn.L1Loss / nn.MSELoss (not a
    subclass), else None."""
    if criterion is None or (type(criterion) is nn.L1Loss and criterion.reduction == "mean"):
        return "l1"
    if type(criterion) is nn.MSELoss and criterion.reduction == "mean":
        return "mse"
    return None


def head_params(head):
    """The parameters of an energy head geossl_energy_head_fwd serves, in kernel order, or None: Linear(F, 1) / Dense(F,
    1) without an activation, or PaiNN's create_output_layers() at its defaults (Dense(F, F/2, silu), Dense(F/2, 1)),
    with biases and fp32 CUDA parameters at a served width."""
    import torch.nn.functional as F
    from .Geom3D.models.painn import Dense
    plain = lambda m: type(m) is nn.Linear or (type(m) is Dense and type(m.activation) is nn.Identity)
    if plain(head):
        ps, ok, width = (head.weight, head.bias), head.out_features == 1 and head.bias is not None, head.in_features
    elif type(head) is nn.Sequential and len(head) == 2 and all(type(m) is Dense for m in head):
        l0, l1 = head[0], head[1]
        ps = (l0.weight, l0.bias, l1.weight, l1.bias)
        ok = (l0.bias is not None and l1.bias is not None and l0.activation is F.silu
              and type(l1.activation) is nn.Identity and l0.out_features * 2 == l0.in_features
              and l1.in_features == l0.out_features and l1.out_features == 1)
        width = l0.in_features
    else:
        return None
    if not ok or not all(isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float32 for p in ps):
        return None
    return ps if ops.property_width_ok(width) else None


def _check_model_3d(args):
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))


def _x_of(args, batch):
    """The backbone's first argument in :34-39: batch.x as it is (1-D, datasets_MD17.py:61); of an [N, C] x SchNet gets
    the atom-type column (PaiNN slices it itself, painn.py:226-229)."""
    x = batch.x
    return x if args.model_3d == "painn" or x.dim() == 1 else x[:, 0]


def _cuda_batch(batch):
    pos = getattr(batch, "positions", None)
    return (isinstance(pos, torch.Tensor) and pos.is_cuda and pos.dtype == torch.float32
            and isinstance(batch.batch, torch.Tensor) and batch.batch.is_cuda and batch.batch.numel() > 0)


def _targets_ok(batch, pos):
    y, f = getattr(batch, "y", None), getattr(batch, "force", None)
    return (isinstance(y, torch.Tensor) and isinstance(f, torch.Tensor) and y.is_cuda and f.is_cuda
            and y.dtype == torch.float32 and f.dtype == torch.float32 and tuple(f.shape) == tuple(pos.shape))


# ---------------------------------------------------------------------------------------------------------- steps
def md17_energy_force_aten(args, batch_data, model, graph_pred_linear, create_graph=True):
    """:32-46 (and :85-99) as the reference writes them, on our backbone -> (pred_energy, -dE/dpos with its graph)."""
    positions = batch_data.positions
    positions.requires_grad_()
    x = _x_of(args, batch_data)

    if args.model_3d == "schnet":
        molecule_3D_repr = model(x, positions, batch_data.batch)
    elif args.model_3d == "painn":
        molecule_3D_repr = model(x, positions, batch_data.radius_edge_index, batch_data.batch)

    if graph_pred_linear is not None:
        pred_energy = graph_pred_linear(molecule_3D_repr).squeeze(1)
    else:
        pred_energy = molecule_3D_repr.squeeze(1)

    pred_force = -grad(outputs=pred_energy, inputs=positions, grad_outputs=torch.ones_like(pred_energy),
                       create_graph=create_graph, retain_graph=True)[0]
    return pred_energy, pred_force


def do_MD17(args, batch, model, graph_pred_linear, criterion=None):
    """examples/finetune_md17.py:31-51 -> the fp32 loss, whose autograd graph goes through the force (:46
    ``create_graph=True``): ``loss.backward()`` gives the gradients of backbone and head.  Reads args.model_3d,
    args.md17_energy_coeff and args.md17_force_coeff (config.py: 0.05 / 0.95); criterion None is the script's
    nn.L1Loss().  batch: x (1-D atom types, or [N, C]), positions, batch, y [B], force [N, 3] (and radius_edge_index for
    PaiNN) - a collated batch or a DeviceLoader handle of a dataset with ``force``.  For a stock mean L1 / MSE criterion
    on CUDA tensors the loss is ``ops.energy_force_loss`` (the library's kernels; the second-order tape behind it); another
    criterion, ``graph_pred_linear=None`` (``molecule_3D_repr.squeeze(1)``) or CPU tensors run the reference's ATen lines."""
    _check_model_3d(args)
    if getattr(batch, "_dataset", None) is not None:
        batch = _HandleView(batch)
    kind = loss_kind(criterion)
    ce, cf = args.md17_energy_coeff, args.md17_force_coeff
    if kind is None or graph_pred_linear is None or not _cuda_batch(batch) or not _targets_ok(batch, batch.positions):
        if criterion is None:
            criterion = nn.L1Loss()
        pred_energy, pred_force = md17_energy_force_aten(args, batch, model, graph_pred_linear)
        actual_energy = batch.y
        actual_force = batch.force
        loss = ce * criterion(pred_energy, actual_energy) + cf * criterion(pred_force, actual_force)
        return loss
    positions = batch.positions.detach().requires_grad_(True)                                           # :33
    if args.model_3d == "schnet":
        rep = model(_x_of(args, batch), positions, batch.batch)
    else:
        rep = model(_x_of(args, batch), positions, batch.radius_edge_index, batch.batch)
    pred_energy = graph_pred_linear(rep).squeeze(1)
    dE = grad(outputs=pred_energy, inputs=positions, grad_outputs=torch.ones_like(pred_energy), create_graph=True,
              retain_graph=True)[0]                                                                     # :46
    return ops.energy_force_loss(pred_energy, batch.y.reshape(-1), dE, batch.force, ce, cf, kind)       # :48-51


class _HandleView:
    """A DeviceLoader handle as the collated batch the reference's lines read: its gathered tensors with y and force."""

    def __init__(self, handle):
        b = handle.materialize()
        self.x, self.positions, self.batch, self.radius_edge_index = b.x, b.positions, b.batch, b.radius_edge_index
        self._sizes, self.num_graphs = b._sizes, handle.num_graphs
        y = handle.y
        self.y = None if y is None else y.reshape(-1)
        self.force = handle.force


# -------------------------------------------------------------------------------------------------------- predict
def _core_node(h):
    """The fused backbone node behind the latent h (its ctx: what fused_backward reads), or None: the general-width
    path, or a latent something else was applied to."""
    node = h.grad_fn
    return node if node is not None and hasattr(node, "saved") and hasattr(node, "pos") else None


def _energy_and_gradient(model_3d, model, ps, x, positions, bvec, rei):
    """(energy [B], dE/dpos [N, 3]) by launches alone: the backbone's latent, geossl_energy_head_fwd (energies and the
    seed d(sum E)/dh), the backbone's fused first-order backward for the positions only.  None when the backbone did
    not run as its fused node."""
    from .Geom3D.models.painn import _PaiNNCore
    from .Geom3D.models.schnet import _SchNetCore
    pos = positions.detach().requires_grad_(True)
    with torch.enable_grad():
        h = latent(model, model_3d, x, pos, bvec, rei)
    node = _core_node(h)
    if node is None:
        return None
    with torch.no_grad():
        energy, seed = ops.energy_head(h, ps, get_layout(bvec), readout_of(model))
        core = _SchNetCore if model_3d == "schnet" else _PaiNNCore
        dpos, _ = core.fused_backward(node, seed, True, False, False)
    return energy, dpos


def _fused_predict_ok(model, graph_pred_linear, batch):
    ps = head_params(graph_pred_linear)
    if ps is None or readout_of(model) is None or model_width(model) != ps[0].size(1) or not _cuda_batch(batch):
        return None
    sizes = getattr(batch, "_sizes", None)
    if sizes is not None and len(sizes) and max(sizes) > 255:   # (a sparse layout: forces there are out of scope)
        return None
    if sizes is None and get_layout(batch.batch).sparse:
        return None
    return ps


class _Predictor(StructureGraphs):
    """The captured forward-with-forces graphs of (backbone, head), one per batch structure (StructureGraphs' docstring);
    PaiNN only on the interned complete pair list: a frame's own edge list is an input whose length a graph would bind."""

    def __init__(self, model, head, model_3d, max_graphs=16):
        super().__init__(max_graphs)
        self.model, self.head, self.model_3d = model, head, model_3d
        self.bound = parameter_addresses(model, head)

    def unchanged(self):
        return self.bound == parameter_addresses(self.model, self.head)

    def _eager(self, ps, x, pos, bvec, rei):
        x = x if self.model_3d == "painn" or x.dim() == 1 else x[:, 0]
        return _energy_and_gradient(self.model_3d, self.model, ps, x, pos, bvec, rei)

    def run(self, ps, batch, use_graph):
        """-> (energy, dE/dpos), or None (not the fused node).  Replayed: the graph's static outputs, valid until the
        next call."""
        rei = getattr(batch, "radius_edge_index", None) if self.model_3d == "painn" else None
        sizes = getattr(batch, "_sizes", None)
        hit = (use_graph and sizes is not None and (self.model_3d != "painn" or getattr(batch, "_complete", False))
               and self.lookup(sizes_key(batch.batch.numel(), sizes) + (tuple(batch.x.shape),),
                               lambda: bk.is_uniform(batch), lambda: self._capture(ps, batch, rei)))
        if not hit:
            return self._eager(ps, batch.x, batch.positions, batch.batch, rei)
        g, made = hit
        if not made:   # (a new graph's static inputs are clones of this batch)
            copy_static([(g["x"], batch.x), (g["pos"], batch.positions)])
        g["graph"].replay()
        _lib.poll_status(self.model)
        return g["out"]

    def _capture(self, ps, batch, rei):
        x, pos = batch.x.clone(), batch.positions.detach().clone()   # (PaiNN: the interned vector and edges)
        bvec = batch.batch if self.model_3d == "painn" else owned_batch_vector(batch.batch, batch._sizes)
        if self._eager(ps, x, pos, bvec, rei) is None:
            return None

        def passes():   # (cached layouts, kernel attributes, the loop's block plan)
            self._eager(ps, x, pos, bvec, rei)
            if self.model_3d == "schnet":
                get_layout(bvec).loop_plan()
        warm_up(passes)
        with capture(self, "the MD17 forward with forces", "enabled") as cap:
            graph, out = cap.record(lambda: self._eager(ps, x, pos, bvec, rei))
        if not cap.ok:
            return None
        return dict(graph=graph, x=x, pos=pos, out=out, bvec=bvec, rei=rei, layout=get_layout(bvec))


def _predictor(model, head, model_3d):
    pr = model.__dict__.get("_geossl_md17_predict")
    if pr is None or pr.head is not head or pr.model_3d != model_3d or not pr.unchanged():
        pr = model.__dict__["_geossl_md17_predict"] = _Predictor(model, head, model_3d)
    return pr


def _energy_and_gradient_of(args, batch, model, graph_pred_linear, use_graph):
    """The fused route of one batch -> (energy, dE/dpos, collated batch) or None."""
    b = _collated(batch)
    ps = _fused_predict_ok(model, graph_pred_linear, b)
    if ps is None:
        return None
    if args.model_3d == "painn":
        b = with_complete_edges(b, model)
    out = _predictor(model, graph_pred_linear, args.model_3d).run(ps, b, use_graph)
    return None if out is None else (out[0], out[1], b)


def predict_MD17(args, batch, model, graph_pred_linear, use_graph=True):
    """eval()'s forward of one batch (finetune_md17.py:83-99) -> (pred_energy [B], force [N, 3]), detached.  The fused
    route - a head geossl_energy_head_fwd serves (Linear(F, 1), Dense(F, 1), PaiNN's default output layers at F = 64 /
    128 / 256), an unscaled backbone of that width with a mean / add readout, CUDA tensors, structures of at most 255
    atoms - launches the latent, the energy head with its seed and the backbone's first-order position gradient, without
    the autograd engine; with ``use_graph`` the whole pass is one captured graph per batch structure (host sizes; PaiNN on
    the interned complete pair list, else eagerly on the batch's own edges).  Anything else runs the reference's lines."""
    _check_model_3d(args)
    got = _energy_and_gradient_of(args, batch, model, graph_pred_linear, use_graph)
    if got is not None:
        return got[0].clone(), got[1].neg()
    b = batch if getattr(batch, "_dataset", None) is None else _HandleView(batch)
    pred_energy, pred_force = md17_energy_force_aten(args, b, model, graph_pred_linear)
    return pred_energy.detach(), pred_force.detach_()


def eval_MD17(args, loader, model, graph_pred_linear, use_graph=True):
    """examples/finetune_md17.py eval(), :70-123 -> (energy_mae, force_mae) as Python floats: the mean absolute error
    over all energies and over all force ELEMENTS of the loader.  The reference's NaN rule (:104-107) is kept: elements
    whose PREDICTED force is NaN are dropped on both sides; energies are never dropped.  Known difference: the reference
    reshapes the surviving elements to (-1, 3) and raises when their number is no multiple of 3 - here elements are
    counted, and such a batch is averaged over what survives.  On the fused route (predict_MD17's) every batch adds its
    error sums onto one accumulator on the device (geossl_force_metrics_accumulate: fp32 differences, fp64 sums) and the
    host reads it once behind the loop: no per-batch ``torch.cat``, no sync inside the loop.  Batches are moved to the
    backbone's device."""
    _check_model_3d(args)
    model.eval()
    if graph_pred_linear is not None:
        graph_pred_linear.eval()
    params = list(model.parameters())
    device = params[0].device if params else torch.device("cpu")
    acc = None
    sums = [torch.zeros((), dtype=torch.float64, device=device) for _ in range(2)]
    counts = [0, torch.zeros((), dtype=torch.int64, device=device)]
    for batch_data in loader:
        if hasattr(batch_data, "to"):
            batch_data = batch_data.to(device)
        got = _energy_and_gradient_of(args, batch_data, model, graph_pred_linear, use_graph)
        if got is not None and _targets_ok(batch_data, got[2].positions):
            if acc is None:
                acc = ops.force_metrics_buffer(got[0].device)
            ops.force_metrics_accumulate(got[0], batch_data.y.reshape(-1), got[1], batch_data.force, acc)
            continue
        b = batch_data if getattr(batch_data, "_dataset", None) is None else _HandleView(batch_data)
        if got is not None:
            pred_energy, force = got[0], got[1].neg()
        else:
            pred_energy, force = md17_energy_force_aten(args, b, model, graph_pred_linear)
            pred_energy, force = pred_energy.detach(), force.detach_()
        keep = ~torch.isnan(force)                                                                      # :104-107
        diff_f = torch.where(keep, force - b.force, torch.zeros_like(force)).abs()
        sums[0] += (pred_energy - b.y.reshape(-1).to(pred_energy.dtype)).abs().double().sum()
        sums[1] += diff_f.double().sum()
        counts[0] += int(pred_energy.numel())
        counts[1] += keep.sum()
    se, sf, ne, nf = float(sums[0]), float(sums[1]), counts[0], int(counts[1])
    if acc is not None:
        a = ops.force_metrics_read(acc)
        se, sf, ne, nf = se + a[0], sf + a[1], ne + a[2], nf + a[3]
    nan = float("nan")
    return (se / ne if ne else nan), (sf / nf if nf else nan)


# -------------------------------------------------------------------------------------------------------- trainer
class MD17Trainer(ForceTrainer):
    """The body of ``train()`` (finetune_md17.py:17-67) on ``graphed.ForceTrainer`` - the second-order tape, the whole step
    one captured HIP graph per batch structure, backbone and head in one flat buffer under one fused Adam launch - taking
    the batch as the reference's loop does: ``step(batch) -> loss`` reads ``batch.y`` and ``batch.force``.  A batch is a
    collated batch with host sizes or a ``DeviceLoader`` handle of a ``DeviceDataset(..., y=, force=)`` (gathered on the
    device: no host collation in the loop; once its structure has a graph, straight into the graph's static inputs).
    PaiNN batches whose molecules all have one size n <= 33 run on the interned
    complete pair list (module docstring; ``GEOSSL_MD17_COMPLETE_EDGES``), so one graph replays for a whole shuffled
    trajectory; any other batch is handed to ``ForceTrainer.step`` unchanged.  ``predict(batch)``, ``evaluate(loader)``:
    ``predict_MD17`` / ``eval_MD17`` with the trainer's modules; ``set_lr(lr)`` between epochs applies a schedule."""

    def __init__(self, model, head, model_3d="schnet", lr=5e-4, weight_decay=0.0, energy_coeff=0.05, force_coeff=0.95,
                 loss="l1", use_graph=True):
        if model_3d not in ("schnet", "painn"):
            raise Exception("3D model {} not included.".format(model_3d))
        super().__init__(model, head, model_3d=model_3d, lr=lr, weight_decay=weight_decay, energy_coeff=energy_coeff,
                         force_coeff=force_coeff, loss=loss, use_graph=use_graph)
        self.args = types.SimpleNamespace(model_3d=model_3d, md17_energy_coeff=float(energy_coeff),
                                          md17_force_coeff=float(force_coeff))
        self._predict_graphs = use_graph

    @property
    def lr(self):
        return self.opt.lr

    def set_lr(self, lr):
        """The learning rate of the following steps (an epoch-level scheduler: optim.cosine_annealing_lr)."""
        self.opt.lr = float(lr)

    def _replay_from_handle(self, handle):
        """A DeviceLoader handle whose structure already has a graph: its atoms, energies and forces are gathered from
        the dataset straight into the graph's static inputs - one pinned upload of the molecules' offsets and three
        launches, nothing collated - then the replay and Adam, as ForceTrainer.step ends.  -> the loss, or None (no
        graph yet, a masked handle, several targets per molecule: the collated route)."""
        ds = handle._dataset
        if (not self.use_graph or handle._mask is not None or ds.y is None or ds.y.size(1) != 1
                or getattr(ds, "force", None) is None or torch.cuda.is_current_stream_capturing()):
            return None
        B, N = handle.num_graphs, handle.n_atoms
        ei = bvec = None
        if self.model_3d == "painn":   # (the interned tensors the collated route would put into its batch)
            if not switches.md17_complete_edges(complete_applies(handle, self.model)):
                return None
            ei, bvec = complete_edges(B, _uniform_size(handle), ds.device)
        g = self.get(self._key(bvec, ei, handle._sizes, N))
        if g is None or tuple(g["x"].shape) != (N, ds.x_cols):   # (another x: the collated route uses this key next)
            return None
        mol_ptr = get_layout(g["bvec"]).mol_ptr
        ds.gather_into(handle, g["x"], g["pos"], mol_ptr)
        src_off = ds.__dict__["_src_off_dev"]   # (the offsets gather_into uploaded: stream order keeps them for these two)
        ops.property_targets(ds.y, 0, ds.mol_off(), src_off.data_ptr(), B, g["y_e"])
        ops.gather_atom_rows(ds.force, src_off, mol_ptr, B, N, out=g["y_f"])
        g["graph"].replay()
        loss = g["loss"].clone()
        self.opt.step()
        return loss

    def step(self, batch):
        """One training step on batch.y / batch.force -> the loss on the device."""
        if getattr(batch, "_dataset", None) is not None:
            loss = self._replay_from_handle(batch)
            if loss is not None:
                return loss
        y, force = batch.y, batch.force
        if y is None or force is None:
            raise ValueError("MD17Trainer.step reads batch.y (one energy per molecule) and batch.force (a row per atom)")
        b = _collated(batch)
        if self.model_3d == "painn" and getattr(b, "_sizes", None) is not None:
            b = with_complete_edges(b, self.model)
        return super().step(b, y.reshape(-1), force)

    def predict(self, batch):
        """eval()'s (energies, forces) of one batch with the trainer's parameters."""
        return predict_MD17(self.args, batch, self.model, self.head, use_graph=self._predict_graphs)

    def evaluate(self, loader):
        """eval() over a loader -> (energy_mae, force_mae)."""
        return eval_MD17(self.args, loader, self.model, self.head, use_graph=self._predict_graphs)
