"""Step API of ``examples/pretrain_3DInfoGraph.py`` (the 3D InfoGraph baseline of GeoSSL) on the HIP path.

``Discriminator`` is the reference module (same state_dict key, shape and init distribution; its ``forward`` is the
reference's ATen code), ``cycle_index`` the one of ``examples/util.py``.  ``do_InfoGraph(node_repr, molecule_repr, batch,
criterion, discriminator)`` has the reference's signature and returns ``(loss, acc)``; it runs the fused loss kernels
(csrc/infograph_head.hip) when it can and the reference's ATen code otherwise.  ``do_3DInfoGraph(args, batch, model,
discriminator)`` is the loop body :92-108 as one call: the backbone's latent, then the fused head with the readout inside
it (sigmoid summary, discriminator scores of every atom against its own and the next molecule, both BCE means and the
accuracy counts), forward + backward replayed from HIP graphs by ``autograd_step._AutogradStep`` when gradients are
wanted.  Its loss supports the reference's own ``optimizer.zero_grad(); loss.backward(); optimizer.step()`` with a stock
``torch.optim.Adam``.  ``InfoGraphTrainer`` is the ``train()`` body with all parameters in one flat buffer (one fused
Adam launch, one all-reduce per step) and no host sync in ``step``.
"""
import math

import torch
import torch.nn as nn

from . import ops
from .step import Args, Objective, StepTrainer, backbone_forward, backbone_latent, run_graphed, with_counts
from .step import stock_bce as criterion_ok  # (a stock mean nn.BCEWithLogitsLoss: what the fused loss computes)


def uniform(size, value):
    """torch_geometric.nn.inits.uniform: U(-1 / sqrt(size), 1 / sqrt(size)) in place (restated: PyG is not needed)."""
    if value is not None:
        bound = 1.0 / math.sqrt(size)
        value.data.uniform_(-bound, bound)


class Discriminator(nn.Module):
    """examples/pretrain_3DInfoGraph.py:19-31."""

    def __init__(self, hidden_dim):
        super(Discriminator, self).__init__()
        self.weight = nn.Parameter(torch.Tensor(hidden_dim, hidden_dim))
        self.reset_parameters()

    def reset_parameters(self):
        size = self.weight.size(0)
        uniform(size, self.weight)

    def forward(self, x, summary):
        h = torch.matmul(summary, self.weight)
        return torch.sum(x * h, dim=1)


def cycle_index(num, shift):
    """examples/util.py:19-22."""
    arr = torch.arange(num) + shift
    arr[-shift:] = torch.arange(shift)
    return arr


def fused_head_ok(discriminator):
    """The reference's Discriminator (not a subclass) with a square fp32 weight on the GPU at a width of the kernels."""
    w = getattr(discriminator, "weight", None)
    return (type(discriminator) is Discriminator and isinstance(w, torch.Tensor) and w.dim() == 2
            and w.size(0) == w.size(1) and w.is_cuda and w.dtype == torch.float32 and ops.infograph_width_ok(w.size(0)))


def readout_of(model):
    """The backbone's readout as the fused head computes it ("mean" / "add" / "sum"), or None (scaled or other)."""
    r = getattr(model, "readout", None)
    if r not in ops.INFOGRAPH_READOUTS or getattr(model, "scale", None) is not None:
        return None
    return r


def infograph_acc(counts, N):
    """The reference's acc (:72-74): the fp32 count tensor divided by float(2 N), as a Python float."""
    c = int(counts[0]) + int(counts[1])
    return (torch.tensor(c).to(torch.float32) / float(2 * N)).item()


def _infograph_aten(node_repr, molecule_repr, batch, criterion, infograph_discriminator_SSL_model):
    """:56-76 as the reference writes it."""
    summary_repr = torch.sigmoid(molecule_repr)
    positive_expanded_summary_repr = summary_repr[batch.batch]
    shifted_summary_repr = summary_repr[cycle_index(len(summary_repr), 1)]
    negative_expanded_summary_repr = shifted_summary_repr[batch.batch]

    positive_score = infograph_discriminator_SSL_model(node_repr, positive_expanded_summary_repr)
    negative_score = infograph_discriminator_SSL_model(node_repr, negative_expanded_summary_repr)
    infograph_loss = criterion(positive_score, torch.ones_like(positive_score)) + \
        criterion(negative_score, torch.zeros_like(negative_score))

    num_sample = float(2 * len(positive_score))
    infograph_acc = (torch.sum(positive_score > 0) +
                     torch.sum(negative_score < 0)).to(torch.float32) / num_sample
    infograph_acc = infograph_acc.detach().cpu().item()

    return infograph_loss, infograph_acc


def _fused_loss_ok(node_repr, molecule_repr, batch, criterion, discriminator):
    b = getattr(batch, "batch", None)
    return (criterion_ok(criterion) and fused_head_ok(discriminator) and isinstance(b, torch.Tensor) and b.is_cuda
            and b.dtype == torch.long and b.dim() == 1 and node_repr.is_cuda and molecule_repr.is_cuda
            and node_repr.dtype == torch.float32 and molecule_repr.dtype == torch.float32 and node_repr.dim() == 2
            and molecule_repr.dim() == 2 and node_repr.size(0) == b.numel() and node_repr.size(0) > 0
            and molecule_repr.size(1) == node_repr.size(1) == discriminator.weight.size(0))


def do_InfoGraph(node_repr, molecule_repr, batch, criterion, infograph_discriminator_SSL_model):
    """examples/pretrain_3DInfoGraph.py:56-76 -> (infograph_loss fp32 scalar, infograph_acc Python float).  The fused
    loss kernels run for a stock BCEWithLogitsLoss, the reference Discriminator at a served width (64, 128, 256) and CUDA
    fp32 inputs with a sorted batch vector; anything else - another criterion, a subclass, CPU tensors - runs the
    reference's ATen code."""
    disc = infograph_discriminator_SSL_model
    if _fused_loss_ok(node_repr, molecule_repr, batch, criterion, disc):
        from .layout import get_layout
        lay = get_layout(batch.batch)
        if lay.B == molecule_repr.size(0):
            loss, counts = ops.infograph_loss(node_repr, molecule_repr, disc.weight, lay)
            return loss, infograph_acc(counts.tolist(), node_repr.size(0))
    return _infograph_aten(node_repr, molecule_repr, batch, criterion, disc)


def infograph_step_fused(args, batch, model, discriminator):
    """The step as eager launches: the backbone's latent, then the fused head with the backbone's readout in it ->
    (loss fp32 scalar, counts int32 [2] on the device).  (A one-view capacity bucket: lay.mol_ptr holds the B real
    offsets of view 0, so the readout and the scores see exact molecules.)"""
    readout = readout_of(model)
    h, lay, dyn = backbone_latent(args.model_3d, batch, model, what="3D InfoGraph", layout=True)
    return ops.infograph_head(h, discriminator.weight, lay, readout, dyn=dyn)


# (no random draws; forward -> (loss, counts): the counts are a static output of the forward graph)
INFOGRAPH = Objective("InfoGraph",
                      lambda owner, args, batch, noise: infograph_step_fused(args, batch, owner.model, owner.n1),
                      result=with_counts)


def infograph_step_aten(args, batch, model, discriminator, criterion):
    """:92-108 on our backbone with the caller's criterion: the backbone's own readout, then do_InfoGraph."""
    molecule_repr, node_repr = backbone_forward(args, batch, model, True)
    return do_InfoGraph(node_repr, molecule_repr, batch, criterion, discriminator)


def _fused_batch_ok(batch):
    if getattr(batch, "_dataset", None) is not None:   # a DeviceLoader handle: float32 / int64 tensors on its device
        return batch.device.type == "cuda"
    pos, b = getattr(batch, "positions", None), getattr(batch, "batch", None)
    return (pos is not None and b is not None and pos.is_cuda and not pos.requires_grad
            and pos.dtype == torch.float32 and b.is_cuda and b.dtype == torch.long and b.numel() > 0)


def _n_atoms(batch):
    return batch.n_atoms if getattr(batch, "_dataset", None) is not None else int(batch.batch.numel())


def do_3DInfoGraph(args, batch, model, discriminator, criterion=None, graph=None):
    """examples/pretrain_3DInfoGraph.py:92-108 -> (CL_loss fp32 scalar tensor, CL_acc Python float).  args.model_3d
    picks the backbone call ("schnet" / "painn"); criterion None is the reference's nn.BCEWithLogitsLoss().  The fused
    step runs whenever the criterion, the discriminator, the backbone's readout and the batch allow it; anything else
    runs the backbone's own readout and do_InfoGraph.  graph: replay HIP graphs of forward + backward (default:
    ``args.step_graph`` if present, else on unless GEOSSL_NO_STEP_GRAPH is set)."""
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    if criterion is None:
        criterion = nn.BCEWithLogitsLoss()
    if not (criterion_ok(criterion) and fused_head_ok(discriminator) and readout_of(model) is not None
            and _fused_batch_ok(batch)):
        return infograph_step_aten(args, batch, model, discriminator, criterion)
    N = _n_atoms(batch)
    got = run_graphed(args, graph, model, "_geossl_infograph_step", INFOGRAPH, Args(args.model_3d), batch, n1=discriminator)
    if got is not None:
        loss, counts = got
        return loss, infograph_acc(counts, N)
    loss, counts = infograph_step_fused(args, batch, model, discriminator)
    return loss, infograph_acc(counts.tolist(), N)


class InfoGraphTrainer(StepTrainer):
    """The body of ``train()`` (examples/pretrain_3DInfoGraph.py:79-125): backbone latent, fused InfoGraph head with the
    readout in it, backward, gradient all-reduce, Adam - backbone and discriminator in one flat buffer (one fused Adam
    launch at one learning rate: both of the reference's groups run at lr * gnn_3d_lr_scale), no host sync inside
    ``step``.  ``step(batch) -> (loss, counts)``: both on the device (infograph_acc turns the counts into the reference's
    acc).  ``use_graph=True``: forward + backward are captured into HIP graphs and replayed (StepGraphs: ragged SchNet /
    PaiNN batches and DeviceLoader handles share one ONE-view capacity-bucket graph per batch size, for a discriminator
    of width 128; anything else one graph per structure).  There are no random draws in this step."""

    def __init__(self, model, discriminator, lr=5e-4, weight_decay=0.0, model_3d="schnet", use_graph=False,
                 max_graphs=256, graph_mode="auto"):
        if not fused_head_ok(discriminator) or readout_of(model) is None:
            raise ValueError("InfoGraphTrainer needs the reference Discriminator at a width of the fused head (64, 128 or "
                             "256) on the GPU and a backbone with an unscaled mean / add readout; use do_3DInfoGraph for "
                             "anything else")
        self.discriminator = discriminator
        super().__init__([model, discriminator], INFOGRAPH, Args(model_3d), lr, weight_decay, use_graph, max_graphs,
                         graph_mode)

    with_extra = True   # step(batch) -> (loss, counts)
