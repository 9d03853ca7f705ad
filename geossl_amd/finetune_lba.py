"""Step API of ``examples/finetune_lba.py`` (ligand binding affinity on protein pockets of up to 500 atoms) on the HIP
path.

``do_LBA(args, batch, model, graph_pred_linear, criterion)`` is the body of ``train()``, :34-47, as one call -> the fp32
loss: the backbone's latent (SchNet on the sparse pair list for structures above 255 atoms, geossl_amd/layout.py; PaiNN
on its per-atom kernels), then the fused head of csrc/property_head.hip with the readout inside it.  The loss supports
the reference's own ``optimizer.zero_grad(); loss.backward(); optimizer.step()`` with a stock ``torch.optim.Adam``.
Unlike ``do_Supervised`` there is no target normalisation, no task column (``batch.y`` holds one value per structure)
and no failure at B = 1: ``train()`` has no ``pred.size()[0]`` line.  ``eval_LBA`` mirrors ``eval()``, :68-101.

The trainer of this script is ``SupervisedTrainer(model, graph_pred_linear, 0.0, 1.0, task_id=0, loss="mse")``
(geossl_amd/pretrain_Supervised.py): with mean 0, std 1 and one target column its step is this one.  Anything the
kernels do not serve runs the reference's own ATen lines on our backbone - the fallback rules of ``do_Supervised``.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .pretrain_Supervised import _stats_tensor, fused_ok, head_params, loss_kind, model_width, readout_of
from .step import backbone_latent


def _forward_aten(args, batch, model, graph_pred_linear):
    """:36-44 as the reference writes them, on our backbone."""
    if args.model_3d == "schnet":
        molecule_3D_repr = model(batch.x, batch.positions, batch.batch)
    elif args.model_3d == "painn":
        molecule_3D_repr = model(batch.x, batch.positions, batch.radius_edge_index, batch.batch)
    else:
        raise Exception("3D model {} not included.".format(args.model_3d))

    if graph_pred_linear is not None:
        pred = graph_pred_linear(molecule_3D_repr).squeeze()
    else:
        pred = molecule_3D_repr.squeeze()
    return pred


def _fused_batch_ok(batch):
    pos, b, y, x = (getattr(batch, k, None) for k in ("positions", "batch", "y", "x"))
    if not (isinstance(pos, torch.Tensor) and isinstance(b, torch.Tensor) and isinstance(y, torch.Tensor)
            and isinstance(x, torch.Tensor)):
        return False
    if not (pos.is_cuda and pos.dtype == torch.float32 and not pos.requires_grad and b.is_cuda and b.dtype == torch.long
            and b.numel() > 0 and y.is_cuda and y.dtype == torch.float32 and not y.requires_grad):
        return False
    return y.dim() == 1 and y.numel() == int(batch.num_graphs)


def _latent(args, batch, model):
    # (the reference hands batch.x itself to either backbone, :37,39: DatasetLBA's x is the 1-D atomic number)
    return backbone_latent(args.model_3d, batch, model, x=batch.x, what="LBA", layout=True)


def do_LBA(args, batch, model, graph_pred_linear, criterion=None):
    """examples/finetune_lba.py:34-47 -> the fp32 loss.  args.model_3d picks the backbone call ("schnet" / "painn");
    criterion None means the script's nn.MSELoss().  The fused step runs for a stock mean MSE / L1 criterion,
    graph_pred_linear = Linear(F, 1) or PaiNN's default create_output_layers(), an unscaled backbone with a mean / add
    readout at a served width, and CUDA batches with one float32 target per structure; anything else runs the
    reference's ATen lines.  SchNet takes structures of up to 1024 atoms, B = 1 included."""
    if criterion is None:
        criterion = nn.MSELoss()
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    if not (fused_ok(model, graph_pred_linear, criterion) and _fused_batch_ok(batch)):
        pred = _forward_aten(args, batch, model, graph_pred_linear)
        actual = batch.y
        return criterion(pred, actual)
    h, lay, dyn = _latent(args, batch, model)
    loss, _ = ops.property_head(h, head_params(graph_pred_linear), lay, readout_of(model), batch.y,
                                _stats_tensor(h.device, 0.0, 1.0), loss_kind(criterion), dyn=dyn)
    return loss


def average_ranks(a):
    """Ranks 1 .. n of a 1-D array, ties given the average of the ranks they span (scipy.stats.rankdata's default)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    order = np.argsort(a, kind="mergesort")
    s = a[order]
    group = np.cumsum(np.concatenate([[True], s[1:] != s[:-1]])) - 1 if a.size else np.zeros(0, dtype=np.int64)
    counts = np.bincount(group) if a.size else np.zeros(0, dtype=np.int64)
    ends = np.cumsum(counts)
    avg = (2 * ends - counts + 1) / 2.0     # mean of the ranks ends - counts + 1 .. ends
    ranks = np.empty(a.size, dtype=np.float64)
    ranks[order] = avg[group]
    return ranks


def spearman(a, b):
    """scipy.stats.spearmanr(a, b)[0]: the Pearson correlation of the average ranks."""
    return np.corrcoef(average_ranks(a), average_ranks(b))[0, 1]


@torch.no_grad()
def predict_LBA(args, batch, model, graph_pred_linear):
    """eval()'s forward for one batch, :79-87 -> the predictions [B] (a 0-d tensor at B = 1 on the ATen lines)."""
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    ps = head_params(graph_pred_linear)
    if (ps is None or readout_of(model) is None or model_width(model) != ps[0].size(1) or not _fused_batch_ok(batch)):
        return _forward_aten(args, batch, model, graph_pred_linear)
    h, lay, dyn = _latent(args, batch, model)
    return ops.property_predict(h, ps, lay, readout_of(model), _stats_tensor(h.device, 0.0, 1.0), dyn=dyn)


@torch.no_grad()
def eval_LBA(args, loader, model, graph_pred_linear, use_graph=False):
    """examples/finetune_lba.py eval(), :68-101 -> (rmse, pearson, spearman, y_true, y_pred).  Batches are moved to the
    backbone's device; Pearson is np.corrcoef, Spearman the Pearson correlation of average ranks.  ``use_graph=True`` (GPU
    modules; CPU modules take the loop below whole): the loop is ``evaluate.Evaluator.run`` - forward-only graphs on the
    training step's routing, no read inside the loop - and y_true / y_pred are float32 numpy arrays read once.  The one
    known difference: the RMSE is sqrt(sum of the fp32 squared errors in fp64 over all rows / rows) instead of the sum of
    per-batch fp32 means times B."""
    model.eval()
    if graph_pred_linear is not None:
        graph_pred_linear.eval()
    device = next(model.parameters()).device
    if use_graph and device.type == "cuda":
        if args.model_3d not in ("schnet", "painn"):
            raise Exception("3D model {} not included.".format(args.model_3d))
        from .evaluate import evaluator_for
        ev = evaluator_for(model, graph_pred_linear, args.model_3d, "property", 0)
        ev.stats.set(0.0, 1.0)
        _, sum_s, rows, y_true, y_pred = ev.run(loader, eager=lambda b: predict_LBA(args, b, model, graph_pred_linear))
        return (np.sqrt(sum_s / rows), np.corrcoef(y_true, y_pred)[0, 1], spearman(y_true, y_pred), y_true, y_pred)

    loss_all, total = 0, 0
    y_true, y_pred = [], []

    for batch in loader:
        batch = batch.to(device)
        output = predict_LBA(args, batch, model, graph_pred_linear)
        y = batch.y

        B = y.size()[0]

        loss = F.mse_loss(output.reshape(y.shape), y)
        loss_all += loss.item() * B
        total += B
        y_true.extend(y.tolist())
        y_pred.extend(output.reshape(-1).tolist())

    pearson_corr = np.corrcoef(y_true, y_pred)[0, 1]
    spearman_corr = spearman(y_true, y_pred)

    return np.sqrt(loss_all / total), pearson_corr, spearman_corr, y_true, y_pred
