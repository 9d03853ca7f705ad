"""float64 torch twin of the Charge Prediction objective (examples/pretrain_ChargePrediction.py:15-25,62-81), written
from its definition, for the charge tests: differentiable, so torch autograd gives the twin's d node_repr / dW / db."""
import torch


def mask_count(M, ratio):
    """sampled_M of :64."""
    return int(M * ratio)


def charge_loss(node_repr, W, b, masked_index, labels):
    """mean_j (logsumexp(z_j) - z_j[y_j]), z_j = W h[idx_j] + b, in float64 -> (loss, logits [k, C]).  k = 0: NaN (the
    mean over no rows)."""
    h = node_repr.double()
    idx = torch.as_tensor(masked_index, dtype=torch.long)
    z = h[idx] @ W.double().t() + b.double()
    y = torch.as_tensor(labels, dtype=torch.long)
    terms = torch.logsumexp(z, dim=1) - z.gather(1, y.view(-1, 1)).view(-1)
    return terms.sum() / idx.numel(), z
