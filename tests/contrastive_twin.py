"""float64 torch twins of the two contrastive losses (examples/pretrain_GeoSSL.py:103-176), written from their
definitions, for the contrastive tests: differentiable, so torch autograd gives the twin's dX / dY."""
import torch


def infonce(X, Y, T):
    """(CE(X Y^T / T, arange) + CE(Y X^T / T, arange)) / 2 -> (loss, row hits, column hits): a hit is a row (column)
    whose FIRST maximum is its diagonal entry."""
    X, Y = X.double(), Y.double()
    S = X @ Y.t() / T
    d = torch.diagonal(S)
    loss = ((torch.logsumexp(S, 1) - d).mean() + (torch.logsumexp(S, 0) - d).mean()) / 2
    idx = torch.arange(S.size(0))
    return loss, int((first_argmax(S, 1) == idx).sum()), int((first_argmax(S, 0) == idx).sum())


def first_argmax(S, dim):
    """Index of the first maximum along `dim` (torch's rule, stated without relying on it)."""
    m = S.max(dim=dim, keepdim=True).values
    n = S.size(dim)
    pos = torch.arange(n).view((-1, 1) if dim == 0 else (1, -1)).expand_as(S)
    return torch.where(S == m, pos, torch.full_like(pos, n)).min(dim=dim).values


def ebm_nce(X, Y, num_neg):
    """(mean softplus(-<x_i, y_i>) + num_neg mean softplus(<x_i, y_{(i+k) mod B}>)) / (1 + num_neg), k = 1..num_neg
    -> (loss, #pos > 0, #neg < 0)."""
    X, Y = X.double(), Y.double()
    B = X.size(0)
    pos = (X * Y).sum(1)
    neg = torch.cat([(X * Y[(torch.arange(B) + k) % B]).sum(1) for k in range(1, num_neg + 1)])
    sp = torch.nn.functional.softplus
    loss = (sp(-pos).mean() + num_neg * sp(neg).mean()) / (1 + num_neg)
    return loss, int((pos > 0).sum()), int((neg < 0).sum())


def infonce_acc(hr, hc, B):
    return (hr * 1. / B + hc * 1. / B) / 2


def ebm_acc(hp, hn, B, num_neg):
    return float((torch.tensor(float(hp + hn), dtype=torch.float32) / (B * (1 + num_neg))).item())
