"""float64 torch twin of the Supervised step after the backbone (examples/pretrain_Supervised.py:92-101), written from its
definition, for the Supervised tests: differentiable, so torch autograd gives the twin's d molecule_repr and head
gradients."""
import torch


def readout(x, batch, B, kind):
    """torch_scatter's sum / mean (sum / max(count, 1)) over the molecules, in float64."""
    x = x.double()
    out = torch.zeros(B, x.size(1), dtype=torch.float64).index_add_(0, batch, x)
    if kind == "mean":
        cnt = torch.bincount(batch, minlength=B).clamp(min=1).to(torch.float64)
        out = out / cnt[:, None]
    return out


def head(m, params):
    """Linear(F, 1) for (w, b); Dense(F, F/2, silu) then Dense(F/2, 1) for (W1, b1, w2, b2) -> [B]."""
    m = m.double()
    if len(params) == 2:
        w, b = (p.double() for p in params)
        return (m @ w.t() + b).reshape(-1)
    W1, b1, w2, b2 = (p.double() for p in params)
    a = torch.nn.functional.silu(m @ W1.t() + b1)
    return (a @ w2.t() + b2).reshape(-1)


def target(y, B, task_id, mean, std):
    return (torch.as_tensor(y).double().view(B, -1)[:, task_id] - mean) / std


def loss(pred, t, kind):
    d = pred - t
    return d.abs().mean() if kind == "mae" else (d * d).mean()
