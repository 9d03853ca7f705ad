"""float64 torch twin of the 3D InfoGraph objective (examples/pretrain_3DInfoGraph.py:19-31,56-76), written from its
definition, for the InfoGraph tests: differentiable, so torch autograd gives the twin's d node_repr / d molecule_repr /
dW."""
import torch


def cycle_index(B):
    """cycle_index(B, 1) of examples/util.py:19-22: (b + 1) mod B."""
    return (torch.arange(B) + 1) % B


def readout(x, batch, B, kind):
    """torch_scatter's sum / mean (sum / max(count, 1)) over the molecules, in float64."""
    x = x.double()
    out = torch.zeros(B, x.size(1), dtype=torch.float64).index_add_(0, batch, x)
    if kind == "mean":
        cnt = torch.bincount(batch, minlength=B).clamp(min=1).to(torch.float64)
        out = out / cnt[:, None]
    return out


def infograph_loss(node_repr, molecule_repr, W, batch):
    """softplus(-pos).mean() + softplus(neg).mean() in float64 -> (loss, pos [N], neg [N])."""
    x = node_repr.double()
    B = molecule_repr.size(0)
    h = torch.sigmoid(molecule_repr.double()) @ W.double()
    batch = torch.as_tensor(batch, dtype=torch.long)
    pos = (x * h[batch]).sum(1)
    neg = (x * h[cycle_index(B)][batch]).sum(1)
    loss = torch.nn.functional.softplus(-pos).mean() + torch.nn.functional.softplus(neg).mean()
    return loss, pos, neg


def counts(pos, neg):
    return int((pos > 0).sum()), int((neg < 0).sum())
