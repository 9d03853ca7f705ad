"""float64 torch twin of angle prediction on atom triples (examples/pretrain_TorsionAnglePrediction.py:16-27,73-78) and of
the library's angle definition, written from their definitions, for the torsion tests: differentiable, so torch autograd
gives the twin's d node_repr / dW / db."""
import torch


def torsion_loss(node_repr, W, b, super_edge_index, angle):
    """mean_t (W . cat(h_u, h_v, h_w) + b - angle_t)^2 in float64 -> (loss, pred [T]).  T = 0: NaN (the mean of an empty
    tensor)."""
    h = node_repr.double()
    W, b = W.double().reshape(-1), b.double().reshape(-1)
    u, v, w = super_edge_index[0].long(), super_edge_index[1].long(), super_edge_index[2].long()
    F = h.size(1)
    pred = h[u] @ W[:F] + h[v] @ W[F:2 * F] + h[w] @ W[2 * F:] + b[0]
    return (pred - angle.double().reshape(-1)).pow(2).mean(), pred


def triple_angles(positions, super_edge_index):
    """The angle at the middle atom of every triple in float64: atan2(|a x b|, a . b), a = pos_u - pos_v,
    b = pos_w - pos_v; in [0, pi], 0 when a or b is zero."""
    pos = positions.double()
    u, v, w = super_edge_index[0].long(), super_edge_index[1].long(), super_edge_index[2].long()
    a, b = pos[u] - pos[v], pos[w] - pos[v]
    y = torch.linalg.cross(a, b, dim=1).norm(dim=1)
    x = (a * b).sum(1)
    out = torch.atan2(y, x)
    zero = (a.abs().sum(1) == 0) | (b.abs().sum(1) == 0)
    return torch.where(zero, torch.zeros_like(out), out)
