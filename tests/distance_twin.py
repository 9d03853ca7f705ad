"""float64 torch twin of the Distance Prediction objective (examples/pretrain_DistancePrediction.py:15-25,71-77), written
from its definition, for the distance tests: differentiable, so torch autograd gives the twin's d node_repr / dW / db."""
import torch


def distance_loss(node_repr, W, b, positions, super_edge_index):
    """mean_e |W . cat(h_u, h_v) + b - |pos_u - pos_v|| in float64 -> (loss, pred [S], target [S]).  S = 0: NaN (the
    mean of an empty tensor)."""
    h = node_repr.double()
    W, b = W.double().reshape(-1), b.double().reshape(-1)
    u, v = super_edge_index[0].long(), super_edge_index[1].long()
    F = h.size(1)
    pred = h[u] @ W[:F] + h[v] @ W[F:] + b[0]
    pos = positions.double()
    target = (pos[u] - pos[v]).pow(2).sum(1).sqrt()
    return (pred - target).abs().mean(), pred, target
