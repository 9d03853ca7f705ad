"""``AutoEncoder``: the head of GeoSSL-RR (``do_RR``, examples/pretrain_GeoSSL.py:77-100, constructed at :320-321).

**This class is this project's own definition.**  The reference script imports ``AutoEncoder`` from ``Geom3D.models``,
but the reference tree does not contain it, so nothing here is pinned to reference code: only the constructor call
``AutoEncoder(emb_dim=, loss=, detach_target=, beta=)`` and the call ``AE_model(x, y) -> loss`` are the reference's.  It
is the plain (non-variational) representation-reconstruction head: a two-layer MLP with batch normalisation predicts the
other view's representation, and ``loss`` compares the prediction with it.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

AE_LOSSES = ("l1", "l2", "cosine")


def ae_loss(p, y, kind):
    """The loss over all B * F elements: l1 mean |p - y|, l2 mean (p - y)^2, cosine - mean over the rows of
    cosine_similarity(p, y, dim=-1) (torch's eps)."""
    if kind == "l1":
        return F.l1_loss(p, y)
    if kind == "l2":
        return F.mse_loss(p, y)
    return -F.cosine_similarity(p, y, dim=-1).mean()


class AutoEncoder(nn.Module):
    """``AutoEncoder(emb_dim, loss, detach_target, beta=1)``; ``forward(x, y)`` -> a 0-dim fp32 loss of
    ``fc_layers(x)`` against ``y`` (``y.detach()`` with ``detach_target``).  ``beta`` is accepted and unused: it belongs
    to a variational variant that pretrain_GeoSSL.py never constructs.  state_dict: ``fc_layers.{0,1,3}.*``, torch's
    default initialisation.

    ``forward`` is ATen code.  The fused HIP kernels (csrc/rr_head.hip) run both heads of a step together and are reached
    through ``geossl_amd.pretrain_GeoSSL.do_RR`` / ``rr_heads_loss``; they serve two distinct AutoEncoders of width 128
    in training mode (``pretrain_GeoSSL.fused_head_ok``)."""

    def __init__(self, emb_dim, loss, detach_target, beta=1):
        super(AutoEncoder, self).__init__()
        if loss not in AE_LOSSES:
            raise ValueError("AutoEncoder: loss is one of %s, got %r" % (AE_LOSSES, loss))
        self.emb_dim = emb_dim
        self.loss = loss
        self.detach_target = detach_target
        self.beta = beta
        self.fc_layers = nn.Sequential(
            nn.Linear(self.emb_dim, self.emb_dim),
            nn.BatchNorm1d(self.emb_dim),
            nn.ReLU(),
            nn.Linear(self.emb_dim, self.emb_dim),
        )

    def forward(self, x, y):
        if self.detach_target:
            y = y.detach()
        return ae_loss(self.fc_layers(x), y, self.loss)
