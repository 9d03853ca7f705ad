"""float64 torch twin of the LEP step after the backbone (examples/finetune_lep.py:40-45), written from its definition,
for the LEP tests: differentiable, so torch autograd gives the twin's d latent and head gradients.  Also the reader of
fixture G25's uncollated items."""
import numpy as np
import torch


def readout(h, batch, S, kind):
    """torch_scatter's sum / mean (sum / max(count, 1)) over the S structures, in float64."""
    h = h.double()
    out = torch.zeros(S, h.size(1), dtype=torch.float64).index_add(0, batch, h)
    if kind == "mean":
        cnt = torch.bincount(batch, minlength=S).clamp(min=1).to(torch.float64)
        out = out / cnt[:, None]
    return out


def logits(m_active, m_inactive, w, b):
    """graph_pred_linear(cat((active, inactive), dim=1)).squeeze() for Linear(2F, 1) -> [B]."""
    m = torch.cat((m_active.double(), m_inactive.double()), dim=1)
    return (m @ w.double().t() + b.double()).reshape(-1)


def bce(z, y):
    """Mean BCE-with-logits from its definition: -[y log sigmoid(z) + (1 - y) log(1 - sigmoid(z))], written with
    softplus so that it stays finite for any z."""
    y = torch.as_tensor(y).double()
    sp = torch.nn.functional.softplus
    return (y * sp(-z) + (1.0 - y) * sp(z)).mean()


def head_on_fused(h, batch, B, kind, w, b, y):
    """The head on the latent of the 2B-structure batch [active 0 .. B-1 | inactive 0 .. B-1] -> (loss, z)."""
    m = readout(h, batch, 2 * B, kind)
    z = logits(m[:B], m[B:], w, b)
    return bce(z, y), z


def fixture_items(g):
    """The uncollated items of a G25 file as our loader's ``Data`` objects (edge lists back to int64)."""
    from geossl_amd.Geom3D.dataloaders import Data
    sa, si = g["sizes_active"], g["sizes_inactive"]
    split = {"active": np.concatenate([[0], np.cumsum(sa)]), "inactive": np.concatenate([[0], np.cumsum(si)])}
    items = []
    for b in range(len(sa)):
        d = {}
        for k in g:
            if not k.startswith("items/"):
                continue
            name = k[len("items/"):]
            if name == "y":
                d[name] = torch.from_numpy(g[k][b:b + 1].copy())
            elif "edge_index" in name:
                off = np.concatenate([[0], np.cumsum(g["items_edges/" + name])])
                d[name] = torch.from_numpy(g[k][:, off[b]:off[b + 1]].astype(np.int64))
            else:
                off = split[name.rsplit("_", 1)[1]]
                d[name] = torch.from_numpy(g[k][off[b]:off[b + 1]].copy())
        items.append(Data(**d))
    return items
