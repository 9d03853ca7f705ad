"""The pieces the fused loss heads share (csrc/head_common.h, the readout of csrc/common.h), pinned where a copy could
drift: a head's readout has the bits of the backbone's (ops.segment_reduce), and the one-block loss step is right when
there are more slots than threads."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
# around a wave (63 / 64 / 65) and at the bucket limit (255); eight structures = four pairs for the pair head
SIZES = [1, 2, 5, 18, 63, 64, 65, 255]
READOUTS = {"add": 0, "mean": 1}
_CACHE = {}


def _mol_ptr(sizes):
    sizes = torch.as_tensor(sizes, dtype=torch.long)
    return torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)]).to(torch.int32).to(DEV)


def _backbone_readout(F, readout):
    """(h [N, F] on the device, ops.segment_reduce(h)): seeded normal rows as drawn - a sum of up to 255 of them rounds at
    nearly every step, so another summation order shows in the low bits.  Computed once per (F, readout), never changed."""
    from geossl_amd import ops
    if (F, readout) not in _CACHE:
        g = torch.Generator().manual_seed(4100 + F)
        h = (torch.randn(sum(SIZES), F, generator=g) * 0.37).to(DEV)
        lay = types.SimpleNamespace(mol_ptr=_mol_ptr(SIZES), B=len(SIZES))
        _CACHE[F, readout] = (h, lay, ops.segment_reduce(h, lay, readout))
    return _CACHE[F, readout]


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("readout", ["add", "mean"])
@pytest.mark.parametrize("F", [64, 128, 256])
def test_property_head_readout_has_the_backbone_bits(F, readout):
    from geossl_amd import _lib
    from geossl_amd._lib import ptr, stream
    h, lay, want = _backbone_readout(F, readout)
    B, N = lay.B, h.size(0)
    g = torch.Generator().manual_seed(F)
    w, b = (torch.randn(1, F, generator=g) / F ** 0.5).to(DEV), torch.zeros(1, device=DEV)
    y = torch.randn(B, generator=g).to(DEV)
    stats = torch.tensor([0.3, 1.7], device=DEV)
    f = lambda *shape: torch.full(shape, NAN, device=DEV)
    m, pred, loss = f(B, F), f(B), f()
    ws = f(int(_lib.load().geossl_property_workspace_floats(B)))
    _lib.call("geossl_property_fwd", ptr(h), N, F, ptr(lay.mol_ptr), B, READOUTS[readout], 0, ptr(w), ptr(b), None, None,
              ptr(y), 1, ptr(stats), 0, ptr(m), None, ptr(pred), ptr(ws), ptr(loss), stream())
    torch.cuda.synchronize()
    assert torch.isfinite(m).all()
    assert _same_bits(m, want)


@pytest.mark.parametrize("readout", ["add", "mean"])
@pytest.mark.parametrize("F", [32, 64, 128])
def test_pair_head_readout_has_the_backbone_bits(F, readout):
    from geossl_amd import _lib
    from geossl_amd._lib import ptr, stream
    h, lay, want = _backbone_readout(F, readout)   # structures [active 0..3 | inactive 0..3]
    B, N = lay.B // 2, h.size(0)
    g = torch.Generator().manual_seed(F)
    w, b = (torch.randn(1, 2 * F, generator=g) / F ** 0.5).to(DEV), torch.zeros(1, device=DEV)
    y = torch.tensor([1.0, 0.0, 0.0, 1.0], device=DEV)
    f = lambda *shape: torch.full(shape, NAN, device=DEV)
    m, z, loss = f(2 * B, F), f(B), f()
    ws = f(int(_lib.load().geossl_pair_head_workspace_floats(B)))
    _lib.call("geossl_pair_head_fwd", ptr(h), N, F, ptr(lay.mol_ptr), B, READOUTS[readout], ptr(w), ptr(b), ptr(y),
              ptr(m), ptr(z), ptr(ws), ptr(loss), stream())
    torch.cuda.synchronize()
    assert torch.isfinite(m).all()
    assert _same_bits(m[:B], want[:B]) and _same_bits(m[B:], want[B:])   # the active and the inactive halves


@pytest.mark.parametrize("readout", ["add", "mean"])
@pytest.mark.parametrize("F", [64, 128, 256])
def test_infograph_summary_is_the_sigmoid_of_the_backbone_readout(F, readout):
    """The InfoGraph ABI returns s = sigmoid(readout) only, so its readout is pinned bitwise by code sharing (readout_col)
    and here through s: the fp32 sigmoid 1 / (1 + expf(-m)) of the backbone's m is within 4 ulp of the fp64 sigmoid of
    the same m (expf 1 ulp, scaled by e / (1 + e) < 1; the add and the divide half an ulp each; one more for the
    rounding of the comparison's own fp32 input)."""
    from geossl_amd import _lib
    from geossl_amd._lib import ptr, stream
    h, lay, want = _backbone_readout(F, readout)
    B, N = lay.B, h.size(0)
    g = torch.Generator().manual_seed(F)
    W = ((torch.rand(F, F, generator=g) * 2 - 1) / F ** 0.5).to(DEV)
    f = lambda *shape: torch.full(shape, NAN, device=DEV)
    s, hh, scores, loss = f(B, F), f(B, F), f(2, N), f()
    ws = f(int(_lib.load().geossl_infograph_fwd_workspace_floats(B)))
    counts = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    _lib.call("geossl_infograph_fwd", ptr(h), N, F, ptr(W), ptr(lay.mol_ptr), B, READOUTS[readout], None, ptr(s), ptr(hh),
              ptr(scores), ptr(ws), ptr(loss), ptr(counts), stream())
    torch.cuda.synchronize()
    ref = torch.sigmoid(want.double().cpu())
    err = (s.double().cpu() - ref).abs()
    assert bool((err <= 4 * 2.0 ** -23 * ref).all()), float((err / ref).max())


@pytest.mark.parametrize("loss_kind", ["mae", "mse"])
@pytest.mark.parametrize("B", [1, 257])
def test_loss_step_with_more_slots_than_threads(B, loss_kind):
    """k_head_loss on the property head's per-molecule slots, at one slot and at one slot past the 256-thread stride:
    the loss is the fp64 mean of the returned per-molecule terms rounded to fp32 (1 fp32 ulp for that final rounding),
    and those terms are the ones recomputed on the host from pred and y in fp64."""
    from geossl_amd import _lib
    from geossl_amd._lib import ptr, stream
    F = 64
    g = torch.Generator().manual_seed(900 + B)
    sizes = [(3, 1, 7, 2)[i % 4] for i in range(B)]
    N = sum(sizes)
    h = (torch.randn(N, F, generator=g) * 0.5).to(DEV)
    w, b = (torch.randn(1, F, generator=g) / F ** 0.5).to(DEV), torch.tensor([0.1], device=DEV)
    y = (torch.randn(B, generator=g) * 2.0 + 0.7).to(DEV)
    stats = torch.tensor([0.3, 1.7], device=DEV)
    f = lambda *shape: torch.full(shape, NAN, device=DEV)
    m, pred, loss = f(B, F), f(B), f()
    ws = f(int(_lib.load().geossl_property_workspace_floats(B)))
    _lib.call("geossl_property_fwd", ptr(h), N, F, ptr(_mol_ptr(sizes)), B, 1, 0, ptr(w), ptr(b), None, None, ptr(y), 1,
              ptr(stats), {"mae": 0, "mse": 1}[loss_kind], ptr(m), None, ptr(pred), ptr(ws), ptr(loss), stream())
    torch.cuda.synchronize()
    terms = ws.view(torch.float64)[:B].cpu()                     # the returned per-molecule terms (fp64 slots)
    # ... are the terms of pred and y: in fp64, t = (y - mean) / std, d = pred - t; the kernel forms t with two fp32
    # roundings and d with one (2^-23 (2 |t| + |d|) at most on d), then |d| exactly or d d with one more rounding
    st = stats.double().cpu()
    t64 = (y.double().cpu() - st[0]) / st[1]
    d64 = pred.double().cpu() - t64
    derr = 2.0 ** -23 * (2 * t64.abs() + d64.abs())
    if loss_kind == "mae":
        ref, bound = d64.abs(), derr
    else:
        ref, bound = d64 * d64, 2 * d64.abs() * derr + derr * derr + 2.0 ** -23 * d64 * d64
    assert bool(((terms - ref).abs() <= bound).all())
    want = torch.tensor(terms.sum().item() / B, dtype=torch.float64).float()
    ulp = 2.0 ** -23 * 2.0 ** torch.floor(torch.log2(want.abs().double())).item()
    print("B=%d %s: loss %.9g, fp64 mean of the terms %.9g" % (B, loss_kind, float(loss), float(want)))
    assert abs(float(loss) - float(want)) <= ulp
