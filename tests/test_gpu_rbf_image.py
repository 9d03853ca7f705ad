"""The per-step image of the filter backward's Gaussian fragments (csrc/rbf_frag.h, k_rbf_fragments) and the launches that
copy it instead of building the fragments for every layer (geossl_cfconv_filter_bwd_frag / _frag_dyn).

The fragments are THE SAME WORDS wherever they are built, so every comparison between the two routes is `torch.equal`:
(a) the image against the items of the shared device function in plain order, put where the layout says by a host
    restatement of the layout - and, so that the shared function itself is looked at, decoded on the host against the
    Gaussians in fp64 with the row order (`kperm`), the padded Gaussians and the column of ones restated here;
(b) the four weight gradients of the `_frag` launch against those of the launch that builds its own fragments;
(c) the `_dyn` forms at a capacity above the real row count, the image pre-filled with NaN: every word written and
    finite, the gradients those of (b);
(d) one eager SchNet forward + backward with GEOSSL_RBF_IMAGE = 0, unset and 1, whichever form the pair graph has;
(e) the captured DDM step, where the image is the default, against GEOSSL_RBF_IMAGE = 0.

Shapes: molecules of 5, 18 and 33 atoms in two views - P = 1382 pair slots = 43 tiles of 32 rows and a tail of 6, more
than one block per layer, tiles inside one molecule and across two; G = 51 (ones column at 63), 64 (no free column) and
20 (ones column and a whole padded block of Gaussians); F = 128 / 64 / 32 (one, two and four items per role-B lane)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [5, 18, 33, 5, 18, 33]
CUTOFF = 5.0
L = 2
TILE_BYTES = 8192
_CACHE = {}


def _smearing(G):
    offset = torch.linspace(0.0, CUTOFF, G).to(DEV)
    return offset, -0.5 / float(offset[1] - offset[0]) ** 2


def _geometry():
    """Layout and dense pair slots of the two views (made once, never written again)."""
    if "geo" not in _CACHE:
        from geossl_amd import ops
        from geossl_amd.layout import MolLayout
        from geossl_amd.synthetic import make_batch
        b = make_batch(0, seed=17, sizes=list(SIZES))
        sizes = [int(n) for n in b["sizes"]]
        assert sizes == SIZES
        batch = torch.arange(len(sizes), device=DEV).repeat_interleave(torch.tensor(sizes, device=DEV))
        lay = MolLayout(batch, len(sizes), sizes=sizes)
        pos = torch.from_numpy(np.array(b["positions"], dtype=np.float32)).to(DEV)
        d, c, fl = ops.pair_geometry(pos, lay, CUTOFF)
        assert lay.P == 1382 and lay.P % 32 != 0
        _CACHE["geo"] = (lay, d, c, fl)
    return _CACHE["geo"]


def _image(pair_d, P, G, dyn_P=None, prefill=None, plain=False):
    """geossl_rbf_fragments(_dyn) -> uint8 [ntiles * 8 KB]; plain: geossl_rbf_fragment_items (the same bytes per item,
    [tile][item][piece])."""
    from geossl_amd import _lib
    from geossl_amd._lib import call, ptr, stream
    offset, coeff = _smearing(G)
    nbytes = _lib.load().geossl_rbf_fragments_bytes(P)
    assert nbytes == (P + 31) // 32 * TILE_BYTES
    img = torch.zeros(nbytes, dtype=torch.uint8, device=DEV) if prefill is None else \
        torch.full((nbytes,), prefill, dtype=torch.uint8, device=DEV)
    dp = None if dyn_P is None else ptr(dyn_P)
    if plain:
        call("geossl_rbf_fragment_items", ptr(pair_d), P, G, ptr(offset), coeff, ptr(img), dp, stream())
    elif dyn_P is None:
        call("geossl_rbf_fragments", ptr(pair_d), P, G, ptr(offset), coeff, ptr(img), stream())
    else:
        call("geossl_rbf_fragments_dyn", ptr(pair_d), P, G, ptr(offset), coeff, ptr(img), dp, stream())
    torch.cuda.synchronize()
    return img


def _expected_gaussians(pair_d, n, ntiles, G):
    """fp64 [tile][gb][ks][lane][e]: the value behind element e of item (gb, ks, lane) - the layout restated:
    row = 16 ks + (e & 3) + 8 (e >> 2) + 4 (lane >> 5), Gaussian g = 32 gb + (lane & 31); rows at and past n take the
    last real row's distance; g >= G is 0, except g = 63 when G < 64: 1."""
    offset, coeff = _smearing(G)
    d = pair_d.double().cpu().numpy()
    off = offset.double().cpu().numpy()
    tile, gb, ks, lane, e = np.meshgrid(np.arange(ntiles), np.arange(2), np.arange(2), np.arange(64), np.arange(8),
                                        indexing="ij")
    row = 32 * tile + 16 * ks + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
    g = 32 * gb + (lane & 31)
    dv = d[np.minimum(row, n - 1)]
    v = np.exp(coeff * (dv - off[np.minimum(g, G - 1)]) ** 2)
    v = np.where(g < G, v, np.where((g == 63) & (G < 64), 1.0, 0.0))
    return v, g


@pytest.mark.parametrize("G", [51, 64, 20])
def test_image_holds_the_shared_functions_items_where_the_layout_says(G):
    """(a).  Exact part: word (it >> 6) * 128 + piece * 64 + (it & 63) of a tile of the image is piece `piece` of item it
    of the plain list (one device function, two kernels).  Decoded part: (h + l) / 2^14 against the fp64 Gaussian.  The
    bound is reasoned, not measured: two fp16 pieces of v 2^14 <= 2^14 leave 2^-11 of |v 2^14 - h| <= 8, i.e. 2^-22 of
    full scale; the fp32 chain coeff * diff^2 -> * log2(e) -> 2^x is three roundings and a 1-ulp exp2 on an argument
    x, worth (4 * 2^-24) x e^-x <= 2^-23 of full scale; the rounding of d - offset, 2^-24 * max(d, offset), goes
    through the steepest slope of a Gaussian, sqrt(2 |coeff|) e^-1/2.  Padded Gaussians and the ones column are exact."""
    lay, d, _, _ = _geometry()
    P, ntiles = lay.P, (lay.P + 31) // 32
    img = _image(d, P, G, prefill=0xFF)
    plain = _image(d, P, G, plain=True)
    a = img.view(ntiles, 4, 2, 64, 16)                              # [tile][gb, ks][piece][lane][16 bytes]
    b = plain.view(ntiles, 4, 64, 2, 16).permute(0, 1, 3, 2, 4)     # [tile][item >> 6][item & 63][piece] -> the same
    assert torch.equal(a, b.contiguous())
    again = _image(d, P, G, dyn_P=torch.tensor([P], dtype=torch.int32, device=DEV), prefill=0xFF)
    assert torch.equal(img, again)
    halves = img.cpu().numpy().view("<f2").astype(np.float64).reshape(ntiles, 2, 2, 2, 64, 8)
    assert np.isfinite(halves).all()
    got = (halves[:, :, :, 0] + halves[:, :, :, 1]) / 16384.0
    want, g = _expected_gaussians(d, P, ntiles, G)
    _, coeff = _smearing(G)
    tol = 2.0 ** -22 + 2.0 ** -23 + math.sqrt(2 * abs(coeff)) * math.exp(-0.5) * 2.0 ** -24 * max(float(d.max()), CUTOFF)
    err = np.abs(got - want)
    print("G=%d  largest |decoded - fp64| %.3e  bound %.3e" % (G, err.max(), tol))
    assert (got[g >= G] == want[g >= G]).all()
    assert err.max() <= tol


def _problem(F, G):
    """Weights, atom tensors, saved hidden rows and the gradients of the launch that builds its own fragments - (b)'s
    reference, computed once per (F, G) and shared."""
    key = ("problem", F, G)
    if key not in _CACHE:
        from geossl_amd import _lib
        from geossl_amd._lib import call, ptr, stream
        lay, d, c, fl = _geometry()
        gen = torch.Generator().manual_seed(100 * F + G)
        offset, coeff = _smearing(G)
        ws = [[(torch.randn(F, G, generator=gen) / G ** 0.5).to(DEV), (0.3 * torch.randn(F, generator=gen)).to(DEV),
               (torch.randn(F, F, generator=gen) / F ** 0.5).to(DEV), (0.3 * torch.randn(F, generator=gen)).to(DEV)]
              for _ in range(L)]
        fw = _lib.FilterWeights()
        for l, w in enumerate(ws):
            fw.w1[l], fw.b1[l], fw.w2[l], fw.b2[l] = (ptr(x) for x in w)
        xs = [torch.randn(lay.N, F, generator=gen).to(DEV) for _ in range(L)]
        daggs = [torch.randn(lay.N, F, generator=gen).to(DEV) for _ in range(L)]
        T = torch.empty(L, lay.P, F, device=DEV)
        Wf = torch.empty(L, lay.P, F, device=DEV)
        call("geossl_cfconv_filter_fwd", ptr(d), ptr(c), lay.P, C.byref(fw), L, F, G, ptr(offset), coeff, ptr(T), ptr(Wf),
             stream())
        p = dict(F=F, G=G, lay=lay, ws=ws, fw=fw, xs=xs, daggs=daggs, T=T, offset=offset, coeff=coeff)
        p["ref"] = _bwd(p, (d, c, fl, lay.pair_i, lay.pair_j), lay.P, T, image=None)
        assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in p["ref"])
        _CACHE[key] = p
    return _CACHE[key]


def _bwd(p, rows, P, T, image, dyn_P=None, use_dyn=False):
    """One weight-gradient launch -> [dw1, db1, dw2, db2] per layer, flat; outputs and workspace start as NaN."""
    from geossl_amd import _lib
    from geossl_amd._lib import call, ptr, stream
    F, G = p["F"], p["G"]
    gin, gout = _lib.FilterGradIn(), _lib.FilterGradOut()
    nan = float("nan")
    outs = [[torch.full((F, G), nan, device=DEV), torch.full((F,), nan, device=DEV), torch.full((F, F), nan, device=DEV),
             torch.full((F,), nan, device=DEV)] for _ in range(L)]
    for l in range(L):
        gin.x[l], gin.dagg[l] = ptr(p["xs"][l]), ptr(p["daggs"][l])
        gout.dw1[l], gout.db1[l], gout.dw2[l], gout.db2[l] = (ptr(o) for o in outs[l])
    wsp = torch.full((_lib.load().geossl_cfconv_filter_bwd_workspace_floats(P, L, F, G),), nan, device=DEV)
    args = tuple(ptr(a) for a in rows) + (P, p["lay"].N, C.byref(p["fw"]), C.byref(gin), L, F, G, ptr(p["offset"]),
                                         p["coeff"], ptr(T), C.byref(gout), ptr(wsp), 0)
    dyn = (None if dyn_P is None else ptr(dyn_P), None)
    if image is None:
        call(*(("geossl_cfconv_filter_bwd_dyn",) + args + dyn if use_dyn else ("geossl_cfconv_filter_bwd",) + args), stream())
    else:
        call(*(("geossl_cfconv_filter_bwd_frag_dyn",) + args + dyn if use_dyn else ("geossl_cfconv_filter_bwd_frag",) + args),
             ptr(image), stream())
    torch.cuda.synchronize()
    return [t_ for o in outs for t_ in o]


SHAPES = [(128, 51), (128, 64), (128, 20), (64, 51), (32, 20)]


@pytest.mark.parametrize("F, G", SHAPES)
def test_frag_launch_gives_the_gradients_of_the_launch_that_builds_its_own(F, G):
    """(b): dW1, db1, dW2, db2 of both layers, bit for bit."""
    p = _problem(F, G)
    lay, d, c, fl = _geometry()
    img = _image(d, lay.P, G)
    got = _bwd(p, (d, c, fl, lay.pair_i, lay.pair_j), lay.P, p["T"], image=img)
    for k, (g, r) in enumerate(zip(got, p["ref"])):
        assert torch.equal(g, r), (F, G, k)


def _padded(cap):
    """The pair list at a capacity: rows past the real count as the library's lists leave them (flag 0, atoms 0, C = 0,
    d = cutoff)."""
    lay, d, c, fl = _geometry()
    n = cap - lay.P
    z32 = torch.zeros(n, dtype=torch.int32, device=DEV)
    return (torch.cat([d, torch.full((n,), CUTOFF, device=DEV)]), torch.cat([c, torch.zeros(n, device=DEV)]),
            torch.cat([fl, torch.zeros(n, dtype=torch.uint8, device=DEV)]), torch.cat([lay.pair_i, z32]),
            torch.cat([lay.pair_j, z32]))


@pytest.mark.parametrize("F, G", SHAPES)
def test_dyn_forms_at_a_capacity_above_the_row_count(F, G):
    """(c).  Capacity 1408: the tile count of the exact launch (44), 26 unused rows in the tail tile - one block per
    tile and one partial per block as in (b), so the gradients are (b)'s.  Capacity 1509: three whole unused tiles and a
    tail behind them; their blocks add zero partials, which regroups the fixed-order reduction of the partial list
    (four slices of the block count), so the launch that builds its own fragments AT THAT CAPACITY is the reference
    there.  The image starts as NaN bytes at both: every word of the capacity is written and finite."""
    p = _problem(F, G)
    lay = p["lay"]
    dyn_P = torch.tensor([lay.P], dtype=torch.int32, device=DEV)
    for cap in (1408, 1509):
        rows = _padded(cap)
        T = torch.full((L, cap, F), float("nan"), device=DEV)   # (the layer stride of T is the capacity)
        T[:, :lay.P] = p["T"]
        img = _image(rows[0], cap, G, dyn_P=dyn_P, prefill=0xFF)
        assert bool(torch.isfinite(img.view(torch.float16)).all()), cap
        got = _bwd(p, rows, cap, T, image=img, dyn_P=dyn_P, use_dyn=True)
        ref = p["ref"] if cap == 1408 else _bwd(p, rows, cap, T, image=None, dyn_P=dyn_P, use_dyn=True)
        for k, (g, r) in enumerate(zip(got, ref)):
            assert bool(torch.isfinite(g).all()), (cap, k)
            assert torch.equal(g, r), (F, G, cap, k)


MODEL_CFG = dict(hidden_channels=128, num_filters=128, num_interactions=2, num_gaussians=51, cutoff=3.0, node_class=9,
                 readout="add")


@pytest.mark.parametrize("form", ["live list", "every slot", "sparse", "positions + parameters"])
def test_eager_schnet_gradients_do_not_depend_on_the_switch(form, monkeypatch):
    """(d): GEOSSL_RBF_IMAGE = 0, unset and 1 - every parameter gradient bit-identical; = 1 makes the two image launches,
    = 0 and (outside a capture) unset make neither."""
    import geossl_amd.Geom3D.models.schnet as sm
    from geossl_amd import ops
    from geossl_amd.synthetic import make_batch
    from helpers import product_schnet, t, unique_named_grads
    for k in ("GEOSSL_LIVE_PAIRS", "GEOSSL_SPARSE_PAIRS", "GEOSSL_FILTER_BWD_BF16X3", "GEOSSL_ARITH_24BIT",
              "GEOSSL_FILTER_RECOMPUTE_T"):
        monkeypatch.delenv(k, raising=False)
    if form == "every slot":
        monkeypatch.setenv("GEOSSL_LIVE_PAIRS", "0")
    if form == "sparse":
        monkeypatch.setenv("GEOSSL_SPARSE_PAIRS", "1")
    b = make_batch(0, seed=17, sizes=list(SIZES))
    names = []
    real = sm.call
    for mod in (sm, ops):
        monkeypatch.setattr(mod, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    model = product_schnet(MODEL_CFG, DEV)
    w = torch.cos(torch.arange(128, dtype=torch.float32, device=DEV))
    grads = {}
    for mode in ("0", None, "1"):
        if mode is None:
            monkeypatch.delenv("GEOSSL_RBF_IMAGE", raising=False)
        else:
            monkeypatch.setenv("GEOSSL_RBF_IMAGE", mode)
        model.zero_grad()
        del names[:]
        pos = t(b["positions"], DEV).requires_grad_(form == "positions + parameters")
        out, h = model(t(b["x"], DEV)[:, 0], pos, t(b["batch"], DEV), return_latent=True)
        ((h ** 2).sum() + (out * w).sum()).backward()
        torch.cuda.synchronize()
        image = [n for n in names if n in ("geossl_rbf_fragments_dyn", "geossl_cfconv_filter_bwd_frag_dyn")]
        assert image == (["geossl_rbf_fragments_dyn", "geossl_cfconv_filter_bwd_frag_dyn"] if mode == "1" else []), (mode, names)
        assert ("geossl_cfconv_filter_bwd_dyn" in names) == (mode != "1")
        grads[mode] = {k: v.clone() for k, v in unique_named_grads(model).items()}
    assert len(grads["0"]) > 0
    for mode in (None, "1"):
        assert grads[mode].keys() == grads["0"].keys()
        for k, v in grads[mode].items():
            assert bool(torch.isfinite(v).all()) and torch.equal(v, grads["0"][k]), (mode, k)


def test_captured_ddm_step_uses_the_image_by_default_and_keeps_every_bit(monkeypatch):
    """(e): three DDMTrainer steps replayed from a structure graph, GEOSSL_RBF_IMAGE unset (the capture makes the image
    launches) against = 0 (it makes neither): losses and parameters bit-identical."""
    import geossl_amd.Geom3D.models.schnet as sm
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import draw_noise, make_batch
    from helpers import product_ncsn, product_schnet, t
    cfg = dict(MODEL_CFG, cutoff=5.0, readout="mean")
    names = []
    real = sm.call
    for mod in (sm, ops):
        monkeypatch.setattr(mod, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    out = {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("GEOSSL_RBF_IMAGE", raising=False)
        else:
            monkeypatch.setenv("GEOSSL_RBF_IMAGE", mode)
        del names[:]
        tr = pg.DDMTrainer(product_schnet(cfg, DEV), product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9),
                           lr=5e-4, use_graph=True)
        losses = []
        for step in range(3):
            b = make_batch(32, seed=70 + step, mode="A")
            noise = {k: t(v, DEV) for k, v in draw_noise(b, seed=170 + step).items()}
            losses.append(float(tr.step(pg.Batch.from_numpy(b, DEV), noise)))
        assert tr.use_graph, "capture fell back to eager"
        assert ("geossl_cfconv_filter_bwd_frag_dyn" in names) == (mode is None), sorted(set(names))
        assert ("geossl_rbf_fragments_dyn" in names) == (mode is None)
        out[mode] = (losses, tr.flat.flat.detach().clone())
    assert all(math.isfinite(v) for v in out[None][0])
    assert out[None][0] == out["0"][0], (out[None][0], out["0"][0])
    assert torch.equal(out[None][1], out["0"][1])
