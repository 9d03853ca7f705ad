"""The two tile heights of the filter backward (filter_bwd.hip, k_filter_bwd_h): 64 pair rows per tile - two 32-row M
blocks behind one build phase, one barrier pair and one atom window - and the 32-row form GEOSSL_FILTER_BWD_TILE32 selects.

Every case launches geossl_cfconv_filter_bwd (and _frag / the _dyn forms where it says so) through the raw C ABI at BOTH
heights and holds all four weight gradients of every layer to the fp64 twin, per element:
|got - ref| <= 8 u S with ref and S from tests/filter_twin.py::_filter_ref_and_bound and u = 2^-22, the bound of
tests/test_gpu_filter_classes.py for the two-piece form - no new tolerance.  Outputs and workspace start as NaN.

Shapes are the smallest at which the tile logic can go wrong: row counts around the edges of a 32- and a 64-row tile,
and batches built for the atom-window decisions.  A block keeps its window only across the tiles of its own range, and
the launcher starts 256 / L blocks per layer, so the window cases run L = 12 layers (21 blocks per layer) on enough
molecules for ranges of several tiles; `window_kinds` restates the kernel's decision on the host and every window case
asserts that it holds the sequence it was built for."""
import ctypes as C

import numpy as np
import pytest
import torch

import filter_twin as ft
from elementwise import assert_sees_a_dropped_term, assert_within, pick_term
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U22 = 2.0 ** -22
C_BWD = 8.0
SWITCH = "GEOSSL_FILTER_BWD_TILE32"
HEIGHTS = (64, 32)
CAP = {64: 48, 32: 40}          # atoms a staged window holds (filter_bwd.hip: BwdLdsH::CAP)
NAMES = ("dw1", "db1", "dw2", "db2")
NAN = float("nan")

# molecule sizes whose dense pair slots sum n (n - 1) / 2 give the row count
ROW_CASES = {1: [2], 31: [8, 3], 32: [8, 3, 2], 33: [8, 3, 2, 2], 63: [10, 6, 3], 64: [10, 6, 3, 2], 65: [10, 6, 3, 2, 2],
             127: [16, 4, 2], 128: [16, 4, 2, 2], 129: [16, 4, 2, 2, 2]}
WINDOW_L = 12
WINDOW_CASES = {
    "18-atom molecules": [18] * 40,                            # a window serves two molecules
    "33 and 2 alternating": [33, 2] * 11,                      # a window change inside a tile's neighbourhood
    "33-atom molecules": [33] * 22,                            # 528 rows each: one window for more than eight tiles
    "tiny molecules": [2] * 600 + [3, 4, 5, 2] * 6,            # the unstaged fallback
    "fresh window every tile": ([10] + [2] * 10) * 75,         # the hazard of the single window buffer
}

_CACHE = {}


def problem(sizes, F=128, G=51, L=1, seed=7):
    """The tensors of a case and its twin, made once and never written again."""
    key = (tuple(sizes), F, G, L, seed)
    if key not in _CACHE:
        from test_gpu_round2 import _filter_problem
        lay, daggs, run, _ = _filter_problem(0, seed=seed, F=F, G=G, L=L, sizes=list(sizes))
        run.lay = lay
        _CACHE[key] = dict(F=F, G=G, L=L, lay=lay, daggs=daggs, run=run, inp=run.inputs,
                           refs=ft._filter_ref_and_bound(run, daggs))
    return _CACHE[key]


def set_height(monkeypatch, rows):
    for k in ("GEOSSL_FILTER_BWD_BF16X3", "GEOSSL_ARITH_24BIT"):
        monkeypatch.delenv(k, raising=False)
    if rows == 32:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)


def image_of(pair_d, P, p, dyn_P=None):
    from geossl_amd import _lib
    from geossl_amd._lib import call, ptr, stream
    img = torch.full((_lib.load().geossl_rbf_fragments_bytes(P),), 0xFF, dtype=torch.uint8, device=DEV)
    call("geossl_rbf_fragments_dyn", ptr(pair_d), P, p["G"], ptr(p["inp"]["offset"]), p["inp"]["coeff"], ptr(img),
         None if dyn_P is None else ptr(dyn_P), stream())
    return img


def launch(p, saved=True, image=False, rows=None, xs=None, daggs=None, T=None, N=None, dyn_P=None):
    """One weight-gradient launch -> [dw1, db1, dw2, db2] per layer, flat.  `rows`: (pair_d, pair_c, pair_flag, pair_i,
    pair_j) at a capacity, with `xs`, `daggs`, `T`, `N` and the device-side count `dyn_P` that go with them."""
    from geossl_amd import _lib
    from geossl_amd._lib import call, ptr, stream
    inp, lay, F, G, L = p["inp"], p["lay"], p["F"], p["G"], p["L"]
    if rows is None:
        rows = (inp["pair_d"], inp["pair_c"], inp["pair_flag"], lay.pair_i, lay.pair_j)
        xs, daggs, N = inp["xs"], p["daggs"], lay.N
    P = rows[0].numel()
    if T is None and saved:
        T = saved_rows(p)
    gin, gout = _lib.FilterGradIn(), _lib.FilterGradOut()
    outs = [[torch.full((F, G), NAN, device=DEV), torch.full((F,), NAN, device=DEV), torch.full((F, F), NAN, device=DEV),
             torch.full((F,), NAN, device=DEV)] for _ in range(L)]
    for l in range(L):
        gin.x[l], gin.dagg[l] = ptr(xs[l]), ptr(daggs[l])
        gout.dw1[l], gout.db1[l], gout.dw2[l], gout.db2[l] = (ptr(o) for o in outs[l])
    wsp = torch.full((_lib.load().geossl_cfconv_filter_bwd_workspace_floats(P, L, F, G),), NAN, device=DEV)
    args = tuple(ptr(a) for a in rows) + (P, N, C.byref(inp["fw"]), C.byref(gin), L, F, G, ptr(inp["offset"]), inp["coeff"],
                                         ptr(T) if saved else None, C.byref(gout), ptr(wsp), 0)
    dyn = () if dyn_P is None else (ptr(dyn_P), None)
    name = "geossl_cfconv_filter_bwd" + ("_frag" if image else "") + ("_dyn" if dyn_P is not None else "")
    if image:
        call(name, *args, *dyn, ptr(image_of(rows[0], P, p, dyn_P)), stream())
    else:
        call(name, *args, *dyn, stream())
    torch.cuda.synchronize()
    return [t for o in outs for t in o]


def saved_rows(p):
    """The hidden rows T of the case, from the forward kernel (once)."""
    if "T" not in p:
        from geossl_amd._lib import call, ptr, stream
        inp, P = p["inp"], p["inp"]["P"]
        T = torch.empty(p["L"], P, p["F"], device=DEV)
        Wf = torch.empty(p["L"], P, p["F"], device=DEV)
        call("geossl_cfconv_filter_fwd", ptr(inp["pair_d"]), ptr(inp["pair_c"]), P, C.byref(inp["fw"]), p["L"], p["F"], p["G"],
             ptr(inp["offset"]), inp["coeff"], ptr(T), ptr(Wf), stream())
        torch.cuda.synchronize()
        p["T"] = T
    return p["T"]


def check(got, refs, what):
    for l, r in enumerate(refs):
        for k, name in enumerate(NAMES):
            err = (got[4 * l + k].double() - r["ref"][k]).abs()
            ratio = float(torch.where(r["S"][k] > 0, err / (U22 * r["S"][k]), err * float("inf")).nan_to_num(0.0).max())
            print("ratio %-40s layer %2d %s %8.3f" % (what, l, name, ratio))
    for l, r in enumerate(refs):
        for k, name in enumerate(NAMES):
            assert_within(got[4 * l + k], r["ref"][k], r["S"][k], C_BWD, U22, "%s layer %d %s" % (what, l, name))


def window_kinds(pair_i, pair_j, rows, cap, L):
    """decide() of filter_bwd.hip on the host: per tile 's' (window kept), 'f' (fresh window) or 'u' (unstaged), the
    tiles of a block's contiguous range in a row, blocks separated by '|'."""
    pi, pj = pair_i.cpu().tolist(), pair_j.cpu().tolist()
    P = len(pi)
    ntiles = (P + rows - 1) // rows
    nb = max(1, min(256 // L, ntiles))
    per = (ntiles + nb - 1) // nb
    out = []
    for b in range(nb):
        have, walo, kinds = False, 0, ""
        for t in range(b * per, min(ntiles, (b + 1) * per)):
            alo, amax = pi[t * rows], max(pj[t * rows:(t + 1) * rows]) + 1
            if have and alo >= walo and amax - walo <= cap:
                kinds += "s"
            elif amax - alo <= cap:
                kinds += "f"
                have, walo = True, alo
            else:
                kinds += "u"
        out.append(kinds)
    return "|".join(out)


# ------------------------------------------------------------------------------------------------------ tile edges
@pytest.mark.parametrize("P", sorted(ROW_CASES))
def test_row_counts_around_the_tile_edges(P, monkeypatch):
    """The tail tile, an odd number of 32-row image tiles under a 64-row tile (P = 33, 65, 129: the last M block lies
    past the image), a block whose range is a single tile; saved rows with the kernel's own Gaussians and with the image."""
    p = problem(ROW_CASES[P])
    assert p["inp"]["P"] == P
    for rows in HEIGHTS:
        set_height(monkeypatch, rows)
        for image in (False, True):
            check(launch(p, image=image), p["refs"], "P=%d rows=%d image=%d" % (P, rows, image))


def test_dyn_forms_ignore_the_rows_past_the_count(monkeypatch):
    """Capacity 256, 65 real rows: the rows past the count point at two atoms of their own; those atoms and the hidden
    rows past the count are NaN.  Nothing of them may reach a gradient."""
    p = problem(ROW_CASES[65])
    inp, lay, L, F = p["inp"], p["lay"], p["L"], p["F"]
    P, N, cap = 65, lay.N, 256
    n = cap - P
    dead = torch.tensor([N, N + 1], dtype=torch.int32, device=DEV)
    rows = (torch.cat([inp["pair_d"], torch.full((n,), inp["cutoff"], device=DEV)]), torch.cat([inp["pair_c"], torch.zeros(n, device=DEV)]),
            torch.cat([inp["pair_flag"], torch.zeros(n, dtype=torch.uint8, device=DEV)]),
            torch.cat([lay.pair_i, dead[:1].expand(n)]), torch.cat([lay.pair_j, dead[1:].expand(n)]))
    pad = lambda ts: [torch.cat([t, torch.full((2, F), NAN, device=DEV)]) for t in ts]
    T = torch.full((L, cap, F), NAN, device=DEV)
    T[:, :P] = saved_rows(p)
    dyn_P = torch.tensor([P], dtype=torch.int32, device=DEV)
    kw = dict(rows=rows, xs=pad(inp["xs"]), daggs=pad(p["daggs"]), T=T, N=N + 2, dyn_P=dyn_P)
    for h in HEIGHTS:
        set_height(monkeypatch, h)
        for image in (False, True):
            check(launch(p, image=image, **kw), p["refs"], "dyn rows=%d image=%d" % (h, image))


# ---------------------------------------------------------------------------------------------------- window logic
def _window_problem(name):
    p = problem(WINDOW_CASES[name], L=WINDOW_L)
    kinds = {h: window_kinds(p["lay"].pair_i, p["lay"].pair_j, h, CAP[h], WINDOW_L) for h in HEIGHTS}
    print(name, {h: k[:80] for h, k in kinds.items()})
    return p, kinds


@pytest.mark.parametrize("name", sorted(WINDOW_CASES))
def test_atom_window_decisions(name, monkeypatch):
    p, kinds = _window_problem(name)
    k64 = kinds[64]
    if name == "18-atom molecules":
        assert "fs" in k64 and "u" not in k64               # a window is kept across tiles (two molecules fit)
    elif name == "33 and 2 alternating":
        assert "sfs" in k64 and "u" not in k64              # a fresh window between tiles that keep theirs
    elif name == "33-atom molecules":
        assert "s" * 8 in k64 and "u" not in k64            # one window for more than eight tiles
    elif name == "tiny molecules":
        assert "u" in k64 and "u" in kinds[32]              # the unstaged path at both heights
    else:
        assert "fff" in k64                                 # consecutive tiles each overwrite the one window buffer
    for rows in HEIGHTS:
        set_height(monkeypatch, rows)
        check(launch(p), p["refs"], "%s rows=%d" % (name, rows))


# ------------------------------------------------------------------------------------------------- widths and forms
FORM_SIZES = [18, 7, 33, 2, 18, 12, 5, 33]


@pytest.mark.parametrize("F, G", [(F, G) for F in (128, 64, 32) for G in (51, 40)])
def test_widths_and_gaussian_counts(F, G, monkeypatch):
    p = problem(FORM_SIZES, F=F, G=G, L=2)
    for rows in HEIGHTS:
        set_height(monkeypatch, rows)
        check(launch(p), p["refs"], "F=%d G=%d rows=%d" % (F, G, rows))


def test_rebuilt_hidden_rows_and_shared_image(monkeypatch):
    """T == NULL (the hidden rows rebuilt in the kernel), and three layers of one launch on one image."""
    p = problem(FORM_SIZES, L=3)
    for rows in HEIGHTS:
        set_height(monkeypatch, rows)
        check(launch(p, saved=False), p["refs"], "recompute rows=%d" % rows)
        check(launch(p, image=True), p["refs"], "image, 3 layers, rows=%d" % rows)


# --------------------------------------------------------------------------------------------- teeth, determinism
def test_a_dropped_row_is_seen(monkeypatch):
    """One pair row's product taken out of dw2 in the reference - a row of the SECOND M block of a 64-row tile: the
    checker flags exactly that element."""
    p = problem(FORM_SIZES, L=2)
    set_height(monkeypatch, 64)
    got = launch(p)
    r = p["refs"][0]
    rows = torch.arange(r["dO"].size(0), device=DEV)
    cand = rows[(rows % 64) >= 32]
    terms = r["dO"][cand][:, :, None] * r["tt"][cand][:, None, :]                      # [row, c, h]
    bound = C_BWD * U22 * r["S"][2][None] + (got[2].double() - r["ref"][2]).abs()[None]
    k, ratio = pick_term(terms, bound.expand_as(terms), torch.ones_like(terms, dtype=torch.bool))
    assert ratio > 2.0, ("no single product stands above the bound", ratio)
    kp, kc, kh = (int(v) for v in np.unravel_index(k, tuple(terms.shape)))
    assert_sees_a_dropped_term(got[2], r["ref"][2], r["S"][2], C_BWD, U22, (kc, kh), float(terms[kp, kc, kh]),
                               "dw2 without row %d" % int(cand[kp]))


def test_two_launches_at_64_rows_are_bit_identical(monkeypatch):
    p, _ = _window_problem("fresh window every tile")
    set_height(monkeypatch, 64)
    a, b = launch(p), launch(p)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), k
