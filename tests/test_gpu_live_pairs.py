"""The live-pair list of a dense layout (csrc/sparse_pairs.hip: k_live_pairs) and everything that runs on it: the list
build against a numpy stable compaction, the filter forward through the row map (Wf at the dense slot, T at the list's
row, dead Wf slots unwritten), the filter backward on the list against the fp64 twin, every aggregation form on filter
tensors whose dead rows were never written, and the fused SchNet / the DDM trainer with GEOSSL_LIVE_PAIRS on against
off."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import filter_twin as ft
from test_gpu_packed_kernels import assert_within
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
TOL_OUT, TOL_GRAD = 1e-5, 1e-4      # the suite's tolerances
U22, U24 = 2.0 ** -22, 2.0 ** -24
C_BWD = 8.0                         # |got - ref| <= c u S of the filter backward (tests/test_gpu_filter_classes.py)
SIZES = [1, 2, 18, 3, 33, 18, 2]    # 839 pair slots; molecule 1 is stretched (no live pair), molecule 3 squeezed (all live)
SIZES_CAPPED = [1, 2, 40, 3, 33, 18, 2]   # a 40-atom molecule: the general geometry kernel (neighbour cap, bit matrix)


# ------------------------------------------------------------------------------------------------------------ geometry
def _geometry(sizes, seed=5):
    """Random-tree molecules; the first 2-atom molecule stretched to 50 A (dead at every cutoff used here), the first
    3-atom molecule squeezed into 0.3 A (live at every cutoff used here) -> (layout, positions on the device, host
    intra-molecular pair distances in slot order)."""
    from geossl_amd.layout import MolLayout
    from geossl_amd.synthetic import make_batch
    b = make_batch(0, seed=seed, sizes=sizes)
    pos = np.array(b["positions"], dtype=np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)])
    m2, m3 = sizes.index(2), sizes.index(3)
    pos[off[m2] + 1] = pos[off[m2]] + np.float32([50.0, 0.0, 0.0])
    pos[off[m3]:off[m3] + 3] = pos[off[m3]] + np.float32([[0, 0, 0], [0.3, 0, 0], [0, 0.3, 0]])
    batch = torch.arange(len(sizes), device=DEV).repeat_interleave(torch.tensor(sizes, device=DEV))
    lay = MolLayout(batch, len(sizes), sizes=sizes)
    d = []
    for m, n in enumerate(sizes):
        i, j = np.triu_indices(n, k=1)
        p = pos[off[m]:off[m] + n].astype(np.float64)
        d.append(np.linalg.norm(p[i] - p[j], axis=1))
    return lay, torch.from_numpy(pos).to(DEV), np.concatenate(d) if d else np.zeros(0)


def _cutoff_for(dists, k):
    """A cutoff that leaves exactly k pair slots inside it: half way between the k-th and the (k + 1)-th distance."""
    s = np.sort(dists)
    assert s[k] - s[k - 1] > 1e-3, "no clear gap at %d" % k
    return float(0.5 * (s[k - 1] + s[k]))


def _widest_gap(dists, candidates):
    """Among the candidate live counts, the one with the widest gap between the neighbouring distances."""
    s = np.sort(dists)
    return max(candidates, key=lambda k: s[k] - s[k - 1])


def _best_multiple_of_32(dists, lo=5, hi=12):
    return _widest_gap(dists, [32 * q for q in range(lo, hi + 1)])


def _dense(lay, pos, cutoff):
    from geossl_amd import ops
    mol_live = torch.full((lay.B,), -1, dtype=torch.int32, device=DEV)
    d, c, fl = ops.pair_geometry(pos, lay, cutoff, mol_live=mol_live)
    return d, c, fl, mol_live


def _compact_ref(d, c, fl, pi, pj, P, cap, cutoff):
    """numpy: the rows with a flag, in slot order, then the tail convention."""
    d, c, fl, pi, pj = (a.cpu().numpy() for a in (d, c, fl, pi, pj))
    live = np.flatnonzero(fl[:P] != 0)
    n = live.size
    out = dict(pair_d=np.full(cap, np.float32(cutoff)), pair_c=np.zeros(cap, np.float32), pair_flag=np.zeros(cap, np.uint8),
               pair_i=np.zeros(cap, np.int32), pair_j=np.zeros(cap, np.int32), row_slot=np.zeros(cap, np.int32))
    out["pair_d"][:n], out["pair_c"][:n], out["pair_flag"][:n] = d[live], c[live], fl[live]
    out["pair_i"][:n], out["pair_j"][:n], out["row_slot"][:n] = pi[live], pj[live], live
    return out, n


def _assert_list(lp, ref, n, what):
    assert int(lp.n_live) == n, (what, int(lp.n_live), n)
    for k, want in ref.items():
        got = getattr(lp, k).cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, (what, k)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (what, k)   # (bit for bit, floats included)


# ------------------------------------------------------------------------------------------------------- the list build
@pytest.mark.parametrize("sizes", [SIZES, SIZES_CAPPED], ids=["flat", "capped"])
def test_live_pair_list_is_the_stable_compaction(sizes):
    """geossl_pair_geometry_live + geossl_live_pairs_build against numpy on the kernel's own dense arrays: a live count
    that is a multiple of 32 and one more than that, a molecule without a live pair, one with all of them, one-atom
    molecules; then a shorter list into the same buffers (the tail is rewritten)."""
    from geossl_amd import ops
    lay, pos, dists = _geometry(sizes)
    k32 = _best_multiple_of_32(dists)
    k33 = _widest_gap(dists, [32 * q + 1 for q in range(5, 13)])
    k_short = _widest_gap(dists, range(100, 150))   # (above the ~90 bonded pairs at 1.4 A, which have no gap between them)
    lp = None
    seen = {}
    for k in (k33, k32, k_short):      # the last list is the shortest: rows of the earlier ones must be gone
        cutoff = _cutoff_for(dists, k)
        d, c, fl, mol_live = _dense(lay, pos, cutoff)
        flags = fl.cpu().numpy()
        pp = lay.pair_ptr.cpu().numpy()
        per_mol = [int((flags[pp[m]:pp[m + 1]] != 0).sum()) for m in range(lay.B)]
        assert mol_live.cpu().tolist() == per_mol
        n_flag = int((flags != 0).sum())
        if max(sizes) <= 33:           # (no neighbour cap in play: the flags are the plain threshold test)
            assert n_flag == k, (n_flag, k)
        m2, m3 = sizes.index(2), sizes.index(3)
        assert per_mol[m2] == 0 and per_mol[m3] == 3 and per_mol[sizes.index(1)] == 0
        lp = ops.live_pairs(d, c, fl, lay, mol_live, cutoff, out=lp)
        ref, n = _compact_ref(d, c, fl, lay.pair_i, lay.pair_j, lay.P, lay.P, cutoff)
        assert n == n_flag
        _assert_list(lp, ref, n, "k = %d" % k)
        assert bool((lp.pair_i[:n - 1] <= lp.pair_i[1:n]).all())     # (what the backward's window logic relies on)
        seen[k] = n
    if max(sizes) <= 33:
        assert seen[k33] % 32 == 1 and seen[k32] % 32 == 0
    assert seen[k_short] < min(seen[k32], seen[k33])


def test_live_pair_list_in_a_capacity_larger_than_the_real_slot_count():
    """The capacity launch: every array has more rows than the batch has slots, the real slot count is on the device
    (dyn_P), and the slots past it hold junk with flags set - none of it may reach the list."""
    from geossl_amd._lib import call, ptr, stream
    lay, pos, dists = _geometry(SIZES)
    cutoff = _cutoff_for(dists, _best_multiple_of_32(dists))
    d, c, fl, mol_live = _dense(lay, pos, cutoff)
    P, cap = lay.P, lay.P + 197
    pad = lambda a, v: torch.cat([a, torch.full((cap - P,), v, dtype=a.dtype, device=DEV)])
    dd, cc, ff = pad(d, 1.0), pad(c, 0.5), pad(fl, 3)
    pi, pj = pad(lay.pair_i, 7), pad(lay.pair_j, 9)
    dyn_P = torch.tensor([P], dtype=torch.int32, device=DEV)
    out = types.SimpleNamespace(
        pair_d=torch.full((cap,), -1.0, device=DEV), pair_c=torch.full((cap,), -1.0, device=DEV),
        pair_flag=torch.full((cap,), 9, dtype=torch.uint8, device=DEV),
        pair_i=torch.full((cap,), -1, dtype=torch.int32, device=DEV), pair_j=torch.full((cap,), -1, dtype=torch.int32, device=DEV),
        row_slot=torch.full((cap,), -1, dtype=torch.int32, device=DEV), n_live=torch.full((1,), -1, dtype=torch.int32, device=DEV))
    call("geossl_live_pairs_build", ptr(dd), ptr(cc), ptr(ff), ptr(pi), ptr(pj), ptr(lay.mol_ptr), ptr(lay.pair_ptr),
         ptr(mol_live), lay.B, cap, cutoff, ptr(dyn_P), ptr(out.pair_d), ptr(out.pair_c), ptr(out.pair_flag), ptr(out.pair_i),
         ptr(out.pair_j), ptr(out.row_slot), ptr(out.n_live), stream())
    ref, n = _compact_ref(d, c, fl, lay.pair_i, lay.pair_j, P, cap, cutoff)
    _assert_list(out, ref, n, "capacity")
    assert 0 < n < P


# ------------------------------------------------------------------------------------------- forward through the row map
def _weights(F, G, L, seed):
    from geossl_amd import _lib
    from geossl_amd._lib import ptr
    gen = torch.Generator().manual_seed(seed)
    ws = [[(torch.randn(F, G, generator=gen) / G ** 0.5).to(DEV), (0.3 * torch.randn(F, generator=gen)).to(DEV),
           (torch.randn(F, F, generator=gen) / F ** 0.5).to(DEV), (0.3 * torch.randn(F, generator=gen)).to(DEV)]
          for _ in range(L)]
    fw = _lib.FilterWeights()
    for l, w in enumerate(ws):
        fw.w1[l], fw.b1[l], fw.w2[l], fw.b2[l] = (ptr(x) for x in w)
    return ws, fw, gen


def _smearing(G, cutoff):
    offset = torch.linspace(0.0, cutoff, G).to(DEV)
    return offset, -0.5 / float(offset[1] - offset[0]) ** 2


_NAN_BITS = torch.full((GUARD,), float("nan")).view(torch.int32)


def _guarded(*shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _assert_guards(buf, what):
    bits, pat = buf.view(torch.int32), _NAN_BITS.to(DEV)
    assert torch.equal(bits[:GUARD], pat) and torch.equal(bits[-GUARD:], pat), (what, "guard floats were written")


@pytest.mark.parametrize("form", ["two-piece", "bf16x3"])
@pytest.mark.parametrize("F, G", [(128, 51), (64, 20), (32, 8)])
def test_filter_forward_through_the_row_map(F, G, form, monkeypatch):
    """geossl_cfconv_filter_fwd_rows on the live-pair list of a 3 A graph (more than 30 % of the 839 slots dead) into
    NaN-filled T and Wf: the Wf rows of live slots are the plain call's bits, dead slots stay NaN, T is compact
    (T[:, r] = the plain T at row_slot[r], rows past n_live unwritten) and nothing is written outside either buffer."""
    from geossl_amd import ops
    from geossl_amd._lib import call, ptr, stream
    monkeypatch.delenv("GEOSSL_ARITH_24BIT", raising=False)
    if form == "bf16x3":
        monkeypatch.setenv("GEOSSL_FILTER_FWD_BF16X3", "1")
    else:
        monkeypatch.delenv("GEOSSL_FILTER_FWD_BF16X3", raising=False)
    L, cutoff = 2, 3.0
    lay, pos, _ = _geometry(SIZES)
    d, c, fl, mol_live = _dense(lay, pos, cutoff)
    lp = ops.live_pairs(d, c, fl, lay, mol_live, cutoff)
    P, n = lay.P, int(lp.n_live)
    live = fl != 0
    assert n == int(live.sum()) and n % 32 != 0 and P - n >= 0.3 * P, (n, P)
    ws, fw, _ = _weights(F, G, L, 11)
    offset, coeff = _smearing(G, cutoff)
    T0, W0 = torch.empty(L, P, F, device=DEV), torch.empty(L, P, F, device=DEV)
    call("geossl_cfconv_filter_fwd", ptr(d), ptr(c), P, C.byref(fw), L, F, G, ptr(offset), coeff, ptr(T0), ptr(W0), stream())
    tb, T = _guarded(L, P, F)
    wb, Wf = _guarded(L, P, F)
    call("geossl_cfconv_filter_fwd_rows", ptr(lp.pair_d), ptr(lp.pair_c), P, C.byref(fw), L, F, G, ptr(offset), coeff,
         ptr(T), ptr(Wf), lp.dyn_P, ptr(lp.row_slot), stream())
    torch.cuda.synchronize()
    _assert_guards(tb, "T")
    _assert_guards(wb, "Wf")
    assert not bool(W0[:, live].isnan().any())
    assert torch.equal(Wf[:, live], W0[:, live])
    assert bool(Wf[:, ~live].isnan().all())
    slots = lp.row_slot[:n].long()
    assert torch.equal(T[:, :n], T0[:, slots])
    assert bool(T[:, n:].isnan().all())
    # without T (inference): the same filter rows
    wb2, Wf2 = _guarded(L, P, F)
    call("geossl_cfconv_filter_fwd_rows", ptr(lp.pair_d), ptr(lp.pair_c), P, C.byref(fw), L, F, G, ptr(offset), coeff,
         None, ptr(Wf2), lp.dyn_P, ptr(lp.row_slot), stream())
    torch.cuda.synchronize()
    _assert_guards(wb2, "Wf, T == NULL")
    assert torch.equal(Wf2[:, live], W0[:, live]) and bool(Wf2[:, ~live].isnan().all())


# ------------------------------------------------------------------------------------------------- backward on the list
BWD_SIZES = [18, 33] + [2] * 60 + [3] * 30 + [1] * 5 + [18, 2, 2, 3]


@pytest.fixture(scope="module")
def bwd_problem():
    return _bwd_problem()


def _bwd_problem():
    """Runs of 2- and 3-atom molecules (one slot per two atoms: a 32-row tile spans more than the 40 atoms of the
    backward's staged window, so the global-index path runs) between larger ones, at 3 A; the fp64 twin once."""
    from geossl_amd import ops
    from geossl_amd._lib import call, ptr, stream
    F, G, L, cutoff = 128, 51, 2, 3.0
    lay, pos, _ = _geometry(BWD_SIZES, seed=8)
    d, c, fl, mol_live = _dense(lay, pos, cutoff)
    lp = ops.live_pairs(d, c, fl, lay, mol_live, cutoff)
    n = int(lp.n_live)
    # a tile of 32 rows of the list inside the run of small molecules touches more than 40 atoms
    pi, pj = lp.pair_i[:n].cpu().numpy(), lp.pair_j[:n].cpu().numpy()
    spans = [int(pj[r:r + 32].max() - pi[r:r + 32].min() + 1) for r in range(0, n, 32)]
    assert max(spans) > 40 and min(spans) <= 40, spans
    assert 0 < n < lay.P
    ws, fw, gen = _weights(F, G, L, 21)
    offset, coeff = _smearing(G, cutoff)
    xs = [torch.randn(lay.N, F, generator=gen).to(DEV) for _ in range(L)]
    daggs = [torch.randn(lay.N, F, generator=gen).to(DEV) for _ in range(L)]
    P = lay.P
    T = torch.empty(L, P, F, device=DEV)
    Wf = torch.empty(L, P, F, device=DEV)
    call("geossl_cfconv_filter_fwd", ptr(d), ptr(c), P, C.byref(fw), L, F, G, ptr(offset), coeff, ptr(T), ptr(Wf), stream())
    Tc = torch.full((L, P, F), float("nan"), device=DEV)
    call("geossl_cfconv_filter_fwd_rows", ptr(lp.pair_d), ptr(lp.pair_c), P, C.byref(fw), L, F, G, ptr(offset), coeff,
         ptr(Tc), ptr(Wf), lp.dyn_P, ptr(lp.row_slot), stream())
    run = types.SimpleNamespace(inputs=dict(pair_d=d, pair_c=c, pair_flag=fl, ws=ws, xs=xs, offset=offset, coeff=coeff),
                                lay=lay)
    refs = ft._filter_ref_and_bound(run, daggs)
    # (fw holds raw addresses: the weight tensors live as long as the problem does)
    return dict(F=F, G=G, L=L, lay=lay, lp=lp, d=d, c=c, fl=fl, fw=fw, ws=ws, offset=offset, coeff=coeff, xs=xs, daggs=daggs,
                T=T, Tc=Tc, refs=refs)


def _filter_bwd(p, compact, saved_T=True):
    from geossl_amd import _lib
    from geossl_amd._lib import call, ptr, stream
    F, G, L, lay, lp = p["F"], p["G"], p["L"], p["lay"], p["lp"]
    gin, gout = _lib.FilterGradIn(), _lib.FilterGradOut()
    outs = [[torch.full((F, G), float("nan"), device=DEV), torch.full((F,), float("nan"), device=DEV),
             torch.full((F, F), float("nan"), device=DEV), torch.full((F,), float("nan"), device=DEV)] for _ in range(L)]
    for l in range(L):
        gin.x[l], gin.dagg[l] = ptr(p["xs"][l]), ptr(p["daggs"][l])
        gout.dw1[l], gout.db1[l], gout.dw2[l], gout.db2[l] = (ptr(o) for o in outs[l])
    P = lay.P
    wsp = torch.full((_lib.load().geossl_cfconv_filter_bwd_workspace_floats(P, L, F, G),), float("nan"),
                     device=DEV)       # (the launch must write every partial sum it reads)
    if compact:
        rows = (lp.pair_d, lp.pair_c, lp.pair_flag, lp.pair_i, lp.pair_j)
        T, dyn_P = p["Tc"], lp.dyn_P
    else:
        rows = (p["d"], p["c"], p["fl"], lay.pair_i, lay.pair_j)
        T, dyn_P = p["T"], None
    call("geossl_cfconv_filter_bwd_dyn", *(ptr(a) for a in rows), P, lay.N, C.byref(p["fw"]), C.byref(gin), L, F, G,
         ptr(p["offset"]), p["coeff"], ptr(T) if saved_T else None, C.byref(gout), ptr(wsp), 0, dyn_P, None, stream())
    torch.cuda.synchronize()
    return [t_ for o in outs for t_ in o]


@pytest.mark.parametrize("form", ["saved", "recompute", "bf16x3"])
def test_filter_backward_on_the_live_pair_list(bwd_problem, form, monkeypatch):
    """geossl_cfconv_filter_bwd_dyn on the compact rows, the compact T and dyn_P = n_live: all four weight gradients of
    every layer against the fp64 twin of the DENSE problem (the dead rows contribute nothing) - per element at the
    bound of the existing suite and as a whole at TOL_GRAD -, against the dense launch of the same build (two
    summation orders of the same terms: at most twice that bound apart), and bit-identical over repeated launches."""
    p = bwd_problem
    monkeypatch.delenv("GEOSSL_ARITH_24BIT", raising=False)
    if form == "bf16x3":
        monkeypatch.setenv("GEOSSL_FILTER_BWD_BF16X3", "1")
    else:
        monkeypatch.delenv("GEOSSL_FILTER_BWD_BF16X3", raising=False)
    u = U24 if form == "bf16x3" else U22
    saved = form != "recompute"
    got = _filter_bwd(p, compact=True, saved_T=saved)
    dense = _filter_bwd(p, compact=False, saved_T=saved)
    names = ("dw1", "db1", "dw2", "db2")
    for l, r in enumerate(p["refs"]):
        for k, name in enumerate(names):
            g, dn, ref, S = got[4 * l + k], dense[4 * l + k], r["ref"][k], r["S"][k]
            scale = float(ref.abs().max())
            e_list, e_dense = float((g.double() - ref).abs().max()) / scale, float((dn.double() - ref).abs().max()) / scale
            e_pair = float((g.double() - dn.double()).abs().max()) / scale
            print("bwd %-9s layer %d %-3s  list %.3e  dense %.3e  list-dense %.3e" % (form, l, name, e_list, e_dense, e_pair))
    for l, r in enumerate(p["refs"]):
        for k, name in enumerate(names):
            g, dn, ref, S = got[4 * l + k], dense[4 * l + k], r["ref"][k], r["S"][k]
            what = "%s layer %d %s" % (form, l, name)
            assert not bool(g.isnan().any()), what
            assert float((g.double() - ref).abs().max() / ref.abs().max()) < TOL_GRAD, what
            assert_within(g, ref, S, C_BWD, u, what)
            assert_within(g, dn.double(), S, 2 * C_BWD, u, what + " against the dense launch")
    for rep in range(3):
        again = _filter_bwd(p, compact=True, saved_T=saved)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), (form, rep)


# -------------------------------------------------------------------------- aggregation on filter rows never written
def _agg_layout(sizes):
    from geossl_amd.layout import MolLayout
    batch = torch.arange(len(sizes), device=DEV).repeat_interleave(torch.tensor(sizes, device=DEV))
    return MolLayout(batch, len(sizes), sizes=sizes)


# ("work": GEOSSL_AGG_TARGETS_MAX=0 - the work list of register walks that launches above 256 molecules take)
AGG_CASES = [("register walk, 18 atoms", [18] * 12, 128, "agg"),
             ("register walk, class above 20", [26] * 6, 128, "work"),
             ("work list, ragged", [1, 2, 18, 3, 33, 18, 2, 27, 21], 128, "work"),
             ("target lists, ragged", [1, 2, 18, 3, 33, 18, 2, 27, 21], 128, "agg"),
             ("target lists, above 33 atoms", [40, 18, 2, 1, 57], 128, "agg"),
             ("one block per molecule, F = 32", [18, 7, 2, 1, 20], 32, "agg"),
             ("F = 64", [18] * 5 + [9, 33], 64, "agg"),
             ("layer loop, uniform", [18] * 40, 128, "loop"),
             ("layer loop, block form", [5, 9, 18, 20, 2, 1, 13, 17, 20, 11, 3, 16, 33, 27], 128, "loop")]


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("what, sizes, F, how", AGG_CASES, ids=[c[0] for c in AGG_CASES])
def test_unwritten_filter_rows_are_harmless(what, sizes, F, how, swap, monkeypatch):
    """Every aggregation form drops the filter row of a slot without an edge by a select, never by arithmetic: with NaN
    in the dead rows it returns the bits it returns with zeros there."""
    from geossl_amd import ops
    from geossl_amd.synthetic import make_batch
    if how == "work":
        monkeypatch.setenv("GEOSSL_AGG_TARGETS_MAX", "0")
    else:
        monkeypatch.delenv("GEOSSL_AGG_TARGETS_MAX", raising=False)
    lay = _agg_layout(sizes)
    assert lay.agg_targets == (how != "work" and max(sizes) > 20)
    pos = torch.from_numpy(np.array(make_batch(0, seed=3, sizes=sizes)["positions"], dtype=np.float32)).to(DEV)
    _, _, fl = ops.pair_geometry(pos, lay, 3.0)
    dead = fl == 0
    assert int(dead.sum()) >= 0.2 * lay.P
    gen = torch.Generator().manual_seed(len(sizes))
    x = torch.randn(lay.N, F, generator=gen).to(DEV)
    W = torch.randn(lay.P, F, generator=gen).to(DEV)
    outs = []
    for fill in (0.0, float("nan")):
        Wd = W.clone()
        Wd[dead] = fill
        out = torch.full((lay.N, F), float("nan"), device=DEV)
        if how == "loop":
            assert ops.layer_loop([("agg", x, Wd, out, swap)], lay, fl, lay.N, F), "no layer loop for this shape"
        else:
            ops.aggregate(x, Wd, fl, lay, swap=swap, out=out)
        torch.cuda.synchronize()
        outs.append(out)
    assert not bool(outs[0].isnan().any())
    assert torch.equal(outs[0], outs[1])


# --------------------------------------------------------------------------------------------------------- model level
MODEL_SIZES = [2, 20, 7, 18, 13, 3]


def _model_batch():
    from geossl_amd.synthetic import make_batch
    return make_batch(0, seed=23, sizes=MODEL_SIZES)


@pytest.mark.parametrize("L, cutoff", [(2, 3.0), (3, 5.0), (3, 3.0)])
def test_fused_schnet_on_live_pairs_against_every_slot_and_the_fp64_oracle(L, cutoff, monkeypatch):
    """SchNet(F = 128) on six molecules of 2 .. 20 atoms with GEOSSL_LIVE_PAIRS on and off: the live-pair launches are
    made (and not made), atom features and output bit-identical, every parameter gradient within TOL_GRAD of
    oracle.nets.schnet_forward in fp64 in both modes."""
    import geossl_amd.Geom3D.models.schnet as sm
    from conftest import assert_close, rel_err
    from helpers import product_schnet, schnet_oracle_params, t, unique_named_grads
    from oracle import nets
    b = _model_batch()
    cfg = dict(hidden_channels=128, num_filters=128, num_interactions=L, num_gaussians=51, cutoff=cutoff, node_class=9,
               readout="add")
    w = torch.cos(torch.arange(128, dtype=torch.float64))
    names = []
    real_call = sm.call
    monkeypatch.setattr(sm, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("GEOSSL_LIVE_PAIRS", mode)
        del names[:]
        model = product_schnet(cfg, DEV)
        out, h = model(t(b["x"], DEV)[:, 0], t(b["positions"], DEV), t(b["batch"], DEV), return_latent=True)
        ((h ** 2).sum() + (out * w.float().to(DEV)).sum()).backward()
        assert ("geossl_cfconv_filter_fwd_rows" in names) == (mode == "1"), sorted(set(names))
        assert ("geossl_cfconv_filter_fwd_dyn" in names) == (mode == "0"), sorted(set(names))
        res[mode] = (out.detach(), h.detach(), unique_named_grads(model))
    assert torch.equal(res["1"][0], res["0"][0]) and torch.equal(res["1"][1], res["0"][1])
    P64 = {k: v.detach().double().requires_grad_(v.requires_grad) for k, v in schnet_oracle_params(cfg).items()}
    out64, h64 = nets.schnet_forward(P64, t(b["x"])[:, 0], t(b["positions"]).double(), t(b["batch"]), cutoff, L, "add",
                                     return_latent=True)
    ((h64 ** 2).sum() + (out64 * w).sum()).backward()
    assert_close(res["1"][0].cpu().double(), out64.detach(), TOL_OUT, "out")
    assert_close(res["1"][1].cpu().double(), h64.detach(), TOL_OUT, "h")
    for mode in ("1", "0"):
        grads = res[mode][2]
        assert len(grads) == len([k for k, v in P64.items() if v.requires_grad])
        for k, g in grads.items():
            e = rel_err(g.cpu().double(), P64[k].grad)
            print("L=%d cutoff=%.0f live=%s %-34s %.3e" % (L, cutoff, mode, k, e))
        for k, g in grads.items():
            assert rel_err(g.cpu().double(), P64[k].grad) < TOL_GRAD, (mode, k)


def _ddm_trainer(**kw):
    from geossl_amd import pretrain_GeoSSL as pg
    from helpers import product_ncsn, product_schnet
    cfg = dict(hidden_channels=128, num_filters=128, num_interactions=2, num_gaussians=51, cutoff=5.0, node_class=9,
               readout="mean")
    return pg.DDMTrainer(product_schnet(cfg, DEV), product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9),
                         lr=5e-4, **kw)


def test_structure_graph_replay_is_the_eager_step_on_live_pairs(monkeypatch):
    """Three DDMTrainer steps on equal-sized molecules (a per-structure graph with the layer loop), live pairs on: the
    replayed step gives the eager step's losses and parameters bit for bit while the live count changes with the
    positions."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import draw_noise, make_batch
    from helpers import t
    monkeypatch.setenv("GEOSSL_LIVE_PAIRS", "1")
    out = {}
    for use_graph in (False, True):
        tr = _ddm_trainer(use_graph=use_graph)
        losses = []
        for step in range(3):
            b = make_batch(32, seed=40 + step, mode="A")
            noise = {k: t(v, DEV) for k, v in draw_noise(b, seed=140 + step).items()}
            losses.append(float(tr.step(pg.Batch.from_numpy(b, DEV), noise)))
        assert tr.use_graph == use_graph, "capture fell back to eager"
        out[use_graph] = (losses, tr.flat.flat.detach().clone())
    assert out[True][0] == out[False][0], (out[True][0], out[False][0])
    assert torch.equal(out[True][1], out[False][1])


def test_bucket_graph_replay_is_the_eager_bucket_step_on_live_pairs(monkeypatch):
    """Three steps on ragged batches handed over by DeviceLoader (every batch its own sizes, so the live count and the
    slot count both change between replays of the ONE captured graph), live pairs on: losses and parameters bit-identical
    to the same launches made eagerly on a bucket of the same capacity."""
    from geossl_amd import bucket as bk
    from geossl_amd import ops
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    from geossl_amd.synthetic import make_batch
    monkeypatch.setenv("GEOSSL_LIVE_PAIRS", "1")
    B = 24
    pool = make_batch(96, seed=61, mode="B")
    ds = DeviceDataset.from_numpy(pool, DEV, option="combination")
    handles = list(DeviceLoader(ds, batch_size=B, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(6)))[:3]
    assert len(handles) == 3
    # (the batch with the most pair slots first: a later, larger batch would grow the bucket and capture again)
    handles.sort(key=lambda hb: -int((np.asarray(hb._sizes) * (np.asarray(hb._sizes) - 1)).sum()))
    gen = torch.Generator().manual_seed(7)
    noise = []
    for hb in handles:
        N, S = hb.n_atoms, hb.n_super
        noise.append({"pos_noise": (0.3 * torch.randn(N, 3, generator=gen)).to(DEV),
                      "noise_level_1": torch.randint(0, 50, (B,), generator=gen).to(DEV),
                      "dist_noise_1": torch.randn(S, 1, generator=gen).to(DEV),
                      "noise_level_2": torch.randint(0, 50, (B,), generator=gen).to(DEV),
                      "dist_noise_2": torch.randn(S, 1, generator=gen).to(DEV)})
    # the live share of the batches differs (what the replayed launches read from the device)
    shares = []
    for hb in handles:
        co = ds.collate(hb)
        from geossl_amd.layout import MolLayout
        lay = MolLayout(co.batch, B, sizes=[int(v) for v in hb._sizes])
        shares.append((int((ops.pair_geometry(co.positions, lay, 5.0)[2] != 0).sum()), lay.P))
    assert len(set(shares)) == 3 and all(n < P for n, P in shares), shares

    tr = _ddm_trainer(use_graph=True)
    got = [float(tr.step(hb, nz)) for hb, nz in zip(handles, noise)]
    assert tr.use_graph and tr.step_graphs.captures == 1 and len(tr._graphs) == 1
    keys = [k for k in tr._graphs if isinstance(k, tuple) and k and k[0] == "bucket"]
    assert len(keys) == 1, list(tr._graphs)
    bkt = tr._graphs[keys[0]]["bucket"]

    te = _ddm_trainer(use_graph=False)
    eb = bk.Bucket(torch.device(DEV), B, bkt.caps(), "combination")
    f32 = dict(dtype=torch.float32, device=DEV)
    sn = {"pos_noise": torch.zeros(eb.N_cap, 3, **f32), "dist_noise_1": torch.zeros(eb.S_cap, 1, **f32),
          "dist_noise_2": torch.zeros(eb.S_cap, 1, **f32), "noise_level_1": torch.zeros(B, dtype=torch.long, device=DEV),
          "noise_level_2": torch.zeros(B, dtype=torch.long, device=DEV)}
    eager = []
    for hb, nz in zip(handles, noise):
        N, P, S, W = eb.fill(hb)
        sn["pos_noise"][:N].copy_(nz["pos_noise"])
        sn["dist_noise_1"][:S].copy_(nz["dist_noise_1"])
        sn["dist_noise_2"][:S].copy_(nz["dist_noise_2"])
        sn["noise_level_1"].copy_(nz["noise_level_1"])
        sn["noise_level_2"].copy_(nz["noise_level_2"])
        loss = te._fwd_bwd(eb.batch, sn)
        te.opt.step(grad_scale=te.reduce())
        eager.append(float(loss))
    assert all(math.isfinite(v) for v in got)
    assert got == eager, (got, eager)
    assert torch.equal(tr.flat.flat, te.flat.flat)


def test_position_gradient_path_forms_the_filter_gradients_of_the_live_path(monkeypatch):
    """With a position gradient the forward keeps T and Wf per dense slot (filter_dpos reads both by one index); the
    backward regroups T to the list's rows (geossl_gather_live_rows) and runs the weight-gradient kernel on the list:
    every parameter gradient is the one of the path without the position gradient, bit for bit."""
    import geossl_amd.Geom3D.models.schnet as sm
    from geossl_amd import ops
    from helpers import product_schnet, t, unique_named_grads
    monkeypatch.setenv("GEOSSL_LIVE_PAIRS", "1")
    b = _model_batch()
    cfg = dict(hidden_channels=128, num_filters=128, num_interactions=2, num_gaussians=51, cutoff=3.0, node_class=9,
               readout="add")
    names = []
    real_call = sm.call
    for mod in (sm, ops):   # (the regrouping is launched by the forward's ops.PairGraph)
        monkeypatch.setattr(mod, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    model = product_schnet(cfg, DEV)
    w = torch.cos(torch.arange(128, dtype=torch.float32, device=DEV))
    grads = {}
    for with_pos in (True, False):
        model.zero_grad()
        del names[:]
        pos = t(b["positions"], DEV).requires_grad_(with_pos)
        out = model(t(b["x"], DEV)[:, 0], pos, t(b["batch"], DEV))
        (out * w).sum().backward()
        assert ("geossl_gather_live_rows" in names) == with_pos and ("geossl_cfconv_filter_dpos" in names) == with_pos
        assert ("geossl_cfconv_filter_fwd_rows" in names) == (not with_pos)
        grads[with_pos] = {k: v.clone() for k, v in unique_named_grads(model).items()}
    assert grads[True].keys() == grads[False].keys()
    for k, v in grads[True].items():
        assert torch.equal(v, grads[False][k]), k
