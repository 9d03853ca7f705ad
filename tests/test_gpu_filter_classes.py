"""The filter-network kernels at every Gaussian-count class, through the raw C ABI, against the fp64 twin
(tests/filter_twin.py), element by element.

k_filter_fwd<NMB, K1S>, k_filter_fwd_h<NMB, K1S> and k_filter_dpos<NMB, K1S> are compiled per 16-wide k-step class
K1S = ceil(G / 16); k_filter_bwd<NW> and k_filter_bwd_h<NW, RECOMP> pad the Gaussian dimension by hand and change the
bias sum at G = 64.  The grid below holds the class edges (16|17, 32|33, 48|49), the interior of K1S = 3, G = 1 and the
ones-column boundary 63|64, at every width.  Every test
- checks |got - ref| <= c u S per element (ref, S from the twin; u = 2^-22 for two fp16 pieces, 2^-24 for three bf16
  pieces and for fp32 arithmetic), on outputs with 64 NaN guard floats in front and behind that must stay bit-unchanged,
- on the `main` batch proves it would see the last Gaussian missing, or one Gaussian too many, in a single element,
- launches four times and counts the elements that differ (must be 0).
The constants c of the forward and of the position gradient are four times the worst err / (u S) measured on the MI355X
over the whole grid, rounded up to a power of two (DESIGN.md section 4 holds the measured figures)."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import filter_twin as ft
from test_gpu_packed_kernels import assert_sees_a_dropped_term, assert_within, pick_term
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U22, U24 = 2.0 ** -22, 2.0 ** -24
REPEATS = 4
GUARD = 64
TOL_OUT, TOL_GRAD = 1e-5, 1e-4      # the suite's tolerances

GRID_F = (32, 64, 128)
GRID_G = (1, 16, 17, 32, 33, 40, 48, 49, 63, 64)
DEEP_G = (40, 64)
TINY_G = (16, 17, 48, 63)           # one count per k-step class
CUTOFF = 5.0

# c of |got - ref| <= c u S.  Backward: the value of test_gpu_packed_kernels.py for that family.  Forward and position
# gradient: 4 x the worst err / (u S) measured on the MI355X over every case below, rounded up to a power of two
# (DESIGN.md section 4): two-piece forward 0.594 (T; Wf 0.195), three-piece forward 2.028 (T; Wf 1.448), dd 0.133.
C_BWD = 8.0
C_FWD = {"two-piece": 4.0, "bf16x3": 16.0}
C_DPOS = 1.0

CASES = [("main", F, G) for F in GRID_F for G in GRID_G] + [("edge", F, G) for F in GRID_F for G in GRID_G] + \
        [("deep", F, G) for F in GRID_F for G in DEEP_G] + \
        [(kind, F, G) for F in GRID_F for G in TINY_G for kind in ("tiny1", "tiny31")]


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The worst err / (u S) per family and form over the cases that ran (what DESIGN.md section 4 records)."""
    yield
    for k in sorted(WORST):
        print("worst err/(u S)  %-28s %8.3f  at %s" % ((k,) + WORST[k]))


def note(family, got, ref, S, u, where, extra=None):
    """Record and print err / (u S) of a tensor before it is asserted on."""
    err = (got.double() - ref).abs()
    if extra is not None:
        err = (err - extra).clamp_min(0.0)
    r = torch.where(S > 0, err / (u * S), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = float(r.max()) if r.numel() else 0.0
    print("ratio %-28s %-22s %8.3f" % (family, where, r))
    if family not in WORST or not r <= WORST[family][0]:
        WORST[family] = (r, where)
    return r


# ------------------------------------------------------------------------------------------------------------ problems
def _main_sizes(nmol, seed):
    from geossl_amd.synthetic import molecule_sizes
    # set B plus two single atoms, a 2-atom molecule and a 6-atom molecule whose last two atoms coincide
    return [int(n) for n in molecule_sizes(nmol, "B", np.random.default_rng(seed))] + [1, 2, 1, 6]


def _coincide(positions):
    positions[-1] = positions[-2]


def _edge_geometry(seed):
    """About 1 % of the pair slots moved to d = r_c (1 - 2^-k), k = 6 .. 22, as edges in both directions, the envelope
    recomputed in fp32 op by op as geossl_pair_geometry does: next to the cutoff it rounds to zero."""
    def edit(pair_d, pair_c, pair_flag):
        P = pair_d.numel()
        gen = torch.Generator().manual_seed(seed)
        n = max(P // 100, 34)
        idx = torch.randperm(P - 1, generator=gen)[:n].to(DEV)        # (the last slot stays: the coincident pair)
        k = (6 + torch.arange(n) % 17).double()
        d = (CUTOFF * (1.0 - torch.exp2(-k))).float().to(DEV)
        assert bool((d < CUTOFF).all())
        pair_d[idx] = d
        pair_c[idx] = 0.5 * (torch.cos(d * np.float32(math.pi) / np.float32(CUTOFF)) + 1.0)
        pair_flag[idx] = 3
        edit.slots = idx
    return edit


_PROBLEM = {}


def problem(kind, F, G):
    """The case's tensors (tests/test_gpu_round2.py: _filter_problem) and what its tests share: built once per case,
    one case alive at a time (the fp64 tensors are large)."""
    from test_gpu_round2 import _filter_problem
    key = (kind, F, G)
    if _PROBLEM.get("key") == key:
        return _PROBLEM["value"]
    _PROBLEM.clear()
    torch.cuda.empty_cache()
    seed = 32
    kw = dict(seed=seed, F=F, G=G, cutoff=CUTOFF)
    edit = None
    if kind in ("main", "edge"):
        edit = _edge_geometry(seed) if kind == "edge" else None
        lay, daggs, run, _ = _filter_problem(0, L=2, sizes=_main_sizes(300, seed), move=_coincide, geometry=edit, **kw)
    elif kind == "deep":
        lay, daggs, run, _ = _filter_problem(0, L=6, sizes=_main_sizes(72, seed), move=_coincide, **kw)
    else:
        lay, daggs, run, _ = _filter_problem(0, L=2, sizes=[2] if kind == "tiny1" else [8, 3], **kw)
    run.lay = lay
    inp = run.inputs
    L = len(inp["ws"])
    P = inp["P"]
    if kind in ("main", "edge"):
        # some waves of the forward and of dpos take a second row block, some blocks of the backward a second tile
        assert P % 32 != 0 and (P + 31) // 32 > 8 * (256 // L) and (P + 31) // 32 > 256 // L, P
    if kind == "edge":
        zero = int((inp["pair_c"][edit.slots] == 0).sum())
        assert zero >= 1 and edit.slots.numel() < 0.02 * P and int((inp["pair_c"] == 0).sum()) < 0.02 * P, (zero, P)
    if kind == "tiny1":
        assert P == 1
    if kind == "tiny31":
        assert P == 31
    value = dict(kind=kind, F=F, G=G, L=L, P=P, lay=lay, daggs=daggs, run=run, inp=inp, cache={})
    _PROBLEM.update(key=key, value=value)
    return value


_NAN_BITS = torch.full((GUARD,), float("nan")).view(torch.int32)


def guarded(*shape):
    """A NaN-filled output tensor with GUARD NaN floats in front and behind: (whole buffer, the output's view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def assert_guards(buf, what):
    bits = buf.view(torch.int32)
    pat = _NAN_BITS.to(DEV)
    assert torch.equal(bits[:GUARD], pat) and torch.equal(bits[-GUARD:], pat), (what, "guard floats were written")
    assert not bool(buf[GUARD:-GUARD].isnan().any()), (what, "elements left unwritten (NaN)")


def assert_repeatable(launch, first, what):
    for rep in range(REPEATS - 1):
        again = launch()
        for a, b in zip(first, again):
            n = int((a != b).sum()) + int((a.isnan() != b.isnan()).sum())
            assert n == 0, (what, rep, "%d elements differ between launches" % n)


def _twin_forward(p):
    if "fwd" not in p["cache"]:
        inp = p["inp"]
        p["cache"]["fwd"] = ft.filter_forward(inp["pair_d"], inp["pair_c"], inp["ws"], inp["offset"], inp["coeff"])
    return p["cache"]["fwd"]


def _launch_forward(p):
    from geossl_amd._lib import call, ptr, stream
    inp, L, P, F, G = p["inp"], p["L"], p["P"], p["F"], p["G"]
    tb, T = guarded(L, P, F)
    wb, Wf = guarded(L, P, F)
    call("geossl_cfconv_filter_fwd", ptr(inp["pair_d"]), ptr(inp["pair_c"]), P, C.byref(inp["fw"]), L, F, G,
         ptr(inp["offset"]), inp["coeff"], ptr(T), ptr(Wf), stream())
    torch.cuda.synchronize()
    assert_guards(tb, "T")
    assert_guards(wb, "Wf")
    return T, Wf


def _step(inp, G):
    return float(inp["offset"][1] - inp["offset"][0]) if G > 1 else CUTOFF


def _layer0_variants(inp, G):
    """Layer 0 without its last Gaussian (column G - 1 of w1 zeroed), and with one Gaussian too many (g = G at centre
    offset[G - 1] + step, weighted by column G - 1): (label, weights, centres)."""
    w1, b1, w2, b2 = inp["ws"][0]
    drop = w1.clone()
    drop[:, G - 1] = 0.0
    more = torch.cat([w1, w1[:, G - 1:G]], dim=1)
    centres = torch.cat([inp["offset"].double(), inp["offset"].double()[G - 1:] + _step(inp, G)])
    return [("without Gaussian %d" % (G - 1), [drop, b1, w2, b2], inp["offset"]),
            ("with a Gaussian %d" % G, [more, b1, w2, b2], centres)]


def _teeth(got, ref, S, c, u, other, what, extra=None):
    """`other`: the fp64 value of the same tensor under a one-Gaussian change.  Put it into ONE element of the
    reference, the one where the change stands highest above its bound: the checker must flag exactly that element."""
    terms = ref - other
    bound = c * u * S + (got.double() - ref).abs()
    if extra is not None:
        bound = bound + extra
    k, ratio = pick_term(terms, bound, torch.ones_like(terms, dtype=torch.bool))
    assert ratio > 2.0, (what, "no element where the change stands above the bound", ratio)
    index = tuple(int(v) for v in np.unravel_index(k, tuple(terms.shape)))
    assert_sees_a_dropped_term(got, ref, S, c, u, index, float(terms[index]), what, extra=extra)


# ------------------------------------------------------------------------------------------------------------- forward
def check_forward(case, form, monkeypatch):
    """geossl_cfconv_filter_fwd: k_filter_fwd_h<F/32, ceil(G/16)> (two fp16 pieces, the default) and k_filter_fwd<..>
    (three bf16 pieces, GEOSSL_FILTER_FWD_BF16X3): T and Wf of every layer against the twin."""
    p = problem(*case)
    monkeypatch.delenv("GEOSSL_ARITH_24BIT", raising=False)
    if form == "bf16x3":
        monkeypatch.setenv("GEOSSL_FILTER_FWD_BF16X3", "1")
        u = U24
    else:
        monkeypatch.delenv("GEOSSL_FILTER_FWD_BF16X3", raising=False)
        u = U22
    c = C_FWD[form]
    T, Wf = _launch_forward(p)
    twin = _twin_forward(p)
    where = "%s F=%d G=%d" % case
    for l, r in enumerate(twin):
        note("fwd %s T" % form, T[l], r["T"], r["ST"], u, where)
        note("fwd %s Wf" % form, Wf[l], r["Wf"], r["SWf"], u, where)
    for l, r in enumerate(twin):
        assert_within(T[l], r["T"], r["ST"], c, u, "layer %d T" % l)
        assert_within(Wf[l], r["Wf"], r["SWf"], c, u, "layer %d Wf" % l)
    if case[0] == "main":
        inp, r = p["inp"], twin[0]
        for label, ws, centres in _layer0_variants(inp, p["G"]):
            v = ft.filter_forward(inp["pair_d"], inp["pair_c"], [ws], centres, inp["coeff"])[0]
            _teeth(T[0], r["T"], r["ST"], c, u, v["T"], "T " + label)
            _teeth(Wf[0], r["Wf"], r["SWf"], c, u, v["Wf"], "Wf " + label)
    assert_repeatable(lambda: _launch_forward(p), (T, Wf), "filter fwd %s %s" % (form, where))


# ------------------------------------------------------------------------------------------------------------ backward
def _first(run, n):
    """The first n pair slots of a problem, in the shape _filter_ref_and_bound reads."""
    inp = run.inputs
    return types.SimpleNamespace(
        inputs=dict(inp, pair_d=inp["pair_d"][:n], pair_c=inp["pair_c"][:n], pair_flag=inp["pair_flag"][:n]),
        lay=types.SimpleNamespace(pair_i=run.lay.pair_i[:n], pair_j=run.lay.pair_j[:n]))


def _launch_backward(p, saved, dyn_P=None):
    F, G, L = p["F"], p["G"], p["L"]
    bufs, outs = [], []
    for _ in range(L):
        pairs = [guarded(F, G), guarded(F), guarded(F, F), guarded(F)]
        bufs.append([b for b, _ in pairs])
        outs.append([v for _, v in pairs])
    p["run"](p["daggs"], saved_T=saved, outs=outs, dyn_P=dyn_P)
    for l in range(L):
        for b, name in zip(bufs[l], ("dw1", "db1", "dw2", "db2")):
            assert_guards(b, "layer %d %s" % (l, name))
    return [t for o in outs for t in o]


def check_backward(case, form, monkeypatch):
    """geossl_cfconv_filter_bwd: k_filter_bwd_h<F/32, T == NULL> and k_filter_bwd<F/32> (GEOSSL_FILTER_BWD_BF16X3), and
    the capacity launch with a device-side slot count below P: all four weight gradients of every layer."""
    p = problem(*case)
    monkeypatch.delenv("GEOSSL_ARITH_24BIT", raising=False)
    if form == "bf16x3":
        monkeypatch.setenv("GEOSSL_FILTER_BWD_BF16X3", "1")
        u = U24
    else:
        monkeypatch.delenv("GEOSSL_FILTER_BWD_BF16X3", raising=False)
        u = U22
    c = C_BWD
    where = "%s F=%d G=%d" % case
    dyn_P = None
    if form == "saved-dyn":
        n = p["P"] - min(37, p["P"] // 2)
        dyn_P = torch.tensor([n], dtype=torch.int32, device=DEV)
        refs = ft._filter_ref_and_bound(_first(p["run"], n), p["daggs"])
    else:
        if "bwd" not in p["cache"]:
            p["cache"]["bwd"] = ft._filter_ref_and_bound(p["run"], p["daggs"])
        refs = p["cache"]["bwd"]
    launch = lambda: _launch_backward(p, saved=form != "recompute", dyn_P=dyn_P)
    got = launch()
    names = ("dw1", "db1", "dw2", "db2")
    for l, r in enumerate(refs):
        for k, name in enumerate(names):
            note("bwd %s %s" % (form, name), got[4 * l + k], r["ref"][k], r["S"][k], u, where)
    for l, r in enumerate(refs):
        for k, name in enumerate(names):
            assert_within(got[4 * l + k], r["ref"][k], r["S"][k], c, u, "layer %d %s" % (l, name))
    if case[0] == "main" and dyn_P is None:
        # the last real Gaussian's column dw1[:, G - 1] dropped from one row
        r, G = refs[0], p["G"]
        other = r["ref"][0].clone()
        other[:, G - 1] = 0.0
        _teeth(got[0], r["ref"][0], r["S"][0], c, u, other, "dw1 without column %d in one row" % (G - 1))
    assert_repeatable(launch, got, "filter bwd %s %s" % (form, where))


def test_filter_backward_refuses_zero_gaussians():
    """G = 0 would index the Gaussians at -1: refused before anything is launched, like the forward does."""
    from geossl_amd import _lib
    p = problem("tiny31", 32, 16)
    inp, lay = p["inp"], p["lay"]
    gin, gout = _lib.FilterGradIn(), _lib.FilterGradOut()
    lib = _lib.load()
    rc = lib.geossl_cfconv_filter_bwd(None, None, None, None, None, p["P"], lay.N, C.byref(inp["fw"]), C.byref(gin), p["L"],
                                      p["F"], 0, None, inp["coeff"], None, C.byref(gout), None, 0, _lib.stream())
    assert rc != 0
    rc = lib.geossl_cfconv_filter_bwd(None, None, None, None, None, p["P"], lay.N, C.byref(inp["fw"]), C.byref(gin), p["L"],
                                      p["F"], 65, None, inp["coeff"], None, C.byref(gout), None, 0, _lib.stream())
    assert rc != 0


# --------------------------------------------------------------------------------------------------- position gradient
def _launch_dpos(p, T, Wf):
    from geossl_amd import _lib
    from geossl_amd._lib import call, ptr, stream
    inp, lay, L, P, F, G = p["inp"], p["lay"], p["L"], p["P"], p["F"], p["G"]
    gin = _lib.FilterGradIn()
    for l in range(L):
        gin.x[l], gin.dagg[l] = ptr(inp["xs"][l]), ptr(p["daggs"][l])
    db, dd = guarded(L, P)
    call("geossl_cfconv_filter_dpos", ptr(inp["pair_d"]), ptr(inp["pair_c"]), ptr(inp["pair_flag"]), ptr(lay.pair_i),
         ptr(lay.pair_j), P, C.byref(inp["fw"]), C.byref(gin), L, F, G, ptr(inp["offset"]), inp["coeff"], CUTOFF, ptr(T),
         ptr(Wf), ptr(dd), stream())
    torch.cuda.synchronize()
    assert_guards(db, "dd")
    return dd


def _launch_position_grad(p, dd):
    from geossl_amd._lib import call, ptr, stream
    inp, lay = p["inp"], p["lay"]
    gb, g = guarded(lay.N, 3)
    call("geossl_pair_position_grad", ptr(inp["pos"]), ptr(inp["pair_d"]), ptr(dd), ptr(lay.mol_ptr), ptr(lay.pair_ptr),
         lay.B, p["P"], p["L"], ptr(g), stream())
    torch.cuda.synchronize()
    assert_guards(gb, "dpos")
    return g


def check_position_gradient(case, form, monkeypatch):
    """geossl_cfconv_filter_dpos (k_filter_dpos<F/32, ceil(G/16)>, three bf16 pieces) on the default forward's own T and
    Wf: dd[l][p] against the twin, the C' O term allowed for only where pair_c == 0, slots without an edge flag exactly 0;
    then geossl_pair_position_grad on that dd."""
    p = problem(*case)
    for k in ("GEOSSL_ARITH_24BIT", "GEOSSL_FILTER_FWD_BF16X3"):
        monkeypatch.delenv(k, raising=False)
    inp, lay, L = p["inp"], p["lay"], p["L"]
    where = "%s F=%d G=%d" % case
    T, Wf = _launch_forward(p)
    dd = _launch_dpos(p, T, Wf)
    args = lambda ws, centres: (inp["pair_d"], inp["pair_c"], inp["pair_flag"], lay.pair_i, lay.pair_j, ws, centres,
                                inp["coeff"], CUTOFF, inp["xs"][:len(ws)], p["daggs"][:len(ws)])
    twin = ft.filter_dpos(*args(inp["ws"], inp["offset"]))
    c, u = C_DPOS, U24
    zero_c = inp["pair_c"] == 0
    for l, r in enumerate(twin):
        assert float((r["extra"] * (~zero_c)).abs().max()) == 0.0
        note("dpos dd", dd[l], r["dd"], r["S"], u, where, extra=r["extra"])
    for l, r in enumerate(twin):
        assert_within(dd[l], r["dd"], r["S"], c, u, "layer %d dd" % l, extra=r["extra"])
    assert float((dd * (inp["pair_flag"] == 0)[None, :]).abs().max()) == 0.0
    if case[0] == "edge":
        # the allowance is in use: on the slots the envelope rounded to zero the kernel leaves the C' O term out
        assert float(torch.stack([r["extra"] for r in twin]).max()) > 0.0
    if case[0] == "main":
        r = twin[0]
        for label, ws, centres in _layer0_variants(inp, p["G"]):
            v = ft.filter_dpos(*args([ws], centres))[0]
            _teeth(dd[0], r["dd"], r["S"], c, u, v["dd"], "dd " + label, extra=r["extra"])
    assert_repeatable(lambda: [_launch_dpos(p, T, Wf)], [dd], "filter dpos " + where)
    del twin
    # the scatter to the atoms: a sum over the layers, a division, a difference, a product and a running sum over the
    # other atoms of the molecule, each one fp32 rounding of a partial result that S bounds: c = L + 2 + max_n
    g = _launch_position_grad(p, dd)
    ref, S, _, _ = ft.pair_position_grad(inp["pos"], inp["pair_d"], dd, lay.mol_ptr, lay.pair_ptr)
    cp = float(L + 2 + lay.max_n)
    note("position grad", g, ref, S, U24, where)
    assert_within(g, ref, S, cp, U24, "dpos")
    if case[0] in ("main", "edge", "deep"):
        sizes = (lay.mol_ptr[1:] - lay.mol_ptr[:-1]).tolist()
        assert sizes[-4:] == [1, 2, 1, 6] and float(inp["pair_d"][-1]) == 0.0      # (the coincident pair is the last slot)
        for m in (lay.B - 4, lay.B - 2):                                            # single atoms: no pairs, gradient 0
            assert float(g[int(lay.mol_ptr[m])].abs().max()) == 0.0
    assert_repeatable(lambda: [_launch_position_grad(p, dd)], [g], "position grad " + where)


# One test per (case, part): the parts of a case run one after the other on the same problem (built once).
PARTS = [("forward", "two-piece", check_forward), ("forward", "bf16x3", check_forward),
         ("backward", "saved", check_backward), ("backward", "recompute", check_backward),
         ("backward", "bf16x3", check_backward), ("backward", "saved-dyn", check_backward),
         ("position-gradient", "bf16x3", check_position_gradient)]
RUNS = [(case, part) for case in CASES for part in PARTS
        if not (case[0] == "tiny1" and part[1] == "saved-dyn")]        # (a single slot leaves no count below P)


@pytest.mark.parametrize("case, part", RUNS, ids=["%s-F%d-G%d-" % c + "%s-%s" % q[:2] for c, q in RUNS])
def test_filter_kernels_vs_fp64_twin(case, part, monkeypatch):
    """Every (F, G) grid point on every batch, for the forward (both forms), the backward (saved, recompute, bf16x3 and
    a device-side slot count below P) and the position gradient with its scatter to the atoms."""
    part[2](case, part[1], monkeypatch)


# --------------------------------------------------------------------------------------------------------- model level
MODEL_CASES = [(128, 40, 5.0), (64, 17, 5.0), (32, 33, 10.0), (128, 64, 5.0)]


def _ragged_batch():
    from geossl_amd.synthetic import make_batch
    return make_batch(0, seed=17, sizes=[1, 2, 18, 33, 40, 18, 2, 1, 33])


@pytest.mark.parametrize("F, G, cutoff", MODEL_CASES)
def test_fused_schnet_at_the_new_gaussian_counts_vs_fp64_oracle(F, G, cutoff, monkeypatch):
    """SchNet(hidden = filters = F, num_gaussians = G), three blocks, on a ragged batch (1 .. 40 atoms; at 10 A the
    32-neighbour cap cuts the lists of the 40-atom molecule): output, atom features, every parameter gradient and the
    forces against oracle.nets.schnet_forward in fp64, on the fused kernels."""
    import geossl_amd.Geom3D.models.schnet as sm
    from conftest import assert_close, rel_err
    from geossl_amd import ops
    from helpers import product_schnet, schnet_oracle_params, t, unique_named_grads
    from oracle import nets
    from oracle.graph import radius_graph_np
    b = _ragged_batch()
    if cutoff == 10.0:
        capped = radius_graph_np(b["positions"], cutoff, b["batch"])
        free = radius_graph_np(b["positions"], cutoff, b["batch"], max_num_neighbors=10 ** 6)
        assert capped.shape[1] < free.shape[1]
    cfg = dict(hidden_channels=F, num_filters=F, num_interactions=3, num_gaussians=G, cutoff=cutoff, node_class=9,
               readout="add")
    names = []
    real_call = sm.call

    def spy(name, *args):
        names.append(name)
        return real_call(name, *args)

    monkeypatch.setattr(sm, "call", spy)
    monkeypatch.setattr(ops, "call", spy)   # (the position scatter is launched by the forward's ops.PairGraph)
    model = product_schnet(cfg, DEV)
    w = torch.cos(torch.arange(F, dtype=torch.float64))
    pos = t(b["positions"], DEV).requires_grad_(True)
    out, h = model(t(b["x"], DEV)[:, 0], pos, t(b["batch"], DEV), return_latent=True)
    ((h ** 2).sum() + (out * w.float().to(DEV)).sum()).backward()
    for need in ("geossl_cfconv_filter_fwd_dyn", "geossl_cfconv_filter_bwd_dyn", "geossl_cfconv_filter_dpos",
                 "geossl_pair_position_grad"):
        assert need in names, (need, sorted(set(names)))
    P64 = {k: v.detach().double().requires_grad_(v.requires_grad) for k, v in schnet_oracle_params(cfg).items()}
    p64 = t(b["positions"]).double().requires_grad_(True)
    out64, h64 = nets.schnet_forward(P64, t(b["x"])[:, 0], p64, t(b["batch"]), cutoff, 3, "add", return_latent=True)
    ((h64 ** 2).sum() + (out64 * w).sum()).backward()
    assert_close(out.detach().cpu().double(), out64.detach(), TOL_OUT, "out")
    assert_close(h.detach().cpu().double(), h64.detach(), TOL_OUT, "h")
    grads = unique_named_grads(model)
    assert len(grads) == len([k for k, v in P64.items() if v.requires_grad])
    for k, g in grads.items():
        assert rel_err(g.cpu().double(), P64[k].grad) < TOL_GRAD, k
    assert rel_err(-pos.grad.cpu().double(), -p64.grad) < TOL_GRAD


def test_trainer_graph_replay_matches_eager_at_40_gaussians():
    """One DDM trainer configuration at F = 128, G = 40 (K1S = 3): the captured step replays bit for bit what the eager
    step computes (the pattern of test_trainer_graph_replay_matches_eager)."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import draw_noise, make_batch
    from helpers import product_ncsn, product_schnet, t
    cfg = dict(hidden_channels=128, num_filters=128, num_interactions=3, num_gaussians=40, cutoff=5.0, node_class=9,
               readout="mean")
    losses = {}
    for use_graph in (False, True):
        model = product_schnet(cfg, DEV)
        n1, n2 = product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9)
        tr = pg.DDMTrainer(model, n1, n2, lr=5e-4, use_graph=use_graph)
        out = []
        for step in range(3):
            b = make_batch(32, seed=step, mode="A")
            batch = pg.Batch.from_numpy(b, DEV)
            noise = {k: t(v, DEV) for k, v in draw_noise(b, seed=100 + step).items()}
            out.append(float(tr.step(batch, noise, structure_key=("A", 32, 18))))
        assert tr.use_graph == use_graph, "capture fell back to eager"
        losses[use_graph] = out
    assert losses[True] == losses[False], losses
