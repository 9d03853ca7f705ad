"""The backward of the NCSN head (ncsn_bwd.hip, ncsn_rows.hip, the narrow-gradient and reduction kernels of ddm.hip)
element by element against the fp64 twin (tests/ncsn_twin.py, evaluated with torch's own fp64 on the GPU).

Inputs are CONDITIONED (ncsn_twin.condition): no relu unit of any row within T = 64 * 2^-22 of zero relative to the
propagated magnitude of its pre-activation, so the backward is a smooth function of the inputs and every element of dh
and of the ten parameter gradients has the a-priori bound

    |got - ref| <= c u S + A

* S: the twin's expression on absolute values (ncsn_twin.backward); u = 2^-22 for the one-pass kernel (two fp16 pieces per
  operand), 2^-24 for the two-pass route (GEOSSL_NCSN_SPLIT_BWD, GEOSSL_ARITH_24BIT).
* c = 8: r32 = max |fp32 - fp64| / (2^-24 S) of the twin's own expressions in torch.float32 on the conditioned inputs
  (tests/test_ncsn_twin_cpu.py), largest per quantity over the shapes below: dh 0.043, input_distance_mlp 0.001 / 0.001 /
  0.001 / 0.000, output_mlp.layers.0 0.006 / 0.004, layers.1 0.017 / 0.014, layers.2 0.002 / 0.003; 4 max r32 = 0.17,
  rounded up to a power of two and not below 8.  Not tuned against the kernels.
* A (ncsn_twin.absolute_term): ncsn_bwd.hip takes the fp16 pieces of dz2 and dz1 in units of the RUNNING largest |g| of
  the block's tiles times a weight-only constant; a value 2^17 below that bound carries an absolute error of 2^-39 of it.
  A row's dz2 / dz1 elements get 2^-36 max|g| (max|w3|, resp. the largest column sum of |w3 o2_w|), the maximum over the
  rows from the first one to the end of the row's 32-row tile (never over the launch), dz1 also dz2's share through
  |o2_w|; propagated to dfeat, dh and the weight gradients like S.  At anneal_power 2 it is below 1/64 of c u S for every
  element (asserted); at 0.05 and 10 it is what bounds the atoms of low-noise molecules.

Conditioning (rows, below T at first, removed after four redraws), seed 99:
  ragged40 F = 32: 4357, 22, 0;  F = 64: 3124, 117, 4;  F = 128: 5811, 721, 78;  ragged300 F = 128: 32968, 4203, 481;
  ragged700 F = 128: 81051, 10339, 1372;  one molecule of 9 atoms: 36, 1-2, 0;  of 2 atoms: 1, 0, 0;
  bench (1024 molecules of set A, F = 128): head A 156672, 19882, 2245; head B on A's rows 154427, 18132, 2822
  (each call of `condition` is held to the 3 % cap; the two heads of a step share one super-edge list);
  pairs on ragged40: F = 32 (4357, 19, 0), F = 64 (3120, 98, 5), F = 128 (5733, 651, 51) for head B.

Durations on an MI355X (pytest --durations, conditioning and the fp64 twin on the GPU included): the bench batch 0.27-0.29 s,
the dropped-term cases up to 0.13 s, 700 molecules 0.09 s, every other case at most 0.04 s (the first case of a process
also loads the library: 1.5 s)."""
import ctypes as C
import types

import pytest
import torch

import ncsn_twin as tw
from elementwise import assert_repeatable, assert_sees_a_dropped_term, assert_within, flagged, pick_term

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U22, U24 = 2.0 ** -22, 2.0 ** -24
QUANTITIES = ("dh",) + tw.KEYS
FIELDS = ("in_w1", "in_b1", "in_w2", "in_b2", "o1_w", "o1_b", "o2_w", "o2_b", "o3_w", "o3_b")
SWITCHES = ("GEOSSL_NCSN_SPLIT_BWD", "GEOSSL_ARITH_24BIT", "GEOSSL_NCSN_SEPARATE_HEADS")


@pytest.fixture(autouse=True)
def _default_route(monkeypatch):
    from geossl_amd import _lib
    _lib.load()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def problem(name, rows=None):
    """The conditioned problem on the GPU (cap asserted in ncsn_twin.conditioned); `rows`: only its first rows."""
    q, S0, below, removed = tw.conditioned(name, DEV)
    assert removed <= tw.MAX_REMOVED * S0
    if rows is not None:
        q = tw.take_rows(q, torch.arange(rows, device=DEV))
    assert float(tw.row_margin(q).min()) >= tw.T_MARGIN
    return q


_REF = {}


def reference(p, power, out_scale=1.0, upstream=1.0, key=None):
    """fp64 gradients, S and A of a problem; kept per `key` for the tests that share one."""
    k = None if key is None else (key, power, out_scale, upstream)
    if k is not None and k in _REF:
        return _REF[k]
    bw = tw.backward(p, power, out_scale, upstream)
    A = tw.absolute_term(p, bw)
    out = dict(g=bw["g"], S=bw["S"], A=A, x0=bw["x0"])
    if k is not None:
        _REF[k] = out
    return out


def check(got, ref, u, what, factor=1.0, rows=("dfeat", "demb")):
    """|got - factor ref| <= c u (factor S) + factor A for dh, the ten gradients and the row outputs `got` holds."""
    for k in QUANTITIES + tuple(rows):
        if k not in got:
            continue
        g, S, A = (ref[n][k].view_as(got[k]) * factor for n in ("g", "S", "A"))
        assert_within(got[k], g, S, tw.C_BOUND, u, "%s %s" % (what, k), extra=A)


def assert_A_negligible(ref):
    for k in QUANTITIES:
        S, A = ref["S"][k], ref["A"][k]
        assert bool((A <= tw.C_BOUND * U22 * S / 64).all()), k


def layout_of(p):
    from geossl_amd.layout import get_super_edge_layout
    sei = torch.stack([p["sei0"], p["sei1"]])
    return get_super_edge_layout(p["batch"], sei, p["nl"].numel())


def weights_of(p):
    from geossl_amd import _lib
    w = _lib.NcsnWeights()
    for name, k in zip(FIELDS, tw.KEYS):
        setattr(w, name, p["P"][k].data_ptr())
    w.sigmas = p["P"]["sigmas"].data_ptr()
    return w


def saved_buffers(S, F):
    return dict(a1=nan(S, F), a2=nan(S, F // 2), pd=nan(S), emb=nan(S), gscale=nan(S))


def abi_single(p, power, out_scale=1.0, upstream=1.0):
    """geossl_ddm_loss_fwd (saving), geossl_ddm_loss_bwd_fused, geossl_incidence_gather on NaN-prefilled outputs."""
    from geossl_amd import _lib
    from geossl_amd._lib import call, ptr, stream
    sel, w = layout_of(p), weights_of(p)
    S, (N, F) = p["S"], p["h"].shape
    lib = _lib.load()
    sv_t = saved_buffers(S, F)
    sv = _lib.NcsnSaved(*[ptr(sv_t[k]) for k in ("a1", "a2", "pd", "emb", "gscale")])
    loss_e = nan(S)
    ws = torch.empty(max(int(lib.geossl_ddm_loss_fwd_workspace_floats(F)), 256), device=DEV)
    st = stream()
    call("geossl_ddm_loss_fwd", ptr(p["h"]), ptr(sel.batch), ptr(sel.sei0), ptr(sel.sei1), S, ptr(p["dist"]), ptr(p["nl"]),
         ptr(p["dn"]), C.byref(w), F, float(power), ptr(loss_e), C.byref(sv), ptr(ws), st)
    grads = [torch.full_like(p["P"][k], float("nan")) for k in tw.KEYS]
    g = _lib.NcsnGrads(*[ptr(t) for t in grads])
    dfeat, demb, grow, dh = nan(S, F), nan(S), nan(S), nan(N, F)
    gout = torch.tensor([upstream], dtype=torch.float32, device=DEV)
    ws1 = torch.empty(int(lib.geossl_ddm_loss_bwd_fused_workspace_floats(S, F)), device=DEV)
    call("geossl_ddm_loss_bwd_fused", ptr(p["h"]), ptr(sel.sei0), ptr(sel.sei1), S, N, F, C.byref(w), C.byref(sv),
         ptr(sel.stats), float(out_scale), ptr(gout), ptr(dfeat), ptr(demb), ptr(grow), C.byref(g), ptr(ws1), 0, st)
    call("geossl_incidence_gather", ptr(dfeat), ptr(sel.inc_ptr), ptr(sel.inc_idx), N, F, ptr(dh), 0, st)
    torch.cuda.synchronize()
    out = dict(zip(tw.KEYS, grads))
    out.update(dh=dh, dfeat=dfeat, demb=demb.view(-1, 1), loss_e=loss_e)
    return out


def abi_pair(pa, pb, power, out_scale=0.5, upstream=1.0, capacity=None):
    """geossl_ddm_loss_fwd2_dyn and geossl_ddm_loss_bwd_fused2 on NaN-prefilled outputs.  `capacity` = (atoms, super-edges)
    above the real counts: the _dyn form - ONE feature tensor [head A's atoms ; head B's atoms ; NaN rows], every
    per-row input padded with NaN (indices with 0) up to the capacity, the real counts read from the device."""
    from geossl_amd import _lib
    from geossl_amd._lib import call, ptr, stream
    sel = layout_of(pa)
    S, (N, F) = pa["S"], pa["h"].shape
    lib = _lib.load()
    keep = []
    if capacity is None:
        Nc, Sc, dyn_S, dyn_N = N, S, None, None
        hs = (pa["h"], pb["h"])
        sei0, sei1, batch = sel.sei0, sel.sei1, sel.batch
        dhs = (nan(N, F), nan(N, F))
        pad = lambda t: t
    else:
        Nc, Sc = capacity
        assert Nc > N and Sc > S
        dims = torch.tensor([N, S], dtype=torch.int32, device=DEV)
        dyn_N, dyn_S = dims.data_ptr(), dims.data_ptr() + 4
        h_all = torch.cat([pa["h"], pb["h"], nan(2 * Nc - 2 * N, F)])
        hs = (h_all, h_all)
        zeros = torch.zeros(Sc - S, dtype=torch.int64, device=DEV)
        sei0, sei1 = torch.cat([sel.sei0, zeros]), torch.cat([sel.sei1, zeros])
        batch = torch.cat([sel.batch, torch.zeros(Nc - N, dtype=torch.int64, device=DEV)])
        dh_all = nan(2 * Nc, F)
        dhs = (dh_all, dh_all)
        pad = lambda t: torch.cat([t.reshape(-1), nan(Sc - S)])
        keep += [dims, h_all]
    fwd, bwd = (_lib.NcsnHeadFwd * 2)(), (_lib.NcsnHeadBwd * 2)()
    nws = int(lib.geossl_ddm_loss_bwd_fused_workspace_floats(Sc, F))
    outs = []
    for k, p in enumerate((pa, pb)):
        w = weights_of(p)
        sv_t = saved_buffers(Sc, F)
        d, dn = pad(p["dist"]), pad(p["dn"])
        loss_e, wsf = nan(Sc), torch.empty(256, device=DEV)
        f = fwd[k]
        f.h, f.distance, f.noise_level, f.distance_noise, f.w = ptr(hs[k]), ptr(d), ptr(p["nl"]), ptr(dn), w
        f.anneal_power, f.loss_e, f.workspace = float(power), ptr(loss_e), ptr(wsf)
        grads = [torch.full_like(p["P"][n], float("nan")) for n in tw.KEYS]
        dfeat, demb, grow, ws1 = nan(Sc, F), nan(Sc), nan(Sc), torch.empty(nws, device=DEV)
        b = bwd[k]
        b.h, b.w, b.out_scale = ptr(hs[k]), w, float(out_scale)
        for name in ("a1", "a2", "pd", "emb", "gscale"):
            setattr(f.saved, name, ptr(sv_t[name]))
            setattr(b.saved, name, ptr(sv_t[name]))
        for name, t_ in zip(FIELDS, grads):
            setattr(b.grads, name, ptr(t_))
        b.dfeat, b.demb, b.grow, b.workspace, b.dh = ptr(dfeat), ptr(demb), ptr(grow), ptr(ws1), ptr(dhs[k])
        keep += [sv_t, d, dn, loss_e, wsf, ws1, grow]
        outs.append(dict(zip(tw.KEYS, grads), dfeat=dfeat, demb=demb.view(-1, 1)))
    st = stream()
    gout = torch.tensor([upstream], dtype=torch.float32, device=DEV)
    call("geossl_ddm_loss_fwd2_dyn", C.byref(fwd), ptr(batch), ptr(sei0), ptr(sei1), Sc, F, dyn_S, dyn_N, st)
    if capacity is None:
        call("geossl_ddm_loss_bwd_fused2", C.byref(bwd), ptr(sei0), ptr(sei1), Sc, Nc, F, ptr(sel.stats), ptr(gout),
             ptr(sel.inc_ptr), ptr(sel.inc_idx), 0, st)
    else:
        call("geossl_ddm_loss_bwd_fused2_dyn", C.byref(bwd), ptr(sei0), ptr(sei1), Sc, Nc, F, ptr(sel.stats), ptr(gout),
             ptr(sel.inc_ptr), ptr(sel.inc_idx), 0, dyn_S, dyn_N, st)
    torch.cuda.synchronize()
    del keep
    if capacity is None:
        outs[0]["dh"], outs[1]["dh"] = dhs
    else:
        # nothing past the real counts is written
        assert bool(dh_all[2 * N:].isnan().all())
        for o in outs:
            assert bool(o["dfeat"][S:].isnan().all()) and bool(o["demb"][S:].isnan().all())
            o["dfeat"], o["demb"] = o["dfeat"][:S], o["demb"][:S]
        outs[0]["dh"], outs[1]["dh"] = dh_all[:N], dh_all[N:2 * N]
    return outs


def module_of(p, power):
    from geossl_amd.NCSN import NCSN_version_03
    F, K = p["h"].size(1), p["P"]["sigmas"].numel()
    m = NCSN_version_03(F, 10.0, 0.01, K, "symmetry", power)
    m.load_state_dict({k: v.cpu() for k, v in p["P"].items()})
    return m.to(DEV)


def data_of(p):
    return types.SimpleNamespace(batch=p["batch"], super_edge_index=torch.stack([p["sei0"], p["sei1"]]),
                                 num_graphs=int(p["nl"].numel()))


def module_single(p, power, upstream=1.0, out_scale=1.0, head=None, data=None):
    """NCSN_version_03.forward and loss.backward() of the public module (the route the environment selects)."""
    from helpers import unique_named_grads
    head = module_of(p, power) if head is None else head
    hh = p["h"].clone().requires_grad_()
    loss = head(data_of(p) if data is None else data, hh, p["dist"], noise_level=p["nl"], distance_noise=p["dn"],
                out_scale=out_scale)
    (loss * upstream).backward()
    torch.cuda.synchronize()
    out = {k: v for k, v in unique_named_grads(head).items()}
    out["dh"] = hh.grad
    return out


# ------------------------------------------------------------------------------------------- the one-pass single head
SINGLE = [("ragged40-F32", None), ("ragged40-F64", None), ("ragged40-F128", None), ("ragged700-F128", None)] + \
         [("one2-F%d" % F, None) for F in (32, 64, 128)] + \
         [("one9-F%d" % F, rows) for F in (32, 64, 128) for rows in (31, 32, 33)]


@pytest.mark.parametrize("name,rows", SINGLE, ids=["%s%s" % (n, "" if r is None else "-S%d" % r) for n, r in SINGLE])
def test_one_pass_backward_single_head_vs_fp64(name, rows):
    """geossl_ddm_loss_bwd_fused + geossl_incidence_gather (k_ncsn_bwd_fused<F/32>, k_ncsn_reduce_all): dfeat, demb, dh
    and the ten gradients within c u S + A (u = 2^-22) of fp64.  Ragged 2-26 atoms with S no multiple of the 32-row
    tile and a trailing one-atom molecule (its dh row exact zeros); 700 molecules: several tiles per block, the running
    exponents rising; one molecule (B = 1) with S = 1, 31, 32, 33."""
    p = problem(name, rows)
    if rows is not None:
        assert p["S"] == rows and p["nl"].numel() == 1
    elif name.startswith("ragged"):
        assert p["S"] % 32 != 0
    if name == "ragged700-F128":
        assert (p["S"] + 31) // 32 >= 4 * 256     # every block walks several tiles
    power = 2.0
    got = abi_single(p, power)
    ref = reference(p, power, key=name if rows is None else None)
    assert_A_negligible(ref)
    check(got, ref, U22, name)
    if name.startswith("ragged40"):
        assert int(p["batch"][-1]) == p["nl"].numel() - 1 and int((p["batch"] == p["batch"][-1]).sum()) == 1
        assert bool((got["dh"][-1] == 0).all())


@pytest.mark.parametrize("upstream", [1.0, 1e-9, 1e6])
@pytest.mark.parametrize("power", [0.05, 2.0, 10.0])
def test_one_pass_backward_follows_the_row_gradient_element_by_element(power, upstream):
    """300 ragged molecules at F = 128, anneal_power 0.05 / 2 / 10 (the row gradient spans 1, 3 and 30 orders of magnitude
    between molecules) times an upstream scalar: every element of dfeat, dh and the gradients within c u S + A - the
    atoms of low-noise molecules at their own scale wherever the kernel's contract (A) promises it."""
    name = "ragged300-F128"
    p = problem(name)
    got = abi_single(p, power, out_scale=0.5, upstream=upstream)
    ref = reference(p, power, 0.5, upstream)
    if power == 2.0:
        assert_A_negligible(ref)
    check(got, ref, U22, "%s power %g upstream %g" % (name, power, upstream))


# ------------------------------------------------------------------------------------------------- the pair launch
@pytest.mark.parametrize("dyn", [False, True], ids=["exact", "capacity"])
@pytest.mark.parametrize("F", [32, 64, 128])
def test_pair_launch_vs_fp64(F, dyn):
    """geossl_ddm_loss_bwd_fused2 (k_ncsn_bwd_fused2: both heads of a step in one launch, half the blocks per head) and
    its _dyn form with capacities above the real counts (inputs past the counts NaN: not read; outputs past them stay
    NaN: not written): both heads within c u S + A."""
    name = "ragged40-F%d" % F
    pa, pb, counts = tw.conditioned_pair(name, DEV)
    for rows, _, removed in counts:
        assert removed <= tw.MAX_REMOVED * rows
    assert pa["S"] % 32 != 0
    N, S = pa["h"].size(0), pa["S"]
    outs = abi_pair(pa, pb, 2.0, capacity=(N + 37, S + 300) if dyn else None)
    for tag, p, got in (("A", pa, outs[0]), ("B", pb, outs[1])):
        ref = reference(p, 2.0, 0.5, key=("pair", name, tag))
        assert_A_negligible(ref)
        check(got, ref, U22, "%s head %s" % (name, tag))
        assert bool((got["dh"][-1] == 0).all())


def _bench_launcher():
    from geossl_amd.NCSN import ddm_heads_loss
    from helpers import unique_named_grads
    pa, pb, counts = tw.conditioned_pair("bench", DEV)
    for rows, _, removed in counts:
        assert removed <= tw.MAX_REMOVED * rows
    n1, n2 = module_of(pa, 2.0), module_of(pb, 2.0)
    data = data_of(pa)

    def launch():
        for m in (n1, n2):
            m.zero_grad(set_to_none=True)
        h1, h2 = pa["h"].clone().requires_grad_(), pb["h"].clone().requires_grad_()
        loss = ddm_heads_loss(n1, n2, data, h1, pa["dist"], h2, pb["dist"], noise_level_1=pa["nl"],
                              distance_noise_1=pa["dn"], noise_level_2=pb["nl"], distance_noise_2=pb["dn"])
        loss.backward()
        torch.cuda.synchronize()
        g1, g2 = unique_named_grads(n1), unique_named_grads(n2)
        return [h1.grad, h2.grad] + [g1[k] for k in tw.KEYS] + [g2[k] for k in tw.KEYS]
    return pa, pb, launch


def test_bench_batch_pair_vs_fp64_and_repeatable():
    """The headline launch at its real occupancy through NCSN.ddm_heads_loss: 1024 molecules of set A, two heads with
    weights at scale 1.0 / 0.9, K = 50, anneal_power 2 - dh of both views and the twenty gradients within c u S + A;
    eight launches element-wise identical."""
    pa, pb, launch = _bench_launcher()
    assert pa["nl"].numel() == 1024 and pa["h"].size(1) == 128 and pa["P"]["sigmas"].numel() == 50
    first = launch()
    n = len(tw.KEYS)
    for tag, p, dh, grads in (("A", pa, first[0], first[2:2 + n]), ("B", pb, first[1], first[2 + n:])):
        ref = reference(p, 2.0, 0.5)
        assert_A_negligible(ref)
        check(dict(zip(tw.KEYS, grads), dh=dh), ref, U22, "bench head %s" % tag)
        del ref
    assert_repeatable(launch, first, "bench pair")


# -------------------------------------------------------------------------------------------------- the two-pass route
@pytest.mark.parametrize("switch", ["GEOSSL_NCSN_SPLIT_BWD", "GEOSSL_ARITH_24BIT"])
@pytest.mark.parametrize("F", [32, 64, 128])
def test_two_pass_route_vs_fp64(F, switch, monkeypatch):
    """geossl_ddm_loss_bwd_rows + geossl_ddm_loss_bwd_weights (ncsn_rows.hip, wgrad.h) behind the public module under
    GEOSSL_NCSN_SPLIT_BWD and under GEOSSL_ARITH_24BIT: within c u S + A with u = 2^-24."""
    name = "ragged40-F%d" % F
    p = problem(name)
    monkeypatch.setenv(switch, "1")
    got = module_single(p, 2.0)
    check(got, reference(p, 2.0, key=name), U24, "%s %s" % (name, switch))
    assert bool((got["dh"][-1] == 0).all())


# ------------------------------------------------------------------------------------------------------ accumulate = 1
@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
def test_direct_gradients_accumulate(pair):
    """Inside _lib.direct_grads() the reductions add into p.grad (accumulate = 1): two backwards give twice the
    gradients, within the same bound on the doubled quantities."""
    from geossl_amd import _lib
    from geossl_amd.NCSN import ddm_heads_loss
    name = "ragged40-F128"
    if pair:
        pa, pb, _ = tw.conditioned_pair(name, DEV)
        ps = (pa, pb)
    else:
        ps = (problem(name),)
    heads = [module_of(p, 2.0) for p in ps]
    for m in heads:
        for q in m.parameters():
            if q.requires_grad:
                q.grad = torch.zeros_like(q)
    data = data_of(ps[0])
    with _lib.direct_grads():
        for _ in range(2):
            hs = [p["h"].clone().requires_grad_() for p in ps]
            if pair:
                loss = ddm_heads_loss(heads[0], heads[1], data, hs[0], pa["dist"], hs[1], pb["dist"], noise_level_1=pa["nl"],
                                      distance_noise_1=pa["dn"], noise_level_2=pb["nl"], distance_noise_2=pb["dn"])
            else:
                loss = heads[0](data, hs[0], ps[0]["dist"], noise_level=ps[0]["nl"], distance_noise=ps[0]["dn"], out_scale=0.5)
            loss.backward()
    torch.cuda.synchronize()
    for tag, p, m, hh in zip("AB", ps, heads, hs):
        ref = reference(p, 2.0, 0.5, key=("pair", name, tag) if pair else None)
        got = {k: dict(m.named_parameters())[k].grad for k in tw.KEYS}
        check(got, ref, U22, "twice %s" % tag, factor=2.0)
        check(dict(dh=hh.grad), ref, U22, "dh %s" % tag)


# --------------------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("F", [32, 64, 128])
def test_checker_sees_a_dropped_term(F):
    """At anneal_power 2: one super-edge's dfeat contribution removed from the fp64 dh of one atom (a row in lanes 48-63
    of a 64-row group) - elements of exactly that atom's row are flagged, every one whose term stands above twice its
    bound among them; one row's term removed from one element of output_mlp.layers.0.weight's gradient (one molecule of 9
    atoms) - exactly that element is flagged.  No single term above twice its bound: the test fails."""
    name = "ragged40-F%d" % F
    p = problem(name)
    got = abi_single(p, 2.0)
    ref = reference(p, 2.0, key=name)
    c, u = tw.C_BOUND, U22
    check(got, ref, u, name)
    S_rows = p["S"]
    lanes = (torch.arange(S_rows, device=DEV) % 64) >= 48
    # dh[atom] = sum over incident super-edges of dfeat[row]
    dh, dh_ref, dh_S, dh_A = got["dh"], ref["g"]["dh"], ref["S"]["dh"], ref["A"]["dh"]
    terms = ref["g"]["dfeat"]
    atoms = p["sei0"]
    bound = (c * u * dh_S + dh_A + (dh.double() - dh_ref).abs())[atoms]
    k, ratio = pick_term(terms, bound, lanes[:, None].expand_as(terms))
    assert ratio > 2.0, ("no single super-edge stands above the bound", ratio)
    row, f = divmod(k, F)
    atom = int(atoms[row])
    assert_sees_a_dropped_term(dh, dh_ref, dh_S, c, u, (atom, f), float(terms[row, f]), "dh without row %d" % row, extra=dh_A)
    ref2 = dh_ref.clone()
    ref2[atom] -= terms[row]
    bad = flagged(dh, ref2, dh_S, c, u, dh_A)
    must = terms[row].abs() > 2.0 * bound[row]
    assert bool(bad[atom].any()) and int(bad.sum()) == int(bad[atom].sum()) and bool(bad[atom][must].all())
    # d o1_w[m, f] = sum over rows of dz1[row, m] x0[row, f]: on one molecule of 9 atoms (36 rows, two tiles) - among the
    # thousands of rows of the batch above no single row's term stands above the bound of a sum over all of them at
    # F = 128 (largest ratio 1.3)
    name = "one9-F%d" % F
    p = problem(name)
    got = abi_single(p, 2.0)
    ref = reference(p, 2.0, key=name)
    check(got, ref, u, name)
    key = tw.O0 + ".weight"
    gw, gw_ref, gw_S, gw_A = got[key], ref["g"][key], ref["S"][key], ref["A"][key]
    terms = ref["g"]["dz1"][:, :, None] * ref["x0"][:, None, :]                              # [row, m, f]
    bound = (c * u * gw_S + gw_A + (gw.double() - gw_ref).abs())[None].expand_as(terms)
    k, ratio = pick_term(terms, bound, torch.ones_like(terms, dtype=torch.bool))
    assert ratio > 2.0, ("no single row stands above the bound", ratio)
    kr, rest = divmod(k, terms.size(1) * terms.size(2))
    km, kf = divmod(rest, terms.size(2))
    assert_sees_a_dropped_term(gw, gw_ref, gw_S, c, u, (km, kf), float(terms[kr, km, kf]),
                               "%s without row %d" % (key, kr), extra=gw_A)
