"""GPU tests of the atom-tile PaiNN interaction kernels (csrc/painn_tile.hip): every output element of the forward and the
backward against the fp64 twin with an a-priori bound (tests/painn_tile_twin.py) on one hand-made edge list of 96 atoms
whose degrees straddle the 32-row tile, the proof that the checker sees one dropped term, the list / dyn_nlist / empty /
accumulate forms, repeatability, the shapes that are refused, and the routing of the backbone end to end on structures
above 255 atoms (do_Supervised, do_LEP against the fp64 oracle, the calls counted)."""
import types

import numpy as np
import pytest
import torch

import force_twin as ft
import lba_structures as ls
import lep_twin as lt
import painn_tile_twin as tw
from elementwise import assert_repeatable, assert_sees_a_dropped_term, assert_within, pick_term
from helpers import fill_module_, t, unique_named_grads
from oracle import nets
from oracle.graph import radius_graph_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
N_ATOMS, F = 96, 128
HEAD_DEGREES = (0, 1, 2, 31, 32, 33, 63, 64, 65, 70)
INVALID = 1   # hipErrorInvalidValue


def _edges():
    """[2, E] int64: atom a is the target (row 0) of degree(a) edges, sources drawn with duplicates, edges shuffled."""
    rng = np.random.default_rng(96)
    deg = list(HEAD_DEGREES) + [(5 * a) % 7 for a in range(len(HEAD_DEGREES), N_ATOMS)]
    tgt = np.repeat(np.arange(N_ATOMS), deg)
    src = rng.integers(0, N_ATOMS, size=tgt.size)
    order = rng.permutation(tgt.size)
    assert max(deg) == tw.MAX_DEGREE
    return np.stack([tgt[order], src[order]]).astype(np.int64), deg


_CASES = {}


def _case(R, mu_given, transposed):
    """Inputs on the device (fp32), the edge layout, and the twin's references: built once, left unchanged."""
    key = (R, mu_given, transposed)
    if key in _CASES:
        return _CASES[key]
    from geossl_amd.layout import get_edge_layout
    ei, deg = _edges()
    if transposed:   # the backward walks the edges by SOURCE: the same degrees on that side
        ei = ei[::-1].copy()
    E = ei.shape[1]
    g = torch.Generator().manual_seed(1000 + R + 7 * mu_given)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DEV)
    dirv = torch.randn(E, 3, generator=g)
    dirv = (dirv / dirv.norm(dim=1, keepdim=True)).to(DEV)
    c = dict(R=R, E=E, deg=deg, ei=t(ei, DEV), q=rnd(N_ATOMS, F), mu=rnd(N_ATOMS, 3, F) if mu_given else None,
             xc=rnd(N_ATOMS, 3 * F), phi=torch.rand(E, R, generator=g).to(DEV), fcut=torch.rand(E, generator=g).to(DEV),
             dirv=dirv, Wf=rnd(3 * F, R, scale=0.3), bf=rnd(3 * F, scale=0.2), dq=rnd(N_ATOMS, F), dmu=rnd(N_ATOMS, 3, F))
    batch = torch.zeros(N_ATOMS, dtype=torch.long, device=DEV)
    c["el"] = get_edge_layout(batch, c["ei"], 1)
    side = "j" if transposed else "i"
    iptr = c["el"].inc[side][0].cpu().numpy()
    assert np.array_equal(np.diff(iptr), np.asarray(deg))          # get_edge_layout's incidence lists have these degrees
    _CASES[key] = c
    return c


def _ptr(x):
    return None if x is None else x.data_ptr()


def _fwd(c, atom_list=None, nlist=N_ATOMS, dyn=None):
    from geossl_amd import _lib
    el = c["el"]
    inc_ptr, inc_idx = el.inc["i"]
    q_out, mu_out = torch.full((N_ATOMS, F), NAN, device=DEV), torch.full((N_ATOMS, 3, F), NAN, device=DEV)
    rc = _lib.load().geossl_painn_interaction_fwd_tile(_ptr(c["q"]), _ptr(c["mu"]), _ptr(c["xc"]), _ptr(el.idx_j), _ptr(inc_ptr), _ptr(inc_idx), _ptr(c["phi"]),
            _ptr(c["fcut"]), _ptr(c["dirv"]), _ptr(c["Wf"]), _ptr(c["bf"]), _ptr(atom_list), nlist, _ptr(dyn), F, c["R"],
            _ptr(q_out), _ptr(mu_out), _lib.stream())
    assert rc == 0
    return q_out, mu_out, rc


def _bwd(c, scale=1.0, atom_list=None, nlist=N_ATOMS, dyn=None, accumulate=0, prefill=None):
    from geossl_amd import _lib
    el, R = c["el"], c["R"]
    inc_ptr, inc_idx = el.inc["j"]
    dq, dmu = c["dq"] * scale, c["dmu"] * scale
    dxc = torch.full((N_ATOMS, 3 * F), NAN, device=DEV)
    dmu_in = None if c["mu"] is None else torch.full((N_ATOMS, 3, F), NAN, device=DEV)
    dWf = torch.full((3 * F, R), NAN if prefill is None else prefill, device=DEV)
    dbf = torch.full((3 * F,), NAN if prefill is None else prefill, device=DEV)
    ws = torch.full((int(_lib.load().geossl_painn_interaction_bwd_tile_workspace_floats(nlist, F, R)) + 1,), NAN, device=DEV)
    _lib.call("geossl_painn_interaction_bwd_tile", _ptr(dq), _ptr(dmu), _ptr(c["mu"]), _ptr(c["xc"]), _ptr(el.idx_i),
              _ptr(inc_ptr), _ptr(inc_idx), _ptr(c["phi"]), _ptr(c["fcut"]), _ptr(c["dirv"]), _ptr(c["Wf"]), _ptr(c["bf"]),
              _ptr(atom_list), nlist, _ptr(dyn), F, R, _ptr(dxc), _ptr(dmu_in), _ptr(dWf), _ptr(dbf), _ptr(ws), accumulate,
              _lib.stream())
    return dxc, dmu_in, dWf, dbf


_TWINS = {}


def _twin_fwd(c, key):
    if ("f",) + key not in _TWINS:
        _TWINS[("f",) + key] = tw.forward(c["q"], c["mu"], c["xc"], c["el"].idx_i, c["el"].idx_j, c["phi"], c["fcut"],
                                          c["dirv"], c["Wf"], c["bf"])
    return _TWINS[("f",) + key]


def _twin_bwd(c, key, scale, atoms=None):
    k = ("b",) + key + (scale, None if atoms is None else tuple(int(a) for a in atoms))
    if k not in _TWINS:
        _TWINS[k] = tw.backward(c["dq"] * scale, c["dmu"] * scale, c["mu"], c["xc"], c["el"].idx_i, c["el"].idx_j, c["phi"],
                                c["fcut"], c["dirv"], c["Wf"], c["bf"], atoms=atoms)
    return _TWINS[k]


def _dropped(got, ref, S, c_, terms, owner_index, what):
    """One term removed from the reference: the checker flags exactly its element.  terms [E, ...]: term e belongs to the
    element (owner_index[e], ...), or - owner_index None, a weight gradient - to the element with its trailing index."""
    got = got.cpu()
    bound = c_ * tw.U * S + (got.double() - ref).abs()
    bound = bound[None].expand_as(terms) if owner_index is None else bound[owner_index]
    k, ratio = pick_term(terms, bound, torch.ones_like(terms, dtype=torch.bool))
    assert ratio >= 2.0, (what, "no term stands above twice its bound", ratio)
    idx = tuple(int(v) for v in np.unravel_index(k, tuple(terms.shape)))
    index = idx[1:] if owner_index is None else (int(owner_index[idx[0]]),) + idx[1:]
    assert_sees_a_dropped_term(got, ref, S, c_, tw.U, index, float(terms[idx]), what)


PARAMS = [(20, True), (20, False), (8, True), (8, False)]
IDS = ["R20-mu", "R20-mu0", "R8-mu", "R8-mu0"]
PARAMS16 = PARAMS + [(16, True), (16, False)]          # (R = 16 is compiled and served: the element-wise tests run it too)
IDS16 = IDS + ["R16-mu", "R16-mu0"]


@pytest.mark.parametrize("R,mu_given", PARAMS16, ids=IDS16)
def test_forward_every_element_against_the_twin(R, mu_given):
    from geossl_amd import _lib
    c = _case(R, mu_given, False)
    ref = _twin_fwd(c, (R, mu_given, False))
    q_out, mu_out, _ = _fwd(c)
    i = c["el"].idx_i.cpu()
    for name, got, terms in (("q_out", q_out, ref["terms_q"]), ("mu_out", mu_out, ref["terms_mu"])):
        r, S = ref[name]
        live = S > 0
        err = ((got.cpu().double() - r).abs()[live] / (tw.U * S[live])).max()
        print("forward R=%d mu=%s %s: worst error %.2f u S (bound %.2f)" % (R, mu_given, name, float(err), tw.C_FWD))
        assert_within(got.cpu(), r, S, tw.C_FWD, tw.U, name)
        _dropped(got, r, S, tw.C_FWD, terms, i, name)
    # the per-atom vector kernel on the same inputs: 2e-6 of the tensor scale (the bound of the matrix-pipe forward)
    mu_t = c["mu"] if mu_given else torch.zeros(N_ATOMS, 3, F, device=DEV)
    inc_ptr, inc_idx = c["el"].inc["i"]
    q_v, mu_v = torch.empty_like(q_out), torch.empty_like(mu_out)
    _lib.call("geossl_painn_interaction_fwd", _ptr(c["q"]), _ptr(mu_t), _ptr(c["xc"]), _ptr(c["el"].idx_j), _ptr(inc_ptr),
              _ptr(inc_idx), _ptr(c["phi"]), _ptr(c["fcut"]), _ptr(c["dirv"]), _ptr(c["Wf"]), _ptr(c["bf"]), N_ATOMS, F, R,
              _ptr(q_v), _ptr(mu_v), _lib.stream())
    for got, want in ((q_out, q_v), (mu_out, mu_v)):
        assert float((got - want).abs().max()) <= 2e-6 * float(want.abs().max())
    assert_repeatable(lambda: _fwd(c)[:2], (q_out, mu_out), "forward")


@pytest.mark.parametrize("R,mu_given", PARAMS16, ids=IDS16)
def test_backward_every_element_against_the_twin(R, mu_given):
    c = _case(R, mu_given, True)
    j = c["el"].idx_j.cpu()
    for scale in (1.0, 2.0 ** -20):
        ref = _twin_bwd(c, (R, mu_given, True), scale)
        dxc, dmu_in, dWf, dbf = _bwd(c, scale)
        assert (dmu_in is None) == (not mu_given)
        checks = [("dxc", dxc, tw.C_BWD, ref["terms_dxc"], j), ("dWf", dWf, tw.C_WGRAD, ref["terms_dWf"], None),
                  ("dbf", dbf, tw.C_WGRAD, ref["terms_dbf"], None)]
        if mu_given:
            checks.append(("dmu_in", dmu_in, tw.C_BWD, ref["terms_dmu"], j))
        for name, got, c_, terms, owner in checks:
            r, S = ref[name]
            live = S > 0
            err = ((got.cpu().double() - r).abs()[live] / (tw.U * S[live])).max()
            print("backward R=%d mu=%s scale %g %s: worst error %.2f u S (bound %.2f)" % (R, mu_given, scale, name,
                                                                                          float(err), c_))
            assert_within(got.cpu(), r, S, c_, tw.U, "%s at scale %g" % (name, scale))
            _dropped(got, r, S, c_, terms, owner, name)
    first = _bwd(c, 1.0)
    flat = lambda o: [x for x in o if x is not None]
    assert_repeatable(lambda: flat(_bwd(c, 1.0)), flat(first), "backward")


@pytest.mark.parametrize("R,mu_given", PARAMS16, ids=IDS16)
def test_list_forms(R, mu_given):
    cf, cb = _case(R, mu_given, False), _case(R, mu_given, True)
    i32 = dict(dtype=torch.int32, device=DEV)
    every = torch.arange(N_ATOMS, **i32)
    base_f, base_b = _fwd(cf)[:2], _bwd(cb)
    same = lambda a, b: a is None and b is None or torch.equal(a, b)
    # arange(N) is NULL, bit for bit
    lf, lb = _fwd(cf, atom_list=every)[:2], _bwd(cb, atom_list=every)
    assert all(same(a, b) for a, b in zip(lf + lb, base_f + base_b))
    # a shuffled list: per-atom outputs bit for bit, the filter gradient within its bound (another block order)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(N_ATOMS).astype(np.int32)).to(DEV)
    sf, sb = _fwd(cf, atom_list=perm)[:2], _bwd(cb, atom_list=perm)
    assert all(same(a, b) for a, b in zip(sf + sb[:2], base_f + base_b[:2]))
    ref = _twin_bwd(cb, (R, mu_given, True), 1.0)
    assert_within(sb[2].cpu(), *ref["dWf"], tw.C_WGRAD, tw.U, "dWf of a shuffled list")
    assert_within(sb[3].cpu(), *ref["dbf"], tw.C_WGRAD, tw.U, "dbf of a shuffled list")
    # dyn_nlist = 37 of 96: the rows of unlisted atoms are not touched, the filter gradient is that of the 37 atoms
    dyn = torch.tensor([37], **i32)
    listed = perm[:37].long()
    rest = torch.ones(N_ATOMS, dtype=torch.bool, device=DEV)
    rest[listed] = False
    df, db = _fwd(cf, atom_list=perm, dyn=dyn)[:2], _bwd(cb, atom_list=perm, dyn=dyn)
    for got, base in zip(df + db[:2], base_f + base_b[:2]):
        if got is not None:
            assert torch.equal(got[listed], base[listed]) and bool(got[rest].isnan().all())
    part = _twin_bwd(cb, (R, mu_given, True), 1.0, atoms=listed.cpu().tolist())
    assert_within(db[2].cpu(), *part["dWf"], tw.C_WGRAD, tw.U, "dWf of 37 listed atoms")
    assert_within(db[3].cpu(), *part["dbf"], tw.C_WGRAD, tw.U, "dbf of 37 listed atoms")
    # dyn_nlist = 0: nothing per atom, zero filter gradient
    zero = torch.tensor([0], **i32)
    zf, zb = _fwd(cf, atom_list=perm, dyn=zero)[:2], _bwd(cb, atom_list=perm, dyn=zero)
    assert all(bool(x.isnan().all()) for x in zf + zb[:2] if x is not None)
    assert bool((zb[2] == 0).all()) and bool((zb[3] == 0).all())
    # accumulate = 1 adds onto what is there
    ab = _bwd(cb, accumulate=1, prefill=0.5)   # (0.5 is the first addend of the reduction's last sum: one more term of S)
    assert_within(ab[2].cpu(), ref["dWf"][0] + 0.5, ref["dWf"][1] + 0.5, tw.C_WGRAD, tw.U, "dWf added onto 0.5")
    assert_within(ab[3].cpu(), ref["dbf"][0] + 0.5, ref["dbf"][1] + 0.5, tw.C_WGRAD, tw.U, "dbf added onto 0.5")
    assert float((ab[2] - base_b[2]).mean()) == pytest.approx(0.5, abs=1e-5)


@pytest.mark.parametrize("R,mu_given", PARAMS, ids=IDS)
def test_no_edges_at_all(R, mu_given):
    """E = 0: the forward writes the identities, the backward zero gradients and the residual."""
    from geossl_amd.layout import get_edge_layout
    c = dict(_case(R, mu_given, False))
    c["ei"] = torch.zeros(2, 0, dtype=torch.long, device=DEV)
    c["el"] = get_edge_layout(torch.zeros(N_ATOMS, dtype=torch.long, device=DEV), c["ei"], 1)
    q_out, mu_out, rc = _fwd(c)
    assert rc == 0 and torch.equal(q_out, c["q"])
    assert torch.equal(mu_out, c["mu"] if mu_given else torch.zeros_like(mu_out))
    dxc, dmu_in, dWf, dbf = _bwd(c)
    assert bool((dxc == 0).all()) and bool((dWf == 0).all()) and bool((dbf == 0).all())
    assert dmu_in is None if not mu_given else torch.equal(dmu_in, c["dmu"])


def test_unserved_shapes_are_refused():
    from geossl_amd import _lib
    lib = _lib.load()
    assert lib.geossl_painn_tile_ok(128, 20) == 1 and lib.geossl_painn_tile_ok(128, 32) == 0
    assert lib.geossl_painn_tile_ok(64, 20) == 0
    c = _case(20, True, False)
    el = c["el"]
    inc_ptr, inc_idx = el.inc["i"]
    q_out, mu_out = torch.full((N_ATOMS, F), NAN, device=DEV), torch.full((N_ATOMS, 3, F), NAN, device=DEV)
    ws = torch.empty(1 << 20, device=DEV)
    for Fv, Rv in ((128, 32), (64, 20)):
        rc = lib.geossl_painn_interaction_fwd_tile(_ptr(c["q"]), _ptr(c["mu"]), _ptr(c["xc"]), _ptr(el.idx_j), _ptr(inc_ptr),
                                                   _ptr(inc_idx), _ptr(c["phi"]), _ptr(c["fcut"]), _ptr(c["dirv"]), _ptr(c["Wf"]),
                                                   _ptr(c["bf"]), None, N_ATOMS, None, Fv, Rv, _ptr(q_out), _ptr(mu_out),
                                                   _lib.stream())
        assert rc == INVALID
        rc = lib.geossl_painn_interaction_bwd_tile(_ptr(c["dq"]), _ptr(c["dmu"]), _ptr(c["mu"]), _ptr(c["xc"]), _ptr(el.idx_i),
                                                   _ptr(inc_ptr), _ptr(inc_idx), _ptr(c["phi"]), _ptr(c["fcut"]), _ptr(c["dirv"]),
                                                   _ptr(c["Wf"]), _ptr(c["bf"]), None, N_ATOMS, None, Fv, Rv, _ptr(q_out),
                                                   _ptr(mu_out), _ptr(q_out), _ptr(q_out), _ptr(ws), 0, _lib.stream())
        assert rc == INVALID
    torch.cuda.synchronize()
    assert bool(q_out.isnan().all()) and bool(mu_out.isnan().all())
    # mu == NULL requires dmu_in == NULL
    rc = lib.geossl_painn_interaction_bwd_tile(_ptr(c["dq"]), _ptr(c["dmu"]), None, _ptr(c["xc"]), _ptr(el.idx_i),
                                               _ptr(inc_ptr), _ptr(inc_idx), _ptr(c["phi"]), _ptr(c["fcut"]), _ptr(c["dirv"]),
                                               _ptr(c["Wf"]), _ptr(c["bf"]), None, N_ATOMS, None, 128, 20, _ptr(q_out),
                                               _ptr(mu_out), _ptr(q_out), _ptr(q_out), _ptr(ws), 0, _lib.stream())
    assert rc == INVALID


# ------------------------------------------------------------------------------------------------------ end to end
SIZES, CUTOFF = (300, 7, 257), 5.0
PAINN_CFG = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=CUTOFF, max_z=9, n_out=1, readout="add")
TILE_CALLS = ("geossl_painn_interaction_fwd_tile", "geossl_painn_interaction_bwd_tile")


def _other_interaction_calls(calls):
    return [n for n in calls if n.startswith("geossl_painn_interaction_") and n not in TILE_CALLS]


def _count_calls(monkeypatch):
    import geossl_amd.Geom3D.models.painn as pm
    calls, real = [], pm.call

    def counting(name, *a):
        calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(pm, "call", counting)
    return calls


def _tile_env(monkeypatch, on):
    """The route under test: the default above 255 atoms if the measurement turned it on, else GEOSSL_PAINN_TILE=1."""
    from geossl_amd import switches
    if not on:
        monkeypatch.setenv("GEOSSL_PAINN_TILE", "0")
    elif switches.PAINN_TILE_DEFAULT:
        monkeypatch.delenv("GEOSSL_PAINN_TILE", raising=False)
    else:
        monkeypatch.setenv("GEOSSL_PAINN_TILE", "1")


def _grad_errors(model, head, P, H):
    got = dict(unique_named_grads(model), **{"head." + k: v for k, v in unique_named_grads(head).items()})
    ref = dict({k: v.grad for k, v in P.items()}, **{"head." + k: v.grad for k, v in H.items()})
    return {k: ft.max_err(got[k], v) for k, v in ref.items() if v is not None}


_SUP_REF = {}


def _supervised_reference(model, head, s, ei, y, mean, std, task):
    if not _SUP_REF:
        params, bufs = ft.module_tensors(model)
        P = {k: v.double().requires_grad_(True) for k, v in params.items()}
        C = {k: v.double() for k, v in bufs.items() if v.is_floating_point()}
        H = {k: v.detach().double().cpu().requires_grad_(True) for k, v in head.state_dict().items()}
        rep = nets.painn_forward(dict(P, **C), torch.from_numpy(s["x"]), torch.from_numpy(s["positions"]).double(),
                                 torch.from_numpy(ei), torch.from_numpy(s["batch"]), 128, 3, CUTOFF, "add")
        L = ((ft.head_forward(rep, H) - (torch.from_numpy(y[:, task]).double() - mean) / std) ** 2).mean()
        L.backward()
        _SUP_REF.update(P=P, H=H, L=float(L.detach()))
    return _SUP_REF["P"], _SUP_REF["H"], _SUP_REF["L"]


@pytest.mark.parametrize("tile", [True, False], ids=["tile", "tile-off"])
def test_do_supervised_above_255_atoms(tile, monkeypatch):
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.models import PaiNN
    from geossl_amd.pretrain_Supervised import do_Supervised
    s = ls.checked(SIZES, CUTOFF)
    model = fill_module_(PaiNN(**PAINN_CFG)).to(DEV)
    head = fill_module_(model.create_output_layers()).to(DEV)
    ei = radius_graph_np(s["positions"], CUTOFF, s["batch"])
    y = np.asarray([[0.4, -1.2], [2.0, 0.3], [-0.7, 1.1]], dtype=np.float32)
    mean, std, task = 0.2, 1.5, 1
    b = pg.Batch(t(s["x"], DEV)[:, None].contiguous(), t(s["positions"], DEV), t(s["batch"], DEV), None,
                 radius_edge_index=t(ei, DEV), num_graphs=len(SIZES), sizes=SIZES)
    b.y = t(y.reshape(-1), DEV)
    _tile_env(monkeypatch, tile)
    calls = _count_calls(monkeypatch)
    loss = do_Supervised(types.SimpleNamespace(model_3d="painn", loss="mse"), b, model, head, mean, std, task_id=task,
                         graph=False)
    loss.backward()
    if tile:
        assert [calls.count(n) for n in TILE_CALLS] == [3, 3] and not _other_interaction_calls(calls)
    else:
        assert [calls.count(n) for n in TILE_CALLS] == [0, 0] and len(_other_interaction_calls(calls)) >= 6
    P, H, L = _supervised_reference(model, head, s, ei, y, mean, std, task)
    bounds = ft.BOUNDS["painn"]
    worst = _grad_errors(model, head, P, H)
    loss = float(loss.detach())
    print("do_Supervised %s: loss %.2e worst gradient %.2e" % (tile, abs(loss - L) / abs(L), max(worst.values())))
    assert abs(loss - L) <= bounds["loss"] * abs(L)
    bad = {k: e for k, e in worst.items() if not e <= bounds["grad"]}
    assert not bad, bad


def test_do_lep_on_pairs_above_255_atoms(monkeypatch):
    from geossl_amd.Geom3D.dataloaders import BatchLEP, Data
    from geossl_amd.Geom3D.models import PaiNN
    from geossl_amd.finetune_lep import do_LEP
    sizes_a, sizes_i = SIZES, (257, 300, 7)
    B = len(sizes_a)
    s = ls.checked(sizes_a + sizes_i, CUTOFF)
    off = np.concatenate([[0], np.cumsum(sizes_a + sizes_i)])
    part = lambda k, m: torch.from_numpy(np.ascontiguousarray(s[k][off[m]:off[m + 1]]))
    edges = lambda m: torch.from_numpy(radius_graph_np(s["positions"][off[m]:off[m + 1]], CUTOFF,
                                                       np.zeros(off[m + 1] - off[m], dtype=np.int64)))
    items = [Data(x_active=part("x", b), positions_active=part("positions", b), x_inactive=part("x", B + b),
                  positions_inactive=part("positions", B + b), y=torch.tensor([(b + 1) % 2], dtype=torch.long),
                  radius_edge_index_active=edges(b), radius_edge_index_inactive=edges(B + b)) for b in range(B)]
    model = fill_module_(PaiNN(**PAINN_CFG)).to(DEV)
    head = torch.nn.Linear(2 * 128, 1)
    with torch.no_grad():
        head.weight.copy_(torch.linspace(-1.0, 1.0, 256).reshape(1, 256) * 0.02)
        head.bias.fill_(0.1)
    head = head.to(DEV)
    _tile_env(monkeypatch, True)
    calls = _count_calls(monkeypatch)
    loss = do_LEP(types.SimpleNamespace(model_3d="painn"), BatchLEP.from_data_list(items).to(DEV), model, head,
                  torch.nn.BCEWithLogitsLoss(), graph=False)
    loss.backward()
    assert [calls.count(n) for n in TILE_CALLS] == [3, 3] and not _other_interaction_calls(calls)   # both sides in one pass
    # the fp64 twin: the 2B structures as one batch, the pair head on its readout
    params, bufs = ft.module_tensors(model)
    P = {k: v.double().requires_grad_(True) for k, v in params.items()}
    C = {k: v.double() for k, v in bufs.items() if v.is_floating_point()}
    H = {k: v.detach().double().cpu().requires_grad_(True) for k, v in head.state_dict().items()}
    ei = radius_graph_np(s["positions"], CUTOFF, s["batch"])
    rep = nets.painn_forward(dict(P, **C), torch.from_numpy(s["x"]), torch.from_numpy(s["positions"]).double(),
                             torch.from_numpy(ei), torch.from_numpy(s["batch"]), 128, 3, CUTOFF, "add")
    yv = torch.tensor([float((b + 1) % 2) for b in range(B)])
    L = lt.bce(lt.logits(rep[:B], rep[B:], H["weight"], H["bias"]), yv)
    L.backward()
    bounds = ft.BOUNDS["painn"]
    worst = _grad_errors(model, head, P, H)
    loss, L = float(loss.detach()), float(L.detach())
    print("do_LEP tile: loss %.2e worst gradient %.2e" % (abs(loss - L) / abs(L), max(worst.values())))
    assert abs(loss - L) <= bounds["loss"] * abs(L)
    bad = {k: e for k, e in worst.items() if not e <= bounds["grad"]}
    assert not bad, bad


def test_tile_route_on_small_molecules_agrees_with_the_default_route(monkeypatch):
    """GEOSSL_PAINN_TILE=1 reaches the kernels on 24 molecules of 18 atoms; unset, that layout keeps its kernels."""
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.models import PaiNN
    from geossl_amd.synthetic import make_batch
    sizes = [18] * 24
    bt = pg.Batch.from_numpy(make_batch(len(sizes), seed=3, sizes=sizes), DEV)
    rei = ops.radius_graph(bt.positions, 5.0, bt.batch)
    model = fill_module_(PaiNN(**PAINN_CFG)).to(DEV)
    w = (torch.linspace(-1.0, 1.0, 128) * 0.3 + 0.05).to(DEV)

    def run():
        model.zero_grad(set_to_none=True)
        out, q = model(bt.x, bt.positions, rei, bt.batch, return_latent=True)
        ((out * w).sum() + 0.5 * (q ** 2).sum()).backward()
        return out.detach().clone(), {k: v.clone() for k, v in unique_named_grads(model).items()}

    calls = _count_calls(monkeypatch)
    monkeypatch.delenv("GEOSSL_PAINN_TILE", raising=False)
    out0, g0 = run()
    assert [calls.count(n) for n in TILE_CALLS] == [0, 0]
    del calls[:]
    monkeypatch.setenv("GEOSSL_PAINN_TILE", "1")
    out1, g1 = run()
    assert [calls.count(n) for n in TILE_CALLS] == [3, 3] and not _other_interaction_calls(calls)
    bounds = ft.BOUNDS["painn"]
    assert ft.max_err(out1, out0) <= bounds["energy"]
    bad = {k: ft.max_err(g1[k], g0[k]) for k in g0 if not ft.max_err(g1[k], g0[k]) <= bounds["grad"]}
    assert not bad, bad
