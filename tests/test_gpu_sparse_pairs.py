"""GPU tests of SchNet on the sparse pair list (csrc/sparse_pairs.hip; structures above 255 atoms): the list against the
dense pair-slot form bit for bit, the aggregation against ops.aggregate bit for bit, edge cases (no pairs at all, a
ligand moved 1000 A away, an isolated atom, 256 / 257 / 1024 / 1025 atoms), the whole model against the fp64 oracle on
pocket-sized structures, forced-sparse against dense end to end, determinism, what is refused, the radius graph on 700
atoms, and PaiNN at 300 atoms."""
import types

import numpy as np
import pytest
import torch

import force_twin as ft
import lba_structures as ls
from helpers import fill_module_, t, unique_named_grads
from oracle import nets
from oracle.graph import radius_graph_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MIXED = (1, 2, 33, 34, 64, 65, 128, 129, 255)
REDUCED = dict(hidden_channels=64, num_filters=64, num_interactions=2, num_gaussians=8, node_class=9, readout="mean")
FULL = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, node_class=9, readout="mean")
TOL_OUT, TOL_GRAD = 1e-5, 1e-4   # the suite's bounds on max|got - ref| / max|ref| against fp64


def _poison():
    """Leave NaN bytes in the allocator's free blocks: what torch.empty hands out next is not zeros."""
    junk = [torch.full((n,), NAN, device=DEV) for n in (1 << 22, 1 << 20, 1 << 18, 1 << 16, 1 << 12)]
    del junk


def _layout(batch, sizes, sparse, monkeypatch):
    from geossl_amd.layout import MolLayout
    if sparse is None:
        monkeypatch.delenv("GEOSSL_SPARSE_PAIRS", raising=False)
    else:
        monkeypatch.setenv("GEOSSL_SPARSE_PAIRS", "1" if sparse else "0")
    lay = MolLayout(batch, len(sizes), sizes=list(sizes))
    monkeypatch.delenv("GEOSSL_SPARSE_PAIRS", raising=False)
    return lay


def _slots(sp, lay_dense, n):
    """Dense slot of every real row of the list, in closed form from (pair_i, pair_j, mol_ptr)."""
    mp = lay_dense.mol_ptr.cpu().numpy().astype(np.int64)
    pp = lay_dense.pair_ptr.cpu().numpy().astype(np.int64)
    i, j = sp.pair_i[:n].cpu().numpy().astype(np.int64), sp.pair_j[:n].cpu().numpy().astype(np.int64)
    m = np.searchsorted(mp, i, side="right") - 1
    assert np.array_equal(m, np.searchsorted(mp, j, side="right") - 1)
    nm, a, b = mp[m + 1] - mp[m], i - mp[m], j - mp[m]
    assert np.all(a < b) and np.all(b < nm)
    return pp[m] + a * nm - a * (a + 1) // 2 - a - 1 + b


@pytest.fixture(scope="module")
def mixed():
    s = ls.structures(MIXED, 0)
    return dict(s, pos=t(s["positions"], DEV), b=t(s["batch"], DEV))


# ------------------------------------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize("cutoff", [5.0, 10.0])
def test_list_equals_dense_slots_bit_for_bit(mixed, cutoff, monkeypatch):
    from geossl_amd import ops
    dense = _layout(mixed["b"], MIXED, None, monkeypatch)
    sparse = _layout(mixed["b"], MIXED, True, monkeypatch)
    assert not dense.sparse and sparse.sparse and sparse.pair_i is None and sparse.agg_work is None
    assert sparse.P == ls.pair_capacity(MIXED)
    d, c, fl = ops.pair_geometry(mixed["pos"], dense, cutoff)
    _poison()
    sp = ops.sparse_pair_geometry(mixed["pos"], sparse, cutoff)
    n = int(sp.n_pairs.item())
    assert 0 < n <= sp.P
    slot = torch.from_numpy(_slots(sp, dense, n)).to(DEV)
    i, j = sp.pair_i[:n].long(), sp.pair_j[:n].long()
    key = i * (mixed["pos"].size(0) + 1) + j
    assert torch.all(key[1:] > key[:-1])                                  # lexicographic, molecules in batch order
    assert torch.equal(sp.pair_d[:n], d[slot]) and torch.equal(sp.pair_c[:n], c[slot])
    assert torch.equal(sp.pair_flag[:n], fl[slot]) and torch.all(sp.pair_flag[:n] != 0)
    rest = torch.ones_like(fl, dtype=torch.bool)
    rest[slot] = False
    assert torch.all(fl[rest] == 0)                                       # every slot that was not kept has no edge
    # rows past the real ones
    assert torch.all(sp.pair_flag[n:] == 0) and torch.all(sp.pair_i[n:] == 0) and torch.all(sp.pair_j[n:] == 0)
    assert torch.all(sp.pair_c[n:] == 0) and torch.all(sp.pair_d[n:] == cutoff)
    # incidence lists: complete, ascending partner, the direction bits of the flags
    N = mixed["pos"].size(0)
    ptr_ = sp.inc_ptr.cpu().numpy().astype(np.int64)
    assert ptr_[0] == 0 and ptr_[N] == 2 * n and np.all(np.diff(ptr_) >= 0)
    row = sp.inc_pair[:2 * n].cpu().numpy().astype(np.int64)
    src = sp.inc_src[:2 * n].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    owner = np.repeat(np.arange(N), np.diff(ptr_))
    i_, j_, f_ = i.cpu().numpy(), j.cpu().numpy(), sp.pair_flag[:n].cpu().numpy().astype(np.int64)
    p_ = np.arange(n)
    # expected entries (target, partner, row, partner -> target, target -> partner)
    exp = np.concatenate([np.stack([j_, i_, p_, (f_ >> 1) & 1, f_ & 1], 1), np.stack([i_, j_, p_, f_ & 1, (f_ >> 1) & 1], 1)])
    exp = exp[np.lexsort((exp[:, 1], exp[:, 0]))]
    got = np.stack([owner, src & 0x3FFFFFFF, row, (src >> 30) & 1, (src >> 31) & 1], 1)
    assert np.array_equal(got, exp)


# --------------------------------------------------------------------------------------------- 2. aggregation
@pytest.mark.parametrize("F", [32, 64, 128])
@pytest.mark.parametrize("swap", [False, True])
def test_aggregation_equals_dense_bit_for_bit(mixed, F, swap, monkeypatch):
    from geossl_amd import ops
    cutoff = 10.0
    dense = _layout(mixed["b"], MIXED, None, monkeypatch)
    sparse = _layout(mixed["b"], MIXED, True, monkeypatch)
    _, _, fl = ops.pair_geometry(mixed["pos"], dense, cutoff)
    sp = ops.sparse_pair_geometry(mixed["pos"], sparse, cutoff)
    n = int(sp.n_pairs.item())
    g = torch.Generator(device=DEV).manual_seed(F + swap)
    N = mixed["pos"].size(0)
    x = torch.randn(N, F, device=DEV, generator=g)
    Wd = torch.randn(dense.P, F, device=DEV, generator=g)
    Ws = torch.full((sp.P, F), NAN, device=DEV)                           # (rows past the real ones are never read)
    Ws[:n] = Wd[torch.from_numpy(_slots(sp, dense, n)).to(DEV)]
    ref = ops.aggregate(x, Wd, fl, dense, swap=swap, out=torch.full((N, F), NAN, device=DEV))
    got = ops.aggregate_sparse(x, Ws, sp, swap=swap, out=torch.full((N, F), NAN, device=DEV))
    assert torch.isfinite(ref).all() and torch.equal(got, ref)


# ----------------------------------------------------------------------------------------------- whole model
def _model(cfg, cutoff):
    from geossl_amd.Geom3D.models import SchNet
    return fill_module_(SchNet(cutoff=cutoff, **cfg)).to(DEV)


def _run(model, s, sparse, monkeypatch, head_w=None):
    """Forward + backward of sum_m w . repr_m -> (repr, force = -dL/dpos, {name: grad})."""
    b = t(s["batch"], DEV)
    lay = _layout(b, s["sizes"], sparse, monkeypatch)
    pos = t(s["positions"], DEV).requires_grad_(True)
    model.zero_grad(set_to_none=True)
    rep = model(t(s["x"], DEV), pos, b, layout=lay)
    w = head_w if head_w is not None else _head_w(rep.size(1))
    (rep * w.to(DEV)).sum().backward()
    return rep.detach().cpu(), -pos.grad.cpu(), {k: v.cpu() for k, v in unique_named_grads(model).items()}, lay


def _head_w(F):
    return torch.linspace(-1.0, 1.0, F) * 0.3 + 0.05


def _oracle(model, cfg, cutoff, s, backward=True):
    params, bufs = ft.module_tensors(model)
    P = {k: v.double().requires_grad_(backward) for k, v in params.items()}
    P.update({k: v.double() for k, v in bufs.items() if v.is_floating_point()})
    x = torch.from_numpy(s["positions"]).double().requires_grad_(backward)
    ei = ft.schnet_edges(s["positions"], s["batch"], cutoff)
    rep = nets.schnet_forward(P, torch.from_numpy(s["x"]), x, torch.from_numpy(s["batch"]), cutoff,
                              cfg["num_interactions"], cfg["readout"], edge_index=ei)
    if not backward:
        return rep.detach(), None, None
    (rep * _head_w(rep.size(1)).double()).sum().backward()
    return rep.detach(), -x.grad, {k: v.grad for k, v in P.items() if k in params}


_ORACLE = {}


def _oracle_cached(name, cfg, sizes, cutoff):
    """The fp64 reference of one (configuration, structure set), computed once per session and left unchanged."""
    key = (name, sizes, cutoff)
    if key not in _ORACLE:
        s = ls.checked(sizes, cutoff)
        _ORACLE[key] = (s,) + _oracle(_model(cfg, cutoff), cfg, cutoff, s)
    return _ORACLE[key]


def _compare(got, ref, what):
    rep, force, grads = got
    rrep, rforce, rgrads = ref
    errs = {"repr": ft.max_err(rep, rrep), "force": ft.max_err(force, rforce)}
    errs.update({"grad/" + k: ft.max_err(grads[k], v) for k, v in rgrads.items()})
    worst = max((e for k, e in errs.items() if k.startswith("grad/")), default=0.0)
    print("%s: repr %.2e force %.2e worst gradient %.2e" % (what, errs["repr"], errs["force"], worst))
    bad = {k: e for k, e in errs.items() if not e <= (TOL_GRAD if k.startswith("grad/") else TOL_OUT)}
    assert not bad, (what, bad)


SETS = [((300, 7, 257), 10.0), ((512, 1, 40), 5.0), ((1024,), 5.0)]


@pytest.mark.parametrize("sizes,cutoff", SETS, ids=["300_7_257_r10", "512_1_40_r5", "1024_r5"])
@pytest.mark.parametrize("name,cfg", [("reduced", REDUCED), ("full", FULL)], ids=["reduced", "full"])
def test_model_against_fp64(name, cfg, sizes, cutoff, monkeypatch):
    s, rrep, rforce, rgrads = _oracle_cached(name, cfg, sizes, cutoff)
    _poison()
    rep, force, grads, lay = _run(_model(cfg, cutoff), s, None, monkeypatch)
    assert lay.sparse and lay.P == ls.pair_capacity(sizes)
    _compare((rep, force, grads), (rrep, rforce, rgrads), "%s %r r=%g" % (name, sizes, cutoff))


@pytest.mark.parametrize("switch", ["GEOSSL_FILTER_RECOMPUTE_T", "GEOSSL_ARITH_24BIT"])
def test_switches_keep_working_on_the_sparse_branch(switch, monkeypatch):
    s, rrep, rforce, rgrads = _oracle_cached("reduced", REDUCED, (300, 7, 257), 10.0)
    monkeypatch.setenv(switch, "1")
    rep, force, grads, _ = _run(_model(REDUCED, 10.0), s, None, monkeypatch)
    _compare((rep, force, grads), (rrep, rforce, rgrads), switch)


def test_direct_grads_on_the_sparse_branch(monkeypatch):
    """Inside _lib.direct_grads() the kernels accumulate into p.grad: twice the gradients of one backward after two."""
    from geossl_amd import _lib
    s = ls.checked((300, 7, 257), 10.0)
    model = _model(REDUCED, 10.0)
    _, _, grads, lay = _run(model, s, None, monkeypatch)
    b, pos = t(s["batch"], DEV), t(s["positions"], DEV)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    for _ in range(2):
        rep = model(t(s["x"], DEV), pos, b, layout=lay)
        with _lib.direct_grads():
            (rep * _head_w(rep.size(1)).to(DEV)).sum().backward()
    for k, v in unique_named_grads(model).items():
        assert ft.max_err(v.cpu(), 2 * grads[k]) < 1e-6, k


# ------------------------------------------------------------------------------------- 5. forced sparse = dense
def test_forced_sparse_against_dense_end_to_end(monkeypatch):
    sizes = (64, 33, 1, 129, 255, 2)
    s = ls.structures(sizes, 1)
    model = _model(FULL, 10.0)
    rep_d, force_d, grads_d, lay_d = _run(model, s, None, monkeypatch)
    rep_s, force_s, grads_s, lay_s = _run(model, s, True, monkeypatch)
    assert not lay_d.sparse and lay_s.sparse
    assert ft.max_err(rep_s, rep_d) <= TOL_OUT and ft.max_err(force_s, force_d) <= TOL_OUT
    assert abs(float((rep_s * _head_w(128)).sum() - (rep_d * _head_w(128)).sum())) <= TOL_OUT * float(rep_d.abs().sum())
    for k, v in grads_d.items():
        assert ft.max_err(grads_s[k], v) <= TOL_GRAD, k


# ------------------------------------------------------------------------------------------- 6. determinism
def test_two_runs_are_bitwise_equal(monkeypatch):
    s = ls.checked((300, 7, 257), 10.0)
    model = _model(FULL, 10.0)
    a = _run(model, s, None, monkeypatch)
    _poison()
    b = _run(model, s, None, monkeypatch)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k, v in a[2].items():
        assert torch.equal(v, b[2][k]), k


# --------------------------------------------------------------------------------------------- 3. edge cases
def test_one_atom_molecules_only(monkeypatch):
    from geossl_amd import ops
    sizes = (1,) * 5
    s = ls.structures(sizes, 0)
    lay = _layout(t(s["batch"], DEV), sizes, True, monkeypatch)
    assert lay.sparse and lay.P == 0
    sp = ops.sparse_pair_geometry(t(s["positions"], DEV), lay, 5.0)
    assert int(sp.n_pairs.item()) == 0 and torch.all(sp.inc_ptr == 0)
    model = _model(REDUCED, 5.0)
    rep, force, grads, _ = _run(model, s, True, monkeypatch)
    rrep, rforce, rgrads = _oracle(model, REDUCED, 5.0, s)
    assert ft.max_err(rep, rrep) <= TOL_OUT and torch.all(force == 0)
    for k, v in rgrads.items():
        assert torch.isfinite(grads[k]).all() and (ft.max_err(grads[k], v) <= TOL_GRAD or float(v.abs().max()) == 0.0), k


def test_moved_ligand_and_isolated_atom(monkeypatch):
    """A 300-atom structure with 20 atoms shifted by +1000 A in x (TransformLBA(move_lig=True)) and one atom on its own:
    that atom's rows of the aggregation and of the position gradient are zeros, not NaN."""
    from geossl_amd import ops
    s = ls.structures((300,), 2)
    s["positions"][280:, 0] += 1000.0
    s["positions"][17] = (-500.0, 300.0, 40.0)
    b = t(s["batch"], DEV)
    lay = _layout(b, (300,), None, monkeypatch)
    sp = ops.sparse_pair_geometry(t(s["positions"], DEV), lay, 5.0)
    n = int(sp.n_pairs.item())
    assert int(sp.inc_ptr[18] - sp.inc_ptr[17]) == 0
    ii, jj = sp.pair_i[:n], sp.pair_j[:n]
    assert not torch.any((ii < 280) & (jj >= 280))                        # no pair joins pocket and moved ligand
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(300, 64, device=DEV, generator=g)
    W = torch.full((sp.P, 64), NAN, device=DEV)
    W[:n] = torch.randn(n, 64, device=DEV, generator=g)
    for swap in (False, True):
        out = ops.aggregate_sparse(x, W, sp, swap=swap, out=torch.full((300, 64), NAN, device=DEV))
        assert torch.isfinite(out).all() and torch.all(out[17] == 0)
    model = _model(REDUCED, 5.0)
    rep, force, grads, _ = _run(model, s, None, monkeypatch)
    rrep, rforce, rgrads = _oracle(model, REDUCED, 5.0, s)
    assert torch.isfinite(force).all() and torch.all(force[17] == 0)
    assert ft.max_err(rep, rrep) <= TOL_OUT and ft.max_err(force, rforce) <= TOL_OUT
    for k, v in rgrads.items():
        assert ft.max_err(grads[k], v) <= TOL_GRAD, k


def _edges_of(sp, n):
    """The directed edges (source, target) the list's flags stand for, target-major, sources ascending."""
    i, j, f = sp.pair_i[:n].cpu().numpy(), sp.pair_j[:n].cpu().numpy(), sp.pair_flag[:n].cpu().numpy()
    f0, f1 = (f & 1) > 0, (f & 2) > 0
    e = np.concatenate([np.stack([j[f0], i[f0]]), np.stack([i[f1], j[f1]])], axis=1)
    return e[:, np.lexsort((e[0], e[1]))].astype(np.int64)


@pytest.mark.parametrize("sizes", [(256, 257), (1024,)], ids=["256_257", "1024"])
def test_list_holds_the_edges_of_the_radius_graph(sizes, monkeypatch):
    from geossl_amd import ops
    s = ls.checked(sizes, 5.0)
    lay = _layout(t(s["batch"], DEV), sizes, None, monkeypatch)
    assert lay.sparse
    _poison()
    sp = ops.sparse_pair_geometry(t(s["positions"], DEV), lay, 5.0)
    n = int(sp.n_pairs.item())
    assert n <= sp.P
    assert np.array_equal(_edges_of(sp, n), radius_graph_np(s["positions"], 5.0, s["batch"]))


def test_1024_atoms_forward(monkeypatch):
    s = ls.checked((1024,), 5.0)
    model = _model(REDUCED, 5.0)
    b = t(s["batch"], DEV)
    with torch.no_grad():
        rep = model(t(s["x"], DEV), t(s["positions"], DEV), b, layout=_layout(b, (1024,), None, monkeypatch))
    rrep, _, _ = _oracle(model, REDUCED, 5.0, s, backward=False)
    assert ft.max_err(rep.cpu(), rrep) <= TOL_OUT


def test_1025_atoms_raise(monkeypatch):
    s = ls.structures((1025,), 0)
    model = _model(REDUCED, 5.0)
    b = t(s["batch"], DEV)
    with pytest.raises(ValueError, match="1024"):
        model(t(s["x"], DEV), t(s["positions"], DEV), b, layout=_layout(b, (1025,), None, monkeypatch))
    from geossl_amd import ops
    with pytest.raises(ValueError, match="1024"):
        ops.radius_graph(t(s["positions"], DEV), 5.0, b)


# ----------------------------------------------------------------------------------------------- 7. refusals
def test_second_order_and_tape_widths_are_refused(monkeypatch):
    from geossl_amd.Geom3D.models import SchNet
    s = ls.structures((260,), 0)
    b, x = t(s["batch"], DEV), t(s["x"], DEV)
    model = _model(REDUCED, 5.0)
    pos = t(s["positions"], DEV).requires_grad_(True)
    energy = model(x, pos, b, layout=_layout(b, (260,), None, monkeypatch)).sum()
    with pytest.raises(NotImplementedError, match="255"):
        torch.autograd.grad(energy, pos, create_graph=True)
    odd = fill_module_(SchNet(hidden_channels=48, num_filters=40, num_interactions=1, num_gaussians=8, cutoff=5.0,
                              node_class=9)).to(DEV)
    with pytest.raises(NotImplementedError, match="255"):
        odd(x, t(s["positions"], DEV), b, layout=_layout(b, (260,), None, monkeypatch))
    from geossl_amd import bucket
    assert bucket.MAX_N == 255


# ------------------------------------------------------------------------------------------- 8. radius graph
def test_radius_graph_700_atoms():
    from geossl_amd import ops
    s = ls.checked((700, 3), 5.0)
    ei = ops.radius_graph(t(s["positions"], DEV), 5.0, t(s["batch"], DEV))
    assert np.array_equal(ei.cpu().numpy(), radius_graph_np(s["positions"], 5.0, s["batch"]))


# --------------------------------------------------------------------------------------------------- 9. PaiNN
def test_painn_300_atoms_through_do_supervised():
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.models import PaiNN
    from geossl_amd.pretrain_Supervised import do_Supervised
    sizes, cutoff = (300, 7, 257), 5.0
    s = ls.checked(sizes, cutoff)
    cfg = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=cutoff, max_z=9, n_out=1, readout="add")
    model = fill_module_(PaiNN(**cfg)).to(DEV)
    head = fill_module_(model.create_output_layers()).to(DEV)
    ei = radius_graph_np(s["positions"], cutoff, s["batch"])
    y = np.asarray([[0.4, -1.2], [2.0, 0.3], [-0.7, 1.1]], dtype=np.float32)
    mean, std, task = 0.2, 1.5, 1
    b = pg.Batch(t(s["x"], DEV)[:, None].contiguous(), t(s["positions"], DEV), t(s["batch"], DEV), None,
                 radius_edge_index=t(ei, DEV), num_graphs=len(sizes), sizes=sizes)
    b.y = t(y.reshape(-1), DEV)
    args = types.SimpleNamespace(model_3d="painn", loss="mse")
    loss = do_Supervised(args, b, model, head, mean, std, task_id=task, graph=False)
    loss.backward()
    # the fp64 twin of the same step
    params, bufs = ft.module_tensors(model)
    P = {k: v.double().requires_grad_(True) for k, v in params.items()}
    C = {k: v.double() for k, v in bufs.items() if v.is_floating_point()}
    H = {k: v.detach().double().cpu().requires_grad_(True) for k, v in head.state_dict().items()}
    rep = nets.painn_forward(dict(P, **C), torch.from_numpy(s["x"]), torch.from_numpy(s["positions"]).double(),
                             torch.from_numpy(ei), torch.from_numpy(s["batch"]), 128, 3, cutoff, "add")
    pred = ft.head_forward(rep, H)
    L = ((pred - (torch.from_numpy(y[:, task]).double() - mean) / std) ** 2).mean()
    L.backward()
    bounds = ft.BOUNDS["painn"]
    loss, L = float(loss.detach()), float(L.detach())
    assert abs(loss - L) <= bounds["loss"] * abs(L)
    got = dict(unique_named_grads(model), **{"head." + k: v for k, v in unique_named_grads(head).items()})
    ref = dict({k: v.grad for k, v in P.items()}, **{"head." + k: v.grad for k, v in H.items()})
    worst = {}
    for k, v in ref.items():
        if v is None:
            continue
        worst[k] = ft.max_err(got[k], v)
    print("PaiNN 300 atoms: loss %.2e worst gradient %.2e" % (abs(loss - L) / abs(L), max(worst.values())))
    bad = {k: e for k, e in worst.items() if not e <= bounds["grad"]}
    assert not bad, bad
