"""GPU tests of PaiNN on the sparse capacity bucket (geossl_amd/bucket.py, option "sparse" with an edges part: pockets
of up to 1024 atoms replayed from one graph per batch size under GEOSSL_PAINN_SPARSE_BUCKETS).

1. The incidence-list entry (csrc/painn_inc.hip) through the C ABI on poisoned outputs: entry for entry what
   layout.EdgeLayout builds and what the numpy twin (tests/painn_inc_twin.py) says, the capacity form, the status word,
   the refusals, two runs with the same bits.
2. The atom-tile kernels under dyn_nlist with the lists as a bucket holds them: per-atom outputs bit for bit, the filter
   gradient within the fp64 twin's bound.
3. Bucket replay against the eager step of SupervisedTrainer on ragged batches (stale rows, an outgrown bucket).
4. DeviceLoader-style handles of a DeviceDataset that builds its radius edges itself: two shuffled epochs, one capture.
5. LEP: pair handles of a PairedDeviceDataset built with radius=, one bucket of 2B structures; the errors that stay.
6. Fixtures G24 / G25 (PaiNN) through handles, at the fixtures' own bounds; do_Supervised / do_LEP take the same route.
7. The switch table and the batches and engines that keep their routes."""
import numpy as np
import pytest
import torch

import lba_structures as ls
import painn_inc_twin as itw
from objective_harness import backbone

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUTOFF = 5.0
POISON = -7
INVALID = 1   # hipErrorInvalidValue
SIZES_A, SIZES_B, SIZES_MAX, SIZES_BIG = (300, 2, 64, 1), (33, 257, 129, 5), (1024,), (600, 300, 280, 257)
SIZE_SETS = {"A": SIZES_A, "B": SIZES_B, "1024": SIZES_MAX, "BIG": SIZES_BIG}

_GRAPHS = {}


def graph(name):
    """Structures of a size set with their radius graph at 5 A, EdgeLayout's lists and the twin's: built once."""
    if name not in _GRAPHS:
        from geossl_amd import ops
        from geossl_amd.layout import EdgeLayout, MolLayout
        sizes = SIZE_SETS[name]
        s = ls.structures(sizes, seed=3)
        pos = torch.from_numpy(s["positions"]).to(DEV)
        batch = torch.from_numpy(s["batch"]).to(DEV)
        lay = MolLayout(batch, sizes=list(sizes))
        ei = ops.radius_graph(pos, CUTOFF, batch, layout=lay).contiguous()
        el = EdgeLayout(batch, ei, len(sizes))
        g = dict(s, pos=pos, batch_t=batch, lay=lay, ei=ei, E=int(ei.size(1)), N=int(batch.numel()), B=len(sizes),
                 el=el, twin=itw.layout_twin(ei.cpu().numpy(), sizes))
        assert g["twin"][4] == 0
        _GRAPHS[name] = g
    return _GRAPHS[name]


def run_entry(ei, mol_ptr, N, B, max_n, E_cap=None, N_cap=None, dyn=None, status=None):
    """The entry through the C ABI on poisoned outputs -> (rc, iptr_i, ilist_i, iptr_j, ilist_j, status) on the host.
    dyn = (E, N) as the device sees them: the `_dyn` form with outputs of (E_cap, N_cap)."""
    from geossl_amd import _lib
    lib = _lib.load()
    E = int(ei.size(1))
    E_cap, N_cap = (E if E_cap is None else E_cap), (N if N_cap is None else N_cap)
    src = torch.full((2, max(E_cap, 1)), 0, dtype=torch.int64, device=DEV)
    src[:, :E] = ei
    outs = [torch.full((N_cap + 1,), POISON, dtype=torch.int64, device=DEV),
            torch.full((max(E_cap, 1),), POISON, dtype=torch.int32, device=DEV),
            torch.full((N_cap + 1,), POISON, dtype=torch.int64, device=DEV),
            torch.full((max(E_cap, 1),), POISON, dtype=torch.int32, device=DEV)]
    status = torch.zeros(1, dtype=torch.int32, device=DEV) if status is None else status
    assert lib.geossl_painn_incidence_layout_workspace_bytes(E_cap, N_cap, B) == 0
    p = [o.data_ptr() for o in outs] + [status.data_ptr()]
    if dyn is None:
        rc = lib.geossl_painn_incidence_layout(src[0].data_ptr(), src[1].data_ptr(), E_cap, mol_ptr.data_ptr(), N_cap, B,
                                               max_n, *p, None, _lib.stream())
    else:
        d = torch.tensor(list(dyn), dtype=torch.int32, device=DEV)
        rc = lib.geossl_painn_incidence_layout_dyn(src[0].data_ptr(), src[1].data_ptr(), E_cap, d[0:].data_ptr(),
                                                   mol_ptr.data_ptr(), N_cap, B, max_n, *p, d[1:].data_ptr(), None,
                                                   _lib.stream())
    torch.cuda.synchronize()
    return (rc,) + tuple(o.cpu().numpy() for o in outs) + (int(status.item()),)


@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_entry_equals_edge_layout_and_the_twin(name):
    g = graph(name)
    E, N = g["E"], g["N"]
    assert E > 0
    rc, *got, status = run_entry(g["ei"], g["lay"].mol_ptr, N, g["B"], max(g["sizes"]))
    assert rc == 0 and status == 0
    want = [g["el"].inc["i"][0], g["el"].inc["i"][1][:E], g["el"].inc["j"][0], g["el"].inc["j"][1][:E]]
    for k, what in enumerate(("iptr_i", "ilist_i", "iptr_j", "ilist_j")):
        assert np.array_equal(got[k], want[k].cpu().numpy()), (name, what, "EdgeLayout")
        assert np.array_equal(got[k], g["twin"][k]), (name, what, "twin")
    # two runs, the same bits
    again = run_entry(g["ei"], g["lay"].mol_ptr, N, g["B"], max(g["sizes"]))
    assert all(np.array_equal(a, b) for a, b in zip(got, again[1:5]))


@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_capacity_form_equals_the_exact_form(name):
    g = graph(name)
    E, N = g["E"], g["N"]
    E_cap, N_cap = E + 1000, N + 300
    rc, *exact, st0 = run_entry(g["ei"], g["lay"].mol_ptr, N, g["B"], max(g["sizes"]))
    # (the grid is sized by the capacity's largest structure, as a bucket would)
    rc1, *cap, st1 = run_entry(g["ei"], g["lay"].mol_ptr, N, g["B"], min(1024, N_cap), E_cap=E_cap, N_cap=N_cap,
                               dyn=(E, N))
    assert rc == rc1 == 0 and st0 == st1 == 0
    for k in (0, 2):
        assert np.array_equal(cap[k][:N + 1], exact[k])
        assert np.all(cap[k][N:] == E)                       # the tail atoms: empty lists at E
        assert np.array_equal(cap[k + 1][:E], exact[k + 1][:E])
        assert np.all(cap[k + 1][E:] == POISON)              # nothing at or beyond E is written


def test_dyn_count_above_the_capacity_sets_the_status():
    g = graph("B")
    E, N = g["E"], g["N"]
    rc, *_, status = run_entry(g["ei"], g["lay"].mol_ptr, N, g["B"], max(g["sizes"]), E_cap=E, N_cap=N, dyn=(E + 5, N))
    assert rc == 0 and status == 1
    rc, *_, status = run_entry(g["ei"], g["lay"].mol_ptr, N, g["B"], max(g["sizes"]), E_cap=E, N_cap=N, dyn=(E, N))
    assert rc == 0 and status == 0


def test_structures_in_the_wrong_order_set_the_status():
    g = graph("B")
    ei = g["ei"]
    first = int((ei[0] < g["sizes"][0]).sum())
    swapped = torch.cat([ei[:, first:], ei[:, :first]], dim=1).contiguous()
    assert itw.layout_twin(swapped.cpu().numpy(), g["sizes"])[4] == 1
    rc, *_, status = run_entry(swapped, g["lay"].mol_ptr, g["N"], g["B"], max(g["sizes"]))
    assert rc == 0 and status == 1


def test_an_edge_that_leaves_its_structure_is_dropped():
    g = graph("A")
    ei = g["ei"].clone()
    e = 1000
    assert int(ei[0, e]) < 300
    ei[1, e] = 301
    twin = itw.layout_twin(ei.cpu().numpy(), g["sizes"])
    assert twin[4] == 1
    rc, *got, status = run_entry(ei, g["lay"].mol_ptr, g["N"], g["B"], max(g["sizes"]))
    assert rc == 0 and status == 1
    for k in range(4):
        assert np.array_equal(got[k], twin[k])


def test_refusals_and_the_empty_list():
    from geossl_amd import ops
    from geossl_amd.layout import MolLayout
    g = graph("A")
    # a structure of 1025 atoms: refused by its host size, in C and in Python
    sizes = [1025]
    batch = torch.zeros(1025, dtype=torch.long, device=DEV)
    lay = MolLayout(batch, sizes=sizes)
    ei = torch.stack([torch.arange(1, 1025, device=DEV), torch.arange(0, 1024, device=DEV)])
    rc, *got, status = run_entry(ei, lay.mol_ptr, 1025, 1, 1025)
    assert rc == INVALID and all(np.all(o == POISON) for o in got)
    with pytest.raises(ValueError, match="1024"):
        ops.painn_incidence_layout(ei, lay.mol_ptr, 1025, 1, 1025)
    # ... and one that is larger than the host said gets no edges and sets the status
    rc, *got, status = run_entry(ei, lay.mol_ptr, 1025, 1, 1024)
    assert rc == 0 and status == 1
    # E above INT_MAX (no memory is touched: refused on the host)
    from geossl_amd import _lib
    assert _lib.load().geossl_painn_incidence_layout(None, None, 2 ** 31, None, 10, 1, 10, None, None, None, None, None,
                                                     None, _lib.stream()) == INVALID
    # E = 0: every list is empty
    none = torch.zeros((2, 0), dtype=torch.int64, device=DEV)
    rc, iptr_i, ilist_i, iptr_j, ilist_j, status = run_entry(none, g["lay"].mol_ptr, g["N"], g["B"], max(g["sizes"]))
    assert rc == 0 and status == 0 and np.all(iptr_i == 0) and np.all(iptr_j == 0)
    assert np.all(ilist_i == POISON) and np.all(ilist_j == POISON)


def test_python_wrapper_writes_into_given_buffers():
    from geossl_amd import ops
    g = graph("B")
    E, N = g["E"], g["N"]
    got = ops.painn_incidence_layout(g["ei"], g["lay"].mol_ptr, N, g["B"], max(g["sizes"]))
    torch.cuda.synchronize()
    assert int(got[4].item()) == 0
    for k in range(4):
        assert np.array_equal(got[k].cpu().numpy()[:(E if k % 2 else N + 1)], g["twin"][k])


# ------------------------------------------------------------------------------- 3. replay equals eager (Supervised)
TOL_LOSS, TOL_GRAD = 1e-6, 1e-5     # the replay-vs-eager bounds of test_gpu_sparse_bucket.py


@pytest.fixture
def switch_on(monkeypatch):
    monkeypatch.setenv("GEOSSL_PAINN_SPARSE_BUCKETS", "1")
    monkeypatch.delenv("GEOSSL_SPARSE_BUCKETS", raising=False)
    monkeypatch.delenv("GEOSSL_SPARSE_PAIRS", raising=False)
    monkeypatch.delenv("GEOSSL_PAINN_TILE", raising=False)


def _painn():
    import test_gpu_supervised as sup
    model = backbone("painn")
    return model, sup._head("painn", model)


def _batch(name, T=1):
    """A collated PaiNN batch of a size set: 2-D x, the radius graph at 5 A, host sizes; y [B * T]."""
    from geossl_amd import pretrain_GeoSSL as pg
    from helpers import t
    g = graph(name)
    sizes = g["sizes"]
    b = pg.Batch(t(g["x"], DEV)[:, None].contiguous(), g["pos"], g["batch_t"], None, radius_edge_index=g["ei"],
                 num_graphs=len(sizes), sizes=sizes)
    y = np.random.default_rng(11 + sum(sizes)).standard_normal(len(sizes) * T).astype(np.float32)
    b.y = t(y, DEV)
    return b


def _sup_trainer(model, head):
    from geossl_amd.pretrain_Supervised import SupervisedTrainer
    return SupervisedTrainer(model, head, 0.0, 1.0, task_id=0, loss="mse", lr=0.0, model_3d="painn", use_graph=True,
                             graph_mode="auto")


def _grads(tr):
    return [p.grad.clone() for m in (tr.model, tr.head) for p in m.parameters() if p.grad is not None]


def _eager(tr, b):
    lo = tr._eager(b)
    return lo.clone(), _grads(tr)


def _replay(tr, b):
    lo = tr._graph_fwd_bwd(b)
    return lo.clone(), _grads(tr)


def _assert_close(got, ref, what):
    from conftest import rel_err
    (lg, gg), (lr_, gr) = got, ref
    e = rel_err(lg.cpu(), lr_.cpu())
    worst = max(rel_err(a, c) for a, c in zip(gg, gr))
    print("%s: loss %.2e worst gradient %.2e" % (what, e, worst))
    assert len(gg) == len(gr) and len(gg) > 0
    assert e < TOL_LOSS, what
    assert worst < TOL_GRAD, what


def test_replay_equals_eager_and_leaves_no_stale_row(switch_on):
    model, head = _painn()
    tr = _sup_trainer(model, head)
    batches = [_batch("A"), _batch("B"), _batch("A")]
    ref = [_eager(tr, b) for b in batches]
    got = [_replay(tr, b) for b in batches]
    for k, (g_, r_) in enumerate(zip(got, ref)):
        _assert_close(g_, r_, "batch %d" % k)
    sg = tr.step_graphs
    assert len(sg) == 1 and sg.captures == 1 and next(iter(sg.graphs)) == ("bucket", 4, "sparse")
    bkt = next(iter(sg.graphs.values()))["bucket"]
    assert bkt.kind == "painn" and bkt.E_cap >= graph("A")["E"] and bkt.big_caps == ()
    torch.cuda.synchronize()
    assert int(bkt.el.status.item()) == 0
    # the two A steps, with a smaller batch in between: bitwise equal
    assert torch.equal(got[0][0], got[2][0])
    for a, c in zip(got[0][1], got[2][1]):
        assert torch.equal(a, c)
    # BIG outgrows the bucket: captured again
    big = _batch("BIG")
    ref = _eager(tr, big)
    _assert_close(_replay(tr, big), ref, "outgrown")
    assert sg.captures == 2 and len(sg) == 1
    bkt = next(iter(sg.graphs.values()))["bucket"]
    assert bkt.max_n == 1024 and bkt.N_cap >= sum(SIZES_BIG) and bkt.E_cap >= graph("BIG")["E"]


# ----------------------------------------------------------------------------------------------- 4. DeviceLoader handles
def _pocket_dataset():
    """16 pockets of 40 .. 320 atoms, four of them above 255, with radius edges built by the dataset and two targets."""
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    rng = np.random.default_rng(9)
    sizes = np.concatenate([rng.integers(256, 321, size=4), rng.integers(40, 121, size=12)])
    sizes[0], sizes[4] = 320, 40
    pos = np.concatenate([ls.molecule(int(n), 4, k) for k, n in enumerate(sizes)])
    x = np.stack([(np.arange(pos.shape[0], dtype=np.int64) * 5 % 8) + 1, np.zeros(pos.shape[0], dtype=np.int64)], axis=1)
    y = rng.standard_normal((16, 2)).astype(np.float32)
    return DeviceDataset(x, pos, sizes, DEV, radius=CUTOFF, y=y), sizes, y


class _Quarters:
    """An epoch order in which every batch of four holds one of the four pockets above 255 atoms (ids 0 .. 3)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def batches(self):
        big, small = self.rng.permutation(4), 4 + self.rng.permutation(12)
        return [self.rng.permutation(np.concatenate([[big[k]], small[3 * k:3 * k + 3]])) for k in range(4)]


def test_device_loader_handles_share_one_bucket_graph(switch_on):
    from geossl_amd import ops
    ds, sizes, y = _pocket_dataset()
    # the dataset's own edges of a 320-atom pocket are the radius graph of its positions
    o = ds.off
    ei0 = ops.radius_graph(ds.positions[:o[1]].contiguous(), CUTOFF)
    assert int(sizes[0]) == 320 and torch.equal(ds.edges[:, :int(ds.edge_cnt[0])], ei0)
    model, head = _painn()
    from geossl_amd.pretrain_Supervised import SupervisedTrainer
    tr = SupervisedTrainer(model, head, 0.25, 1.5, task_id=1, loss="mse", lr=0.0, model_3d="painn", use_graph=True)
    order = _Quarters(3)
    for epoch in range(2):
        for k, ids in enumerate(order.batches()):
            hb = ds.batch(ids)
            assert sizes[ids].max() > 255 and hb.n_edges == int(ds.edge_cnt[ids].sum())
            ref = _eager(tr, hb)                                         # (on the handle's materialised batch)
            _assert_close(_replay(tr, hb), ref, "epoch %d handle %d" % (epoch, k))
    sg = tr.step_graphs
    assert len(sg) == 1 and next(iter(sg.graphs)) == ("bucket", 4, "sparse") and sg.captures == 1


def test_datasets_above_1024_atoms_are_refused():
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    n = 1025
    pos = np.random.default_rng(1).uniform(0, 30, size=(n, 3)).astype(np.float32)
    with pytest.raises(ValueError, match="1024"):
        DeviceDataset(np.ones(n, dtype=np.int64), pos, [n], DEV, radius=CUTOFF)


# -------------------------------------------------------------------------------------------------------------- 5. LEP
LEP_A = ((300, 2, 64, 1), (33, 257, 129, 5))
LEP_B = ((260, 40, 17, 3), (1, 5, 64, 3))


def _lep_modules():
    from helpers import fill_module_
    model = backbone("painn")
    head = fill_module_(torch.nn.Linear(256, 1)).to(DEV)
    with torch.no_grad():
        head.weight.mul_(0.05)   # (logits of order one with the filler's weights: no sigmoid saturates)
    return model, head


def _lep_trainer(model, head):
    from geossl_amd.finetune_lep import LEPTrainer
    return LEPTrainer(model, head, lr=0.0, model_3d="painn", use_graph=True)


def test_lep_pair_handles_share_one_bucket_graph(switch_on):
    import test_gpu_lep_bucket as lb
    from geossl_amd.Geom3D.dataloaders import PairedDeviceDataset
    items = lb._items(LEP_A, 0, y=[1, 0, 0, 1]) + lb._items(LEP_B, 1, y=[0, 1, 1, 0])
    ds = PairedDeviceDataset.from_data_list(items, DEV, radius=CUTOFF)
    assert ds.structures.edges is not None and len(ds) == 8
    model, head = _lep_modules()
    tr = _lep_trainer(model, head)
    rng = np.random.default_rng(2)
    seen = []
    for k in range(4):     # shuffled pairs of B = 4: pair 0, 1 or 4 (a structure above 255 atoms) in every batch
        ids = rng.permutation(np.concatenate([[0, 1, 4, 0][k:k + 1], rng.choice([2, 3, 5, 6, 7], size=3, replace=False)]))
        hb = ds.batch(ids)
        assert hb.radius_edge_index_active.size(1) + hb.radius_edge_index_inactive.size(1) == hb.fused().n_edges
        assert int(hb.radius_edge_index_inactive.min()) >= 0
        assert int(hb.radius_edge_index_inactive.max()) < hb.positions_inactive.size(0)
        ref = _eager(tr, hb)
        _assert_close(_replay(tr, hb), ref, "pairs %d" % k)
        seen.append(tuple(hb.y.cpu().tolist()))
    sg = tr.step_graphs
    assert len(set(seen)) >= 2                                           # (label sets differ: data of the one graph)
    assert len(sg) == 1 and sg.captures == 1 and next(iter(sg.graphs)) == ("bucket", 8, "sparse")
    # B = 1 keeps the reference's error; a dataset without radius keeps the "radius edges" error
    with pytest.raises(ValueError):
        tr.step(ds.batch([0]))
    plain = PairedDeviceDataset.from_data_list(items, DEV)
    with pytest.raises(ValueError, match="radius edges"):
        tr.step(plain.batch(np.arange(4)))
    assert plain.batch(np.arange(4)).radius_edge_index_active is None


# ---------------------------------------------------------------------------------------------------------- 7. routing
def test_switch_table_and_what_keeps_its_route(monkeypatch):
    from geossl_amd import bucket as bk
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    from geossl_amd.switches import PAINN_SPARSE_BUCKETS_DEFAULT
    for k in ("GEOSSL_PAINN_SPARSE_BUCKETS", "GEOSSL_SPARSE_BUCKETS", "GEOSSL_SPARSE_PAIRS", "GEOSSL_PAINN_TILE"):
        monkeypatch.delenv(k, raising=False)
    ds, sizes, _ = _pocket_dataset()
    hb, b = ds.batch([0, 5, 6, 7]), _batch("A")
    model, head = _painn()
    sg = _sup_trainer(model, head).step_graphs
    key = ("bucket", 4, "sparse")
    assert sg.bucket_key(b) is None and sg.bucket_key(hb) == (key if PAINN_SPARSE_BUCKETS_DEFAULT else None)
    monkeypatch.setenv("GEOSSL_SPARSE_BUCKETS", "1")                    # (SchNet's switch does not open this bucket)
    assert sg.bucket_key(b) is None
    monkeypatch.delenv("GEOSSL_SPARSE_BUCKETS")
    monkeypatch.setenv("GEOSSL_PAINN_SPARSE_BUCKETS", "0")
    assert sg.bucket_key(b) is None and sg.bucket_key(hb) is None
    monkeypatch.setenv("GEOSSL_PAINN_SPARSE_BUCKETS", "1")
    assert sg.bucket_key(b) == key and sg.bucket_key(hb) == key
    # no kernel takes the bucket's layout without the atom-tile route
    monkeypatch.setenv("GEOSSL_PAINN_TILE", "0")
    assert sg.bucket_key(b) is None
    monkeypatch.delenv("GEOSSL_PAINN_TILE")
    # a dense batch keeps the dense bucket; a handle of a dataset without radius edges has no PaiNN bucket
    dense = ds.batch([4, 5, 6, 7])
    assert sizes[[4, 5, 6, 7]].max() <= 255 and sg.bucket_key(dense) == ("bucket", 4, "combination")
    bare = DeviceDataset(ds.x, ds.positions, sizes, DEV)
    assert sg.bucket_key(bare.batch([0, 5, 6, 7])) is None
    # SchNet's sparse bucket is not this switch's
    import test_gpu_supervised as sup
    schnet = backbone("schnet")
    from geossl_amd.pretrain_Supervised import SupervisedTrainer
    ssg = SupervisedTrainer(schnet, sup._head("schnet", schnet), 0.0, 1.0, task_id=0, loss="mse", use_graph=True).step_graphs
    assert ssg.bucket_key(b) is None and ssg.bucket_key(hb) == key
    # engines that read pair tuples keep their routes
    from geossl_amd.pretrain_DistancePrediction import DistancePredictionTrainer, DistancePredictor
    from helpers import fill_module_
    dist = DistancePredictionTrainer(model, fill_module_(DistancePredictor(128)).to(DEV), model_3d="painn", use_graph=True)
    assert dist.step_graphs.pair_tuples and dist.step_graphs.bucket_key(hb) is None
    # a masked batch above 255 atoms is refused by the bucket with a sentence
    bkt = bk.Bucket.for_batch(hb, bk.SPARSE, "painn", 1)
    masked = ds.batch([0, 5, 6, 7])
    masked._mask = object()
    with pytest.raises(ValueError, match="unmasked"):
        bkt.fill(masked)


# --------------------------------------------------------------------- 2. the tile kernels under dyn_nlist, bucket lists
@pytest.mark.parametrize("mu_given", [True, False], ids=["mu", "mu0"])
def test_tile_kernels_with_the_bucket_lists_under_dyn_nlist(mu_given):
    """The lists as a bucket holds them (capacity form of the layout entry: 96 atoms of 133, E edges of E + 100) and
    nlist = the atom capacity with the real count in memory: an atom's outputs do not depend on nlist, so q, mu, dxc and
    dmu_in are the eager tile route's bit for bit; the filter gradient's block partials follow the grid, so dWf / dbf
    get the bound of tests/painn_tile_twin.py against the fp64 twin."""
    import types
    import painn_tile_twin as tw
    import test_gpu_painn_tile as pt
    from elementwise import assert_within
    from geossl_amd import ops
    R, N, N_cap = 20, pt.N_ATOMS, pt.N_ATOMS + 37
    mol_ptr = torch.tensor([0, N], dtype=torch.int32, device=DEV)
    dyn_N = torch.tensor([N], dtype=torch.int32, device=DEV)
    for transposed in (False, True):
        c = pt._case(R, mu_given, transposed)
        E = c["E"]
        E_cap = E + 100
        rei = torch.zeros(2, E_cap, dtype=torch.int64, device=DEV)
        rei[:, :E] = c["ei"]
        outs = (torch.full((N_cap + 1,), POISON, dtype=torch.int64, device=DEV),
                torch.full((E_cap,), POISON, dtype=torch.int32, device=DEV),
                torch.full((N_cap + 1,), POISON, dtype=torch.int64, device=DEV),
                torch.full((E_cap,), POISON, dtype=torch.int32, device=DEV))
        dyn_E = torch.tensor([E], dtype=torch.int32, device=DEV)
        *_, status = ops.painn_incidence_layout(rei, mol_ptr, N_cap, 1, 256, out=outs, dyn_E=dyn_E, dyn_N=dyn_N)
        assert int(status.item()) == 0
        for side, k in (("i", 0), ("j", 2)):
            assert torch.equal(outs[k][:N + 1], c["el"].inc[side][0]) and torch.equal(outs[k + 1][:E], c["el"].inc[side][1][:E])
        c2 = dict(c)
        c2["el"] = types.SimpleNamespace(idx_i=rei[0], idx_j=rei[1], inc={"i": outs[0:2], "j": outs[2:4]})
        if not transposed:
            base, got = pt._fwd(c)[:2], pt._fwd(c2, nlist=N_cap, dyn=dyn_N)[:2]
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
        else:
            base, got = pt._bwd(c), pt._bwd(c2, nlist=N_cap, dyn=dyn_N)
            assert torch.equal(got[0], base[0])
            assert (got[1] is None and base[1] is None and not mu_given) or torch.equal(got[1], base[1])
            ref = pt._twin_bwd(c, (R, mu_given, True), 1.0)
            assert_within(got[2].cpu(), *ref["dWf"], tw.C_WGRAD, tw.U, "dWf under dyn_nlist")
            assert_within(got[3].cpu(), *ref["dbf"], tw.C_WGRAD, tw.U, "dbf under dyn_nlist")


# ------------------------------------------------------------------------------------------- 6. the reference's fixtures
def test_g24_painn_through_a_handle(switch_on):
    """Fixture G24 (finetune_lba.py's step on PaiNN) from a DeviceDataset that builds its radius edges itself - they are
    the fixture's, entry for entry - through the trainer's bucket graph and through do_Supervised's engine."""
    import types
    import test_gpu_lba as lba
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    from geossl_amd.pretrain_Supervised import SupervisedTrainer, do_Supervised
    assert lba.TOL_OUT == 1e-5 and lba.TOL_GRAD == 1e-4
    case = "g24_lba_painn"
    g, meta, model, head, make, args = lba._setup(case)
    assert sorted(int(n) for n in g["sizes"]) == [7, 257, 300]
    ds = DeviceDataset(g["x"], g["positions"], g["sizes"], DEV, radius=float(meta["cutoff"]), y=g["y"])
    assert torch.equal(ds.edges.cpu(), torch.from_numpy(g["radius_edge_index"].astype(np.int64)))
    hb = ds.batch(np.arange(3))
    tr = SupervisedTrainer(model, head, 0.0, 1.0, task_id=0, loss="mse", lr=0.0, model_3d="painn", use_graph=True)
    for _ in range(2):
        loss = tr._graph_fwd_bwd(hb)
    sg = tr.step_graphs
    assert list(sg.graphs) == [("bucket", 3, "sparse")] and sg.captures == 1
    lba._check(g, model, head, loss, case)
    # predict / eval stay eager, on the handle's materialised batch
    from conftest import rel_err
    assert rel_err(tr.predict(hb).cpu(), g["pred"]) < lba.TOL_OUT and sg.captures == 1
    # do_Supervised on a handle: the same route through its engine, the reference's loss.backward()
    _, _, model2, head2, _, _ = lba._setup(case)
    loss2 = do_Supervised(types.SimpleNamespace(model_3d="painn", loss="mse"), ds.batch(np.arange(3)), model2, head2, 0.0,
                          1.0, task_id=0)
    loss2.backward()
    lba._check(g, model2, head2, loss2, case)
    eng = model2.__dict__["_geossl_supervised_step"]
    assert [k for sg_ in eng.graphs.values() for k in sg_.graphs] == [("bucket", 3, "sparse")]


def test_g25_painn_through_a_pair_handle(switch_on):
    import lep_twin as lt
    import test_gpu_lep as gl
    from geossl_amd.finetune_lep import LEPTrainer, do_LEP
    from geossl_amd.Geom3D.dataloaders import PairedDeviceDataset
    assert gl.TOL_OUT == 1e-5 and gl.TOL_GRAD == 1e-4
    case = "g25_lep_painn"
    g, meta, model, head, make, args = gl._setup(case)
    ds = PairedDeviceDataset.from_data_list(lt.fixture_items(g), DEV, radius=float(meta["cutoff"]))
    B = len(ds)
    hb = ds.batch(np.arange(B))
    for side in ("active", "inactive"):     # the dataset's own edges are the fixture's collated ones
        want = torch.from_numpy(g["batch/radius_edge_index_" + side].astype(np.int64))
        assert torch.equal(getattr(hb, "radius_edge_index_" + side).cpu(), want)
    tr = LEPTrainer(model, head, lr=0.0, model_3d="painn", use_graph=True)
    for _ in range(2):
        loss = tr._graph_fwd_bwd(hb)
    sg = tr.step_graphs
    assert list(sg.graphs) == [("bucket", 2 * B, "sparse")] and sg.captures == 1
    gl._check(g, model, head, loss, case)
    from conftest import rel_err
    assert rel_err(tr.predict(hb).cpu(), g["pred"]) < gl.TOL_OUT and sg.captures == 1
    _, _, model2, head2, _, _ = gl._setup(case)
    loss2 = do_LEP(args, ds.batch(np.arange(B)), model2, head2, torch.nn.BCEWithLogitsLoss())
    loss2.backward()
    gl._check(g, model2, head2, loss2, case)
    eng = model2.__dict__["_geossl_lep_step"]
    assert [k for sg_ in eng.graphs.values() for k in sg_.graphs] == [("bucket", 2 * B, "sparse")]
