"""GPU tests of the sparse capacity bucket (geossl_amd/bucket.py, option "sparse"; LBA's pockets replayed from one graph
per batch size): the `_dyn` build and aggregation of csrc/sparse_pairs.hip against the exact entries bit for bit, bucket
replay against the eager step on ragged batches of 256+ atom structures (stale rows, an outgrown bucket), fixture G24
through the bucket, DeviceLoader handles of a dataset built from a 1-D x, GEOSSL_SPARSE_PAIRS / GEOSSL_SPARSE_BUCKETS,
and the steps that keep their routing.  Collated batches take the bucket with GEOSSL_SPARSE_BUCKETS=1 (the `collated`
fixture), DeviceLoader handles by default."""
import numpy as np
import pytest
import torch

import lba_structures as ls
from conftest import rel_err
from helpers import t
from objective_harness import backbone, replay_vs_eager

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CUTOFF = 10.0
A, B_, C_ = (300, 2, 64, 1), (33, 257, 129, 5), (260, 40, 17, 3)
BIG = (600, 300, 280, 257)
TOL_LOSS, TOL_GRAD = 1e-6, 1e-5     # the bounds of test_gpu_supervised._replay_vs_eager (dense buckets)

_STRUCT = {}


@pytest.fixture
def collated(monkeypatch):
    """The sparse bucket for collated batches: off unless the switch says 1."""
    monkeypatch.setenv("GEOSSL_SPARSE_BUCKETS", "1")


def _structures(sizes, seed=0):
    key = (tuple(sizes), seed)
    if key not in _STRUCT:
        _STRUCT[key] = ls.structures(sizes, seed)
    return _STRUCT[key]


def _batch(sizes, seed=0, T=1):
    """A collated LBA-style batch: 1-D atom types, no pair tuples, host sizes; y [B * T]."""
    from geossl_amd import pretrain_GeoSSL as pg
    s = _structures(sizes, seed)
    b = pg.Batch(t(s["x"], DEV), t(s["positions"], DEV), t(s["batch"], DEV), None, num_graphs=len(sizes), sizes=sizes)
    y = np.random.default_rng(7 + seed + sum(sizes)).standard_normal(len(sizes) * T).astype(np.float32)
    b.y = t(y, DEV)
    return b


def _modules():
    import test_gpu_supervised as sup
    model = backbone("schnet")
    return model, sup._head("schnet", model)


def _trainer(model, head, **kw):
    from geossl_amd.pretrain_Supervised import SupervisedTrainer
    return SupervisedTrainer(model, head, 0.0, 1.0, task_id=0, loss="mse", lr=0.0, use_graph=True, graph_mode="auto", **kw)


def _grads(tr):
    return [p.grad.clone() for m in (tr.model, tr.head) for p in m.parameters() if p.grad is not None]


def _assert_close(got, ref, what):
    (lg, gg), (lr_, gr) = got, ref
    e = rel_err(lg.cpu(), lr_.cpu())
    worst = max(rel_err(a, c) for a, c in zip(gg, gr))
    print("%s: loss %.2e worst gradient %.2e" % (what, e, worst))
    assert len(gg) == len(gr) and len(gg) > 0
    assert e < TOL_LOSS, what
    assert worst < TOL_GRAD, what


def _bucket_keys(tr):
    return [k for k in tr.step_graphs.graphs if k[0] == "bucket"]


# --------------------------------------------------------------------------------------------- 1. the build
def _raw_build(pos, mol_ptr, B, N, max_n, P, dyn=None):
    """geossl_sparse_pairs_build[_dyn] through the C ABI on poisoned outputs."""
    from geossl_amd import _lib
    from geossl_amd._lib import ptr, stream
    i32 = dict(dtype=torch.int32, device=DEV)
    o = dict(pair_i=torch.full((P,), -7, **i32), pair_j=torch.full((P,), -7, **i32),
             pair_d=torch.full((P,), NAN, device=DEV), pair_c=torch.full((P,), NAN, device=DEV),
             pair_flag=torch.full((P,), 77, dtype=torch.uint8, device=DEV), inc_ptr=torch.full((N + 1,), -7, **i32),
             inc_pair=torch.full((2 * P,), -7, **i32), inc_src=torch.full((2 * P,), -7, **i32),
             n_pairs=torch.full((1,), -7, **i32))
    work = torch.full((B + 2 * N,), -7, **i32)
    r2 = float(torch.tensor(CUTOFF * CUTOFF, dtype=torch.float32))
    args = (ptr(pos), ptr(mol_ptr), B, N, max_n, r2, 33, CUTOFF, P, ptr(work), ptr(work[B:]), ptr(work[B + N:]),
            ptr(o["pair_i"]), ptr(o["pair_j"]), ptr(o["pair_d"]), ptr(o["pair_c"]), ptr(o["pair_flag"]), ptr(o["inc_ptr"]),
            ptr(o["inc_pair"]), ptr(o["inc_src"]), ptr(o["n_pairs"]))
    if dyn is None:
        _lib.call("geossl_sparse_pairs_build", *args, stream())
    else:
        _lib.call("geossl_sparse_pairs_build_dyn", *args, ptr(dyn), stream())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("sizes", [A, B_], ids=["300_2_64_1", "33_257_129_5"])
def test_dyn_build_equals_the_exact_build(sizes):
    s = _structures(sizes)
    N, B, hi = int(sum(sizes)), len(sizes), max(sizes)
    N_cap = N + 37
    mol_ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)
    pos = t(s["positions"], DEV)
    ref = _raw_build(pos, mol_ptr, B, N, hi, ls.pair_capacity(sizes))
    pos_cap = torch.cat([pos, torch.full((N_cap - N, 3), NAN, device=DEV)])
    dims = torch.tensor([N], dtype=torch.int32, device=DEV)
    P_cap = 33 * N_cap
    got = _raw_build(pos_cap, mol_ptr, B, N_cap, 512, P_cap, dyn=dims)
    n = int(ref["n_pairs"])
    assert 0 < n <= ls.pair_capacity(sizes) and int(got["n_pairs"]) == n
    for k in ("pair_i", "pair_j", "pair_d", "pair_c", "pair_flag"):
        assert torch.equal(got[k][:n], ref[k][:n]), k
    assert torch.equal(got["inc_ptr"][:N + 1], ref["inc_ptr"][:N + 1])
    assert torch.all(got["inc_ptr"][N + 1:] == -7)                      # nothing past the real atoms is written
    m = int(ref["inc_ptr"][N])
    assert m == 2 * n
    assert torch.equal(got["inc_pair"][:m], ref["inc_pair"][:m]) and torch.equal(got["inc_src"][:m], ref["inc_src"][:m])
    # rows from n_pairs to the capacity: the documented fill
    assert torch.all(got["pair_flag"][n:] == 0) and torch.all(got["pair_i"][n:] == 0) and torch.all(got["pair_j"][n:] == 0)
    assert torch.all(got["pair_c"][n:] == 0) and torch.all(got["pair_d"][n:] == CUTOFF)


# ---------------------------------------------------------------------------------------- 2. the aggregation
@pytest.mark.parametrize("swap", [False, True])
def test_dyn_aggregation_equals_the_exact_one(swap, monkeypatch):
    from geossl_amd import _lib, ops
    from geossl_amd._lib import ptr, stream
    from geossl_amd.layout import MolLayout
    sizes, F = A, 128
    s = _structures(sizes)
    N = int(sum(sizes))
    assert N % 4 != 0                                                    # a block of four waves straddles the real count
    N_cap = N + 37
    lay = MolLayout(t(s["batch"], DEV), len(sizes), sizes=list(sizes))
    assert lay.sparse
    sp = ops.sparse_pair_geometry(t(s["positions"], DEV), lay, CUTOFF)
    n = int(sp.n_pairs.item())
    g = torch.Generator(device=DEV).manual_seed(11 + swap)
    x = torch.full((N_cap, F), NAN, device=DEV)
    x[:N] = torch.randn(N, F, device=DEV, generator=g)
    W = torch.full((sp.P, F), NAN, device=DEV)
    W[:n] = torch.randn(n, F, device=DEV, generator=g)
    ref = ops.aggregate_sparse(x[:N].contiguous(), W, sp, swap=swap, out=torch.full((N, F), NAN, device=DEV))
    out = torch.full((N_cap, F), 123.0, device=DEV)
    dims = torch.tensor([N], dtype=torch.int32, device=DEV)
    _lib.call("geossl_cfconv_aggregate_sparse_dyn", ptr(x), ptr(W), ptr(sp.inc_ptr), ptr(sp.inc_pair), ptr(sp.inc_src),
              N_cap, F, 1 if swap else 0, ptr(out), ptr(dims), stream())
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all() and torch.equal(out[:N], ref)
    assert torch.all(out[N:] == 123.0)                                   # the sentinel rows are untouched


# ------------------------------------------------------------------------------------------------ 3. replay
def _eager_all(tr, batches):
    out = []
    for b in batches:
        lo = tr._eager(b)
        out.append((lo.clone(), _grads(tr)))
    return out


def test_replay_equals_eager_and_leaves_no_stale_row(collated):
    model, head = _modules()
    tr = _trainer(model, head)
    batches = [_batch(A), _batch(B_), _batch(C_), _batch(A)]
    ref = _eager_all(tr, batches)
    got = []
    for b in batches:
        lo = tr._graph_fwd_bwd(b)
        got.append((lo.clone(), _grads(tr)))
    for k, (g_, r_) in enumerate(zip(got, ref)):
        _assert_close(g_, r_, "batch %d" % k)
    sg = tr.step_graphs
    assert len(sg) == 1 and next(iter(sg.graphs))[0] == "bucket" and sg.captures == 1
    assert next(iter(sg.graphs)) == ("bucket", 4, "sparse")
    # the two A steps, with a smaller batch in between: bitwise equal
    assert torch.equal(got[0][0], got[3][0])
    for a, c in zip(got[0][1], got[3][1]):
        assert torch.equal(a, c)


# --------------------------------------------------------------------------------------- 4. outgrown bucket
def test_outgrown_bucket_is_captured_again(collated):
    model, head = _modules()
    tr = _trainer(model, head)
    small, big = _batch(C_), _batch(BIG)
    ref = _eager_all(tr, [big])[0]
    tr._graph_fwd_bwd(small)
    bkt = next(iter(tr.step_graphs.graphs.values()))["bucket"]
    assert bkt.max_n == 512 and bkt.N_cap < sum(BIG)
    lo = tr._graph_fwd_bwd(big)
    got = (lo.clone(), _grads(tr))
    sg = tr.step_graphs
    assert sg.captures == 2 and len(sg) == 1
    bkt = next(iter(sg.graphs.values()))["bucket"]
    assert bkt.max_n == 1024 and bkt.N_cap >= sum(BIG) and bkt.P_cap == 33 * bkt.N_cap
    _assert_close(got, ref, "outgrown")


# ------------------------------------------------------------------------------------------ 5. reference pin
def test_g24_through_the_bucket(collated):
    import test_gpu_lba as lba
    from geossl_amd.pretrain_Supervised import SupervisedTrainer
    case = "g24_lba_schnet_full"
    g, meta, model, head, make, args = lba._setup(case)
    assert sorted(int(n) for n in g["sizes"]) == [40, 260] and g["x"].ndim == 1
    tr = SupervisedTrainer(model, head, 0.0, 1.0, task_id=0, loss="mse", lr=0.0, model_3d="schnet", use_graph=True,
                           graph_mode="auto")
    b = make()
    for _ in range(2):
        loss = tr._graph_fwd_bwd(b)
    assert _bucket_keys(tr) == [("bucket", 2, "sparse")] and len(tr.step_graphs) == 1
    assert lba.TOL_OUT == 1e-5 and lba.TOL_GRAD == 1e-4
    lba._check(g, model, head, loss, case)


# ------------------------------------------------------------------------------------------- 6. DeviceLoader
def _pocket_dataset():
    """24 pockets with 30 to 320 atoms (eight above 255) and two target columns, from a 1-D x."""
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    rng = np.random.default_rng(5)
    sizes = np.concatenate([rng.integers(256, 321, size=8), rng.integers(30, 121, size=16)])
    sizes[0], sizes[8] = 320, 30
    sizes = sizes[rng.permutation(24)]
    pos = np.concatenate([ls.molecule(int(n), 3, k) for k, n in enumerate(sizes)])
    x = (np.arange(pos.shape[0], dtype=np.int64) * 5 % 8) + 1
    y = rng.standard_normal((24, 2)).astype(np.float32)
    return DeviceDataset(x, pos, sizes, DEV, y=y), sizes, y


def _handles(ds, sizes):
    """Four handles of a shuffled epoch, each with a structure above 255 atoms (the first loader seed that gives them:
    a batch without one has a dense layout and keeps its own routing)."""
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    for seed in range(64):
        loader = DeviceLoader(ds, batch_size=4, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(seed))
        hbs = [hb for _, hb in zip(range(4), loader)]
        if all(sizes[hb.ids].max() > 255 for hb in hbs):
            return hbs
    raise AssertionError("no loader seed in range(64) gives four batches with a structure above 255 atoms")


def test_device_loader_handles_share_one_bucket_graph(monkeypatch):
    monkeypatch.delenv("GEOSSL_SPARSE_BUCKETS", raising=False)          # (the default serves handles)
    ds, sizes, y = _pocket_dataset()
    assert ds.x_cols == 1 and tuple(ds.x.shape) == (int(sizes.sum()), 1)
    hbs = _handles(ds, sizes)
    model, head = _modules()
    from geossl_amd.pretrain_Supervised import SupervisedTrainer
    tr = SupervisedTrainer(model, head, 0.25, 1.5, task_id=1, loss="mse", lr=0.0, use_graph=True, graph_mode="auto")
    for k, hb in enumerate(hbs):
        assert torch.equal(hb.y.cpu(), torch.from_numpy(y[hb.ids]).reshape(-1))
        lo = tr._eager(hb)                                               # (on the handle's collated tensors)
        ref = (lo.clone(), _grads(tr))
        lo = tr._graph_fwd_bwd(hb)
        _assert_close((lo.clone(), _grads(tr)), ref, "handle %d" % k)
    sg = tr.step_graphs
    assert len(sg) == 1 and next(iter(sg.graphs)) == ("bucket", 4, "sparse")
    (gg,) = sg.graphs.values()
    assert torch.equal(gg["noise"]["target"].cpu(), torch.from_numpy(y[hbs[-1].ids, 1]))


def test_do_supervised_takes_the_same_route(collated):
    """The engine of do_Supervised (the same objective) replays such batches from one sparse bucket graph too."""
    import test_gpu_supervised as sup
    model, head = _modules()
    batches = [_batch(C_, T=3), _batch(A, T=3)]
    sg = replay_vs_eager(sup._case(0.25, 1.5, task=2, loss="mse"), "schnet", model, [head], batches)
    assert len(sg) == 1 and next(iter(sg.graphs))[:1] + next(iter(sg.graphs))[2:] == ("bucket", "sparse")


# ------------------------------------------------------------------------------------------ 7. the switches
def test_forced_sparse_pairs_and_the_bucket_switch(collated, monkeypatch):
    monkeypatch.setenv("GEOSSL_SPARSE_PAIRS", "1")
    sizes = [(5, 17, 2, 33), (12, 3, 30, 7)]
    model, head = _modules()
    tr = _trainer(model, head)
    batches = [_batch(s_) for s_ in sizes]
    ref = _eager_all(tr, batches)
    for k, b in enumerate(batches):
        lo = tr._graph_fwd_bwd(b)
        _assert_close((lo.clone(), _grads(tr)), ref[k], "forced sparse %d" % k)
    assert len(tr.step_graphs) == 1 and _bucket_keys(tr) == [("bucket", 4, "sparse")] and tr.step_graphs.captures == 1
    monkeypatch.setenv("GEOSSL_SPARSE_BUCKETS", "0")
    tr2 = _trainer(model, head)
    for k, b in enumerate(batches + batches):
        lo = tr2._graph_fwd_bwd(b)
        _assert_close((lo.clone(), _grads(tr2)), ref[k % 2], "switch off %d" % k)
    assert _bucket_keys(tr2) == []


def test_switch_values_above_255_atoms(monkeypatch):
    """Unset: a DeviceLoader handle takes the bucket, a collated batch keeps the routing it had; 1: both; 0: neither."""
    ds, sizes, _ = _pocket_dataset()
    hb = _handles(ds, sizes)[0]
    model, head = _modules()
    sg = _trainer(model, head).step_graphs
    b = _batch(C_)
    monkeypatch.delenv("GEOSSL_SPARSE_BUCKETS", raising=False)
    assert sg.bucket_key(b) is None and sg.bucket_key(hb) == ("bucket", 4, "sparse")
    monkeypatch.setenv("GEOSSL_SPARSE_BUCKETS", "1")
    assert sg.bucket_key(b) == ("bucket", 4, "sparse") and sg.bucket_key(hb) == ("bucket", 4, "sparse")
    monkeypatch.setenv("GEOSSL_SPARSE_BUCKETS", "0")
    assert sg.bucket_key(b) is None and sg.bucket_key(hb) is None


# ------------------------------------------------------------------------------------------- 8. refusals
def test_other_steps_keep_their_routing(collated):
    """A Distance Prediction or a DDM engine reads pair tuples: a batch with a 260-atom structure makes no bucket there
    (and a PaiNN Supervised trainer none either); the Supervised SchNet trainer does for the very same batch."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.pretrain_DistancePrediction import DistancePredictionTrainer, DistancePredictor
    from geossl_amd.synthetic import combination_pairs
    from helpers import fill_module_, product_ncsn
    import test_gpu_supervised as sup
    s = _structures(C_)
    off = np.concatenate([[0], np.cumsum(C_)])
    sei = np.concatenate([combination_pairs(int(n)) + off[m] for m, n in enumerate(C_)], axis=1).astype(np.int64)
    b = pg.Batch(t(s["x"], DEV)[:, None].contiguous(), t(s["positions"], DEV), t(s["batch"], DEV), t(sei, DEV),
                 num_graphs=len(C_), sizes=C_, canonical="combination")
    b.y = torch.zeros(len(C_), device=DEV)
    model, head = _modules()
    dist = DistancePredictionTrainer(model, fill_module_(DistancePredictor(128)).to(DEV), use_graph=True)
    ddm = pg.DDMTrainer(model, product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9), use_graph=True)
    for tr in (dist, ddm):
        assert tr.step_graphs.pair_tuples and tr.step_graphs.bucket_key(b) is None
    painn = backbone("painn")
    from geossl_amd.pretrain_Supervised import SupervisedTrainer
    ptr_ = SupervisedTrainer(painn, sup._head("painn", painn), 0.0, 1.0, task_id=0, loss="mse", model_3d="painn",
                             use_graph=True)
    assert ptr_.step_graphs.bucket_key(b) is None
    assert _trainer(model, head).step_graphs.bucket_key(b) == ("bucket", 4, "sparse")
    # a dense batch in the Supervised trainer: the dense bucket, as before
    small = (5, 17, 2, 33)
    s2 = _structures(small)
    off2 = np.concatenate([[0], np.cumsum(small)])
    sei2 = np.concatenate([combination_pairs(int(n)) + off2[m] for m, n in enumerate(small)], axis=1).astype(np.int64)
    b2 = pg.Batch(t(s2["x"], DEV)[:, None].contiguous(), t(s2["positions"], DEV), t(s2["batch"], DEV), t(sei2, DEV),
                  num_graphs=4, sizes=small, canonical="combination")
    assert _trainer(model, head).step_graphs.bucket_key(b2) == ("bucket", 4, "combination")
