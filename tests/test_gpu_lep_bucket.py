"""GPU tests of LEP on the sparse capacity bucket (geossl_amd/finetune_lep.py on bucket.SPARSE with 2B structures;
Geom3D.dataloaders.PairedDeviceDataset): the `_dyn` pair-head kernels against the exact entry points bit for bit, bucket
replay against the eager step on collated pair batches and on DeviceLoader pair handles (stale rows, labels as data, an
outgrown bucket), fixture G25 through a handle (LEPTrainer, do_LEP, eval_LEP), GEOSSL_SPARSE_BUCKETS /
GEOSSL_SPARSE_PAIRS, and what keeps its route or is refused.

Pair batches of B = 4 (active sizes | inactive sizes): one-atom structures on both sides, a structure just above 255
atoms, one in the 1024 class; A's 791 atoms are no multiple of 4."""
import types

import numpy as np
import pytest
import torch

import lba_structures as ls
import lep_twin as lt
from conftest import rel_err
from objective_harness import backbone

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
A = ((300, 2, 64, 1), (33, 257, 129, 5))
B_ = ((260, 40, 17, 3), (1, 5, 64, 3))
C_ = ((12, 3, 30, 7), (5, 17, 2, 33))          # a dense layout: the bucket's only under GEOSSL_SPARSE_PAIRS=1
BIG = ((600, 300, 280, 257), (300, 2, 64, 1))
TOL_LOSS, TOL_GRAD = 1e-6, 1e-5     # the bounds of test_gpu_sparse_bucket.py (sparse bucket replay against eager)

_ITEMS = {}


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    monkeypatch.delenv("GEOSSL_SPARSE_BUCKETS", raising=False)
    monkeypatch.delenv("GEOSSL_SPARSE_PAIRS", raising=False)


@pytest.fixture
def collated(monkeypatch):
    """The sparse bucket for collated batches: off unless the switch says 1."""
    monkeypatch.setenv("GEOSSL_SPARSE_BUCKETS", "1")


def _items(pair_sizes, seed=0, y=None):
    """The reference's LEP records of these pairs: 1-D atom types, float32 positions, an integer label each."""
    from geossl_amd.Geom3D.dataloaders import Data
    key = (tuple(pair_sizes[0]), tuple(pair_sizes[1]), seed, None if y is None else tuple(y))
    if key not in _ITEMS:
        active, inactive = pair_sizes
        sa, si = ls.structures(active, seed), ls.structures(inactive, seed + 17)
        oa, oi = np.concatenate([[0], np.cumsum(active)]), np.concatenate([[0], np.cumsum(inactive)])
        f = torch.from_numpy
        _ITEMS[key] = [Data(x_active=f(sa["x"][oa[b]:oa[b + 1]].copy()),
                            positions_active=f(sa["positions"][oa[b]:oa[b + 1]].copy()),
                            x_inactive=f(si["x"][oi[b]:oi[b + 1]].copy()),
                            positions_inactive=f(si["positions"][oi[b]:oi[b + 1]].copy()),
                            y=torch.tensor([(b + seed) % 2 if y is None else y[b]], dtype=torch.long))
                       for b in range(len(active))]
    return _ITEMS[key]


def _batch(pair_sizes, seed=0):
    from geossl_amd.Geom3D.dataloaders import BatchLEP
    return BatchLEP.from_data_list(_items(pair_sizes, seed)).to(DEV)


def _modules():
    from helpers import fill_module_
    model = backbone("schnet")
    head = fill_module_(torch.nn.Linear(256, 1)).to(DEV)
    with torch.no_grad():
        head.weight.mul_(0.05)   # (logits of order one with the filler's weights: no sigmoid saturates)
    return model, head


def _trainer(model, head, **kw):
    from geossl_amd.finetune_lep import LEPTrainer
    return LEPTrainer(model, head, lr=0.0, use_graph=True, **kw)


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


def _eager(tr, b):
    lo = tr._eager(b)
    return lo.clone(), _grads(tr)


def _replay(tr, b):
    lo = tr._graph_fwd_bwd(b)
    return lo.clone(), _grads(tr)


# ------------------------------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("readout", ["mean", "add"])
@pytest.mark.parametrize("F", [32, 128])
def test_dyn_pair_head_equals_the_exact_kernels(F, readout):
    import test_gpu_lep as gl
    from geossl_amd import _lib, ops
    from geossl_amd._lib import ptr, stream
    sizes = list(gl.SIZES_ACTIVE + (9,) + gl.SIZES_INACTIVE + (4,))     # B = 5: a second, partly filled tile
    B, N = 5, sum(sizes)
    assert N % 4 != 0 and min(sizes[:B]) == 1 and min(sizes[B:]) == 1
    N_cap = N + 37
    gen = torch.Generator().manual_seed(2600 + F)
    h = torch.randn(N, F, generator=gen).to(DEV)
    w = (torch.randn(1, 2 * F, generator=gen) / (2 * F) ** 0.5).to(DEV)
    b = torch.randn(1, generator=gen).to(DEV)
    y = torch.tensor([1.0, 0.0, 0.0, 1.0, 1.0], device=DEV)
    gout = torch.tensor(1.3, device=DEV)
    mol_ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)
    kind = ops.PROPERTY_READOUTS[readout]
    nws = int(_lib.load().geossl_pair_head_workspace_floats(B))
    SENT = 123.0

    def run(dyn):
        rows = N if dyn is None else N_cap
        nan = lambda *shape: torch.full(shape, NAN, dtype=torch.float32, device=DEV)
        hh = h if dyn is None else torch.cat([h, nan(N_cap - N, F)])
        m, z, zp, loss, dw, db, ws, ws2 = nan(2 * B, F), nan(B), nan(B), nan(1), nan(1, 2 * F), nan(1), nan(nws), nan(nws)
        dh = torch.full((rows, F), SENT, device=DEV)
        tail = () if dyn is None else (ptr(dyn),)
        sfx = "" if dyn is None else "_dyn"
        _lib.call("geossl_pair_head_fwd" + sfx, ptr(hh), rows, F, ptr(mol_ptr), B, kind, ptr(w), ptr(b), ptr(y), ptr(m),
                  ptr(z), ptr(ws), ptr(loss), *tail, stream())
        _lib.call("geossl_pair_head_predict" + sfx, ptr(hh), rows, F, ptr(mol_ptr), B, kind, ptr(w), ptr(b), ptr(zp),
                  *tail, stream())
        _lib.call("geossl_pair_head_bwd" + sfx, rows, F, ptr(mol_ptr), B, kind, ptr(w), ptr(m), ptr(z), ptr(y), ptr(gout),
                  ptr(dh), ptr(dw), ptr(db), ptr(ws2), 0, *tail, stream())
        torch.cuda.synchronize()
        return dict(m=m, z=z, zp=zp, loss=loss, dh=dh, dw=dw, db=db)

    ref = run(None)
    got = run(torch.tensor([N], dtype=torch.int32, device=DEV))
    assert all(torch.isfinite(v).all() for v in ref.values()) and torch.equal(ref["z"], ref["zp"])
    for k in ("m", "z", "zp", "loss", "dw", "db"):
        assert torch.equal(got[k], ref[k]), k
    assert torch.equal(got["dh"][:N], ref["dh"]) and not (ref["dh"] == SENT).any()
    assert torch.all(got["dh"][N:] == SENT)                              # nothing at or past the real count is written
    # the wrapper without dyn passes a null dyn_N: the exact form on the same rows
    lay = types.SimpleNamespace(mol_ptr=mol_ptr, B=2 * B, N=N)
    assert torch.equal(ops.pair_predict(h, w, b, lay, readout), ref["z"])


# ------------------------------------------------------------------------ 2. replay equals eager, no stale row
def test_replay_equals_eager_and_leaves_no_stale_row(collated):
    model, head = _modules()
    tr = _trainer(model, head)
    batches = [_batch(A), _batch(B_, 1), _batch(A)]
    ref = [_eager(tr, b) for b in batches]
    got = [_replay(tr, b) for b in batches]
    for k, (g_, r_) in enumerate(zip(got, ref)):
        _assert_close(g_, r_, "batch %d" % k)
    sg = tr.step_graphs
    assert len(sg) == 1 and sg.captures == 1 and next(iter(sg.graphs)) == ("bucket", 8, "sparse")
    # the two A steps, with a smaller batch in between: bitwise equal
    assert torch.equal(got[0][0], got[2][0])
    for a, c in zip(got[0][1], got[2][1]):
        assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------------- 3. handles
def _pair_dataset(y_dtype=np.int64):
    """12 pairs of 30 .. 320 atoms; the four structures above 255 sit in pairs 0, 3, 6 and 9, on alternating sides."""
    from geossl_amd.Geom3D.dataloaders import PairedDeviceDataset
    rng = np.random.default_rng(25)
    sizes = rng.integers(30, 121, size=(2, 12))
    for k, m in enumerate((0, 3, 6, 9)):
        sizes[k % 2, m] = (320, 256, 300, 270)[k]
    y = (np.arange(12) * 5 % 3 > 0).astype(y_dtype)
    items = _items((tuple(int(n) for n in sizes[0]), tuple(int(n) for n in sizes[1])), seed=3, y=[int(v) for v in y])
    return PairedDeviceDataset.from_data_list(items, DEV), items, sizes, y


def _handles(ds, sizes):
    """The three handles of a shuffled epoch, each with a structure above 255 atoms (the first loader seed that gives
    them: a batch without one has a dense layout and keeps its own routing)."""
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    for seed in range(64):
        loader = DeviceLoader(ds, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(seed))
        hbs = list(loader)
        if all(sizes[:, hb.ids].max() > 255 for hb in hbs):
            return hbs
    raise AssertionError("no loader seed in range(64) gives three batches with a structure above 255 atoms")


def test_pair_handles_share_one_bucket_graph():
    from geossl_amd.Geom3D.dataloaders import BatchLEP, PairedBatch
    ds, items, sizes, y = _pair_dataset()
    assert len(ds) == 12 and ds.y.dtype == torch.float32 and y.dtype == np.int64     # (an integer y, stored as float32)
    hbs = _handles(ds, sizes)
    assert len(hbs) == 3 and all(isinstance(hb, PairedBatch) and hb.num_graphs == 4 for hb in hbs)
    model, head = _modules()
    tr = _trainer(model, head)
    for k, hb in enumerate(hbs):
        assert torch.equal(hb.y.cpu(), torch.from_numpy(y[hb.ids]).float())
        cb = BatchLEP.from_data_list([items[i] for i in hb.ids]).to(DEV)
        for name in ("x_active", "positions_active", "batch_active", "x_inactive", "positions_inactive",
                     "batch_inactive"):
            got_t, want_t = getattr(hb, name), getattr(cb, name)
            assert got_t.dtype == want_t.dtype and torch.equal(got_t, want_t), name
        assert np.array_equal(hb._sizes_active, cb._sizes_active) and np.array_equal(hb._sizes_inactive, cb._sizes_inactive)
        ref = _eager(tr, cb)                                             # (on the host-collated batch of the same records)
        _assert_close(_eager(tr, hb), ref, "handle %d, eager on its materialised tensors" % k)
        _assert_close(_replay(tr, hb), ref, "handle %d" % k)
    sg = tr.step_graphs
    assert len(sg) == 1 and sg.captures == 1 and next(iter(sg.graphs)) == ("bucket", 8, "sparse")
    (gg,) = sg.graphs.values()
    assert gg["noise"]["target"].numel() == 8                           # one row per structure; the pairs' labels lead
    assert torch.equal(gg["noise"]["target"][:4].cpu(), torch.from_numpy(y[hbs[-1].ids]).float())


# ----------------------------------------------------------------------------------------- 4. labels are data
def test_labels_are_data_of_the_graph():
    ds, items, sizes, y = _pair_dataset()
    hbs = _handles(ds, sizes)
    model, head = _modules()
    tr = _trainer(model, head)
    first = _replay(tr, hbs[0])
    assert tr.step_graphs.captures == 1
    ds.y.copy_(1.0 - ds.y)                                               # other labels for the same structures
    again = ds.batch(hbs[0].ids)
    assert torch.equal(again.y.cpu(), 1.0 - torch.from_numpy(y[again.ids]).float())
    ref = _eager(tr, again)
    got = _replay(tr, again)
    assert tr.step_graphs.captures == 1 and len(tr.step_graphs) == 1
    _assert_close(got, ref, "flipped labels")
    assert abs(float(got[0]) - float(first[0])) > 1e-3 * abs(float(first[0]))       # (it IS another loss)


# ----------------------------------------------------------------------------------------- 5. outgrown bucket
def test_outgrown_bucket_is_captured_again(collated):
    model, head = _modules()
    tr = _trainer(model, head)
    small, big = _batch(B_, 1), _batch(BIG, 2)
    ref = _eager(tr, big)
    _replay(tr, small)
    bkt = next(iter(tr.step_graphs.graphs.values()))["bucket"]
    n_big = sum(BIG[0]) + sum(BIG[1])
    assert bkt.max_n == 512 and bkt.B == 8 and bkt.N_cap < n_big
    got = _replay(tr, big)
    sg = tr.step_graphs
    assert sg.captures == 2 and len(sg) == 1
    bkt = next(iter(sg.graphs.values()))["bucket"]
    assert bkt.max_n == 1024 and bkt.N_cap >= n_big and bkt.P_cap == 33 * bkt.N_cap
    _assert_close(got, ref, "outgrown")


# ------------------------------------------------------------------------------------------- 6. reference pin
@pytest.mark.parametrize("case", ["g25_lep_schnet_full", "g25_lep_schnet_reduced"])
def test_g25_through_a_pair_handle(case):
    """Fixture G25 from a PairedDeviceDataset, one handle of all pairs.  The full case (width 128) replays the sparse
    bucket of 2B structures; the reduced one (width 64: bucket.modules_ok serves the F = 128 chain path) keeps its
    per-structure graph - the key is asserted either way."""
    import test_gpu_lep as gl
    from geossl_amd.finetune_lep import LEPTrainer, do_LEP, eval_LEP
    from geossl_amd.Geom3D.dataloaders import DeviceLoader, PairedDeviceDataset
    assert gl.TOL_OUT == 1e-5 and gl.TOL_GRAD == 1e-4
    g, meta, model, head, make, args = gl._setup(case)
    ds = PairedDeviceDataset.from_data_list(lt.fixture_items(g), DEV)
    B = len(ds)
    assert B == len(g["sizes_active"]) and ds.x_cols == 1 and ds.x_1d
    hb = ds.batch(np.arange(B))
    tr = LEPTrainer(model, head, lr=0.0, model_3d="schnet", use_graph=True)
    for _ in range(2):
        loss = tr._graph_fwd_bwd(hb)
    want = [("bucket", 2 * B, "sparse")] if meta["emb_dim"] == 128 else []
    assert _bucket_keys(tr) == want and len(tr.step_graphs) == 1 and tr.step_graphs.captures == 1
    gl._check(g, model, head, loss, case)

    # do_LEP on the same handle: the same route through its engine, the reference's loss.backward()
    _, _, model2, head2, _, _ = gl._setup(case)
    loss2 = do_LEP(args, ds.batch(np.arange(B)), model2, head2, torch.nn.BCEWithLogitsLoss())
    loss2.backward()
    gl._check(g, model2, head2, loss2, case)
    eng = model2.__dict__["_geossl_lep_step"]
    keys = [k for sg in eng.graphs.values() for k in sg.graphs if k[0] == "bucket"]
    assert keys == want

    # eval() from handles
    loader = DeviceLoader(ds, batch_size=B, shuffle=False)
    bce, roc, pr, y_true, y_pred = eval_LEP(args, loader, model, head)
    assert rel_err(torch.tensor(y_pred), g["pred"]) < gl.TOL_OUT and np.array_equal(y_true, g["batch/y"].astype(np.float64))
    assert abs(bce - float(g["bce"])) < gl.TOL_OUT * float(g["bce"])
    assert abs(roc - float(g["roc"])) < gl.TOL_OUT and abs(pr - float(g["pr"])) < gl.TOL_OUT
    assert rel_err(tr.predict(hb).cpu(), g["pred"]) < gl.TOL_OUT


# ------------------------------------------------------------------------------------- 7. routing and refusals
def test_switch_values_for_handles_and_collated_batches(monkeypatch):
    """Unset: a pair handle takes the bucket, a collated batch keeps the routing it had; 1: both; 0: neither."""
    from geossl_amd.finetune_lep import fused_batch
    from geossl_amd.Geom3D.dataloaders import PairedDeviceDataset
    model, head = _modules()
    sg = _trainer(model, head).step_graphs
    assert sg.pair_tuples is False
    hb = fused_batch(PairedDeviceDataset.from_data_list(_items(A), DEV).batch(np.arange(4)))
    b = fused_batch(_batch(A))
    key = ("bucket", 8, "sparse")
    assert sg.bucket_key(b) is None and sg.bucket_key(hb) == key
    monkeypatch.setenv("GEOSSL_SPARSE_BUCKETS", "1")
    assert sg.bucket_key(b) == key and sg.bucket_key(hb) == key
    monkeypatch.setenv("GEOSSL_SPARSE_BUCKETS", "0")
    assert sg.bucket_key(b) is None and sg.bucket_key(hb) is None


def test_what_keeps_its_route(collated, monkeypatch):
    import test_gpu_lep as gl
    from geossl_amd.finetune_lep import LEPTrainer, fused_batch
    from geossl_amd.Geom3D.dataloaders import PairedDeviceDataset
    # all structures <= 255 atoms: a dense layout
    g, meta, model, head, make, args = gl._setup("g25_lep_schnet_dense")
    assert LEPTrainer(model, head, use_graph=True).step_graphs.bucket_key(fused_batch(make())) is None
    # PaiNN: the sparse bucket is SchNet's
    g, meta, model, head, make, args = gl._setup("g25_lep_painn")
    assert int(max(g["sizes_active"].max(), g["sizes_inactive"].max())) > 255
    assert LEPTrainer(model, head, model_3d="painn", use_graph=True).step_graphs.bucket_key(fused_batch(make())) is None
    # batch C, collated and as a handle: dense without GEOSSL_SPARSE_PAIRS - no bucket of any kind - sparse with it
    model, head = _modules()
    tr = _trainer(model, head)
    c = _batch(C_)
    hc = PairedDeviceDataset.from_data_list(_items(C_), DEV).batch(np.arange(4))
    assert tr.step_graphs.bucket_key(fused_batch(c)) is None and tr.step_graphs.bucket_key(fused_batch(hc)) is None
    # (no step has run on them yet: a layout, once built, is cached on the batch vector and keeps its kind)
    monkeypatch.setenv("GEOSSL_SPARSE_PAIRS", "1")
    ref = _eager(tr, c)
    _assert_close(_replay(tr, c), ref, "forced sparse, collated")
    _assert_close(_replay(tr, hc), ref, "forced sparse, handle")
    assert _bucket_keys(tr) == [("bucket", 8, "sparse")] and tr.step_graphs.captures == 1


def test_refusals():
    import test_gpu_lep as gl
    from geossl_amd.finetune_lep import do_LEP
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    ds, items, sizes, y = _pair_dataset()
    with pytest.raises(ValueError, match="mask_ratio"):
        DeviceLoader(ds, batch_size=4, mask_ratio=0.3)
    model, head = _modules()
    tr = _trainer(model, head)
    one = ds.batch([0])
    args = types.SimpleNamespace(model_3d="schnet")
    with pytest.raises(ValueError, match="[Tt]arget size"):             # the reference's squeeze() against a [1] target
        do_LEP(args, one, model, head)
    with pytest.raises(ValueError, match="B >= 2"):
        tr.step(one)
    # a bucket holds the loader's batch size: 8 pairs do not go into one built for 4
    _replay(tr, ds.batch([0, 1, 2, 3]))
    (gg,) = tr.step_graphs.graphs.values()
    with pytest.raises(ValueError, match="bucket of 8 molecules got a batch of 16"):
        gg["bucket"].fill(ds.batch(np.arange(8)).fused())
    # PaiNN pairs are collated by the reference's loader: a handle holds no radius edges
    g, meta, pmodel, phead, make, pargs = gl._setup("g25_lep_painn")
    with pytest.raises(ValueError, match="radius edges"):
        do_LEP(pargs, one, pmodel, phead)
