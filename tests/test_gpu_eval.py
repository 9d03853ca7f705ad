"""GPU tests of the evaluation passes (geossl_amd/evaluate.py, csrc/eval_collect.hip): the collect kernel against its numpy
twin on poisoned result arrays; forward-only bucket graphs of SchNet and PaiNN against the eager route on a ragged
DeviceLoader (dense buckets), on pockets above 255 atoms (sparse bucket, fixture G24) and on LEP's pair handles (fixture
G25); stale rows and live parameters; the fallbacks inside one loader; and the shape of the loop - per replayed batch one
gather / fill, one target launch, one graph launch, one collect, and no device read before the loop ends."""
import types

import numpy as np
import pytest
import torch

import eval_twin as et
import lba_structures as ls
from conftest import rel_err
from objective_harness import backbone
from test_gpu_lep import TOL_OUT
from test_gpu_sparse_bucket import A, B_, TOL_LOSS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
K_LOSS_BLOCK = 256     # head_common.h kLossBlock: one row more exercises the strided loop


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    for k in ("GEOSSL_SPARSE_BUCKETS", "GEOSSL_PAINN_SPARSE_BUCKETS", "GEOSSL_SPARSE_PAIRS", "GEOSSL_PAINN_TILE",
              "GEOSSL_NO_BUCKETS"):
        monkeypatch.delenv(k, raising=False)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


# ----------------------------------------------------------------------------------------- 1. the kernel and its twin
def _rows(B, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == et.BCE:
        z = rng.uniform(-30.0, 30.0, size=B).astype(np.float32)
        z[0] = 30.0 if seed % 2 else -30.0
        return z, rng.integers(0, 2, size=B).astype(np.float32)
    return (rng.standard_normal(B) * 3.0).astype(np.float32), (rng.standard_normal(B) * 3.0).astype(np.float32)


def _check_sums(got, want, kind):
    assert got[2] == want[2]                                              # rows: exact
    if kind == et.REGRESSION:     # single correctly-rounded fp32 terms, identical in numpy: fp64 reassociation remains
        assert abs(got[0] - want[0]) <= 1e-12 * abs(want[0]) and abs(got[1] - want[1]) <= 1e-12 * abs(want[1])
    else:                         # log1pf / expf of the device against numpy's: the bound G25's BCE loss is held to
        assert abs(got[0] - want[0]) <= TOL_OUT * abs(want[0]) and got[1] == 0.0


@pytest.mark.parametrize("kind", [et.REGRESSION, et.BCE], ids=["regression", "bce"])
@pytest.mark.parametrize("offset", [0, 7])
@pytest.mark.parametrize("B", [1, 5, K_LOSS_BLOCK + 1])
def test_collect_kernel_against_the_twin(B, offset, kind):
    from geossl_amd import ops
    M = offset + B + 5 + 9
    p1, t1 = _rows(B, kind, 10 * B + offset)
    p2, t2 = _rows(5, kind, 10 * B + offset + 1)
    runs = []
    for _ in range(2):
        acc = ops.eval_buffer(DEV)
        op, ot = torch.full((M,), NAN, device=DEV), torch.full((M,), NAN, device=DEV)
        ops.eval_collect(torch.from_numpy(p1).to(DEV), torch.from_numpy(t1).to(DEV), kind, offset, op, ot, acc)
        first = ops.eval_read(acc)
        ops.eval_collect(torch.from_numpy(p2).to(DEV), torch.from_numpy(t2).to(DEV), kind, offset + B, op, ot, acc)
        runs.append((first, ops.eval_read(acc), op.cpu().numpy(), ot.cpu().numpy(), acc.cpu()))
    first, both, op, ot, _ = runs[0]
    tp, tt = np.full(M, NAN, np.float32), np.full(M, NAN, np.float32)
    w1 = et.collect(p1, t1, kind, offset, tp, tt)
    w2 = et.collect(p2, t2, kind, offset + B, tp, tt, acc=w1)
    print("B %d offset %d kind %d: sums %r twin %r" % (B, offset, kind, both, w2))
    _check_sums(first, w1, kind)
    _check_sums(both, w2, kind)
    # the rows [offset, offset + B + 5) hold the inputs bit for bit; nothing else was written
    assert np.array_equal(_bits(op), _bits(tp)) and np.array_equal(_bits(ot), _bits(tt))
    assert np.isnan(op[:offset]).all() and np.isnan(op[offset + B + 5:]).all() and np.isfinite(op[offset:offset + B + 5]).all()
    # two runs: the same bits
    assert torch.equal(runs[0][4], runs[1][4]) and np.array_equal(_bits(runs[0][2]), _bits(runs[1][2]))
    # null outputs: the sums alone
    acc = ops.eval_buffer(DEV)
    ops.eval_collect(torch.from_numpy(p1).to(DEV), torch.from_numpy(t1).to(DEV), kind, offset, None, None, acc)
    only_pred = torch.full((M,), NAN, device=DEV)
    ops.eval_collect(torch.from_numpy(p2).to(DEV), torch.from_numpy(t2).to(DEV), kind, offset + B, only_pred, None, acc)
    assert torch.equal(acc.cpu(), runs[0][4])
    assert np.array_equal(_bits(only_pred.cpu().numpy()[offset + B:offset + B + 5]), _bits(p2))
    assert torch.isnan(only_pred[:offset + B]).all()


def test_collect_entry_refuses_bad_arguments():
    from geossl_amd import _lib, ops
    from geossl_amd._lib import ptr, stream
    fn = _lib.load().geossl_eval_collect
    acc = ops.eval_buffer(DEV)
    p = torch.ones(4, device=DEV)
    out = torch.full((8,), NAN, device=DEV)
    bad = int(1)                                                          # hipErrorInvalidValue
    assert fn(None, None, 0, 0, 0, None, None, ptr(acc), stream()) == 0   # B = 0: no launch, nothing needed
    assert fn(ptr(p), ptr(p), 4, 2, 0, ptr(out), ptr(out), ptr(acc), stream()) == bad      # kind
    assert fn(ptr(p), ptr(p), -1, 0, 0, ptr(out), ptr(out), ptr(acc), stream()) == bad     # B
    assert fn(ptr(p), ptr(p), 4, 0, -1, ptr(out), ptr(out), ptr(acc), stream()) == bad     # offset
    assert fn(ptr(p), ptr(p), 4, 0, 0, ptr(out), ptr(out), None, stream()) == bad          # acc
    assert fn(None, ptr(p), 4, 0, 0, ptr(out), ptr(out), ptr(acc), stream()) == bad        # pred
    assert fn(ptr(p), None, 4, 1, 0, ptr(out), ptr(out), ptr(acc), stream()) == bad        # target
    torch.cuda.synchronize()
    assert not acc.cpu().any() and torch.isnan(out).all()
    with pytest.raises(ValueError):
        ops.eval_collect(p, p, 0, 6, out, out, acc)                       # offset + B past the result array
    with pytest.raises(ValueError):
        ops.eval_collect(p, p, "huber", 0, out, out, acc)
    with pytest.raises(ValueError):
        ops.eval_collect(p, p[:3], 0, 0, out, out, acc)


# ------------------------------------------------------------------------------------------------ shared modules
_MODULES = {}


def _modules(kind):
    import test_gpu_supervised as sup
    if kind not in _MODULES:
        model = backbone(kind)
        _MODULES[kind] = (model, sup._head(kind, model))
    return _MODULES[kind]


def _args(kind):
    return types.SimpleNamespace(model_3d=kind, loss="mae")


def _eager_scores(kind, loader, model, head, mean=0.0, std=1.0):
    from geossl_amd.pretrain_Supervised import predict_Supervised
    return torch.cat([predict_Supervised(_args(kind), hb, model, head, mean, std) for hb in loader]).cpu().numpy()


# --------------------------------------------------------------------------------------------- 2. dense buckets
SIZES_22 = (2, 33, 17, 5, 21, 9, 30, 12, 3, 26, 18, 7, 33, 14, 2, 23, 11, 28, 6, 19, 31, 16)


def _dense_loader(kind, sizes=SIZES_22, batch_size=8, T=3):
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    from geossl_amd.synthetic import make_molecules
    mols = make_molecules(len(sizes), seed=13, sizes=sizes)
    y = np.random.default_rng(5).standard_normal((len(sizes), T)).astype(np.float32)
    ds = DeviceDataset.from_numpy(mols, DEV, y=y, **({"radius": 5.0} if kind == "painn" else {}))
    return DeviceLoader(ds, batch_size=batch_size, shuffle=False), y


@pytest.fixture(scope="module", params=["schnet", "painn"])
def dense(request):
    """One evaluator per backbone, captured by a first pass over 22 ragged molecules in batches of 8, 8, 6."""
    from geossl_amd.evaluate import evaluator_for
    from geossl_amd.pretrain_Supervised import eval_Supervised
    kind = request.param
    model, head = _modules(kind)
    model.__dict__.pop("_geossl_evaluator", None)
    loader, y = _dense_loader(kind)
    first = eval_Supervised(_args(kind), loader, model, head, 0.0, 1.0, task_id=1, use_graph=True)
    ev = evaluator_for(model, head, kind, "property", 1)
    return types.SimpleNamespace(kind=kind, model=model, head=head, loader=loader, y=y, first=first, ev=ev,
                                 captures=ev.captures)


def test_dense_buckets_two_captures_then_none(dense):
    from geossl_amd.pretrain_Supervised import eval_Supervised
    assert [hb.num_graphs for hb in dense.loader] == [8, 8, 6]
    assert dense.captures == 2
    assert sorted(dense.ev.graphs.graphs) == [("bucket", 6, "combination"), ("bucket", 8, "combination")]
    mae, y_true, y_scores = dense.first
    again = eval_Supervised(_args(dense.kind), dense.loader, dense.model, dense.head, 0.0, 1.0, task_id=1, use_graph=True)
    assert dense.ev.captures == 2
    assert np.array_equal(_bits(again[1]), _bits(y_true)) and np.array_equal(_bits(again[2]), _bits(y_scores))
    assert y_true.dtype == np.float32 and np.array_equal(y_true, dense.y[:, 1]) and y_true.shape == (22,)
    # stats (0, 1): de-normalising hides nothing
    ref = _eager_scores(dense.kind, dense.loader, dense.model, dense.head)
    e = rel_err(y_scores, ref)
    print("%s dense buckets: replay against eager %.3e" % (dense.kind, e))
    assert e < TOL_LOSS
    ref_mae = np.mean(np.abs(y_scores - y_true))
    assert mae.tobytes() == ref_mae.tobytes()
    # the device sums: fp64 over fp32 terms; numpy's fp32 pairwise mean of 22 values carries ~ log2(22) 2^-24
    only = eval_Supervised(_args(dense.kind), dense.loader, dense.model, dense.head, 0.0, 1.0, task_id=1, use_graph=True,
                           arrays=False)
    assert isinstance(only, float) and abs(only - float(ref_mae)) <= 1e-6 * float(ref_mae)
    sum_a, sum_s, rows, _, _ = dense.ev.run(dense.loader, arrays=False)
    assert rows == 22 and sum_s > 0 and sum_a / rows == only


# ------------------------------------------------------------------------------ 3. stale rows and live parameters
def test_stale_rows_and_live_parameters():
    """One bucket: a batch near the capacity, then a much smaller one; then the head's bias and (mean, std) change in
    place - no new capture, the eager route's values under the new ones."""
    from geossl_amd.pretrain_Supervised import SupervisedTrainer
    import test_gpu_supervised as sup
    model = backbone("schnet")
    head = sup._head("schnet", model)
    sizes = (33, 31, 32, 30, 33, 29, 32, 31) + (2, 3, 2, 4, 3, 2, 5, 2)
    loader, y = _dense_loader("schnet", sizes=sizes, T=1)
    tr = SupervisedTrainer(model, head, 0.0, 1.0, task_id=0, loss="mae", lr=0.0, use_graph=True)
    mae, y_true, y_scores = tr.evaluate(loader)
    ev = model.__dict__["_geossl_evaluator"]
    assert ev.captures == 1 and ev.stats is tr.stats and np.array_equal(y_true, y[:, 0])
    ref = _eager_scores("schnet", loader, model, head)
    e_big, e_small = rel_err(y_scores[:8], ref[:8]), rel_err(y_scores[8:], ref[8:])
    print("stale rows: big batch %.3e, small batch behind it %.3e" % (e_big, e_small))
    assert e_big < TOL_LOSS and e_small < TOL_LOSS
    with torch.no_grad():
        head.bias.add_(1.0)
    tr.set_stats(0.5, 2.0)
    mae2, _, scores2 = tr.evaluate(loader)
    assert ev is model.__dict__["_geossl_evaluator"] and ev.captures == 1
    ref2 = _eager_scores("schnet", loader, model, head, 0.5, 2.0)
    assert rel_err(scores2, ref2) < TOL_LOSS
    assert rel_err(scores2, y_scores * 2.0 + 2.5) < 1e-5 and float(mae2) != float(mae)   # (p + 1) 2 + 0.5
    assert torch.equal(tr.predict(next(iter(loader))).cpu(), torch.from_numpy(scores2[:8]))
    import copy
    assert copy.deepcopy(ev) is None


# ------------------------------------------------------------------------------------------------ 4. sparse bucket
def _pocket_loader(kind):
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    s = ls.structures(A + B_, 0)
    y = np.random.default_rng(8).standard_normal(8).astype(np.float32)
    ds = DeviceDataset(s["x"], s["positions"], s["sizes"], DEV, y=y, **({"radius": 5.0} if kind == "painn" else {}))
    return DeviceLoader(ds, batch_size=4, shuffle=False), y


def _as_records(hb):
    from geossl_amd import pretrain_GeoSSL as pg
    m = hb.materialize()
    b = pg.Batch(m.x[:, 0].contiguous(), m.positions, m.batch, None, radius_edge_index=m.radius_edge_index,
                 num_graphs=hb.num_graphs, sizes=[int(n) for n in hb._sizes])
    b.y = hb.y
    return b


@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_sparse_bucket_pockets(kind):
    import test_gpu_supervised as sup
    from geossl_amd.finetune_lba import eval_LBA, predict_LBA
    model = backbone(kind)        # (its own modules: the `dense` fixture keeps an evaluator on the shared ones)
    head = sup._head(kind, model)
    loader, y = _pocket_loader(kind)
    args = _args(kind)
    got = eval_LBA(args, loader, model, head, use_graph=True)
    ev = model.__dict__["_geossl_evaluator"]
    assert ev.captures == 1 and list(ev.graphs.graphs) == [("bucket", 4, "sparse")]
    again = eval_LBA(args, loader, model, head, use_graph=True)
    assert ev.captures == 1 and np.array_equal(_bits(again[4]), _bits(got[4]))
    # the eager route on the handles' own gathered tensors, x as LBA's records hold it (1-D: predict_LBA hands batch.x
    # to the backbone as it is, and a handle of such a dataset shows it as one column)
    collated = [_as_records(hb) for hb in loader]
    ref = eval_LBA(args, collated, model, head)
    eager = torch.cat([predict_LBA(args, b, model, head) for b in collated]).cpu().numpy()
    e = rel_err(got[4], eager)
    print("%s sparse bucket: replay against eager %.3e" % (kind, e))
    assert e < TOL_LOSS
    assert got[3].dtype == np.float32 and np.array_equal(got[3], y) and np.array_equal(got[3], np.float32(ref[3]))
    assert abs(got[0] - ref[0]) <= TOL_OUT * ref[0]
    assert abs(got[1] - ref[1]) <= TOL_OUT and abs(got[2] - ref[2]) <= TOL_OUT


@pytest.mark.parametrize("case", ["g24_lba_schnet_full", "g24_lba_painn"])
def test_g24_through_the_evaluator(case):
    import test_gpu_lba as lba
    from geossl_amd.finetune_lba import eval_LBA
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    g, meta, model, head, make, args = lba._setup(case)
    kw = {"radius": float(meta["cutoff"])} if meta["kind"] == "painn" else {}
    ds = DeviceDataset(g["x"], g["positions"], g["sizes"], DEV, y=g["y"], **kw)
    loader = DeviceLoader(ds, batch_size=len(g["sizes"]), shuffle=False)
    rmse, pearson, spearman, y_true, y_pred = eval_LBA(args, loader, model, head, use_graph=True)
    assert model.__dict__["_geossl_evaluator"].captures == 1
    assert rel_err(torch.tensor(y_pred), g["pred"]) < lba.TOL_OUT and np.array_equal(np.float32(y_true), g["y"])
    assert abs(rmse - float(g["rmse"])) < lba.TOL_OUT * float(g["rmse"])
    assert abs(pearson - float(g["pearson"])) < lba.TOL_OUT and abs(spearman - float(g["spearman"])) < lba.TOL_OUT


# --------------------------------------------------------------------------------------------------------- 5. LEP
PAIRS_6 = ((260, 40, 64, 5, 33, 20), (40, 270, 17, 129, 257, 300))


def test_lep_pair_handles():
    import test_gpu_lep_bucket as lb
    from geossl_amd.finetune_lep import eval_LEP, predict_LEP
    from geossl_amd.Geom3D.dataloaders import DeviceLoader, PairedDeviceDataset
    model, head = lb._modules()
    ds = PairedDeviceDataset.from_data_list(lb._items(PAIRS_6), DEV)
    loader = DeviceLoader(ds, batch_size=4, shuffle=False)
    assert [hb.num_graphs for hb in loader] == [4, 2]
    args = types.SimpleNamespace(model_3d="schnet")
    got = eval_LEP(args, loader, model, head, use_graph=True)
    ev = model.__dict__["_geossl_evaluator"]
    assert ev.kind == "pair" and ev.captures == 2
    assert sorted(ev.graphs.graphs) == [("bucket", 4, "sparse"), ("bucket", 8, "sparse")]
    again = eval_LEP(args, loader, model, head, use_graph=True)
    assert ev.captures == 2 and np.array_equal(_bits(again[4]), _bits(got[4]))
    ref = eval_LEP(args, loader, model, head)
    e = rel_err(got[4], ref[4])
    print("LEP pair handles: replay against eager %.3e" % e)
    assert e < TOL_LOSS
    assert got[3].dtype == np.float32 and np.array_equal(got[3], np.float32(ref[3])) and got[3].shape == (6,)
    assert np.array_equal(got[3], ds.y.cpu().numpy())
    assert abs(got[0] - ref[0]) <= TOL_OUT * ref[0]
    assert abs(got[1] - ref[1]) <= TOL_OUT and abs(got[2] - ref[2]) <= TOL_OUT
    # a B = 1 tail batch takes the ATen lines and lands in order (a loader without a length)
    tail = [ds.batch([0, 1, 2, 3]), ds.batch([4])]
    t_got = eval_LEP(args, tail, model, head, use_graph=True)
    assert ev.captures == 2 and t_got[4].shape == (5,)
    assert np.array_equal(_bits(t_got[4][:4]), _bits(got[4][:4]))
    one = predict_LEP(args, ds.batch([4]), model, head)
    assert one.dim() == 0 and _bits(t_got[4][4:]) == _bits(one.cpu().numpy().reshape(1))
    assert np.array_equal(t_got[3], ds.y.cpu().numpy()[:5])


@pytest.mark.parametrize("case", ["g25_lep_schnet_full", "g25_lep_painn"])
def test_g25_through_the_trainer(case):
    import lep_twin as lt
    import test_gpu_lep as gl
    from geossl_amd.finetune_lep import LEPTrainer
    from geossl_amd.Geom3D.dataloaders import DeviceLoader, PairedDeviceDataset
    g, meta, model, head, make, args = gl._setup(case)
    kw = {"radius": float(meta["cutoff"])} if meta["kind"] == "painn" else {}
    ds = PairedDeviceDataset.from_data_list(lt.fixture_items(g), DEV, **kw)
    tr = LEPTrainer(model, head, lr=0.0, model_3d=meta["kind"], use_graph=True)
    bce, roc, pr, y_true, y_pred = tr.evaluate(DeviceLoader(ds, batch_size=len(ds), shuffle=False))
    assert model.__dict__["_geossl_evaluator"].captures == 1
    assert rel_err(torch.tensor(y_pred), g["pred"]) < gl.TOL_OUT and np.array_equal(y_true, g["batch/y"].astype(np.float32))
    assert abs(bce - float(g["bce"])) < gl.TOL_OUT * float(g["bce"])
    assert abs(roc - float(g["roc"])) < gl.TOL_OUT and abs(pr - float(g["pr"])) < gl.TOL_OUT
    assert rel_err(tr.predict(ds.batch(np.arange(len(ds)))).cpu(), g["pred"]) < gl.TOL_OUT


# ------------------------------------------------------------------------------- 6. fallbacks inside one loader
def test_fallbacks_inside_one_loader():
    """A width-64 head (no bucket serves it: a structure's own graph from its SECOND sighting, eager launches at the
    first) and a collated batch without host sizes: no capture, today's predictions bit for bit, in loader order - over
    more rows than the result arrays start with."""
    import test_gpu_supervised as sup
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.models import SchNet
    from geossl_amd.pretrain_Supervised import eval_Supervised, predict_Supervised
    from helpers import fill_module_
    cfg = dict(hidden_channels=64, num_filters=64, num_interactions=2, num_gaussians=8, cutoff=5.0, node_class=9)
    model = fill_module_(SchNet(**cfg)).to(DEV)
    head = fill_module_(torch.nn.Linear(64, 1)).to(DEV)
    batches = sup._target_batches(9, 8, 31)
    b = batches[4]
    by_hand = pg.Batch(b.x, b.positions, b.batch, b.super_edge_index, num_graphs=8)
    by_hand.y = b.y
    assert getattr(by_hand, "_sizes", None) is None
    batches[4] = by_hand
    args = _args("schnet")
    mae, y_true, y_scores = eval_Supervised(args, batches, model, head, 0.3, 1.4, task_id=2, use_graph=True)
    ev = model.__dict__["_geossl_evaluator"]
    assert ev.captures == 0 and y_scores.shape == (72,)
    want = torch.cat([predict_Supervised(args, bb, model, head, 0.3, 1.4) for bb in batches]).cpu().numpy()
    assert np.array_equal(_bits(y_scores), _bits(want))
    assert np.array_equal(y_true, torch.cat([bb.y.view(8, -1)[:, 2] for bb in batches]).cpu().numpy())
    ref = eval_Supervised(args, batches, model, head, 0.3, 1.4, task_id=2, use_graph=False)
    assert np.array_equal(_bits(ref[2]), _bits(y_scores)) and ref[0].tobytes() == mae.tobytes()


# ---------------------------------------------------------------------------------------------- 7. the loop's shape
def test_loop_shape(dense, monkeypatch):
    """A replayed batch of a handle loader: one gather / fill, one target launch, one graph launch, one collect - and no
    .item() / .cpu() / .tolist() before the loop ends."""
    from test_gpu_step_engine_launches import _Recorder
    rec = _Recorder(monkeypatch.setattr)
    reads, replays, at_collect = [0], [0], []
    for name in ("item", "cpu", "tolist"):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, **k):
            reads[0] += 1
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    real_replay = torch.cuda.CUDAGraph.replay

    def replay(self):
        replays[0] += 1
        return real_replay(self)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", replay)
    real_record = rec._record

    def record(name, *a):
        if name == "geossl_eval_collect":
            at_collect.append(reads[0])
        return real_record(name, *a)
    rec._record = record
    captures = dense.ev.captures
    out = rec.step(lambda: dense.ev.run(dense.loader, arrays=True))
    (names,) = rec.steps
    print("calls of one pass:", " ".join(names))
    assert dense.ev.captures == captures and replays[0] == 3 and out[2] == 22
    # (the fill is Bucket.fill's, as the training step makes it: the gather launch, and for PaiNN the edge layout of the
    # gathered radius edges behind it)
    fill = {"schnet": ["gather_molecules"], "painn": ["gather_molecules", "painn_edge_layout"]}[dense.kind]
    assert names == (fill + ["property_targets", "eval_collect"]) * 3
    assert at_collect == [0, 0, 0]                 # nothing was read before the last batch was collected
    assert reads[0] >= 3                           # ... and behind the loop: the accumulator and the two arrays
