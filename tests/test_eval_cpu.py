"""CPU tests of the evaluation passes (geossl_amd/evaluate.py, csrc/eval_collect.hip): the C ABI of the new entry, the
numpy twin of the kernel against closed forms, eval_Supervised on CPU modules against fixture G21 (the reference's lines),
and eval_LBA / eval_LEP with use_graph=True on CPU loaders, which take today's loop whole."""
import inspect
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import eval_twin as et
import test_supervised_cpu as sc
from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ surface
def test_entry_is_declared_bound_and_exported():
    import geossl_amd
    from geossl_amd import _lib, build, evaluate, ops
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    assert re.search(r"\bint geossl_eval_collect\(", h)
    assert "geossl_eval_collect" in _lib.PROTOTYPES
    assert getattr(_lib.load(), "geossl_eval_collect") is not None
    assert "eval_collect.hip" in build._sources()
    assert build.SOURCE_FLAGS.get("eval_collect.hip") == ["-fno-slp-vectorize"]
    for name in ("eval_buffer", "eval_collect", "eval_read"):
        assert callable(getattr(ops, name))
    assert "evaluate" in geossl_amd.__doc__
    sig = inspect.signature(evaluate.Evaluator).parameters
    assert list(sig)[:4] == ["model", "head", "model_3d", "kind"]
    assert (sig["task_id"].default, sig["max_graphs"].default, sig["graph_mode"].default) == (0, 64, "auto")
    assert sorted(evaluate.USE_GRAPH_DEFAULT) == ["pair", "property"]
    assert all(isinstance(v, bool) for v in evaluate.USE_GRAPH_DEFAULT.values())


def test_public_signatures():
    from geossl_amd.finetune_lba import eval_LBA
    from geossl_amd.finetune_lep import LEPTrainer, eval_LEP
    from geossl_amd.pretrain_Supervised import SupervisedTrainer, eval_Supervised
    ps = inspect.signature(eval_Supervised).parameters
    assert list(ps)[:8] == ["args", "loader", "model", "graph_pred_linear", "TRAIN_mean", "TRAIN_std", "task_id",
                            "use_graph"]
    assert ps["task_id"].default == 6 and ps["arrays"].default is True
    assert inspect.signature(eval_LBA).parameters["use_graph"].default is False
    assert inspect.signature(eval_LEP).parameters["use_graph"].default is False
    assert inspect.signature(SupervisedTrainer.evaluate).parameters["arrays"].default is True
    assert callable(LEPTrainer.evaluate)


# --------------------------------------------------------------------------------------------- the twin, closed forms
def test_twin_bce_at_large_logits():
    """|z| = 30: exp(-30) = 9.4e-14 is below half an ulp of 1 and of 30, so log1p(exp(-30)) = exp(-30) in fp32 and the
    term is that (z and y agree in sign) or 30 (+ exp(-30), absorbed) exactly."""
    tiny = np.float32(np.exp(np.float32(-30.0)))
    z = np.array([30.0, 30.0, -30.0, -30.0], dtype=np.float32)
    y = np.array([1.0, 0.0, 1.0, 0.0], dtype=np.float32)
    a, s = et.terms(z, y, et.BCE)
    assert a.dtype == np.float32 and not s.any()
    assert a[0] == tiny and a[3] == tiny and a[1] == np.float32(30.0) and a[2] == np.float32(30.0)
    acc = et.collect(z[[0, 3]], y[[0, 3]], et.BCE)
    assert acc == [2.0 * float(tiny), 0.0, 2]
    acc = et.collect(z[[1, 2]], y[[1, 2]], et.BCE, acc=acc)
    assert acc[2] == 4 and acc[1] == 0.0 and abs(acc[0] - 60.0) < 1e-12
    # z = 0: log 2 for either label
    a0, _ = et.terms([0.0, 0.0], [0.0, 1.0], et.BCE)
    assert np.all(a0 == np.float32(np.log1p(np.float32(1.0))))


def test_twin_regression_closed_forms():
    a, s = et.terms([1.5, -2.0], [1.5, -2.0], et.REGRESSION)           # d = 0
    assert not a.any() and not s.any()
    acc = et.collect([3.0], [1.0], et.REGRESSION)                      # B = 1
    assert acc == [2.0, 4.0, 1]
    op, ot = np.full(6, np.nan, np.float32), np.full(6, np.nan, np.float32)
    acc = et.collect([0.5, -1.0], [1.0, 1.0], et.REGRESSION, offset=3, out_pred=op, out_true=ot, acc=acc)
    assert acc == [2.0 + 0.5 + 2.0, 4.0 + 0.25 + 4.0, 3]
    assert np.isnan(op[:3]).all() and np.isnan(op[5]) and list(op[3:5]) == [0.5, -1.0] and list(ot[3:5]) == [1.0, 1.0]
    # the terms are fp32: a difference that fp32 cannot hold is rounded before it is squared
    a, s = et.terms([np.float32(1.0) + np.float32(2.0 ** -23)], [1.0], et.REGRESSION)
    assert a[0] == np.float32(2.0 ** -23) and s[0] == np.float32(2.0 ** -46)


# --------------------------------------------------------------------------------------------- eval_Supervised on CPU
def _g21(case):
    g = load_golden(case)
    meta = json.loads(str(g["meta"]))
    keys, ps = sc._head_params(g)
    head, _ = sc._cpu_head(keys, ps)
    batch = types.SimpleNamespace(x=torch.from_numpy(g["x"]), positions=torch.from_numpy(g["positions"]),
                                  batch=torch.from_numpy(g["batch"]), y=torch.from_numpy(g["y"]),
                                  radius_edge_index=torch.from_numpy(g["radius_edge_index"]) if "radius_edge_index" in g
                                  else None)
    return g, meta, sc._Fixed(torch.from_numpy(g["molecule_repr"])), head, batch


@pytest.mark.parametrize("use_graph", [False, True, None])
@pytest.mark.parametrize("case", sc.CASES)
def test_eval_supervised_on_cpu_reproduces_g21(case, use_graph):
    """CPU modules and CPU batches run the reference's lines (whatever use_graph says): G21's predictions de-normalised,
    the raw target column, and the MAE as the reference's line computes it from the two arrays."""
    from geossl_amd.pretrain_Supervised import eval_Supervised
    g, meta, model, head, batch = _g21(case)
    mean, std, task = float(g["TRAIN_mean"]), float(g["TRAIN_std"]), int(g["task_id"])
    args = types.SimpleNamespace(model_3d=meta["kind"], loss=meta["loss"])
    mae, y_true, y_scores = eval_Supervised(args, [batch, batch], model, head, mean, std, task_id=task,
                                            use_graph=use_graph)
    B = g["sizes"].size
    assert y_true.dtype == np.float32 and y_scores.dtype == np.float32 and y_true.shape == y_scores.shape == (2 * B,)
    col = g["y"].reshape(B, -1)[:, task]
    assert np.array_equal(y_true, np.concatenate([col, col]))
    want = np.concatenate([g["pred"].reshape(-1)] * 2).astype(np.float64) * std + mean
    sc._close(torch.from_numpy(y_scores), want, 1e-5, "y_scores")
    ref = np.mean(np.abs(y_scores - y_true))
    assert mae.dtype == ref.dtype and mae.tobytes() == ref.tobytes()
    only = eval_Supervised(args, [batch, batch], model, head, mean, std, task_id=task, use_graph=use_graph, arrays=False)
    assert isinstance(only, float) and only == float(ref)
    with pytest.raises(Exception, match="not included"):
        eval_Supervised(types.SimpleNamespace(model_3d="egnn"), [batch], model, head, mean, std)


# --------------------------------------------------------------------------------------- eval_LBA / eval_LEP on CPU
class _Backbone(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3, 4)

    def forward(self, x, positions, batch):
        B = int(batch.max()) + 1
        return torch.zeros(B, 4).index_add_(0, batch, self.lin(positions) * x[:, None])


class _Pockets:
    def __init__(self, n):
        g = torch.Generator().manual_seed(n)
        self.x = torch.arange(1, 4 * n + 1, dtype=torch.float32)
        self.positions = torch.randn(4 * n, 3, generator=g)
        self.batch = torch.repeat_interleave(torch.arange(n), 4)
        self.y = torch.randn(n, generator=g)
        self.num_graphs = n

    def to(self, device):
        return self


class _Pairs:
    def __init__(self, n):
        a, i = _Pockets(n), _Pockets(n + 7)
        self.x_active, self.positions_active, self.batch_active = a.x, a.positions, a.batch
        self.x_inactive, self.positions_inactive = i.x[:4 * n], i.positions[:4 * n]
        self.batch_inactive = a.batch
        self.y = (torch.arange(n) % 2).long()
        self.num_graphs = n

    def to(self, device):
        return self


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_eval_lba_and_lep_with_use_graph_on_cpu_take_todays_loop():
    from geossl_amd.finetune_lba import eval_LBA
    from geossl_amd.finetune_lep import eval_LEP
    torch.manual_seed(0)
    args = types.SimpleNamespace(model_3d="schnet")
    model, head = _Backbone(), torch.nn.Linear(4, 1)
    loader = [_Pockets(3), _Pockets(2), _Pockets(1)]
    ref = eval_LBA(args, loader, model, head)
    got = eval_LBA(args, loader, model, head, use_graph=True)
    assert len(ref) == 5 and len(ref[3]) == 6 and all(_same(r, g_) for r, g_ in zip(ref, got))
    head2 = torch.nn.Linear(8, 1)
    pairs = [_Pairs(4), _Pairs(3), _Pairs(2)]
    ref = eval_LEP(args, pairs, model, head2)
    got = eval_LEP(args, pairs, model, head2, use_graph=True)
    assert len(ref) == 5 and ref[3].shape == (9,) and np.isfinite(ref[0]) and all(_same(r, g_) for r, g_ in zip(ref, got))
    assert "evaluator" not in "".join(model.__dict__)   # (no evaluator was made for CPU modules)
