"""`step.run_graphed`, the routing every do_* function shares, decides without a device: whether a step goes to the graph
engine at all (the `graph=` argument, then `args.step_graph`, then the GEOSSL_NO_STEP_GRAPH switch; only with gradients
wanted) and what it hands the engine (the step-args object with `step_graph_mode` on it, the batch, the caller's noise).
The engine is a stub: `step.engine_for` is replaced, so nothing here builds graphs or touches a GPU."""
import types

import pytest
import torch


class _Engine:
    def __init__(self):
        self.runs = []

    def run(self, args, batch, noise=None):
        self.runs.append((args, batch, noise))
        return "replayed"


@pytest.fixture
def route(monkeypatch):
    """-> (run_graphed with the stub engine behind it, the list of engine_for calls, the stub)."""
    from geossl_amd import step
    built, eng = [], _Engine()

    def engine_for(model, slot, objective, n1=None, n2=None):
        built.append((model, slot, objective, n1, n2))
        return eng
    monkeypatch.setattr(step, "engine_for", engine_for)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.delenv("GEOSSL_NO_STEP_GRAPH", raising=False)

    def run(args, graph, **kw):
        return step.run_graphed(args, graph, "model", "slot", "objective", types.SimpleNamespace(), "batch", **kw)
    return run, built, eng


def test_default_is_on_and_the_engine_gets_the_step(route):
    run, built, eng = route
    assert run(types.SimpleNamespace(), None, noise={"k": 1}, n1="head") == "replayed"
    assert built == [("model", "slot", "objective", "head", None)]
    (step_args, batch, noise), = eng.runs
    assert batch == "batch" and noise == {"k": 1} and step_args.step_graph_mode == "auto"


def test_explicit_graph_beats_args_step_graph(route):
    run, built, eng = route
    assert run(types.SimpleNamespace(step_graph=True), False) is None and not built
    assert run(types.SimpleNamespace(step_graph=False), True) == "replayed" and len(built) == 1


def test_args_step_graph_beats_the_environment_switch(route, monkeypatch):
    run, built, eng = route
    monkeypatch.setenv("GEOSSL_NO_STEP_GRAPH", "1")
    assert run(types.SimpleNamespace(), None) is None and not built               # the switch alone: off
    assert run(types.SimpleNamespace(step_graph=True), None) == "replayed"        # args.step_graph over the switch
    monkeypatch.delenv("GEOSSL_NO_STEP_GRAPH")
    assert run(types.SimpleNamespace(step_graph=False), None) is None and len(built) == 1


def test_no_engine_without_gradients_or_inside_a_capture(route, monkeypatch):
    run, built, eng = route
    with torch.no_grad():
        assert run(types.SimpleNamespace(), True) is None
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert run(types.SimpleNamespace(), True) is None
    assert not built and not eng.runs


def test_step_graph_mode_is_handed_over_and_prepare_sees_the_engine(route):
    run, built, eng = route
    seen = []
    assert run(types.SimpleNamespace(step_graph_mode="structure"), True, prepare=seen.append) == "replayed"
    assert seen == [eng] and eng.runs[0][0].step_graph_mode == "structure"


def test_one_stock_bce_predicate():
    from geossl_amd import finetune_lep, pretrain_3DInfoGraph, pretrain_GeoSSL
    from geossl_amd.step import stock_bce
    nn = torch.nn
    assert stock_bce(nn.BCEWithLogitsLoss()) and not stock_bce(None) and stock_bce(None, or_none=True)
    for c in (nn.BCEWithLogitsLoss(pos_weight=torch.ones(1)), nn.BCEWithLogitsLoss(reduction="sum"),
              nn.BCEWithLogitsLoss(weight=torch.ones(1)), nn.MSELoss(), type("Sub", (nn.BCEWithLogitsLoss,), {})()):
        assert not stock_bce(c) and not stock_bce(c, or_none=True)
    assert pretrain_3DInfoGraph.criterion_ok is stock_bce and finetune_lep.stock_bce is stock_bce
    assert pretrain_GeoSSL._stock_bce(None) and not pretrain_GeoSSL._stock_bce(nn.MSELoss())
