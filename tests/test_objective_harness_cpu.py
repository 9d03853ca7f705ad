"""The shared comparator of the objectives' GPU tests catches what each private one caught: compare_runs and
assert_one_bucket on hand-made CPU values."""
import pytest
import torch

from objective_harness import assert_one_bucket, compare_runs


def _run(loss=1.0, extras=(0.75, 3), grads=None):
    g = torch.Generator().manual_seed(0)
    grads = [torch.randn(7, 5, generator=g, dtype=torch.float64), torch.randn(11, generator=g, dtype=torch.float64)] \
        if grads is None else grads
    return torch.tensor(loss, dtype=torch.float64), extras, grads


def test_equal_runs_pass():
    compare_runs(_run(), _run(), "equal")
    compare_runs(_run(extras=()), _run(extras=()), "no extras")
    compare_runs(_run(loss=1.0), _run(loss=1.0 + 0.5e-6), "loss within the bound")
    grads = [g * (1 + 0.5e-5) for g in _run()[2]]
    compare_runs(_run(), _run(grads=grads), "gradients within the bound")
    mask = torch.arange(6)
    compare_runs(_run(extras=(mask,)), _run(extras=(mask.clone(),)), "tensor extras")


def _off(which):
    loss, extras, grads = _run()
    if which == "loss":
        loss = loss * (1 + 2e-6)
    elif which == "gradient":
        grads[1] = grads[1] * (1 + 2e-5)
    elif which == "count":
        extras = (0.75, 4)
    elif which == "tensor extra":
        return _run(extras=(torch.arange(6),)), _run(extras=(torch.arange(6).flip(0),))
    elif which == "missing gradient":
        grads = grads[:1]
    elif which == "nan":
        grads[0][3, 2] = float("nan")
    return _run(), (loss, extras, grads)


@pytest.mark.parametrize("which", ["loss", "gradient", "count", "tensor extra", "missing gradient", "nan"])
def test_a_run_that_differs_is_caught(which):
    eager, replayed = _off(which)
    with pytest.raises(AssertionError):
        compare_runs(eager, replayed, which)


def test_an_objectives_own_bound_is_used():
    eager, replayed = _run(), _run(loss=1.0 + 2e-7)
    compare_runs(eager, replayed, "default")
    with pytest.raises(AssertionError):
        compare_runs(eager, replayed, "tighter", loss_tol=1e-7)


class _Table:
    """The surface of replay.StepGraphs that assert_one_bucket reads."""

    def __init__(self, keys, views):
        self.graphs, self.views = {k: object() for k in keys}, views

    def __len__(self):
        return len(self.graphs)


def test_assert_one_bucket():
    assert_one_bucket(_Table([("bucket", 24, "permutation")], 1))
    assert_one_bucket(_Table([("bucket", 24, "permutation")], 1), views=1)
    for table, views in ((_Table([("bucket", 24, "permutation"), ("bucket", 32, "permutation")], 1), None),
                         (_Table([("sizes", "permutation", 100)], 1), None),
                         (_Table([], 1), None),
                         (_Table([("bucket", 24, "permutation")], 2), 1)):
        with pytest.raises(AssertionError):
            assert_one_bucket(table, views)
