"""What the GPU tests of every objective's replayed step share: the stock backbones, the ragged batches and DeviceLoader
handles they run on, and the checks themselves - a replayed step against the eager one, one capacity-bucket graph, the
reference loop with a stock torch.optim.Adam against the trainer, a profile with the library's kernels only.  An objective
states what is its own in one ``Case``; nothing here knows an objective by name."""
import re
import types

import numpy as np
import pytest
import torch

from conftest import rel_err
from helpers import fill_module_

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def lib_loaded():
    """Loads the library once per test module that imports this fixture by name."""
    from geossl_amd import _lib
    _lib.load()


# ------------------------------------------------------------------------------------------------------- builders
def backbone(kind):
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    return (fill_module_(SchNet(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51,
                                cutoff=10.0, node_class=9)) if kind == "schnet" else
            fill_module_(PaiNN(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1,
                               readout="add"))).to(DEV)


def device_batch(collated, rng=None):
    from geossl_amd import pretrain_GeoSSL as pg
    return pg.Batch.from_numpy(collated, DEV)


def ragged_batches(n, B, seed, option="permutation", decorate=device_batch):
    """n batches of B molecules drawn in shuffled order from a pool of 4 B ragged ones.  ``decorate(collated, rng)`` turns
    one collated host batch (synthetic.collate_subset's dict) into the device batch, right after its molecules were
    drawn: where an objective hangs its targets (from ``rng``, the stream the molecules came from) or its triples."""
    from geossl_amd.synthetic import collate_subset, make_batch
    pool = make_batch(4 * B, seed=seed, mode="B", option=option)
    rng = np.random.default_rng(seed)
    return [decorate(collate_subset(pool, rng.permutation(4 * B)[:B], option=option), rng) for _ in range(n)]


def with_radius_edges(batches, r=5.0):
    from geossl_amd import ops
    for b in batches:
        b.radius_edge_index = ops.radius_graph(b.positions, r, b.batch)
    return batches


def loader_handles(kind, n=4, dataset_kw=None, loader_kw=None, dataset=None):
    """The first n handles of a shuffled DeviceLoader over 200 ragged molecules (or over ``dataset``)."""
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    from geossl_amd.synthetic import make_molecules
    if dataset is None:
        kw = {"option": "permutation"}
        if kind == "painn":
            kw["radius"] = 5.0
        kw.update(dataset_kw or {})
        mols = kw.pop("mols", None)
        dataset = DeviceDataset.from_numpy(make_molecules(200, seed=3, mode="C") if mols is None else mols, DEV, **kw)
    kw = dict(batch_size=32, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(2))
    kw.update(loader_kw or {})
    return [hb for _, hb in zip(range(n), DeviceLoader(dataset, **kw))]


# ------------------------------------------------------------------------------------------------------- the case
class Case:
    """One objective's replayed step, as data and callables.

    name, slot       the objective, and the attribute of the backbone its step engine lives under
    heads(kind, model) -> the list of head modules
    args(kind)       -> the namespace the step reads
    step(args, batch, model, heads, graph) -> (loss, extras): the do_* entry point; ``extras`` is a tuple compared
                     exactly (tensors bit for bit), empty where the step returns a loss alone
    aten_step(args, batch, model, heads) -> (loss, extras): what the three-way reference loop measures against
    trainer(model, heads, **kw) -> the StepTrainer
    head_weight(heads) -> the head parameter whose trajectory the Adam comparisons follow
    batches(n, B, seed) -> the ragged batches of the Adam comparisons
    prepare(batch, k) -> reset(): called once per batch; ``reset`` runs before the eager and before the replayed step
    observe(batch)   -> more extras, read off the batch after either step
    begin_loop()     runs before each training loop of the Adam comparisons
    loss_of(out)     the loss in what trainer.step returns
    views            views of the molecules in the bucket
    loss_tol, grad_tol   replayed against eager, where an objective's differ from compare_runs' own"""

    def __init__(self, name, slot, heads, args, step, trainer, aten_step=None, head_weight=None, batches=ragged_batches,
                 prepare=lambda batch, k: (lambda: None), observe=lambda batch: (), begin_loop=lambda: None,
                 loss_of=lambda out: out, views=1, loss_tol=1e-6, grad_tol=1e-5):
        self.name, self.slot, self.heads, self.args, self.step, self.trainer = name, slot, heads, args, step, trainer
        self.aten_step, self.head_weight, self.batches = aten_step, head_weight, batches
        self.prepare, self.observe, self.begin_loop, self.loss_of = prepare, observe, begin_loop, loss_of
        self.views, self.loss_tol, self.grad_tol = views, loss_tol, grad_tol


def kind_args(**kw):
    """``Case.args`` of an objective whose namespace is model_3d plus constants."""
    return lambda kind: types.SimpleNamespace(model_3d=kind, **kw)


# ------------------------------------------------------------------------------------------------------- comparisons
def _same(a, b):
    return torch.equal(a, b) if torch.is_tensor(a) else a == b


def compare_runs(eager, replayed, where, loss_tol=1e-6, grad_tol=1e-5):
    """A run is (loss, extras, gradients): the replayed one has the eager one's loss and every gradient within the
    bounds (relative l2; a NaN passes neither), its extras exactly, and as many gradients."""
    assert rel_err(replayed[0].cpu(), eager[0].cpu()) < loss_tol, where
    assert len(replayed[1]) == len(eager[1]) and all(_same(a, c) for a, c in zip(replayed[1], eager[1])), where
    assert len(replayed[2]) == len(eager[2]), where
    for a, c in zip(replayed[2], eager[2]):
        assert rel_err(a, c) < grad_tol, where


def _zero_grad(model, heads):
    for m in [model] + list(heads):
        m.zero_grad(set_to_none=True)


def _grads(model, heads):
    return [p.grad.clone() for m in [model] + list(heads) for p in m.parameters() if p.grad is not None]


def replay_vs_eager(case, kind, model, heads, batches):
    """Every batch through the eager step, then the replayed one: same loss, extras and gradients.  Returns the engine's
    single StepGraphs."""
    args = case.args(kind)
    for k, b in enumerate(batches):
        out = []
        reset = case.prepare(b, k)
        for graph in (False, True):
            reset()
            _zero_grad(model, heads)
            loss, extras = case.step(args, b, model, heads, graph)
            loss.backward()
            out.append((loss.detach().clone(), extras + case.observe(b), _grads(model, heads)))
        compare_runs(out[0], out[1], (kind, k), case.loss_tol, case.grad_tol)
    eng = model.__dict__[case.slot]
    (sg,) = eng.graphs.values()
    return sg


def assert_one_bucket(sg, views=None):
    """The graph table holds one graph, a capacity bucket's (of ``views`` views of the molecules, where given)."""
    assert len(sg) == 1 and next(iter(sg.graphs))[0] == "bucket"
    assert views is None or sg.views == views


# ------------------------------------------------------------------------------------------------------- stock Adam
def _stock_adam(model, heads):
    return torch.optim.Adam([{"params": model.parameters(), "lr": 1e-4},
                             {"params": [p for h in heads for p in h.parameters()], "lr": 1e-4}], lr=1e-4)


def _assert_same_weights(case, m2, h2, m1, h1):
    assert rel_err(case.head_weight(h2).detach().cpu(), case.head_weight(h1).detach().cpu()) < 1e-4
    assert rel_err(m2.lin2.weight.detach().cpu(), m1.lin2.weight.detach().cpu()) < 1e-4


def _three_way(case, n, B, seed):
    args = case.args("schnet")

    def ref_loop(fused):
        m = backbone("schnet")
        hd = case.heads("schnet", m)
        opt = _stock_adam(m, hd)
        case.begin_loop()
        losses, extras = [], []
        for b in case.batches(n, B, seed):
            loss, ex = case.step(args, b, m, hd, True) if fused else case.aten_step(args, b, m, hd)
            losses.append(float(loss.detach()))
            extras.append(ex)
            opt.zero_grad()
            loss.backward()
            opt.step()
        return losses, extras, m, hd

    ref, ref_extras, m1, h1 = ref_loop(False)
    rep, rep_extras, _, _ = ref_loop(True)
    np.testing.assert_allclose(rep, ref, rtol=1e-4)
    m2 = backbone("schnet")
    h2 = case.heads("schnet", m2)
    tr = case.trainer(m2, h2, lr=1e-4, use_graph=True)
    case.begin_loop()
    got = [tr.step(b) for b in case.batches(n, B, seed)]
    np.testing.assert_allclose([float(case.loss_of(o)) for o in got], ref, rtol=1e-4)
    _assert_same_weights(case, m2, h2, m1, h1)
    assert_one_bucket(tr.step_graphs)
    return types.SimpleNamespace(ref_extras=ref_extras, rep_extras=rep_extras, trainer_out=got, trainer=tr)


def _lock_step(case, n, B, seed):
    batches = case.batches(n, B, seed)
    assert len({tuple(b._sizes) for b in batches}) == n   # (no size sequence repeats)
    m1 = backbone("schnet")
    h1 = case.heads("schnet", m1)
    m2 = backbone("schnet")
    h2 = case.heads("schnet", m2)
    opt = _stock_adam(m1, h1)
    tr = case.trainer(m2, h2, lr=1e-4, use_graph=True)
    args = case.args("schnet")
    for k, b in enumerate(batches):
        loss, _ = case.step(args, b, m1, h1, False)
        opt.zero_grad()
        loss.backward()
        opt.step()
        l2 = case.loss_of(tr.step(b))
        assert rel_err(l2.cpu(), loss.detach().cpu()) < 1e-4, k
    _assert_same_weights(case, m2, h2, m1, h1)
    # one graph for the batch size (a batch that outgrows the first bucket's capacity replaces it by a larger one)
    assert len(tr.step_graphs) == 1 and 1 <= tr.step_graphs.captures <= 2
    (key, g), = tr.step_graphs.graphs.items()
    assert key[0] == "bucket" and g["bucket"].views == case.views
    return types.SimpleNamespace(batches=batches, trainer=tr)


def reference_loop_vs_trainer(case, n, B, seed, per_step):
    """n steps at lr 1e-4 on ragged batches of B, a stock torch.optim.Adam over the reference's two groups against the
    trainer's replayed bucket graph, to 1e-4 on the losses and on a head and a backbone weight.

    per_step: the loop on eager launches and the trainer advance batch by batch, each loss compared as it comes.
    Otherwise three whole runs: the reference's ATen loop, the reference loop on replayed steps, the trainer."""
    return (_lock_step if per_step else _three_way)(case, n, B, seed)


# ------------------------------------------------------------------------------------------------------- launches
ATEN_BOOKKEEPING = {"aten::empty", "aten::empty_like", "aten::empty_strided", "aten::to", "aten::_to_copy", "aten::detach",
                    "detach", "aten::contiguous", "aten::slice", "aten::as_strided", "aten::view", "aten::lift_fresh",
                    "aten::alias", "aten::resize_", "aten::copy_"}


def gpu_kernels(prof):
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
            and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]


def library_kernel(name):
    return (re.match(r"(void )?(geossl::)?k_\w+", name.replace("(anonymous namespace)::", "")) is not None
            and "at::" not in name)


def assert_only_library_kernels(fn, also_allowed=()):
    """``fn()`` (run with gradients added into dense .grad buffers, as a replayed step captures it) calls no ATen
    operator besides allocation and view bookkeeping and launches only the library's kernels.  Returns their names."""
    from torch.profiler import ProfilerActivity, profile
    from geossl_amd import _lib
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with _lib.direct_grads():
            fn()
        torch.cuda.synchronize()
    allowed = ATEN_BOOKKEEPING | set(also_allowed)
    names = {e.name for e in prof.events() if e.name.startswith("aten::")}
    assert names <= allowed, names - allowed
    kernels = gpu_kernels(prof)
    others = sorted({n for n in kernels if not library_kernel(n)})
    assert kernels and not others, others
    return kernels
