"""_SchNetCore makes the same launches, in the same order, whichever form the radius graph of the forward has.

One eager forward + backward of a small SchNet per case, with `call` of `schnet`, `ops` and `_lib` wrapped by a recorder:
the sequence of C entry points must be the literal list below.  The lists were RECORDED ON THE PARENT of the commit that
gave `_SchNetCore` its pair-graph object (ops.PairGraph) and its one operation list per pass - by the same few lines of
recorder, run from a job script on the code before the refactor, not on the code under test - so the test states that
the refactor (and whatever touches the graph form next) changes no launch.  What the launches compute is the subject
of the parity tests (test_gpu_live_pairs.py, test_gpu_sparse_pairs.py, test_gpu_parity.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUTOFF = 3.0
SWITCHES = ("GEOSSL_NO_LAYER_LOOP", "GEOSSL_LAYER_LOOP", "GEOSSL_LIVE_PAIRS", "GEOSSL_SPARSE_PAIRS", "GEOSSL_NO_CHAIN",
            "GEOSSL_ARITH_24BIT", "GEOSSL_NO_RAGGED_LOOP")
UNIFORM, RAGGED, LONE = (5, 5, 5, 5), (1, 2, 3, 7, 12), (1, 1, 1)
# case: (molecule sizes, switches, parameter gradients, position gradient, torch.no_grad())
# (Launched eagerly the layer loop is attempted only under GEOSSL_LAYER_LOOP=1 - by default it belongs to graph captures
# - so "uniform, loop" sets it; "uniform, default" is the same batch with no switch at all.)
CASES = {
    "uniform, loop": (UNIFORM, {"GEOSSL_LAYER_LOOP": "1"}, True, False, False),
    "uniform, default": (UNIFORM, {}, True, False, False),
    "uniform, no loop": (UNIFORM, {"GEOSSL_NO_LAYER_LOOP": "1"}, True, False, False),
    "ragged, live list": (RAGGED, {}, True, False, False),
    "ragged, every slot": (RAGGED, {"GEOSSL_LIVE_PAIRS": "0"}, True, False, False),
    "ragged, positions only": (RAGGED, {}, False, True, False),          # (no list is built)
    "ragged, positions + parameters": (RAGGED, {}, True, True, False),   # (list built, forward dense, T regrouped)
    "sparse": (RAGGED, {"GEOSSL_SPARSE_PAIRS": "1"}, True, True, False),
    "no pairs": (LONE, {}, True, False, False),                          # (every P > 0 guard)
    "one Linear per launch": (RAGGED, {"GEOSSL_NO_CHAIN": "1"}, True, False, False),
    "inference": (RAGGED, {}, True, False, True),
}
# entry points without their "geossl_" prefix, in launch order
EXPECTED = {
    'uniform, loop': """
        embedding_fwd_dyn pair_geometry_live live_pairs_build cfconv_filter_fwd_rows chain_prepare
        schnet_layer_loop_ragged segment_reduce_fwd segment_reduce_bwd schnet_layer_loop_ragged linear_wgrad_dyn
        embedding_bwd_dyn cfconv_filter_bwd_dyn""",
    'uniform, default': """
        embedding_fwd_dyn pair_geometry_live live_pairs_build cfconv_filter_fwd_rows chain_prepare linear_chain_dyn
        cfconv_aggregate linear_chain_dyn cfconv_aggregate linear_chain_dyn linear_chain_dyn segment_reduce_fwd
        segment_reduce_bwd linear_chain_dyn linear_chain_dyn cfconv_aggregate linear_chain_dyn cfconv_aggregate
        linear_chain_dyn linear_wgrad_dyn embedding_bwd_dyn cfconv_filter_bwd_dyn""",
    'uniform, no loop': """
        embedding_fwd_dyn pair_geometry_live live_pairs_build cfconv_filter_fwd_rows chain_prepare linear_chain_dyn
        cfconv_aggregate linear_chain_dyn cfconv_aggregate linear_chain_dyn linear_chain_dyn segment_reduce_fwd
        segment_reduce_bwd linear_chain_dyn linear_chain_dyn cfconv_aggregate linear_chain_dyn cfconv_aggregate
        linear_chain_dyn linear_wgrad_dyn embedding_bwd_dyn cfconv_filter_bwd_dyn""",
    'ragged, live list': """
        embedding_fwd_dyn pair_geometry_live live_pairs_build cfconv_filter_fwd_rows chain_prepare linear_chain_dyn
        cfconv_aggregate linear_chain_dyn cfconv_aggregate linear_chain_dyn linear_chain_dyn segment_reduce_fwd
        segment_reduce_bwd linear_chain_dyn linear_chain_dyn cfconv_aggregate linear_chain_dyn cfconv_aggregate
        linear_chain_dyn linear_wgrad_dyn embedding_bwd_dyn cfconv_filter_bwd_dyn""",
    'ragged, every slot': """
        embedding_fwd_dyn pair_geometry cfconv_filter_fwd_dyn chain_prepare linear_chain_dyn cfconv_aggregate
        linear_chain_dyn cfconv_aggregate linear_chain_dyn linear_chain_dyn segment_reduce_fwd segment_reduce_bwd
        linear_chain_dyn linear_chain_dyn cfconv_aggregate linear_chain_dyn cfconv_aggregate linear_chain_dyn
        linear_wgrad_dyn embedding_bwd_dyn cfconv_filter_bwd_dyn""",
    'ragged, positions only': """
        embedding_fwd_dyn pair_geometry cfconv_filter_fwd_dyn chain_prepare linear_chain_dyn cfconv_aggregate
        linear_chain_dyn cfconv_aggregate linear_chain_dyn linear_chain_dyn segment_reduce_fwd segment_reduce_bwd
        chain_prepare linear_chain_dyn linear_chain_dyn cfconv_aggregate linear_chain_dyn cfconv_aggregate
        linear_chain_dyn cfconv_filter_dpos pair_position_grad""",
    'ragged, positions + parameters': """
        embedding_fwd_dyn pair_geometry_live live_pairs_build cfconv_filter_fwd_dyn chain_prepare linear_chain_dyn
        cfconv_aggregate linear_chain_dyn cfconv_aggregate linear_chain_dyn linear_chain_dyn segment_reduce_fwd
        segment_reduce_bwd linear_chain_dyn linear_chain_dyn cfconv_aggregate linear_chain_dyn cfconv_aggregate
        linear_chain_dyn linear_wgrad_dyn embedding_bwd_dyn gather_live_rows cfconv_filter_bwd_dyn
        cfconv_filter_dpos pair_position_grad""",
    'sparse': """
        embedding_fwd_dyn sparse_pairs_build cfconv_filter_fwd_dyn chain_prepare linear_chain_dyn
        cfconv_aggregate_sparse linear_chain_dyn cfconv_aggregate_sparse linear_chain_dyn linear_chain_dyn
        segment_reduce_fwd segment_reduce_bwd linear_chain_dyn linear_chain_dyn cfconv_aggregate_sparse
        linear_chain_dyn cfconv_aggregate_sparse linear_chain_dyn linear_wgrad_dyn embedding_bwd_dyn
        cfconv_filter_bwd_dyn cfconv_filter_dpos pair_position_grad_sparse""",
    'no pairs': """
        embedding_fwd_dyn chain_prepare linear_chain_dyn cfconv_aggregate linear_chain_dyn cfconv_aggregate
        linear_chain_dyn linear_chain_dyn segment_reduce_fwd segment_reduce_bwd linear_chain_dyn linear_chain_dyn
        cfconv_aggregate linear_chain_dyn cfconv_aggregate linear_chain_dyn linear_wgrad_dyn embedding_bwd_dyn""",
    'one Linear per launch': """
        embedding_fwd_dyn pair_geometry_live live_pairs_build cfconv_filter_fwd_rows linear_prepare linear_prepared
        cfconv_aggregate linear_prepared linear_prepared linear_prepared cfconv_aggregate linear_prepared
        linear_prepared linear linear segment_reduce_fwd segment_reduce_bwd linear linear linear_prepare
        linear_prepared linear_prepared cfconv_aggregate linear_prepared linear_prepared linear_prepared
        cfconv_aggregate linear_prepared linear_wgrad_dyn embedding_bwd_dyn cfconv_filter_bwd_dyn""",
    'inference': """
        embedding_fwd_dyn pair_geometry_live live_pairs_build cfconv_filter_fwd_rows chain_prepare linear_chain_dyn
        cfconv_aggregate linear_chain_dyn cfconv_aggregate linear_chain_dyn linear_chain_dyn segment_reduce_fwd""",
}


def _batch(sizes):
    from geossl_amd.synthetic import make_batch
    return make_batch(0, seed=11, sizes=list(sizes))


def test_ragged_batch_has_dead_and_live_slots():
    """At 3.0 A the ragged batch has pair slots with and without an edge: the live-list and every-slot cases differ."""
    b = _batch(RAGGED)
    pos, off = b["positions"].astype(np.float64), np.concatenate([[0], np.cumsum(b["sizes"])])
    d = np.concatenate([np.linalg.norm(pos[o:e, None] - pos[None, o:e], axis=2)[np.triu_indices(e - o, k=1)]
                        for o, e in zip(off[:-1], off[1:])])
    assert d.size == sum(n * (n - 1) // 2 for n in RAGGED) and (d < CUTOFF - 1e-3).any() and (d > CUTOFF + 1e-3).any()
    assert EXPECTED["ragged, live list"] != EXPECTED["ragged, every slot"]


@pytest.mark.parametrize("case", list(CASES))
def test_schnet_core_launch_sequence(case, monkeypatch):
    import geossl_amd.Geom3D.models.schnet as sm
    from geossl_amd import _lib, ops
    from helpers import product_schnet, t
    sizes, switches, want_params, want_pos, no_grad = CASES[case]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    b = _batch(sizes)
    model = product_schnet(dict(hidden_channels=128, num_filters=128, num_interactions=2, num_gaussians=8, cutoff=CUTOFF,
                                node_class=9, readout="add"), DEV)
    for p in model.parameters():
        p.requires_grad_(want_params and p.requires_grad)
    pos = t(b["positions"], DEV).requires_grad_(want_pos)
    w = torch.cos(torch.arange(128, dtype=torch.float32, device=DEV))
    names = []
    real = _lib.call

    def recorder(name, *a):
        names.append(name)
        return real(name, *a)

    for mod in (sm, ops, _lib):
        monkeypatch.setattr(mod, "call", recorder)
    with torch.set_grad_enabled(not no_grad):
        out, h = model(t(b["x"], DEV)[:, 0], pos, t(b["batch"], DEV), return_latent=True)
        if not no_grad:
            ((h ** 2).sum() + (out * w).sum()).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(h).all()
    assert names == ["geossl_" + n for n in EXPECTED[case].split()], names
