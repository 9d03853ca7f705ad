"""_PaiNNCore makes the same launches, in the same order, with the same arguments, on every interaction route.

One eager forward + backward of a small PaiNN per case, with `call` of `painn`, `ops` and `_lib` wrapped by a recorder:
the sequence of C entry points AND of their arguments must be the literal below.  An argument that is None, a float or
an integer below 2^31 is recorded by value (`-` = None/NULL); everything else - device addresses, stream handles, ctypes
references - as the placeholder `*`.  That pins `stage_f`, the list lengths, `acc`, the 0 / 1 of
geossl_painn_edge_grads and every NULL (mu, mu3, dmu, dN), which a change of route keeps the names of.  The literals
were RECORDED ON THE PARENT of the commit that gave `_PaiNNCore` its route object (ops.PaiNNRoute) - by `run_case`
below, run from a job script on the code before the refactor, not on the code under test - so the test states that the
refactor (and whatever adds a route next) changes no launch.  What the launches compute is the subject of the parity
tests (test_gpu_parity.py, test_gpu_painn_mma.py, test_gpu_painn_tile.py, test_gpu_round5.py).  The bucket routes run
through geossl_amd/bucket.py (test_gpu_masked_painn_bucket.py, test_gpu_painn_sparse_bucket.py)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUTOFF = 5.0
RAGGED, BIG, TILE, LONE = (1, 2, 3, 7, 12), (3, 80), (260, 3), (1, 1, 1)
# case: (molecule sizes, n_atom_basis, switches, parameter gradients, position gradient, torch.no_grad())
CASES = {
    "matrix pipe": (RAGGED, 128, {}, True, False, False),
    "vector": (RAGGED, 128, {"GEOSSL_PAINN_VECTOR": "1"}, True, False, False),
    "F = 64": (RAGGED, 64, {}, True, False, False),                    # (one chained launch per block, silu launches)
    "80 atoms, default": (BIG, 128, {}, True, False, False),           # (forward off the matrix pipe, backward split)
    "80 atoms, forward split": (BIG, 128, {"GEOSSL_PAINN_MMA_CAP": "44"}, True, False, False),
    "80 atoms, no split": (BIG, 128, {"GEOSSL_PAINN_NO_SPLIT": "1"}, True, False, False),
    "tile by switch": (RAGGED, 128, {"GEOSSL_PAINN_TILE": "1"}, True, False, False),
    "tile by size": (TILE, 128, {}, True, False, False),
    "forces + parameters": (RAGGED, 128, {}, True, True, False),
    "forces only": (RAGGED, 128, {}, False, True, False),
    "mu kept": (RAGGED, 128, {"GEOSSL_PAINN_NO_MU_ZERO": "1"}, True, False, False),
    "one Linear per launch": (RAGGED, 128, {"GEOSSL_PAINN_NO_CHAIN": "1"}, True, False, False),
    "silu launches": (RAGGED, 128, {"GEOSSL_PAINN_SILU_KERNELS": "1"}, True, False, False),
    "inference": (RAGGED, 128, {}, True, False, True),
    "no edges": (LONE, 128, {}, True, False, False),
}


def _value(a):
    if a is None:
        return "-"
    if isinstance(a, float) or (isinstance(a, int) and not isinstance(a, bool) and -2 ** 31 <= a < 2 ** 31):
        return repr(a)
    return "*"


def run_case(case, setenv, delenv, patch):
    """-> (the launches of one forward + backward as "name(arg,arg,...)" without the geossl_ prefix, the values q, out,
    dpos and every parameter gradient).  setenv / delenv / patch: monkeypatch's (or a job script's own)."""
    import geossl_amd.Geom3D.models.painn as pm
    from filler import fill_module_
    from geossl_amd import _lib, ops
    from geossl_amd.layout import prepare_batch
    from geossl_amd.synthetic import make_batch
    from helpers import t
    sizes, F, switches, want_params, want_pos, no_grad = CASES[case]
    for k in [k for k in os.environ if k.startswith("GEOSSL_PAINN_")]:
        delenv(k)
    for k, v in switches.items():
        setenv(k, v)
    b = make_batch(0, seed=11, sizes=list(sizes))
    model = fill_module_(pm.PaiNN(n_atom_basis=F, n_interactions=2, n_rbf=20, cutoff=CUTOFF, n_out=1,
                                  readout="add")).to(DEV)
    for p in model.parameters():
        p.requires_grad_(want_params)
    pos, batch = t(b["positions"], DEV), t(b["batch"], DEV)
    prepare_batch(batch, None, sizes, lazy=True)   # (host sizes, as a loader leaves them: without them nothing splits)
    edges = ops.radius_graph(pos, CUTOFF, batch)
    pos.requires_grad_(want_pos)
    w = torch.cos(torch.arange(F, dtype=torch.float32, device=DEV))
    launches = []
    real = _lib.call

    def recorder(name, *a):
        launches.append("%s(%s)" % (name[len("geossl_"):], ",".join(_value(x) for x in a)))
        return real(name, *a)

    for mod in (pm, ops, _lib):
        patch(mod, "call", recorder)
    with torch.set_grad_enabled(not no_grad):
        out, q = model(t(b["x"], DEV), pos, edges, batch, return_latent=True)
        if not no_grad:
            ((q ** 2).sum() + (out * w).sum()).backward()
    torch.cuda.synchronize()
    for mod in (pm, ops, _lib):
        patch(mod, "call", real)
    values = {"q": q.detach(), "out": out.detach()}
    if pos.grad is not None:
        values["dpos"] = pos.grad
    values.update({"grad/" + n: p.grad for n, p in model.named_parameters() if p.grad is not None})
    return launches, values


def test_big_batch_is_above_both_stage_caps():
    """The 80-atom molecule lies above the LDS rows of the staged forward and of the staged backward, as the library
    reports them: the three "80 atoms" cases take three different sets of launches."""
    from geossl_amd import _lib
    lib = _lib.load()
    caps = [int(lib.geossl_painn_stage_cap(which, 128, 20)) for which in (0, 2)]
    assert all(0 < c < max(BIG) for c in caps), caps
    assert EXPECTED["80 atoms, forward split"] != EXPECTED["80 atoms, default"]
    assert EXPECTED["80 atoms, no split"] != EXPECTED["80 atoms, default"]


@pytest.mark.parametrize("case", list(CASES))
def test_painn_core_launch_sequence(case, monkeypatch):
    launches, values = run_case(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False),
                                monkeypatch.setattr)
    assert all(torch.isfinite(v).all() for v in values.values())
    assert launches == EXPECTED[case].split(), launches


# in launch order; written by the job script that ran `run_case` on the parent commit
EXPECTED = {
    'matrix pipe': """
        painn_edge_geom_dyn(*,*,*,182,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,25,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mma_dyn(*,-,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mma_dyn(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,-,-,0)
        segment_reduce_fwd(*,*,5,128,0,*,0) chain_prepare(*,22,128,0,0)
        painn_mix_post_bwd_dyn(*,-,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,384,*,25,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,256,*,75,128,-,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_mix_post_bwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,256,*,75,128,-,0)
        painn_interaction_bwd_mol(*,*,-,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,-,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) linear_wgrad_dyn(*,12,25,128,128,384,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,25,128,128,128,256,256,*,0,-,0)
        linear_wgrad_dyn(*,4,75,128,128,256,128,128,*,0,-,0)
        linear_wgrad_dyn(*,2,25,128,128,128,128,128,*,0,-,0) embedding_bwd_dyn(*,2,*,100,25,128,*,*,0,-,0)""",
    'vector': """
        painn_edge_geom_dyn(*,*,*,182,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,25,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,-,-,0)
        segment_reduce_fwd(*,*,5,128,0,*,0) chain_prepare(*,22,128,0,0)
        painn_mix_post_bwd_dyn(*,-,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,384,*,25,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,256,*,75,128,-,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_mix_post_bwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,256,*,75,128,-,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) linear_wgrad_dyn(*,12,25,128,128,384,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,25,128,128,128,256,256,*,0,-,0)
        linear_wgrad_dyn(*,4,75,128,128,256,128,128,*,0,-,0)
        linear_wgrad_dyn(*,2,25,128,128,128,128,128,*,0,-,0) embedding_bwd_dyn(*,2,*,100,25,128,*,*,0,-,0)""",
    'F = 64': """
        painn_edge_geom_dyn(*,*,*,182,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,25,64,*,*,-,0)
        chain_prepare(*,22,64,1,0) linear_chain_dyn(*,64,*,25,64,-,0) silu_fwd(*,1600,*,0)
        linear_chain_dyn(*,64,*,25,64,-,0) linear_chain_dyn(*,64,*,25,64,-,0) linear_chain_dyn(*,64,*,25,64,-,0)
        painn_interaction_fwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,64,20,*,*,0)
        linear_chain_dyn(*,64,*,75,64,-,0) linear_chain_dyn(*,64,*,75,64,-,0)
        painn_mix_pre_fwd_dyn(*,*,25,64,1e-08,*,*,-,0) linear_chain_dyn(*,128,*,25,64,-,0)
        linear_chain_dyn(*,128,*,25,64,-,0) silu_fwd(*,1600,*,0) linear_chain_dyn(*,64,*,25,64,-,0)
        linear_chain_dyn(*,64,*,25,64,-,0) linear_chain_dyn(*,64,*,25,64,-,0)
        painn_mix_post_fwd_dyn(*,*,*,*,*,25,64,*,*,-,0) linear_chain_dyn(*,64,*,25,64,-,0) silu_fwd(*,1600,*,0)
        linear_chain_dyn(*,64,*,25,64,-,0) linear_chain_dyn(*,64,*,25,64,-,0) linear_chain_dyn(*,64,*,25,64,-,0)
        painn_interaction_fwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,64,20,*,*,0)
        linear_chain_dyn(*,64,*,75,64,-,0) linear_chain_dyn(*,64,*,75,64,-,0)
        painn_mix_pre_fwd_dyn(*,*,25,64,1e-08,*,*,-,0) linear_chain_dyn(*,128,*,25,64,-,0)
        linear_chain_dyn(*,128,*,25,64,-,0) silu_fwd(*,1600,*,0) linear_chain_dyn(*,64,*,25,64,-,0)
        linear_chain_dyn(*,64,*,25,64,-,0) linear_chain_dyn(*,64,*,25,64,-,0)
        painn_mix_post_fwd_dyn(*,*,*,*,*,25,64,*,-,-,0) segment_reduce_fwd(*,*,5,64,0,*,0)
        chain_prepare(*,22,64,0,0) painn_mix_post_bwd_dyn(*,-,*,*,*,25,64,*,*,-,0)
        linear_chain_dyn(*,192,*,25,64,-,0) linear_chain_dyn(*,192,*,25,64,-,0)
        linear_chain_dyn(*,192,*,25,64,-,0) silu_bwd(*,*,1600,*,0) linear_chain_dyn(*,64,*,25,64,-,0)
        linear_chain_dyn(*,64,*,25,64,-,0) painn_mix_pre_bwd_dyn(*,*,*,*,25,64,*,*,-,0)
        linear_chain_dyn(*,128,*,75,64,-,0) linear_chain_dyn(*,128,*,75,64,-,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,64,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,192,*,25,64,-,0) linear_chain_dyn(*,192,*,25,64,-,0)
        linear_chain_dyn(*,192,*,25,64,-,0) silu_bwd(*,*,1600,*,0) linear_chain_dyn(*,64,*,25,64,-,0)
        painn_mix_post_bwd_dyn(*,*,*,*,*,25,64,*,*,-,0) linear_chain_dyn(*,192,*,25,64,-,0)
        linear_chain_dyn(*,192,*,25,64,-,0) linear_chain_dyn(*,192,*,25,64,-,0) silu_bwd(*,*,1600,*,0)
        linear_chain_dyn(*,64,*,25,64,-,0) linear_chain_dyn(*,64,*,25,64,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,25,64,*,*,-,0) linear_chain_dyn(*,128,*,75,64,-,0)
        linear_chain_dyn(*,128,*,75,64,-,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,64,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,192,*,25,64,-,0) linear_chain_dyn(*,192,*,25,64,-,0)
        linear_chain_dyn(*,192,*,25,64,-,0) silu_bwd(*,*,1600,*,0) linear_chain_dyn(*,64,*,25,64,-,0)
        linear_wgrad_dyn(*,12,25,64,64,192,64,64,*,0,-,0) linear_wgrad_dyn(*,4,25,64,64,64,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,75,64,64,128,64,64,*,0,-,0) linear_wgrad_dyn(*,2,25,64,64,64,64,64,*,0,-,0)
        embedding_bwd_dyn(*,2,*,100,25,64,*,*,0,-,0)""",
    '80 atoms, default': """
        painn_edge_geom_dyn(*,*,*,2471,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,83,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,83,128,-,0)
        painn_interaction_fwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,2,80,83,128,20,*,*,0)
        linear_chain_dyn(*,128,*,249,128,-,0) painn_mix_pre_fwd_dyn(*,*,83,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,83,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,83,128,*,*,-,0)
        linear_chain_dyn(*,128,*,83,128,-,0)
        painn_interaction_fwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,2,80,83,128,20,*,*,0)
        linear_chain_dyn(*,128,*,249,128,-,0) painn_mix_pre_fwd_dyn(*,*,83,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,83,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,83,128,*,-,-,0)
        segment_reduce_fwd(*,*,2,128,0,*,0) chain_prepare(*,22,128,0,0)
        painn_mix_post_bwd_dyn(*,-,*,*,*,83,128,*,*,-,0) linear_chain_dyn(*,384,*,83,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,83,128,*,*,-,0) linear_chain_dyn(*,256,*,249,128,-,0)
        painn_interaction_bwd_mol_skip(*,*,*,*,*,*,*,*,*,*,*,*,*,2,80,83,128,20,*,*,*,*,*,0,0)
        painn_interaction_bwd_atoms(*,*,*,*,*,*,*,*,*,*,*,*,*,80,-,128,20,*,*,*,*,*,1,0)
        linear_chain_dyn(*,384,*,83,128,-,0) painn_mix_post_bwd_dyn(*,*,*,*,*,83,128,*,*,-,0)
        linear_chain_dyn(*,384,*,83,128,-,0) painn_mix_pre_bwd_dyn(*,*,*,*,83,128,*,*,-,0)
        linear_chain_dyn(*,256,*,249,128,-,0)
        painn_interaction_bwd_mol_skip(*,*,*,*,*,*,*,*,*,*,*,*,*,2,80,83,128,20,*,*,*,*,*,0,0)
        painn_interaction_bwd_atoms(*,*,*,*,*,*,*,*,*,*,*,*,*,80,-,128,20,*,*,*,*,*,1,0)
        linear_chain_dyn(*,384,*,83,128,-,0) linear_wgrad_dyn(*,12,83,128,128,384,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,83,128,128,128,256,256,*,0,-,0)
        linear_wgrad_dyn(*,4,249,128,128,256,128,128,*,0,-,0)
        linear_wgrad_dyn(*,2,83,128,128,128,128,128,*,0,-,0) embedding_bwd_dyn(*,2,*,100,83,128,*,*,0,-,0)""",
    '80 atoms, forward split': """
        painn_edge_geom_dyn(*,*,*,2471,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,83,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,83,128,-,0)
        painn_interaction_fwd_mma_dyn(*,*,*,*,*,*,*,*,*,*,*,*,*,2,44,83,128,20,*,*,-,0)
        painn_interaction_fwd_atoms(*,*,*,*,*,*,*,*,*,*,*,*,80,-,128,20,*,*,0)
        linear_chain_dyn(*,128,*,249,128,-,0) painn_mix_pre_fwd_dyn(*,*,83,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,83,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,83,128,*,*,-,0)
        linear_chain_dyn(*,128,*,83,128,-,0)
        painn_interaction_fwd_mma_dyn(*,*,*,*,*,*,*,*,*,*,*,*,*,2,44,83,128,20,*,*,-,0)
        painn_interaction_fwd_atoms(*,*,*,*,*,*,*,*,*,*,*,*,80,-,128,20,*,*,0)
        linear_chain_dyn(*,128,*,249,128,-,0) painn_mix_pre_fwd_dyn(*,*,83,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,83,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,83,128,*,-,-,0)
        segment_reduce_fwd(*,*,2,128,0,*,0) chain_prepare(*,22,128,0,0)
        painn_mix_post_bwd_dyn(*,-,*,*,*,83,128,*,*,-,0) linear_chain_dyn(*,384,*,83,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,83,128,*,*,-,0) linear_chain_dyn(*,256,*,249,128,-,0)
        painn_interaction_bwd_mol_skip(*,*,*,*,*,*,*,*,*,*,*,*,*,2,80,83,128,20,*,*,*,*,*,0,0)
        painn_interaction_bwd_atoms(*,*,*,*,*,*,*,*,*,*,*,*,*,80,-,128,20,*,*,*,*,*,1,0)
        linear_chain_dyn(*,384,*,83,128,-,0) painn_mix_post_bwd_dyn(*,*,*,*,*,83,128,*,*,-,0)
        linear_chain_dyn(*,384,*,83,128,-,0) painn_mix_pre_bwd_dyn(*,*,*,*,83,128,*,*,-,0)
        linear_chain_dyn(*,256,*,249,128,-,0)
        painn_interaction_bwd_mol_skip(*,*,*,*,*,*,*,*,*,*,*,*,*,2,80,83,128,20,*,*,*,*,*,0,0)
        painn_interaction_bwd_atoms(*,*,*,*,*,*,*,*,*,*,*,*,*,80,-,128,20,*,*,*,*,*,1,0)
        linear_chain_dyn(*,384,*,83,128,-,0) linear_wgrad_dyn(*,12,83,128,128,384,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,83,128,128,128,256,256,*,0,-,0)
        linear_wgrad_dyn(*,4,249,128,128,256,128,128,*,0,-,0)
        linear_wgrad_dyn(*,2,83,128,128,128,128,128,*,0,-,0) embedding_bwd_dyn(*,2,*,100,83,128,*,*,0,-,0)""",
    '80 atoms, no split': """
        painn_edge_geom_dyn(*,*,*,2471,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,83,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,83,128,-,0)
        painn_interaction_fwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,2,80,83,128,20,*,*,0)
        linear_chain_dyn(*,128,*,249,128,-,0) painn_mix_pre_fwd_dyn(*,*,83,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,83,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,83,128,*,*,-,0)
        linear_chain_dyn(*,128,*,83,128,-,0)
        painn_interaction_fwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,2,80,83,128,20,*,*,0)
        linear_chain_dyn(*,128,*,249,128,-,0) painn_mix_pre_fwd_dyn(*,*,83,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,83,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,83,128,*,-,-,0)
        segment_reduce_fwd(*,*,2,128,0,*,0) chain_prepare(*,22,128,0,0)
        painn_mix_post_bwd_dyn(*,-,*,*,*,83,128,*,*,-,0) linear_chain_dyn(*,384,*,83,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,83,128,*,*,-,0) linear_chain_dyn(*,256,*,249,128,-,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,2,80,83,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,83,128,-,0) painn_mix_post_bwd_dyn(*,*,*,*,*,83,128,*,*,-,0)
        linear_chain_dyn(*,384,*,83,128,-,0) painn_mix_pre_bwd_dyn(*,*,*,*,83,128,*,*,-,0)
        linear_chain_dyn(*,256,*,249,128,-,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,2,80,83,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,83,128,-,0) linear_wgrad_dyn(*,12,83,128,128,384,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,83,128,128,128,256,256,*,0,-,0)
        linear_wgrad_dyn(*,4,249,128,128,256,128,128,*,0,-,0)
        linear_wgrad_dyn(*,2,83,128,128,128,128,128,*,0,-,0) embedding_bwd_dyn(*,2,*,100,83,128,*,*,0,-,0)""",
    'tile by switch': """
        painn_edge_geom_dyn(*,*,*,182,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,25,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_tile(*,-,*,*,*,*,*,*,*,*,*,-,25,-,128,20,*,*,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_tile(*,*,*,*,*,*,*,*,*,*,*,-,25,-,128,20,*,*,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,-,-,0)
        segment_reduce_fwd(*,*,5,128,0,*,0) chain_prepare(*,22,128,0,0)
        painn_mix_post_bwd_dyn(*,-,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,384,*,25,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,256,*,75,128,-,0)
        painn_interaction_bwd_tile(*,*,*,*,*,*,*,*,*,*,*,*,-,25,-,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_mix_post_bwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,256,*,75,128,-,0)
        painn_interaction_bwd_tile(*,*,-,*,*,*,*,*,*,*,*,*,-,25,-,128,20,*,-,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) linear_wgrad_dyn(*,12,25,128,128,384,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,25,128,128,128,256,256,*,0,-,0)
        linear_wgrad_dyn(*,4,75,128,128,256,128,128,*,0,-,0)
        linear_wgrad_dyn(*,2,25,128,128,128,128,128,*,0,-,0) embedding_bwd_dyn(*,2,*,100,25,128,*,*,0,-,0)""",
    'tile by size': """
        painn_edge_geom_dyn(*,*,*,8338,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,263,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,263,128,-,0)
        painn_interaction_fwd_tile(*,-,*,*,*,*,*,*,*,*,*,-,263,-,128,20,*,*,0)
        linear_chain_dyn(*,128,*,789,128,-,0) painn_mix_pre_fwd_dyn(*,*,263,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,263,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,263,128,*,*,-,0)
        linear_chain_dyn(*,128,*,263,128,-,0)
        painn_interaction_fwd_tile(*,*,*,*,*,*,*,*,*,*,*,-,263,-,128,20,*,*,0)
        linear_chain_dyn(*,128,*,789,128,-,0) painn_mix_pre_fwd_dyn(*,*,263,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,263,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,263,128,*,-,-,0)
        segment_reduce_fwd(*,*,2,128,0,*,0) chain_prepare(*,22,128,0,0)
        painn_mix_post_bwd_dyn(*,-,*,*,*,263,128,*,*,-,0) linear_chain_dyn(*,384,*,263,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,263,128,*,*,-,0) linear_chain_dyn(*,256,*,789,128,-,0)
        painn_interaction_bwd_tile(*,*,*,*,*,*,*,*,*,*,*,*,-,263,-,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,263,128,-,0) painn_mix_post_bwd_dyn(*,*,*,*,*,263,128,*,*,-,0)
        linear_chain_dyn(*,384,*,263,128,-,0) painn_mix_pre_bwd_dyn(*,*,*,*,263,128,*,*,-,0)
        linear_chain_dyn(*,256,*,789,128,-,0)
        painn_interaction_bwd_tile(*,*,-,*,*,*,*,*,*,*,*,*,-,263,-,128,20,*,-,*,*,*,0,0)
        linear_chain_dyn(*,384,*,263,128,-,0) linear_wgrad_dyn(*,12,263,128,128,384,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,263,128,128,128,256,256,*,0,-,0)
        linear_wgrad_dyn(*,4,789,128,128,256,128,128,*,0,-,0)
        linear_wgrad_dyn(*,2,263,128,128,128,128,128,*,0,-,0) embedding_bwd_dyn(*,2,*,100,263,128,*,*,0,-,0)""",
    'forces + parameters': """
        painn_edge_geom_dyn(*,*,*,182,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,25,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mma_dyn(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mma_dyn(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,-,-,0)
        segment_reduce_fwd(*,*,5,128,0,*,0) chain_prepare(*,22,128,0,0)
        painn_mix_post_bwd_dyn(*,-,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,384,*,25,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,256,*,75,128,-,0)
        painn_edge_grads(*,*,*,*,*,*,*,*,*,*,*,182,128,20,*,*,*,0,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_mix_post_bwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,256,*,75,128,-,0) painn_edge_grads(*,*,*,*,*,*,*,*,*,*,*,182,128,20,*,*,*,1,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_edge_geom_bwd(*,*,*,182,5.0,*,*,20,*,*,*,*,0)
        painn_position_grad(*,*,*,*,*,25,*,0) linear_wgrad_dyn(*,12,25,128,128,384,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,25,128,128,128,256,256,*,0,-,0)
        linear_wgrad_dyn(*,4,75,128,128,256,128,128,*,0,-,0)
        linear_wgrad_dyn(*,2,25,128,128,128,128,128,*,0,-,0) embedding_bwd_dyn(*,2,*,100,25,128,*,*,0,-,0)""",
    'forces only': """
        painn_edge_geom_dyn(*,*,*,182,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,25,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mma_dyn(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mma_dyn(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,-,-,0)
        segment_reduce_fwd(*,*,5,128,0,*,0) chain_prepare(*,22,128,0,0)
        painn_mix_post_bwd_dyn(*,-,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,384,*,25,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,256,*,75,128,-,0)
        painn_edge_grads(*,*,*,*,*,*,*,*,*,*,*,182,128,20,*,*,*,0,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_mix_post_bwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,256,*,75,128,-,0) painn_edge_grads(*,*,*,*,*,*,*,*,*,*,*,182,128,20,*,*,*,1,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_edge_geom_bwd(*,*,*,182,5.0,*,*,20,*,*,*,*,0)
        painn_position_grad(*,*,*,*,*,25,*,0)""",
    'mu kept': """
        painn_edge_geom_dyn(*,*,*,182,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,25,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mma_dyn(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mma_dyn(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        segment_reduce_fwd(*,*,5,128,0,*,0) chain_prepare(*,22,128,0,0)
        painn_mix_post_bwd_dyn(*,*,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,384,*,25,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,256,*,75,128,-,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_mix_post_bwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,384,*,25,128,-,0) painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,256,*,75,128,-,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) linear_wgrad_dyn(*,12,25,128,128,384,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,25,128,128,128,256,256,*,0,-,0)
        linear_wgrad_dyn(*,4,75,128,128,256,128,128,*,0,-,0)
        linear_wgrad_dyn(*,2,25,128,128,128,128,128,*,0,-,0) embedding_bwd_dyn(*,2,*,100,25,128,*,*,0,-,0)""",
    'one Linear per launch': """
        painn_edge_geom_dyn(*,*,*,182,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,25,128,*,*,-,0)
        linear(*,128,*,*,-,-,*,128,25,128,128,1,1,0) silu_fwd(*,3200,*,0)
        linear(*,128,*,*,-,-,*,384,25,128,128,1,1,0) linear(*,128,*,*,-,-,*,384,25,128,128,1,1,0)
        linear(*,128,*,*,-,-,*,384,25,128,128,1,1,0)
        painn_interaction_fwd_mma_dyn(*,-,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear(*,128,*,-,-,-,*,256,75,128,128,1,0,0) linear(*,128,*,-,-,-,*,256,75,128,128,1,0,0)
        painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0) linear(*,256,*,*,-,-,*,128,25,128,128,1,1,0)
        linear(*,256,*,-,*,-,*,128,25,128,128,1,4,0) silu_fwd(*,3200,*,0)
        linear(*,128,*,*,-,-,*,384,25,128,128,1,1,0) linear(*,128,*,*,-,-,*,384,25,128,128,1,1,0)
        linear(*,128,*,*,-,-,*,384,25,128,128,1,1,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear(*,128,*,*,-,-,*,128,25,128,128,1,1,0) silu_fwd(*,3200,*,0)
        linear(*,128,*,*,-,-,*,384,25,128,128,1,1,0) linear(*,128,*,*,-,-,*,384,25,128,128,1,1,0)
        linear(*,128,*,*,-,-,*,384,25,128,128,1,1,0)
        painn_interaction_fwd_mma_dyn(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear(*,128,*,-,-,-,*,256,75,128,128,1,0,0) linear(*,128,*,-,-,-,*,256,75,128,128,1,0,0)
        painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0) linear(*,256,*,*,-,-,*,128,25,128,128,1,1,0)
        linear(*,256,*,-,*,-,*,128,25,128,128,1,4,0) silu_fwd(*,3200,*,0)
        linear(*,128,*,*,-,-,*,384,25,128,128,1,1,0) linear(*,128,*,*,-,-,*,384,25,128,128,1,1,0)
        linear(*,128,*,*,-,-,*,384,25,128,128,1,1,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,-,-,0)
        segment_reduce_fwd(*,*,5,128,0,*,0) painn_mix_post_bwd_dyn(*,-,*,*,*,25,128,*,*,-,0)
        linear(*,384,*,-,-,-,*,128,25,128,128,0,0,0) linear(*,384,*,-,*,-,*,128,25,128,128,0,4,0)
        linear(*,384,*,-,*,-,*,128,25,128,128,0,4,0) silu_bwd(*,*,3200,*,0)
        linear(*,128,*,-,-,-,*,256,25,128,128,0,0,0) linear(*,128,*,-,-,-,*,256,25,128,128,0,0,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0) linear(*,256,*,-,-,-,*,128,75,128,128,0,0,0)
        linear(*,256,*,-,*,-,*,128,75,128,128,0,4,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,*,*,*,0,0)
        linear(*,384,*,-,-,-,*,128,25,128,128,0,0,0) linear(*,384,*,-,*,-,*,128,25,128,128,0,4,0)
        linear(*,384,*,-,*,-,*,128,25,128,128,0,4,0) silu_bwd(*,*,3200,*,0)
        linear(*,128,*,-,*,-,*,128,25,128,128,0,4,0) painn_mix_post_bwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear(*,384,*,-,-,-,*,128,25,128,128,0,0,0) linear(*,384,*,-,*,-,*,128,25,128,128,0,4,0)
        linear(*,384,*,-,*,-,*,128,25,128,128,0,4,0) silu_bwd(*,*,3200,*,0)
        linear(*,128,*,-,-,-,*,256,25,128,128,0,0,0) linear(*,128,*,-,-,-,*,256,25,128,128,0,0,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0) linear(*,256,*,-,*,-,*,128,75,128,128,0,4,0)
        linear(*,256,*,-,*,-,*,128,75,128,128,0,4,0)
        painn_interaction_bwd_mol(*,*,-,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,-,*,*,*,0,0)
        linear(*,384,*,-,-,-,*,128,25,128,128,0,0,0) linear(*,384,*,-,*,-,*,128,25,128,128,0,4,0)
        linear(*,384,*,-,*,-,*,128,25,128,128,0,4,0) silu_bwd(*,*,3200,*,0)
        linear(*,128,*,-,*,-,*,128,25,128,128,0,4,0) linear_wgrad_dyn(*,12,25,128,128,384,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,25,128,128,128,256,256,*,0,-,0)
        linear_wgrad_dyn(*,4,75,128,128,256,128,128,*,0,-,0)
        linear_wgrad_dyn(*,2,25,128,128,128,128,128,*,0,-,0) embedding_bwd_dyn(*,2,*,100,25,128,*,*,0,-,0)""",
    'silu launches': """
        painn_edge_geom_dyn(*,*,*,182,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,25,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,25,128,-,0) silu_fwd(*,3200,*,0)
        linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mma_dyn(*,-,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) silu_fwd(*,3200,*,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,128,*,25,128,-,0)
        silu_fwd(*,3200,*,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mma_dyn(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) silu_fwd(*,3200,*,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,-,-,0) segment_reduce_fwd(*,*,5,128,0,*,0)
        chain_prepare(*,22,128,0,0) painn_mix_post_bwd_dyn(*,-,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,384,*,25,128,-,0) silu_bwd(*,*,3200,*,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,256,*,75,128,-,0)
        painn_interaction_bwd_mol(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) silu_bwd(*,*,3200,*,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_mix_post_bwd_dyn(*,*,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,384,*,25,128,-,0)
        silu_bwd(*,*,3200,*,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,25,128,*,*,-,0) linear_chain_dyn(*,256,*,75,128,-,0)
        painn_interaction_bwd_mol(*,*,-,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,-,*,*,*,0,0)
        linear_chain_dyn(*,384,*,25,128,-,0) silu_bwd(*,*,3200,*,0) linear_chain_dyn(*,128,*,25,128,-,0)
        linear_wgrad_dyn(*,12,25,128,128,384,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,25,128,128,128,256,256,*,0,-,0)
        linear_wgrad_dyn(*,4,75,128,128,256,128,128,*,0,-,0)
        linear_wgrad_dyn(*,2,25,128,128,128,128,128,*,0,-,0) embedding_bwd_dyn(*,2,*,100,25,128,*,*,0,-,0)""",
    'inference': """
        painn_edge_geom_dyn(*,*,*,182,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,25,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mma_dyn(*,-,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,*,-,0)
        linear_chain_dyn(*,128,*,25,128,-,0)
        painn_interaction_fwd_mma_dyn(*,*,*,*,*,*,*,*,*,*,*,*,*,5,12,25,128,20,*,*,-,0)
        linear_chain_dyn(*,128,*,75,128,-,0) painn_mix_pre_fwd_dyn(*,*,25,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,25,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,25,128,*,-,-,0)
        segment_reduce_fwd(*,*,5,128,0,*,0)""",
    'no edges': """
        painn_edge_geom_dyn(*,0,0,0,5.0,*,*,20,*,*,*,-,0) embedding_fwd_dyn(*,2,*,100,3,128,*,*,-,0)
        chain_prepare(*,22,128,1,0) linear_chain_dyn(*,128,*,3,128,-,0)
        painn_interaction_fwd_mol(*,*,*,0,*,*,*,*,*,*,*,*,3,1,3,128,20,*,*,0)
        linear_chain_dyn(*,128,*,9,128,-,0) painn_mix_pre_fwd_dyn(*,*,3,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,3,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,3,128,*,*,-,0)
        linear_chain_dyn(*,128,*,3,128,-,0)
        painn_interaction_fwd_mol(*,*,*,0,*,*,*,*,*,*,*,*,3,1,3,128,20,*,*,0)
        linear_chain_dyn(*,128,*,9,128,-,0) painn_mix_pre_fwd_dyn(*,*,3,128,1e-08,*,*,-,0)
        linear_chain_dyn(*,256,*,3,128,-,0) painn_mix_post_fwd_dyn(*,*,*,*,*,3,128,*,-,-,0)
        segment_reduce_fwd(*,*,3,128,0,*,0) chain_prepare(*,22,128,0,0)
        painn_mix_post_bwd_dyn(*,-,*,*,*,3,128,*,*,-,0) linear_chain_dyn(*,384,*,3,128,-,0)
        painn_mix_pre_bwd_dyn(*,*,*,*,3,128,*,*,-,0) linear_chain_dyn(*,256,*,9,128,-,0)
        painn_interaction_bwd_mol(*,*,*,*,0,*,*,*,*,*,*,*,*,3,1,3,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,3,128,-,0) painn_mix_post_bwd_dyn(*,*,*,*,*,3,128,*,*,-,0)
        linear_chain_dyn(*,384,*,3,128,-,0) painn_mix_pre_bwd_dyn(*,*,*,*,3,128,*,*,-,0)
        linear_chain_dyn(*,256,*,9,128,-,0)
        painn_interaction_bwd_mol(*,*,*,*,0,*,*,*,*,*,*,*,*,3,1,3,128,20,*,*,*,*,*,0,0)
        linear_chain_dyn(*,384,*,3,128,-,0) linear_wgrad_dyn(*,12,3,128,128,384,128,128,*,0,-,0)
        linear_wgrad_dyn(*,4,3,128,128,128,256,256,*,0,-,0) linear_wgrad_dyn(*,4,9,128,128,256,128,128,*,0,-,0)
        linear_wgrad_dyn(*,2,3,128,128,128,128,128,*,0,-,0) embedding_bwd_dyn(*,2,*,100,3,128,*,*,0,-,0)""",
}
