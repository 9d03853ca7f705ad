"""GPU parity tests added in round 2: the RCCL transport with a single rank, full-size / degenerate PaiNN batches,
the ShiftedSoftplus threshold points on the HIP path, a three-step training trajectory against the reference, the
reference-shaped loader surface on the device, the autograd contract of the custom nodes, deferred index checks."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import assert_close, load_golden, max_abs_rel, rel_err
from helpers import (cfg_of, grad_summary, ncsn_oracle_params, product_ncsn, product_schnet, schnet_oracle_params, t,
                     unique_named_grads)
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_OUT, TOL_GRAD = 1e-5, 1e-4
FULL = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=5.0, node_class=9,
            readout="mean")
PAINN = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")
NOISE_KEYS = ("pos_noise", "noise_level_1", "dist_noise_1", "noise_level_2", "dist_noise_2")


# ------------------------------------------------------------------------------------------------ RCCL, one rank
_RCCL_WORKER = r"""
import os, sys
sys.path.insert(0, {repo!r})
sys.path.insert(0, os.path.join({repo!r}, "tests")); sys.path.insert(0, os.path.join({repo!r}, "tests", "golden"))
import faulthandler
faulthandler.dump_traceback_later(150, exit=True)
import torch, torch.distributed as dist
from geossl_amd import pretrain_GeoSSL as pg
from geossl_amd.parallel import init_distributed, local_device
from geossl_amd.synthetic import draw_noise, make_batch
from helpers import product_ncsn, product_schnet, t
rank, local_rank, world = init_distributed()          # GEOSSL_DIST_BACKEND=nccl, WORLD_SIZE=1: a 1-rank RCCL group
assert dist.is_initialized() and dist.get_backend() == "nccl" and world == 1
dev = torch.device("cuda", local_device(local_rank))
torch.cuda.set_device(dev)
cfg = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=5.0, node_class=9,
           readout="mean")
tr = pg.DDMTrainer(product_schnet(cfg, dev), product_ncsn(128, 50, 2, dev), product_ncsn(128, 50, 2, dev, scale=0.9),
                   lr=5e-4, use_graph=True)
assert tr.reduce.active
losses = []
for step in range(4):
    b = make_batch(64, seed=step, mode="A")
    noise = {{k: t(v, dev) for k, v in draw_noise(b, seed=100 + step).items()}}
    losses.append(float(tr.step(pg.Batch.from_numpy(b, dev), noise, structure_key=("A", 64, 18))))
assert tr.use_graph, "capture fell back to eager"
torch.cuda.synchronize()
torch.save(dict(losses=losses, params=tr.flat.flat.cpu()), os.path.join({out!r}, "rccl.pt"))
dist.barrier()
dist.destroy_process_group()
"""


def test_single_rank_rccl_all_reduce_with_graph_capture(tmp_path):
    """The production transport on a 1-GPU box: a 1-rank `nccl` (= RCCL) process group, DDMTrainer(use_graph=True).
    dist.all_reduce on RCCL, its watchdog thread and the HIP-graph capture of forward + backward meet here; a 1-rank
    sum is the identity, so parameters after four steps must be bit-identical to a run without any group."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import draw_noise, make_batch
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "rccl_worker.py"
    script.write_text(_RCCL_WORKER.format(repo=repo, out=str(tmp_path)))
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0",
               GEOSSL_DIST_BACKEND="nccl", HSA_ENABLE_IPC_MODE_LEGACY="0")
    log = tmp_path / "rccl.log"
    with open(log, "w") as f:
        p = subprocess.Popen([sys.executable, str(script)], env=env, stdout=f, stderr=subprocess.STDOUT)
        try:
            code = p.wait(timeout=240)
        except subprocess.TimeoutExpired:
            p.kill()
            p.wait()
            code = None
    assert code == 0, open(log).read()[-3000:]
    got = torch.load(tmp_path / "rccl.pt", weights_only=False)
    tr = pg.DDMTrainer(product_schnet(FULL, DEV), product_ncsn(128, 50, 2, DEV),
                       product_ncsn(128, 50, 2, DEV, scale=0.9), lr=5e-4, use_graph=True)
    assert not tr.reduce.active
    losses = []
    for step in range(4):
        b = make_batch(64, seed=step, mode="A")
        noise = {k: t(v, DEV) for k, v in draw_noise(b, seed=100 + step).items()}
        losses.append(float(tr.step(pg.Batch.from_numpy(b, DEV), noise, structure_key=("A", 64, 18))))
    assert losses == got["losses"]
    assert torch.equal(tr.flat.flat.cpu(), got["params"])


# ------------------------------------------------------------------------------------------------ S7 thresholds
def test_shifted_softplus_threshold_points_on_the_hip_path():
    """G2 (ShiftedSoftplus of the unmodified reference on a grid incl. +-20, +-25, 19.999, 20.001: softplus switches to
    the identity above its threshold 20) through the HIP ssp(): ops.linear with an identity weight and EPI_SSP, the
    stand-alone module, and its derivative."""
    from geossl_amd import _lib, ops
    from geossl_amd.Geom3D.models.schnet import ShiftedSoftplus
    g = load_golden("g1_g2_smearing_ssp")
    x, y = t(g["ssp_x"], DEV), g["ssp_y"]
    n = x.numel()
    rows = (n + 31) // 32
    X = torch.zeros(rows, 32, device=DEV)
    X.view(-1)[:n] = x
    got = ops.linear(X, torch.eye(32, device=DEV), flags=_lib.EPI_SSP).view(-1)[:n].cpu()
    # the identity product is exact (each output is one x times 1.0), so this is ssp() itself; 2e-7 absolute:
    # float32 resolution of the reference's own log1p(exp(x)) - log 2 near |y| ~ 1, 1e-6 relative for large |x|
    err = (got.double() - torch.from_numpy(y).double()).abs()
    assert float((err / (1.0 + torch.from_numpy(y).double().abs())).max()) < 2e-7, float(err.max())
    mod = ShiftedSoftplus()
    xs = x.clone().requires_grad_(True)
    ys = mod(xs)
    assert torch.equal(ys.detach().cpu(), got)
    ys.sum().backward()
    assert max_abs_rel(xs.grad.cpu(), torch.sigmoid(torch.from_numpy(g["ssp_x"]).double())) < 2e-7


# ------------------------------------------------------------------------------------------------ D4 trajectory
@pytest.mark.parametrize("tag", ["reduced", "full"])
@pytest.mark.parametrize("mode", ["stock_adam", "trainer"])
def test_three_step_training_trajectory_vs_reference(tag, mode):
    """Fixture G12: three steps of the training-loop body (pretrain_GeoSSL.py:258-260) of the unmodified reference with
    stock torch.optim.Adam over the three parameter groups (:333-343).  `stock_adam`: the same loop on the product
    modules (do_DDM + torch.optim.Adam: gradients travel through autograd, no flat buffer).  `trainer`: DDMTrainer
    (flat buffer, direct accumulation, fused Adam).  Losses per step and parameters after step 3 at 1e-5."""
    from geossl_amd import pretrain_GeoSSL as pg
    g = load_golden("g12_ddm_trajectory_" + tag)
    cfg = cfg_of(g)
    F = cfg["hidden_channels"]
    model = product_schnet(cfg, DEV)
    n1, n2 = product_ncsn(F, 50, 2, DEV), product_ncsn(F, 50, 2, DEV, scale=0.9)
    batch = pg.Batch(t(g["x"], DEV), t(g["positions"], DEV), t(g["batch"], DEV), t(g["super_edge_index"], DEV))
    if mode == "stock_adam":
        opt = torch.optim.Adam([{"params": model.parameters(), "lr": 5e-4}, {"params": n1.parameters(), "lr": 5e-4},
                                {"params": n2.parameters(), "lr": 5e-4}], lr=5e-4, weight_decay=0)
    else:
        tr = pg.DDMTrainer(model, n1, n2, lr=5e-4)
    for step in range(3):
        noise = {k: t(g["%s/%d" % (k, step)], DEV) for k in NOISE_KEYS}
        if mode == "stock_adam":
            loss, _ = pg.do_DDM(pg.Args("schnet"), batch, model, None, 0.0, 0.3, NCSN_models=(n1, n2), noise=noise)
            opt.zero_grad()
            loss.backward()
            opt.step()
        else:
            loss = tr.step(batch, noise)
        assert rel_err(loss.detach().cpu(), g["loss/%d" % step]) < TOL_OUT, step
    mods = {"model": dict(model.named_parameters()), "ncsn1": dict(n1.named_parameters()),
            "ncsn2": dict(n2.named_parameters())}
    for k in g:
        if k.startswith("psum/") or k.startswith("param/"):
            _, m, name = k.split("/", 2)
            p = mods[m][name].detach().cpu()
            got = grad_summary(p) if k.startswith("psum/") else p
            assert rel_err(got, g[k]) < TOL_OUT, k


# ------------------------------------------------------------------------------------------------ autograd contract
def test_parameter_gradients_go_through_autograd_outside_the_trainer():
    """Outside DDMTrainer the custom nodes return parameter gradients like any autograd node, whatever state p.grad is
    in: torch.autograd.grad works, .grad is not touched by it, tensor hooks fire, backward() accumulates."""
    from geossl_amd import pretrain_GeoSSL as pg
    g = load_golden("g6_ddm_reduced")
    cfg = cfg_of(g)
    model = product_schnet(cfg, DEV)
    n1, n2 = product_ncsn(32, 50, 2, DEV), product_ncsn(32, 50, 2, DEV, scale=0.9)
    batch = pg.Batch(t(g["x"], DEV), t(g["positions"], DEV), t(g["batch"], DEV), t(g["super_edge_index"], DEV))
    noise = {k: t(g[k], DEV) for k in NOISE_KEYS}
    params = [p for m in (model, n1, n2) for p in m.parameters() if p.requires_grad]
    for p in params:  # dense grads already present: the case the old inference-by-state got wrong
        p.grad = torch.full_like(p, 7.0)
    fired = []
    model.lin2.weight.register_hook(lambda gr: fired.append(gr.clone()))
    loss, _ = pg.do_DDM(pg.Args("schnet"), batch, model, None, 0.0, 0.3, NCSN_models=(n1, n2), noise=noise)
    grads = torch.autograd.grad(loss, params, retain_graph=True)
    assert all(gr is not None for gr in grads) and len(fired) == 1
    assert all(bool((p.grad == 7.0).all()) for p in params)  # autograd.grad leaves .grad alone
    loss.backward()
    for p, gr in zip(params, grads):
        assert torch.equal(p.grad, gr + 7.0)  # accumulated by AccumulateGrad on top of what was there
    by_name = {id(p): gr for p, gr in zip(params, grads)}
    for k in g:
        if k.startswith("grad/model/"):
            assert rel_err(by_name[id(dict(model.named_parameters())[k[11:]])].cpu(), g[k]) < TOL_GRAD, k


def test_out_of_range_atom_type_is_reported():
    """The reference raises IndexError from Embedding for an atom type outside the table (e.g. node_class=9 fed raw
    atomic numbers).  The HIP path flags it on the device: check_status() reports it synchronously, and a later forward
    reports it without anyone asking."""
    from geossl_amd.synthetic import make_batch
    model = product_schnet(FULL, DEV)
    b = make_batch(4, seed=3)
    x = t(b["x"], DEV)
    x[5, 0] = 17
    with torch.no_grad():
        model(x[:, 0], t(b["positions"], DEV), t(b["batch"], DEV))
    with pytest.raises(IndexError):
        model.check_status()
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        for _ in range(3):  # the deferred copy has landed by now: the next forward raises on entry
            model(x[:, 0], t(b["positions"], DEV), t(b["batch"], DEV))


# ------------------------------------------------------------------------------------------------ loader surface
def test_reference_loader_surface_feeds_the_ddm_step():
    """pretrain_GeoSSL.py:289-301 as written: AtomTupleExtractor transform per molecule, DataLoaderAtomTuple,
    batch.to(device), do_DDM.  Same loss as the step on the pre-collated batch."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import AtomTupleExtractor, Data, DataLoaderAtomTuple
    g = load_golden("g6_ddm_reduced")
    sizes = np.bincount(g["batch"]).tolist()
    ext = AtomTupleExtractor(ratio=1, option="combination")
    off, dataset = 0, []
    for n in sizes:
        dataset.append(ext(Data(x=torch.from_numpy(g["x"][off:off + n]), positions=torch.from_numpy(g["positions"][off:off + n]))))
        off += n
    loader = DataLoaderAtomTuple(dataset, batch_size=len(sizes), shuffle=False)
    (batch,) = list(loader)
    batch = batch.to(DEV)
    assert batch.batch.is_cuda and torch.equal(batch.super_edge_index.cpu(), t(g["super_edge_index"]))
    # .to() leaves the collation's host sizes on the tensors; the index structures are built from them (no device
    # read-back) by the first step that needs them - a step that replays a capacity-bucket graph never does
    assert batch.batch._geossl_sizes[0] == sizes and getattr(batch.batch, "_geossl_two_view", None) is None
    cfg = cfg_of(g)
    model = product_schnet(cfg, DEV)
    n1, n2 = product_ncsn(32, 50, 2, DEV), product_ncsn(32, 50, 2, DEV, scale=0.9)
    noise = {k: t(g[k], DEV) for k in NOISE_KEYS}
    loss, _ = pg.do_DDM(pg.Args("schnet"), batch, model, None, 0.0, 0.3, NCSN_models=(n1, n2), noise=noise)
    assert rel_err(loss.detach().cpu(), g["loss"]) < TOL_OUT
    lay2 = batch.batch._geossl_two_view[1]
    assert lay2._sizes_host == sizes + sizes                          # built from the host sizes


@pytest.mark.parametrize("option", ["combination", "permutation"])
def test_atom_tuple_extractor_ratio_on_batch_vector(option):
    """ratio < 1 on the collated path: the same np.random.choice calls in molecule order as the per-molecule
    transform of the reference (fixture G11, seed 123)."""
    from geossl_amd.Geom3D.dataloaders import AtomTupleExtractor
    g = load_golden("g11_loader")
    bvec = t(g["batch/%s_0.5" % option], DEV)
    np.random.seed(123)
    sei = AtomTupleExtractor(ratio=0.5, option=option)(bvec)
    assert sei.is_cuda and torch.equal(sei.cpu(), t(g["sei/%s_0.5" % option]))
    full = AtomTupleExtractor(ratio=1, option=option)(bvec)
    assert torch.equal(full.cpu(), t(g["sei/%s_1" % option]))


# ------------------------------------------------------------------------------------------------ PaiNN (config 5)
def _painn(cfg=PAINN):
    from filler import fill_module_
    from geossl_amd.Geom3D.models import PaiNN
    return fill_module_(PaiNN(**cfg)).to(DEV)


def _painn_oracle_params(cfg=PAINN):
    from test_oracle_golden import painn_params
    return painn_params(cfg)


def _painn_batch(b, radius=5.0):
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    bt = pg.Batch.from_numpy(b, DEV)
    bt.x[:, 0].clamp_(max=8)
    bt.radius_edge_index = ops.radius_graph(bt.positions, radius, bt.batch)  # datasets_3D_Radius.py:120 on the device
    return bt


@pytest.mark.parametrize("molset", ["A", "B"])
def test_painn_full_size_determinism_and_oracle_slice(molset):
    """Config 5 at the bench size: a 1024-molecule PaiNN + DDM step (hydrogens included) twice - bit-identical loss
    and gradients - and its first 64 molecules against oracle.nets.do_ddm_painn on the same noise."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.parallel import shard_batch_numpy
    from geossl_amd.synthetic import draw_noise, make_batch
    from oracle import graph, nets
    b = make_batch(1024, seed=77, mode=molset)
    nz = draw_noise(b, seed=78)
    runs = []
    for _ in range(2):
        model = _painn()
        n1, n2 = product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9)
        bt = _painn_batch(b)
        noise = {k: t(v, DEV) for k, v in nz.items()}
        loss, _ = pg.do_DDM(pg.Args("painn"), bt, model, None, 0.0, 0.3, NCSN_models=(n1, n2), noise=noise)
        loss.backward()
        gr = torch.cat([p.grad.reshape(-1) for m in (model, n1, n2) for p in m.parameters() if p.grad is not None])
        runs.append((float(loss), gr.cpu()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert np.isfinite(runs[0][0]) and bool(torch.isfinite(runs[0][1]).all())
    # 64-molecule slice against the oracle.  The DDM LOSS is compared on the slice; GRADIENTS are compared through the
    # backbone alone (PaiNN is smooth: silu).  Gradients through the NCSN heads are pinned on the small golden batches
    # (G7): with ~2 million relu units in a 64-molecule slice some pre-activation always lies within fp32 rounding of
    # zero (oracle.nets.ncsn_relu_margin is 1e-8 .. 1e-7 for every noise seed tried), relu' of such a unit is
    # undetermined in fp32, and one flipped unit moves the gradient of its two atoms by a finite amount (seen: 5e-3 of
    # |d loss / d q| on 1152 atoms) - a property of the reference's network, not of either implementation.
    small = shard_batch_numpy(b, 0, 16)
    n_at, S = small["positions"].shape[0], small["super_edge_index"].shape[1]
    nzs = dict(pos_noise=nz["pos_noise"][:n_at], noise_level_1=nz["noise_level_1"][:64], dist_noise_1=nz["dist_noise_1"][:S],
               noise_level_2=nz["noise_level_2"][:64], dist_noise_2=nz["dist_noise_2"][:S])
    model = _painn()
    n1, n2 = product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9)
    bt = _painn_batch(small)
    loss, _ = pg.do_DDM(pg.Args("painn"), bt, model, None, 0.0, 0.3, NCSN_models=(n1, n2),
                        noise={k: t(v, DEV) for k, v in nzs.items()})
    rei = graph.collate_np([(small["x"][small["batch"] == m], small["positions"][small["batch"] == m])
                            for m in range(64)], radius=5.0)["radius_edge_index"]
    assert np.array_equal(rei, bt.radius_edge_index.cpu().numpy())
    P, P1, P2 = _painn_oracle_params(), ncsn_oracle_params(128, 50), ncsn_oracle_params(128, 50, 0.9)
    xs = t(small["x"]).clone()
    with torch.no_grad():
        ref = nets.do_ddm_painn(P, P1, P2, xs, t(small["positions"]), t(small["batch"]), t(rei),
                                t(small["super_edge_index"]), t(nzs["pos_noise"]), t(nzs["noise_level_1"]),
                                t(nzs["dist_noise_1"]), t(nzs["noise_level_2"]), t(nzs["dist_noise_2"]), 128, 3, 5.0, 2, "add")
    assert rel_err(loss.detach().cpu(), ref) < TOL_OUT
    pos2 = t(small["positions"]) + t(nzs["pos_noise"])  # the perturbed view: some precomputed edges beyond the cutoff
    model.zero_grad()
    out, q = model(bt.x, pos2.to(DEV), bt.radius_edge_index, bt.batch, return_latent=True)
    ((out ** 2).sum() + 0.5 * (q ** 2).sum()).backward()
    o_ref, q_ref = nets.painn_forward(P, xs, pos2, t(rei), t(small["batch"]), 128, 3, 5.0, "add", return_latent=True)
    ((o_ref ** 2).sum() + 0.5 * (q_ref ** 2).sum()).backward()
    assert_close(q.detach().cpu(), q_ref.detach(), TOL_OUT, "q")
    named = unique_named_grads(model)
    for k, v in P.items():
        if v.grad is not None:
            assert rel_err(named[k].cpu(), v.grad) < TOL_GRAD, k


def test_painn_degenerate_batch_vs_oracle():
    """Ragged / degenerate molecules through PaiNN: a 1-atom molecule (no edges at all), a 2-atom molecule farther apart
    than the cutoff (E = 0 for the molecule, isolated atoms), an atom with no in-edges inside a larger molecule, next
    to ordinary ones - forward and parameter gradients against oracle.nets.painn_forward."""
    from oracle import graph, nets
    rng = np.random.default_rng(12)
    from geossl_amd.synthetic import make_batch
    b = make_batch(0, seed=13, sizes=[1, 2, 9, 18, 1, 5])
    pos = b["positions"].copy()
    off = np.concatenate([[0], np.cumsum(b["sizes"])])
    pos[off[1] + 1] = pos[off[1]] + np.array([9.0, 0.0, 0.0], np.float32)      # 2-atom molecule beyond the cutoff
    pos[off[2] + 8] = pos[off[2]] + np.array([0.0, 30.0, 0.0], np.float32)     # atom 8 of the 9-atom molecule: isolated
    x = b["x"].copy()
    x[:, 0] = rng.integers(0, 9, size=len(x))
    x[off[3]:off[3] + 3, 0] = 0                                                # hydrogens (padding row)
    mols = [(x[off[m]:off[m + 1]], pos[off[m]:off[m + 1]]) for m in range(len(b["sizes"]))]
    c = graph.collate_np(mols, radius=5.0)
    e = c["radius_edge_index"]
    deg = np.bincount(e[0], minlength=len(x))
    assert deg[0] == 0 and deg[off[1]] == 0 and deg[off[2] + 8] == 0 and deg[off[4]] == 0
    model = _painn()
    out, q = model(t(c["x"], DEV), t(c["positions"], DEV), t(e, DEV), t(c["batch"], DEV), return_latent=True)
    loss = (out ** 2).sum() + 0.5 * (q ** 2).sum()
    loss.backward()
    P = _painn_oracle_params()
    o_ref, q_ref = nets.painn_forward(P, t(c["x"]), t(c["positions"]), t(e), t(c["batch"]), 128, 3, 5.0, "add",
                                      return_latent=True)
    ((o_ref ** 2).sum() + 0.5 * (q_ref ** 2).sum()).backward()
    assert_close(out.detach().cpu(), o_ref.detach(), TOL_OUT, "out")
    assert_close(q.detach().cpu(), q_ref.detach(), TOL_OUT, "q")
    named = unique_named_grads(model)
    for k, v in P.items():
        if v.grad is not None:
            assert rel_err(named[k].cpu(), v.grad) < TOL_GRAD, k
    # a batch with no edges at all (every molecule a single atom): the embedding passes through the mixing blocks
    ones = graph.collate_np([(x[i:i + 1], pos[i:i + 1]) for i in range(4)], radius=5.0)
    assert ones["radius_edge_index"].shape == (2, 0)
    out1 = model(t(ones["x"], DEV), t(ones["positions"], DEV), t(ones["radius_edge_index"], DEV), t(ones["batch"], DEV))
    ref1 = nets.painn_forward(P, t(ones["x"]), t(ones["positions"]), t(ones["radius_edge_index"]), t(ones["batch"]),
                              128, 3, 5.0, "add")
    assert_close(out1.detach().cpu(), ref1.detach(), TOL_OUT, "out (E = 0)")


def test_painn_trainer_graph_replay_follows_the_edge_list():
    """A captured graph binds radius_edge_index (and its incidence lists); batches with the same molecule sizes but
    different geometry have different edge lists.  DDMTrainer(use_graph=True) must give the eager losses on every batch,
    not replay batch 0's edges: per-structure graphs (graph_mode="structure") re-capture when the edge list is another
    tensor - bit for bit the eager step; the default mode serves all of them from ONE capacity-bucket graph whose edge
    structures are rewritten per step (round 5) - the eager step within fp32 summation order (partial sums are cut at the
    capacity's block boundaries)."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import draw_noise, make_batch
    batches = [make_batch(32, seed=200 + i, mode="A") for i in range(3)]
    bts = [_painn_batch(b) for b in batches]
    assert len({int(bt.radius_edge_index.size(1)) for bt in bts}) > 1 or not torch.equal(bts[0].radius_edge_index,
                                                                                          bts[1].radius_edge_index)
    losses = {}
    for mode in ("eager", "structure", "auto"):
        tr = pg.DDMTrainer(_painn(), product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9), lr=5e-4,
                           model_3d="painn", use_graph=mode != "eager", graph_mode="auto" if mode == "eager" else mode)
        out = []
        for step in range(6):
            b, bt = batches[step % 3], bts[step % 3]
            noise = {k: t(v, DEV) for k, v in draw_noise(b, seed=300 + step).items()}
            out.append(float(tr.step(bt, noise, structure_key=("A", 32, 18))))
        losses[mode] = out
        if mode == "structure":
            assert tr.step_graphs.captures == 3
        if mode == "auto":
            assert tr.step_graphs.captures == 1 and next(iter(tr._graphs))[0] == "bucket"
    assert losses["structure"] == losses["eager"], losses
    # (the trajectory of this random-weight model amplifies a rounding-level difference about tenfold per Adam step from
    # the fourth step on - measured round 6: 1e-7, 1e-7, 1e-7, 1e-6, 1e-5, 1e-4 between ANY two of the paths that are not
    # bit-identical, e.g. the eager step with and without the mu-zero shortcut - so the bound follows it)
    for step, (a, c) in enumerate(zip(losses["auto"], losses["eager"])):
        assert abs(a - c) <= 2e-6 * 10.0 ** max(0, step - 2) * abs(c), (step, losses)


# ------------------------------------------------------------------------------------------------ chained row GEMMs
@pytest.mark.parametrize("F,R", [(128, 36864), (128, 77), (64, 1000), (32, 33), (128, 32 * 1100 + 5)])
@pytest.mark.parametrize("transB", [True, False])
def test_linear_chain_vs_fp64(F, R, transB):
    """geossl_linear_chain (up to three F -> F layers in one launch, results passed on in registers) against an fp64
    evaluation of the same chain, every epilogue form, stored and unstored stages, ragged row counts, a grid that gives
    some blocks a second row group (R > 256 blocks x 128 rows)."""
    from geossl_amd import _lib, ops
    torch.manual_seed(F + R)
    X = torch.randn(R, F, device=DEV)
    Ws = [torch.randn(F, F, device=DEV) / F ** 0.5 for _ in range(4)]
    bs = [torch.randn(F, device=DEV) * 0.1 for _ in range(4)]
    res = torch.randn(R, F, device=DEV)
    tprev = torch.randn(R, F, device=DEV)
    imgs = ops.prepare_chain(Ws, transB=transB)
    mm = (lambda a, w: a @ w.double().T) if transB else (lambda a, w: a @ w.double())
    ssp64 = lambda v: torch.nn.functional.softplus(v) - float(np.log(2.0))

    def ref_chain(n):
        y, outs = X.double(), []
        for s in range(n):
            y = mm(y, Ws[s])
            if s != 2:
                y = y + bs[s].double()
            if s == 0:
                y = ssp64(y)
            if s == 1:
                y = y + res.double()
            if s == 2:
                y = y * (1.0 - 0.5 * torch.exp(-tprev.double()))
            outs.append(y)
        return outs

    for n in (1, 2, 3):
        stages = [dict(image=imgs[0], bias=bs[0], flags=_lib.EPI_SSP), dict(image=imgs[1], bias=bs[1], res=res, store=(n != 3)),
                  dict(image=imgs[2], tprev=tprev)][:n]
        got = ops.linear_chain(X, stages)
        want = ref_chain(n)
        for s in range(n):
            if got[s] is None:
                assert s == 1 and n == 3
                continue
            scale = float(want[s].abs().max())
            assert float((got[s].double() - want[s]).abs().max()) < 3e-6 * scale * (s + 1), (n, s)
    # a chain is deterministic, and a one-stage chain agrees with geossl_linear to rounding
    a = ops.linear_chain(X, [dict(image=imgs[0], bias=bs[0], flags=_lib.EPI_SSP)])[0]
    b = ops.linear_chain(X, [dict(image=imgs[0], bias=bs[0], flags=_lib.EPI_SSP)])[0]
    assert torch.equal(a, b)
    c = ops.linear(X, Ws[0], bias=bs[0], flags=_lib.EPI_SSP, transB=transB)
    assert max_abs_rel(a, c) < 2e-6


def test_schnet_chain_path_matches_per_layer_launches():
    """The chained atom-row path (default) against the one-launch-per-Linear path (GEOSSL_NO_CHAIN=1) on the full
    configuration: same loss and gradients to rounding (both pinned to the reference by the golden tests)."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import draw_noise, make_batch
    b = make_batch(64, seed=5, mode="B")
    nz = draw_noise(b, seed=6)
    res = {}
    for tag, env in (("chain", None), ("per_layer", "1")):
        if env is None:
            os.environ.pop("GEOSSL_NO_CHAIN", None)
        else:
            os.environ["GEOSSL_NO_CHAIN"] = env
        try:
            model = product_schnet(FULL, DEV)
            n1, n2 = product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9)
            loss, _ = pg.do_DDM(pg.Args("schnet"), pg.Batch.from_numpy(b, DEV), model, None, 0.0, 0.3,
                                NCSN_models=(n1, n2), noise={k: t(v, DEV) for k, v in nz.items()})
            loss.backward()
            res[tag] = (float(loss), {k: v.clone() for k, v in unique_named_grads(model).items()})
        finally:
            os.environ.pop("GEOSSL_NO_CHAIN", None)
    assert abs(res["chain"][0] - res["per_layer"][0]) < 1e-6 * abs(res["per_layer"][0])
    for k, v in res["per_layer"][1].items():
        assert rel_err(res["chain"][1][k], v) < 2e-5, k


# ------------------------------------------------------------------------------------------------ N3, second order
@pytest.mark.parametrize("tag", ["reduced", "full_r5"])
def test_training_on_forces_vs_reference(tag):
    """finetune_md17.py:46-54 as written: pred_force = -grad(E, pos, create_graph=True), loss = c_E * MSE(E) +
    c_F * MSE(force), loss.backward() into the parameters - the second differentiation of the path.  Fixture G10 is
    the unmodified reference on the same molecules (ragged, incl. 1- and 2-atom ones)."""
    g = load_golden("g10_schnet_force_training_" + tag)
    cfg = cfg_of(g)
    model = product_schnet(cfg, DEV)
    pos = t(g["positions"], DEV).clone().requires_grad_(True)
    out = model(t(g["x"], DEV)[:, 0], pos, t(g["batch"], DEV))
    from filler import fill_module_
    graph_pred_linear = fill_module_(torch.nn.Linear(out.size(1), 1)).to(DEV)   # finetune_md17.py:33
    pred_energy = graph_pred_linear(out).squeeze(1)
    pred_force = -torch.autograd.grad(outputs=pred_energy, inputs=pos, grad_outputs=torch.ones_like(pred_energy),
                                      create_graph=True, retain_graph=True)[0]
    assert_close(pred_energy.detach().cpu(), g["energy"], TOL_OUT, "energy")
    assert rel_err(pred_force.detach().cpu(), g["force"]) < TOL_GRAD
    crit = torch.nn.MSELoss()
    loss = 1.0 * crit(pred_energy, t(g["actual_energy"], DEV)) + 10.0 * crit(pred_force, t(g["actual_force"], DEV))
    assert rel_err(loss.detach().cpu(), g["loss"]) < 1e-4
    loss.backward()
    assert rel_err(pos.grad.cpu(), g["grad_pos"]) < TOL_GRAD
    grads = unique_named_grads(model)
    for k in g:
        if k.startswith("gsum/"):
            assert rel_err(grad_summary(grads[k[5:]].cpu()), g[k]) < TOL_GRAD, k
        if k.startswith("grad/"):
            assert rel_err(grads[k[5:]].cpu(), g[k]) < TOL_GRAD, k
    # the energy head's weights receive a gradient through the force as well (the readout's backward differentiated with
    # respect to its upstream gradient)
    assert rel_err(graph_pred_linear.weight.grad.cpu(), g["head_grad/weight"]) < TOL_GRAD
    assert rel_err(graph_pred_linear.bias.grad.cpu(), g["head_grad/bias"]) < TOL_GRAD


def test_painn_forces_and_training_on_forces_vs_reference():
    """finetune_md17.py:38-54 with the PaiNN backbone and the energy head of create_output_layers(): forces, then a loss
    on energy and force back-propagated into every parameter - fixture G13 (the unmodified reference; hydrogens, a
    2-atom and a 1-atom molecule)."""
    from filler import fill_module_
    g = load_golden("g13_painn_force_training")
    model = _painn(cfg_of(g))
    head = fill_module_(model.create_output_layers()).to(DEV)
    pos = t(g["positions"], DEV).clone().requires_grad_(True)
    rep = model(t(g["x"], DEV), pos, t(g["radius_edge_index"], DEV), t(g["batch"], DEV))
    assert_close(rep.detach().cpu(), g["rep"], TOL_OUT, "representation")
    pred_energy = head(rep).squeeze(1)
    pred_force = -torch.autograd.grad(outputs=pred_energy, inputs=pos, grad_outputs=torch.ones_like(pred_energy),
                                      create_graph=True, retain_graph=True)[0]
    assert rel_err(pred_energy.detach().cpu(), g["energy"]) < TOL_OUT
    assert rel_err(pred_force.detach().cpu(), g["force"]) < TOL_GRAD
    crit = torch.nn.MSELoss()
    loss = 1.0 * crit(pred_energy, t(g["actual_energy"], DEV)) + 10.0 * crit(pred_force, t(g["actual_force"], DEV))
    assert rel_err(loss.detach().cpu(), g["loss"]) < 1e-4
    loss.backward()
    assert rel_err(pos.grad.cpu(), g["grad_pos"]) < TOL_GRAD
    grads = unique_named_grads(model)
    assert float(grads["embedding.weight"][0].abs().max()) == 0.0
    for k in g:
        if k.startswith("gsum/"):
            assert rel_err(grad_summary(grads[k[5:]].cpu()), g[k]) < TOL_GRAD, k
    for name, p in head.named_parameters():
        assert rel_err(p.grad.cpu(), g["head_grad/" + name]) < TOL_GRAD, name


def test_force_evaluation_with_create_graph_uses_the_fused_kernels():
    """The reference's evaluation loop also asks for create_graph=True and then detaches (finetune_md17.py:99): the
    force must be the fused kernels' (bit-identical to create_graph=False), the second-order machinery untouched."""
    from geossl_amd.synthetic import make_batch
    b = make_batch(32, seed=4, mode="B")
    model = product_schnet(dict(FULL, readout="add"), DEV)
    x, bat = t(b["x"], DEV), t(b["batch"], DEV)
    forces = []
    for create_graph in (False, True):
        pos = t(b["positions"], DEV).clone().requires_grad_(True)
        energy = model(x[:, 0], pos, bat).sum(dim=1)
        f = torch.autograd.grad(energy, pos, torch.ones_like(energy), create_graph=create_graph, retain_graph=True)[0]
        assert f.requires_grad == create_graph
        forces.append(f.detach())
    assert torch.equal(forces[0], forces[1])


def test_standalone_mlp_module_matches_torch():
    """MultiLayerPerceptron.forward (NCSN.py:33-43) as a module of its own - the two MLP shapes of NCSN_version_03 -
    against torch.nn.functional on the same weights in fp64, values and gradients (weights, input)."""
    from geossl_amd.NCSN import MultiLayerPerceptron
    torch.manual_seed(3)
    for dims, batch_shape in (((1, [128, 1]), (300,)), ((129, [128, 64, 1]), (7, 33))):
        mlp = MultiLayerPerceptron(dims[0], dims[1], activation="relu").to(DEV)
        for layer in mlp.layers:
            torch.nn.init.normal_(layer.bias, std=0.1)
        x = torch.randn(*batch_shape, dims[0], device=DEV, requires_grad=True)
        y = mlp(x)
        assert y.shape == (*batch_shape, dims[1][-1])
        (y ** 2).sum().backward()
        xr = x.detach().double().requires_grad_(True)
        h = xr
        ws = [(l.weight.detach().double().requires_grad_(True), l.bias.detach().double().requires_grad_(True)) for l in mlp.layers]
        for i, (w, b_) in enumerate(ws):
            h = torch.nn.functional.linear(h, w, b_)
            if i < len(ws) - 1:
                h = torch.relu(h)
        (h ** 2).sum().backward()
        assert max_abs_rel(y.detach(), h.detach()) < 2e-6
        assert rel_err(x.grad, xr.grad) < 1e-5
        for l, (w, b_) in zip(mlp.layers, ws):
            assert rel_err(l.weight.grad, w.grad) < 1e-5 and rel_err(l.bias.grad, b_.grad) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("F,nmol", [(128, 40), (64, 23), (32, 9), (128, 700)])
def test_ncsn_one_pass_backward_matches_two_pass_and_fp64(F, nmol, monkeypatch):
    """ncsn_bwd.hip (row gradients + weight gradients of both dense layers in one pass) against the two-pass form
    (ncsn_rows.hip + the column GEMMs of wgrad.h) on the same inputs, and against an fp64 evaluation of the oracle.
    Ragged molecules, S not a multiple of the 32-row tile; 700 molecules give every block several tiles."""
    import types
    import ncsn_twin as tw
    from oracle import nets
    from geossl_amd.Geom3D.dataloaders.dataloaders_AtomTuple import BatchAtomTuple
    gen = torch.Generator().manual_seed(1234 + F + nmol)
    sizes = torch.randint(2, 27, (nmol,), generator=gen).tolist()
    N = sum(sizes)
    K, power = 30, 2.0
    x = torch.randint(0, 9, (N, 1), generator=gen)
    pos = torch.randn(N, 3, generator=gen)
    data = BatchAtomTuple.from_sizes(x.to(DEV), pos.to(DEV), sizes, option="combination")
    sei = data.super_edge_index.cpu()
    S = sei.size(1)
    assert S % 32 != 0
    h = torch.randn(N, F, generator=gen) * 0.5
    dist = (pos[sei[0]] - pos[sei[1]]).norm(dim=-1, keepdim=True)
    nl = torch.randint(0, K, (nmol,), generator=gen)
    dn = torch.randn(S, 1, generator=gen)
    P64 = {k: v.detach().double().requires_grad_(v.requires_grad) for k, v in ncsn_oracle_params(F, K).items()}
    batch = data.batch.cpu()
    # a relu unit within fp32 rounding of zero makes fp32 and fp64 evaluations differ by a finite amount in that row: the
    # inputs are conditioned (tests/ncsn_twin.py: fresh noise for such rows, at most 3 % of the rows removed)
    prob = dict(h=h, dist=dist, nl=nl, dn=dn, batch=batch, sei0=sei[0].contiguous(), sei1=sei[1].contiguous(), S=S,
                P={k: v.detach().float() for k, v in P64.items()})
    prob, _, removed = tw.condition(prob, generator=torch.Generator().manual_seed(F + nmol))
    assert removed <= tw.MAX_REMOVED * S
    sei, dist, nl, dn, S = torch.stack([prob["sei0"], prob["sei1"]]), prob["dist"], prob["nl"], prob["dn"], prob["S"]
    assert S % 32 != 0
    assert nets.ncsn_relu_margin(P64, batch, sei, h.double(), dist.double(), nl, dn.double()) >= tw.T_MARGIN
    data = types.SimpleNamespace(batch=data.batch, super_edge_index=sei.to(DEV), num_graphs=nmol)
    h64 = h.double().requires_grad_()
    nets.ncsn_v03_forward(P64, batch, sei, h64, dist.double(), nl, dn.double(), power).backward()

    def run(split):
        if split:
            monkeypatch.setenv("GEOSSL_NCSN_SPLIT_BWD", "1")
        else:
            monkeypatch.delenv("GEOSSL_NCSN_SPLIT_BWD", raising=False)
        head = product_ncsn(F, K, power, DEV)
        hh = h.to(DEV).clone().requires_grad_()
        loss = head(data, hh, dist.to(DEV), noise_level=nl.to(DEV), distance_noise=dn.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        out = {k: v.detach().cpu() for k, v in unique_named_grads(head).items()}
        out["h"] = hh.grad.cpu()
        return out

    one, two = run(False), run(True)
    truth = {k: P64[k].grad for k in one if k != "h"}
    truth["h"] = h64.grad
    for k in one:
        assert rel_err(one[k], two[k]) < 2e-6, (k, rel_err(one[k], two[k]))
        assert rel_err(one[k], truth[k]) < 1e-5, (k, rel_err(one[k], truth[k]))
    again = run(False)
    for k in one:
        assert torch.equal(one[k], again[k]), k  # fixed-order reductions: bit-reproducible


@pytest.mark.gpu
@pytest.mark.parametrize("F", [128, 64])
def test_aggregate_work_list_splits_large_molecules_bit_exact(F, monkeypatch):
    """Ragged batch with host sizes: the 21..33-atom molecules are shared by 2 or 4 waves (one group of target atoms
    each, geossl_cfconv_aggregate_work).  Every sum is still formed in the reference's order (sequential index_add per
    target in ascending source order, schnet.py:190,194-195): bit for bit equal to that evaluation and to the one-wave
    walk of geossl_cfconv_aggregate."""
    from geossl_amd import ops, _lib
    from geossl_amd.layout import MolLayout
    from geossl_amd.synthetic import make_batch
    monkeypatch.setenv("GEOSSL_AGG_TARGETS_MAX", "0")   # (the work list by molecule parts: what large launches take)
    sizes = list(make_batch(40, seed=11, mode="B")["sizes"]) + [1, 2, 33, 27, 26, 21, 22, 28, 30, 3, 24, 31, 20, 32]
    batch = torch.arange(len(sizes), device=DEV).repeat_interleave(torch.tensor(sizes, device=DEV))
    lay = MolLayout(batch, len(sizes), sizes=sizes)
    parts = [_lib.load().geossl_aggregate_parts(int(n)) for n in sizes]
    wk = lay.agg_work.cpu().numpy()
    wk = wk[wk != -1]                                   # (eight queues of equal length, padded with -1)
    assert lay.agg_work is not None and wk.size == sum(parts) and max(parts) == 4 and 2 in parts
    assert sorted((wk & 0x00FFFFFF).tolist()) == sorted(m for m, k in enumerate(parts) for _ in range(k))
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(lay.N, F, device=DEV, generator=g)
    W = torch.randn(lay.P, F, device=DEV, generator=g)
    flag = torch.randint(0, 4, (lay.P,), device=DEV, generator=g, dtype=torch.uint8)
    xn, Wn, fn = x.cpu().numpy(), W.cpu().numpy(), flag.cpu().numpy()
    pi, pj = lay.pair_i.cpu().numpy(), lay.pair_j.cpu().numpy()
    monkeypatch.setenv("GEOSSL_AGG_NO_SPLIT", "1")
    lay_one = MolLayout(batch, len(sizes), sizes=sizes)
    assert lay_one.agg_work is None
    for swap in (False, True):
        out_t = ops.aggregate(x, W, flag, lay, swap=swap)
        assert torch.equal(out_t, ops.aggregate(x, W, flag, lay_one, swap=swap))
        out = out_t.cpu().numpy()
        contrib = {}
        for p in range(lay.P):
            i, j, fl = int(pi[p]), int(pj[p]), int(fn[p])
            if swap:
                fl = ((fl & 1) << 1) | ((fl >> 1) & 1)
            if fl & 1:
                contrib.setdefault(i, []).append((j, p))
            if fl & 2:
                contrib.setdefault(j, []).append((i, p))
        ref = np.zeros_like(xn)
        for tgt, lst in contrib.items():
            acc = np.zeros(F, dtype=np.float32)
            for src, p in sorted(lst):
                acc = (acc + (xn[src] * Wn[p]).astype(np.float32)).astype(np.float32)
            ref[tgt] = acc
        assert np.array_equal(out, ref), swap


@pytest.mark.gpu
def test_trainer_draws_its_own_noise_into_the_graph_inputs():
    """DDMTrainer.step(batch, None, structure_key=...) with device_noise=True: the five draws of the step are made on
    the device straight into the captured graph's static inputs (no staging copies).  Same seed -> same losses as
    passing the very same draws explicitly; successive steps see different noise."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import make_batch
    cfg = dict(hidden_channels=128, num_filters=128, num_interactions=2, num_gaussians=51, cutoff=5.0, node_class=9)
    b = make_batch(48, seed=5)
    batch = pg.Batch.from_numpy(b, DEV)

    def trainer():
        return pg.DDMTrainer(product_schnet(cfg, DEV), product_ncsn(128, 50, 2.0, DEV), product_ncsn(128, 50, 2.0, DEV),
                             device_noise=True, use_graph=True)

    tr = trainer()
    torch.cuda.manual_seed(99)
    own = [float(tr.step(batch, None, structure_key="k")) for _ in range(3)]
    assert all(np.isfinite(own)) and len(set(own)) == 3
    tr2 = trainer()
    torch.cuda.manual_seed(99)
    explicit = []
    for _ in range(3):
        nz = tr2._draw_noise(batch)  # the same generator calls in the same order
        explicit.append(float(tr2.step(batch, nz, structure_key="k")))
    assert own == explicit


@pytest.mark.gpu
def test_schnet_latent_only_skips_the_readout():
    g = load_golden("g4_schnet_reduced")
    cfg = cfg_of(g)
    model = product_schnet(cfg, DEV)
    z, pos, batch = t(g["x"], DEV), t(g["positions"], DEV), t(g["batch"], DEV)
    z = z[:, 0] if z.dim() == 2 else z
    out, h = model(z, pos, batch, return_latent=True)
    none, h2 = model(z, pos, batch, return_latent=True, latent_only=True)
    assert none is None and torch.equal(h, h2)


# ------------------------------------------------------------------- two-fp16-piece kernels: scales and accuracy
def _filter_problem(nmol, seed, F=128, G=51, L=2, cutoff=5.0, mode="B", sizes=None, move=None, geometry=None):
    """A two-layer filter-network problem on synthetic molecules, through the raw C ABI: returns the tensors the
    backward kernel consumes and an fp64 evaluation of what it must produce (schnet.py:141-145,186-195 differentiated
    w.r.t. the filter weights).  `sizes`: the molecules' atom counts instead of the set's own; `move(positions)`: edits
    the host positions in place; `geometry(pair_d, pair_c, pair_flag)`: edits the pair-slot tensors in place before
    any kernel reads them."""
    import ctypes as C
    import math
    from geossl_amd import _lib, ops
    from geossl_amd._lib import call, ptr, stream
    from geossl_amd.layout import MolLayout
    from geossl_amd.synthetic import make_batch
    b = make_batch(nmol, seed=seed, mode=mode, sizes=sizes)
    sizes = [int(n) for n in b["sizes"]]
    batch = torch.arange(len(sizes), device=DEV).repeat_interleave(torch.tensor(sizes, device=DEV))
    lay = MolLayout(batch, len(sizes), sizes=sizes)
    positions = np.array(b["positions"], dtype=np.float32)
    if move is not None:
        move(positions)
    pos = torch.from_numpy(positions).to(DEV)
    pair_d, pair_c, pair_flag = ops.pair_geometry(pos, lay, cutoff)
    if geometry is not None:
        geometry(pair_d, pair_c, pair_flag)
    gen = torch.Generator().manual_seed(seed)
    N, P = lay.N, lay.P
    offset = torch.linspace(0.0, cutoff, G).to(DEV)
    # (a single Gaussian has no spacing: it gets the width of the whole range)
    coeff = -0.5 / (float(offset[1] - offset[0]) if G > 1 else float(cutoff)) ** 2
    ws = [[(torch.randn(F, G, generator=gen) / G ** 0.5).to(DEV), (0.3 * torch.randn(F, generator=gen)).to(DEV),
           (torch.randn(F, F, generator=gen) / F ** 0.5).to(DEV), (0.3 * torch.randn(F, generator=gen)).to(DEV)] for _ in range(L)]
    xs = [torch.randn(N, F, generator=gen).to(DEV) for _ in range(L)]
    daggs = [torch.randn(N, F, generator=gen).to(DEV) for _ in range(L)]
    fw = _lib.FilterWeights()
    for l, w in enumerate(ws):
        fw.w1[l], fw.b1[l], fw.w2[l], fw.b2[l] = (ptr(x) for x in w)
    Wf = torch.empty(L, P, F, device=DEV)
    T = torch.empty(L, P, F, device=DEV)
    call("geossl_cfconv_filter_fwd", ptr(pair_d), ptr(pair_c), P, C.byref(fw), L, F, G, ptr(offset), coeff, ptr(T), ptr(Wf), stream())

    def run(daggs_, saved_T=True, outs=None, dyn_P=None):
        """saved_T=False: T = NULL, the kernel rebuilds the hidden rows (GEOSSL_FILTER_RECOMPUTE_T); `outs`: the output
        tensors to write (else zeros); `dyn_P`: an int32 device tensor with the number of pair slots that exist (the
        capacity launch geossl_cfconv_filter_bwd_dyn)."""
        gin, gout = _lib.FilterGradIn(), _lib.FilterGradOut()
        if outs is None:
            outs = [[torch.zeros(F, G, device=DEV), torch.zeros(F, device=DEV), torch.zeros(F, F, device=DEV),
                     torch.zeros(F, device=DEV)] for _ in range(L)]
        for l in range(L):
            gin.x[l], gin.dagg[l] = ptr(xs[l]), ptr(daggs_[l])
            gout.dw1[l], gout.db1[l], gout.dw2[l], gout.db2[l] = (ptr(o) for o in outs[l])
        nfl = _lib.load().geossl_cfconv_filter_bwd_workspace_floats(P, L, F, G)
        wsp = torch.empty(nfl, device=DEV)
        args = (ptr(pair_d), ptr(pair_c), ptr(pair_flag), ptr(lay.pair_i), ptr(lay.pair_j), P, N, C.byref(fw),
                C.byref(gin), L, F, G, ptr(offset), coeff, ptr(T) if saved_T else None, C.byref(gout), ptr(wsp), 0)
        if dyn_P is None:
            call("geossl_cfconv_filter_bwd", *args, stream())
        else:
            call("geossl_cfconv_filter_bwd_dyn", *args, ptr(dyn_P), None, stream())
        torch.cuda.synchronize()
        return outs

    def ref64(daggs_):
        i, j = lay.pair_i.long(), lay.pair_j.long()
        fl = pair_flag.long()
        m0 = ((fl & 1) > 0).double() * pair_c.double()
        m1 = ((fl & 2) > 0).double() * pair_c.double()
        rbf = torch.exp(coeff * (pair_d.double()[:, None] - offset.double()[None, :]) ** 2)
        outs = []
        for l, (w1, b1, w2, b2) in enumerate(ws):
            x, dg = xs[l].double(), daggs_[l].double()
            dO = m0[:, None] * (dg[i] * x[j]) + m1[:, None] * (dg[j] * x[i])
            u = rbf @ w1.double().t() + b1.double()
            tt = torch.nn.functional.softplus(u) - math.log(2.0)
            dU = (dO @ w2.double()) * torch.sigmoid(u)
            outs.append([dU.t() @ rbf, dU.sum(0), dO.t() @ tt, dO.sum(0)])
        return outs

    run.inputs = dict(pair_d=pair_d, pair_c=pair_c, pair_flag=pair_flag, ws=ws, xs=xs, offset=offset, coeff=coeff, P=P,
                      pos=pos, cutoff=cutoff, fw=fw)
    return lay, daggs, run, ref64


def _check_filter_grads(got, ref, tol, what):
    for l, (g4, r4) in enumerate(zip(got, ref)):
        for name, g, r in zip(("dw1", "db1", "dw2", "db2"), g4, r4):
            err = float((g.double() - r).abs().max() / r.abs().max().clamp_min(1e-300))
            assert err < tol, (what, l, name, err)


@pytest.mark.parametrize("F, G", [(128, 51), (64, 20), (32, 8)])
def test_filter_backward_direct_vs_fp64_and_operand_scale_paths(F, G):
    """geossl_cfconv_filter_bwd through the C ABI against fp64.  The kernel runs on two fp16 pieces per operand with
    running power-of-two block scales (csrc/split.h, filter_bwd.hip): upstream gradients of ordinary size, tiny (1e-12),
    large (1e+6), and with magnitudes that RISE and FALL by 2^30 along the atoms (so tiles late in a block's range raise
    the running scale and the accumulators are rescaled) must all keep the accuracy of an fp32 GEMM chain."""
    lay, daggs, run, ref64 = _filter_problem(nmol=300 if F == 128 else 150, seed=11, F=F, G=G)
    N = lay.N
    ramp = torch.exp2(torch.linspace(-20.0, 10.0, N, device=DEV).round())
    cases = {"plain": daggs, "tiny": [d * 1e-12 for d in daggs], "large": [d * 1e6 for d in daggs],
             "rising": [d * ramp[:, None] for d in daggs], "falling": [d * ramp.flip(0)[:, None] for d in daggs]}
    for what, dg in cases.items():
        _check_filter_grads(run(dg), ref64(dg), 3e-6, what)


def test_filter_backward_is_exactly_linear_in_powers_of_two():
    """Scaling the upstream gradient by 2^k scales every operand piece, every operand scale and every accumulator by an
    exact power of two: the weight gradients must come out bit-identical up to that factor."""
    lay, daggs, run, _ = _filter_problem(nmol=120, seed=5)
    base = run(daggs)
    for k in (-24, 17):
        got = run([d * (2.0 ** k) for d in daggs])
        for g4, b4 in zip(got, base):
            for g, b0 in zip(g4, b4):
                assert torch.equal(g, b0 * (2.0 ** k)), k


@pytest.mark.parametrize("scale_w, scale_in", [(1e-3, 1.0), (30.0, 1.0), (1.0, 1e-9), (1.0, 1e5)])
def test_chain_and_wgrad_keep_fp32_accuracy_at_any_operand_scale(scale_w, scale_in):
    """The chained row kernel and the weight-gradient GEMM (two fp16 pieces, per-row / per-block / per-matrix power-of-two
    scales) against fp64 with operands far from 1: rows whose magnitudes span 2^24 inside one launch included."""
    from geossl_amd import ops
    gen = torch.Generator().manual_seed(3)
    R, F = 5000, 128
    rowmag = torch.exp2(torch.randint(-12, 13, (R, 1), generator=gen).float())
    X = (torch.randn(R, F, generator=gen) * rowmag * scale_in).to(DEV)
    Ws = [(torch.randn(F, F, generator=gen) / F ** 0.5 * scale_w).to(DEV) for _ in range(3)]
    bs = [(0.1 * scale_w * scale_in * torch.randn(F, generator=gen)).to(DEV) for _ in range(3)]
    imgs = ops.prepare_chain(Ws)
    outs = [torch.empty(R, F, device=DEV) for _ in range(3)]
    ops.linear_chain(X, [dict(image=imgs[s], bias=bs[s], out=outs[s]) for s in range(3)])
    ref = X.double()
    for s in range(3):
        ref = ref @ Ws[s].double().t() + bs[s].double()
        # per row: rows differ by 2^24 in size, each must be accurate at its own scale
        err = ((outs[s].double() - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-300)).max()
        assert float(err) < 3e-6 * (s + 1), (s, float(err))
    A = X
    B = (torch.randn(R, F, generator=gen) * rowmag.flip(0) * scale_w).to(DEV)
    dW, db = torch.zeros(F, F, device=DEV), torch.zeros(F, device=DEV)
    ops.linear_wgrad([(A, B, dW, db)], R, F, F)
    refW = A.double().t() @ B.double()
    assert float((dW.double() - refW).abs().max() / refW.abs().max()) < 3e-6
    refb = A.double().sum(0)
    assert float((db.double() - refb).abs().max() / refb.abs().max()) < 3e-6
