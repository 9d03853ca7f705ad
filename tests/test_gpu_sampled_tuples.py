"""GPU tests of sampled atom tuples on capacity buckets (``DeviceLoader(tuple_ratio=)``, geossl_sampled_tuples): the
device draw against its Python twin bit for bit, the incidence lists of both modes against geossl_incidence_count +
cumsum + geossl_incidence_fill, numpy mode against the host extractor's collated batch, the replayed DDM and Distance
Prediction steps against the eager ones (handles and marked collated batches, SchNet and PaiNN, one bucket graph), a
trainer run on shuffled handles, and the DDM step on a sampled batch against the fp64 oracle."""
import types

import numpy as np
import pytest
import torch

import sampled_tuples_twin as tw
from conftest import rel_err
from helpers import (fill_module_, ncsn_oracle_params, product_ncsn, product_schnet, schnet_oracle_params, t,
                     unique_named_grads)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [5, 1, 2, 3, 4, 33, 34, 70, 3]
FULL = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=5.0, node_class=9,
            readout="mean")
TOL_OUT, TOL_GRAD = 1e-5, 1e-4     # the bounds of test_gpu_round4's oracle tests of the DDM step
_CACHE = {}


def _molecules(sizes=SIZES, seed=3):
    from geossl_amd.synthetic import add_bonds, make_molecules
    key = (tuple(sizes), seed)
    if key not in _CACHE:
        _CACHE[key] = add_bonds(make_molecules(0, seed=seed, sizes=sizes), seed=seed)
    return _CACHE[key]


def _dataset(option, sizes=SIZES, **kw):
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    return DeviceDataset.from_numpy(_molecules(sizes), DEV, option=option, **kw)


def _loader(ds, **kw):
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    kw.setdefault("batch_size", len(ds))
    kw.setdefault("shuffle", False)
    return DeviceLoader(ds, **kw)


def _bucket(batch, kind="schnet", views=1):
    from geossl_amd import bucket as bk
    bkt = bk.Bucket.for_batch(batch, bk.option_of(batch), kind, views)
    counts = bkt.fill(batch)
    return bkt, counts


def _reference_incidence(bkt, N, S):
    """inc_ptr / inc_idx of the bucket's own list by the kernels the eager SuperEdgeLayout uses."""
    from geossl_amd._lib import call, ptr, stream
    cnt = torch.zeros(N, dtype=torch.int32, device=DEV)
    sei = bkt.sei[:, :S].contiguous()
    call("geossl_incidence_count", ptr(bkt.batch_vec), ptr(sei[0]), ptr(sei[1]), ptr(bkt.sel.se_ptr), N, 3, ptr(cnt),
         stream())
    iptr = torch.zeros(N + 1, dtype=torch.int64, device=DEV)
    iptr[1:] = torch.cumsum(cnt, 0, dtype=torch.int64)
    idx = torch.full((max(2 * S, 1),), -1, dtype=torch.int32, device=DEV)
    call("geossl_incidence_fill", ptr(bkt.batch_vec), ptr(sei[0]), ptr(sei[1]), ptr(bkt.sel.se_ptr), N, 3, ptr(iptr),
         ptr(idx), stream())
    return iptr, idx[:2 * S]


def _check_incidence(bkt, counts, sei_np):
    N, S = counts[0], counts[2]
    iptr, idx = _reference_incidence(bkt, N, S)
    assert torch.equal(bkt.sel.inc_ptr[:N + 1], iptr) and int(iptr[-1]) == 2 * S
    assert torch.equal(bkt.sel.inc_idx[:2 * S], idx)
    p2, i2 = tw.incidence(N, sei_np)
    assert np.array_equal(iptr.cpu().numpy(), p2) and np.array_equal(idx.cpu().numpy(), i2)
    return iptr


# ---------------------------------------------------------------------------------------------------- 1. device mode
@pytest.mark.parametrize("option,ratio", [("combination", 0.3), ("permutation", 0.5)])
@pytest.mark.parametrize("masked", [False, True])
def test_device_draw_is_the_twins(option, ratio, masked):
    """handle.super_edge_index and the bucket's sei are the twin's tuples bit for bit; the incidence lists are those of
    the eager kernels (molecules with k = 0 and atoms of degree 0 included); a second epoch draws other tuples."""
    ds = _dataset(option)
    kw = dict(mask_ratio=0.25) if masked else {}
    loader = _loader(ds, tuple_ratio=ratio, **kw)
    np.random.seed(11)
    (hb,) = list(loader)
    (hb2,) = list(loader)
    want = tw.device_tuples(hb._sizes, hb.ids, option, ratio, hb._tuple_draw.seed)
    assert hb._canonical is None and hb._sampled == (option, ratio) and want.shape[1] == hb.n_super
    if not masked:
        assert hb.tuple_counts.tolist() == tw.brute_counts(SIZES, option, ratio)
    bkt, counts = _bucket(hb)
    S = counts[2]
    assert S == hb.n_super and int(bkt.dims[3]) == S
    assert np.array_equal(bkt.sei[:, :S].cpu().numpy(), want)
    got = hb.super_edge_index
    assert got.dtype == torch.long and np.array_equal(got.cpu().numpy(), want)
    iptr = _check_incidence(bkt, counts, want)
    deg = (iptr[1:] - iptr[:-1]).cpu().numpy()
    assert (deg == 0).any() and (hb.tuple_counts == 0).any()
    bkt.tuple_status.check()
    # the other epoch: another seed, other tuples, the same counts; refilled into the same bucket
    assert hb2._tuple_draw.seed != hb._tuple_draw.seed
    want2 = tw.device_tuples(hb2._sizes, hb2.ids, option, ratio, hb2._tuple_draw.seed)
    assert want2.shape == want.shape and not np.array_equal(want2, want)
    bkt.fill(hb2)
    assert np.array_equal(bkt.sei[:, :S].cpu().numpy(), want2)
    _check_incidence(bkt, counts, want2)


def test_device_draw_of_a_255_atom_molecule():
    """The select that recomputes its keys (64 770 slots of "permutation" at 255 atoms) beside the one-pass form."""
    sizes = [255, 5, 3]
    ds = _dataset("permutation", sizes)
    np.random.seed(2)
    (hb,) = list(_loader(ds, tuple_ratio=0.1))
    assert hb.tuple_counts.tolist() == [6477, 2, 0]
    want = tw.device_tuples(sizes, hb.ids, "permutation", 0.1, hb._tuple_draw.seed)
    bkt, counts = _bucket(hb)
    assert np.array_equal(bkt.sei[:, :counts[2]].cpu().numpy(), want)
    assert np.array_equal(hb.super_edge_index.cpu().numpy(), want)
    _check_incidence(bkt, counts, want)
    bkt.tuple_status.check()


# ----------------------------------------------------------------------------------- 2 / 3. given mode, numpy mode
def _host_collated(d, option, ratio, ids=None, radius=None):
    """BatchAtomTuple.from_data_list over AtomTupleExtractor(ratio)(molecule), moved to the device."""
    from geossl_amd.Geom3D.dataloaders.dataloaders_AtomTuple import AtomTupleExtractor, BatchAtomTuple, Data
    off = np.concatenate([[0], np.cumsum(d["sizes"])])
    ext = AtomTupleExtractor(ratio, option)
    mols = [ext(Data(x=torch.from_numpy(d["x"][off[i]:off[i + 1]]), positions=torch.from_numpy(d["positions"][off[i]:off[i + 1]])))
            for i in (range(len(d["sizes"])) if ids is None else ids)]
    b = BatchAtomTuple.from_data_list(mols).to(DEV)
    if radius is not None:
        from geossl_amd import ops
        b.radius_edge_index = ops.radius_graph(b.positions, radius, b.batch)
    return b


@pytest.mark.parametrize("option,ratio", [("combination", 0.3), ("permutation", 0.5)])
def test_numpy_mode_is_the_host_extractors_batch(option, ratio):
    """tuple_rng="numpy": the handle shows the collated batch of the host extractor on the same molecules and seed, bit
    for bit, and both fill a bucket with that list and the eager kernels' incidence lists (given mode)."""
    ds = _dataset(option)
    np.random.seed(7)
    (hb,) = list(_loader(ds, tuple_ratio=ratio, tuple_rng="numpy"))
    np.random.seed(7)
    co = _host_collated(_molecules(), option, ratio)
    assert co._sampled == hb._sampled == (option, ratio) and co._canonical is None
    for k in ("x", "positions", "batch", "super_edge_index"):
        assert torch.equal(getattr(hb, k), getattr(co, k)), k
    want = co.super_edge_index.cpu().numpy()
    for batch in (hb, co):
        bkt, counts = _bucket(batch)
        assert np.array_equal(bkt.sei[:, :counts[2]].cpu().numpy(), want)
        _check_incidence(bkt, counts, want)
        bkt.tuple_status.check()


def test_a_tuple_that_leaves_its_molecule_sets_the_status():
    np.random.seed(7)
    co = _host_collated(_molecules(), "combination", 0.3)
    bkt, counts = _bucket(co)
    bkt.tuple_status.check()
    sei = co.super_edge_index.clone()
    sei[1, 5] = 0                      # (tuple 5 belongs to the sixth molecule: atom 0 is the first one's)
    co.super_edge_index = sei
    bkt.fill(co)
    with pytest.raises(IndexError, match="super_edge_index"):
        bkt.tuple_status.check()
    iptr = bkt.sel.inc_ptr[:counts[0] + 1]
    assert int(iptr[-1]) == 2 * counts[2] and bool((iptr[1:] >= iptr[:-1]).all())
    idx = bkt.sel.inc_idx[:2 * counts[2]]
    assert int(idx.min()) >= 0 and int(idx.max()) < counts[2]


# ------------------------------------------------------------------------------------------- 4. replay against eager
def _backbone(kind):
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    if kind == "schnet":
        return fill_module_(SchNet(hidden_channels=128, num_filters=128, num_interactions=3, num_gaussians=51,
                                   cutoff=10.0, node_class=9)).to(DEV)
    return fill_module_(PaiNN(n_atom_basis=128, n_interactions=2, n_rbf=20, cutoff=5.0, max_z=9, n_out=1,
                              readout="add")).to(DEV)


def _pool():
    from geossl_amd.synthetic import make_molecules
    if "pool" not in _CACHE:
        _CACHE["pool"] = make_molecules(90, seed=4, mode="B")
    return _CACHE["pool"]


def _four_batches(kind, source, option, ratio):
    """Four ragged batches of nine molecules: handles of a shuffled loader, or the host extractor's marked batches."""
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    rad = {"radius": 5.0} if kind == "painn" else {}
    np.random.seed(21)
    if source == "handles":
        ds = DeviceDataset.from_numpy(_pool(), DEV, option=option, **rad)
        loader = _loader(ds, batch_size=9, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(2),
                         tuple_ratio=ratio)
        return [hb for _, hb in zip(range(4), loader)]
    order = np.random.default_rng(5).permutation(90)
    return [_host_collated(_pool(), option, ratio, order[9 * k:9 * k + 9], rad.get("radius")) for k in range(4)]


def _grads(*modules):
    return [p.grad.detach().clone() for m in modules for p in m.parameters() if p.grad is not None]


def _compare(step, modules, batches):
    """loss 1e-6, gradients 1e-5: the bounds of test_gpu_distance._replay_vs_eager."""
    for k, b in enumerate(batches):
        out = []
        for graph in (False, True):
            for m in modules:
                m.zero_grad(set_to_none=True)
            loss = step(b, graph)
            loss.backward()
            out.append((loss.detach().clone(), _grads(*modules)))
        assert rel_err(out[1][0].cpu(), out[0][0].cpu()) < 1e-6, k
        assert len(out[1][1]) == len(out[0][1]) > 0
        for a, c in zip(out[1][1], out[0][1]):
            assert rel_err(a, c) < 1e-5, k


def _one_bucket_graph(model, slot, option, ratio):
    (sg,) = model.__dict__[slot].graphs.values()
    assert len(sg) == 1
    assert next(iter(sg.graphs)) == ("bucket", 9, (option, ratio))


@pytest.mark.parametrize("source", ["handles", "collated"])
@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_distance_replay_matches_eager(kind, source, monkeypatch):
    from geossl_amd.pretrain_DistancePrediction import DistancePredictor, do_DistancePrediction
    monkeypatch.setenv("GEOSSL_SAMPLED_BUCKETS", "1")
    option, ratio = "permutation", 0.3
    model, dp = _backbone(kind), fill_module_(DistancePredictor(128)).to(DEV)
    args = types.SimpleNamespace(model_3d=kind)
    _compare(lambda b, graph: do_DistancePrediction(args, b, model, dp, graph=graph), (model, dp),
             _four_batches(kind, source, option, ratio))
    _one_bucket_graph(model, "_geossl_distance_step", option, ratio)


@pytest.mark.parametrize("source", ["handles", "collated"])
@pytest.mark.parametrize("kind", ["schnet", "painn"])
def test_ddm_replay_matches_eager(kind, source, monkeypatch):
    """Two views, both heads, the five draws given: the replayed bucket step is the eager step of the same batch."""
    from geossl_amd import pretrain_GeoSSL as pg
    monkeypatch.setenv("GEOSSL_SAMPLED_BUCKETS", "1")
    option, ratio = "combination", 0.3
    model = _backbone(kind)
    n1, n2 = product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9)
    args = pg.Args(kind)
    gen = torch.Generator(device=DEV).manual_seed(9)

    def step(b, graph):
        nz = step.noise.get(id(b))
        if nz is None:
            N, S, B = b.positions.size(0), b.super_edge_index.size(1), b.num_graphs
            nz = step.noise[id(b)] = {
                "pos_noise": 0.3 * torch.randn(N, 3, device=DEV, generator=gen),
                "noise_level_1": torch.randint(0, 50, (B,), device=DEV, generator=gen),
                "dist_noise_1": torch.randn(S, 1, device=DEV, generator=gen),
                "noise_level_2": torch.randint(0, 50, (B,), device=DEV, generator=gen),
                "dist_noise_2": torch.randn(S, 1, device=DEV, generator=gen)}
        return pg.do_DDM(args, b, model, NCSN_models=(n1, n2), noise=nz, graph=graph)[0]
    step.noise = {}
    _compare(step, (model, n1, n2), _four_batches(kind, source, option, ratio))
    _one_bucket_graph(model, "_geossl_autograd_step", option, ratio)


@pytest.mark.parametrize("objective", ["ddm", "distance", "distance_painn"])
def test_trainer_on_shuffled_sampled_handles_keeps_one_graph(objective):
    """Ten shuffled steps (masked handles for DDM and for PaiNN, whose surviving radius edges are counted on the device
    in the same fill): one bucket graph, at most two captures."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    from geossl_amd.pretrain_DistancePrediction import DistancePredictionTrainer, DistancePredictor
    from geossl_amd.synthetic import add_bonds
    if "pool_bonds" not in _CACHE:
        _CACHE["pool_bonds"] = add_bonds(dict(_pool()), seed=1)
    masked, kind = objective != "distance", "painn" if objective == "distance_painn" else "schnet"
    ds = DeviceDataset.from_numpy(_CACHE["pool_bonds"], DEV, option="combination",
                                  **({"radius": 5.0} if kind == "painn" else {}))
    np.random.seed(4)
    loader = _loader(ds, batch_size=9, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(6),
                     tuple_ratio=0.3, **(dict(mask_ratio=0.15) if masked else {}))
    if objective == "ddm":
        tr = pg.DDMTrainer(_backbone("schnet"), product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9),
                           use_graph=True)
    else:
        tr = DistancePredictionTrainer(_backbone(kind), fill_module_(DistancePredictor(128)).to(DEV), model_3d=kind,
                                       use_graph=True)
    losses = [tr.step(hb) for hb in loader]
    assert len(losses) == 10 and all(bool(torch.isfinite(l_)) for l_ in losses)
    sg = tr.step_graphs
    assert tr.use_graph and len(sg) == 1 and sg.captures <= 2
    assert next(iter(sg.graphs)) == ("bucket", 9, ("combination", 0.3))


def test_switch_off_sampled_handles_run_eagerly_and_never_share_a_graph(monkeypatch):
    """GEOSSL_SAMPLED_BUCKETS=0: ten shuffled sampled SchNet handles, each freed before the next is made, through
    DDMTrainer(use_graph=True) give the eager step's loss and gradients and capture nothing - every handle has a
    fingerprint of its own, whatever addresses the interpreter hands out again.  A handle that does come back gets its
    own graph at the second sighting and replays it at the third."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    monkeypatch.setenv("GEOSSL_SAMPLED_BUCKETS", "0")
    ds = DeviceDataset.from_numpy(_pool(), DEV, option="combination")
    np.random.seed(8)
    loader = _loader(ds, batch_size=9, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(3),
                     tuple_ratio=0.3)
    make = lambda use_graph: pg.DDMTrainer(_backbone("schnet"), product_ncsn(128, 50, 2, DEV),
                                           product_ncsn(128, 50, 2, DEV, scale=0.9), use_graph=use_graph)
    tr, ref = make(True), make(False)
    gen = torch.Generator(device=DEV).manual_seed(4)

    def noise(hb):
        N, S, B = hb.n_atoms, hb.n_super, hb.num_graphs
        return {"pos_noise": 0.3 * torch.randn(N, 3, device=DEV, generator=gen),
                "noise_level_1": torch.randint(0, 50, (B,), device=DEV, generator=gen),
                "dist_noise_1": torch.randn(S, 1, device=DEV, generator=gen),
                "noise_level_2": torch.randint(0, 50, (B,), device=DEV, generator=gen),
                "dist_noise_2": torch.randn(S, 1, device=DEV, generator=gen)}

    def same(hb, nz):
        got, want = tr._graph_fwd_bwd(hb, nz), ref._fwd_bwd(hb, nz)
        assert rel_err(got.cpu(), want.cpu()) < 1e-6
        assert rel_err(tr.flat.grad.cpu(), ref.flat.grad.cpu()) < 1e-5

    prints, sizes = set(), set()
    for hb in loader:                       # (no handle outlives its step)
        prints.add(hb.fingerprint())
        sizes.add(hb.n_atoms)
        same(hb, noise(hb))
    assert len(prints) == 10 and len(sizes) > 1
    assert tr.use_graph and len(tr.step_graphs) == 0 and tr.step_graphs.captures == 0
    nz = noise(hb)
    same(hb, nz)                            # second sighting of the last handle: its own graph is captured ...
    assert tr.step_graphs.captures == 1 and next(iter(tr.step_graphs.graphs))[0] == "sampled"
    same(hb, nz)                            # ... and replayed
    assert tr.step_graphs.captures == 1 and len(tr.step_graphs) == 1


def test_a_step_that_reads_no_tuples_runs_on_sampled_handles():
    """InfoNCE reads no pair tuples: on sampled handles it replays the sampled bucket (the draw is made and not read)
    and gives the loss of the eager step on the same molecules and noise."""
    from geossl_amd import pretrain_GeoSSL as pg
    (hb,) = _four_batches("schnet", "handles", "combination", 0.3)[:1]
    model = _backbone("schnet")
    nz = {"pos_noise": 0.3 * torch.randn(hb.n_atoms, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))}
    out = []
    for use_graph in (False, True):
        tr = pg.ContrastiveTrainer(model, "InfoNCE", use_graph=use_graph)
        res = tr._graph_fwd_bwd(hb, nz) if use_graph else tr._eager(hb, nz)
        out.append((res[0] if isinstance(res, tuple) else res).detach().clone())
        if use_graph:
            assert next(iter(tr.step_graphs.graphs)) == ("bucket", 9, ("combination", 0.3))
    assert bool(torch.isfinite(out[0])) and rel_err(out[1].cpu(), out[0].cpu()) < 1e-6


# ----------------------------------------------------------------------------------------------------- 5. fp64 oracle
def test_sampled_ddm_step_vs_fp64_oracle():
    """The replayed DDM step of a sampled handle (the sizes above, "combination" at 0.3: S = 1054) against
    oracle.nets.do_ddm_schnet on the handle's own tuples: loss <= 1e-5, backbone gradients <= 1e-4 - the bounds of the
    full-enumeration oracle test of this step (test_gpu_round4.test_ragged_full_size_through_the_bucket_graph_vs_oracle)."""
    from geossl_amd import pretrain_GeoSSL as pg
    from oracle import nets
    ds = _dataset("combination")
    np.random.seed(13)
    (hb,) = list(_loader(ds, tuple_ratio=0.3))
    N, S, B = hb.n_atoms, hb.n_super, hb.num_graphs
    assert S == 1054
    rng = np.random.default_rng(6)
    nz = {"pos_noise": (0.3 * rng.normal(size=(N, 3))).astype(np.float32),
          "noise_level_1": rng.integers(0, 50, size=B).astype(np.int64),
          "dist_noise_1": rng.normal(size=(S, 1)).astype(np.float32),
          "noise_level_2": rng.integers(0, 50, size=B).astype(np.int64),
          "dist_noise_2": rng.normal(size=(S, 1)).astype(np.float32)}
    tr = pg.DDMTrainer(product_schnet(FULL, DEV), product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9),
                       lr=5e-4, use_graph=True)
    loss = tr._graph_fwd_bwd(hb, {k: t(v, DEV) for k, v in nz.items()})
    assert tr.use_graph and tr.step_graphs.captures == 1
    assert next(iter(tr.step_graphs.graphs)) == ("bucket", 9, ("combination", 0.3))
    Pm, P1, P2 = schnet_oracle_params(FULL), ncsn_oracle_params(128, 50), ncsn_oracle_params(128, 50, 0.9)
    ref = nets.do_ddm_schnet(Pm, P1, P2, hb.x.cpu(), hb.positions.cpu(), hb.batch.cpu(), hb.super_edge_index.cpu(),
                             t(nz["pos_noise"]), t(nz["noise_level_1"]), t(nz["dist_noise_1"]), t(nz["noise_level_2"]),
                             t(nz["dist_noise_2"]), 5.0, 6, 2, "mean")
    ref.backward()
    assert rel_err(loss.cpu(), ref.detach()) < TOL_OUT
    g = unique_named_grads(tr.model)
    for k in ("lin2.weight", "interactions.0.mlp.0.weight", "interactions.5.conv.lin1.weight",
              "interactions.2.conv.lin2.weight", "embedding.weight"):
        assert rel_err(g[k].cpu(), Pm[k].grad) < TOL_GRAD, k
