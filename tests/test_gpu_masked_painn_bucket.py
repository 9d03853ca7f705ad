"""GPU tests of masked PaiNN handles on capacity buckets: Bucket.fill of a DeviceLoader(mask_ratio=r) handle over a
dataset with radius edges - count launch, geossl_masked_edge_offsets, gather, geossl_painn_edge_layout_dyn, nothing read
back - against the unmodified reference (fixture G16), against the fill of the collated twin bit for bit, and through
the DDM and Charge Prediction steps; the by-value edge layout is untouched; GEOSSL_MASKED_PAINN_BUCKETS=0 restores the
collated route."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from helpers import fill_module_, product_ncsn
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _painn():
    """The reduced 3-interaction PaiNN of test_gpu_round6._painn_modules6."""
    from geossl_amd.Geom3D.models import PaiNN
    return fill_module_(PaiNN(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1,
                              readout="add")).to(DEV)


def _dataset(sizes, seed, cut=0.3, option="combination", positions=None):
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    from geossl_amd.synthetic import add_bonds, make_molecules
    mols = make_molecules(0, seed=seed, sizes=sizes)
    if positions is not None:
        mols["positions"] = np.asarray(positions, dtype=np.float32)
    mols = add_bonds(mols, seed=seed, cut=cut)
    return DeviceDataset.from_numpy(mols, DEV, option=option, radius=5.0)


def _round_up(v, g):
    return -(-int(v) // g) * g


def _caps(hbs, option, views):
    """Explicit capacities that hold every handle of `hbs` (edges: their host-side bounds)."""
    from geossl_amd import bucket as bk
    counts = [bk.batch_counts(np.asarray(h._sizes), option, views) for h in hbs]
    caps = tuple(_round_up(max(c[k] for c in counts) + 1, 64) + 64 for k in range(4))
    E_cap = _round_up(max(h.n_edges_bound for h in hbs) + 1, 64)
    hi = max(int(np.max(h._sizes)) for h in hbs)
    return caps, E_cap, bk.max_n_class(hi, None, "painn")


def _bucket(B, caps, E_cap, max_n, option="combination", views=2):
    from geossl_amd import bucket as bk
    return bk.Bucket(torch.device(DEV), B, caps, option, max_n=max_n, kind="painn", E_cap=E_cap, views=views)


def _twin(ds, hb):
    """The collated batch of the handle's masked molecules (from a handle of its own: `hb` stays as it was), as a
    bucket takes a collated batch."""
    from geossl_amd.Geom3D.dataloaders.device_dataset import DatasetBatch
    co = ds.collate(DatasetBatch(ds, hb.ids, hb._mask))
    co._sizes, co._canonical = [int(n) for n in hb._sizes], ds.option
    return co


def _device_E(bkt):
    return int(bkt.blob[bkt.off["e_ptr"] + bkt.B])


def _assert_same_fill(b_ds, b_co, co, shared_history):
    """Every structure of the masked handle's fill (b_ds) against the collated twin's (b_co) over the real counts.
    shared_history: both buckets have seen the same fills, so the uploaded blob in front of the dataset offsets and
    the whole group prefix are equal too; otherwise only what this fill defines is compared."""
    from geossl_amd import bucket as bk
    B, o, V = b_ds.B, b_ds.off, b_ds.views
    N, S, E = co.x.size(0), co.super_edge_index.size(1), co.radius_edge_index.size(1)
    assert b_ds.real == b_co.real and b_ds.real[0] == N and b_ds.real_E is None and b_co.real_E == E
    assert _device_E(b_ds) == E and int(b_ds.dims[bk.D_E2]) == V * E == int(b_co.dims[bk.D_E2])
    if shared_history:
        assert torch.equal(b_ds.blob[:o["src_off"]], b_co.blob[:o["src_off"]])
    assert torch.equal(b_ds.dims[:10], b_co.dims[:10])
    for name, n in (("mol_ptr", 2 * B + 1), ("pair_ptr", 2 * B + 1), ("se_ptr", B + 1), ("stats", 4),
                    ("inc_ptr", 2 * (N + 1))):
        assert torch.equal(b_ds.blob[o[name]:o[name] + n], b_co.blob[o[name]:o[name] + n]), name
    # the device-written edge offsets: the cumulative survivors per molecule
    per_mol = torch.bincount(co.batch[co.radius_edge_index[0]], minlength=B)
    want = torch.cat([per_mol.new_zeros(1), per_mol.cumsum(0)]).to(torch.int32)
    assert torch.equal(b_ds.blob[o["e_ptr"]:o["e_ptr"] + B + 1], want)
    for name, ref in (("x", co.x), ("positions", co.positions), ("batch_vec", co.batch)):
        assert torch.equal(getattr(b_ds, name)[:N], getattr(b_co, name)[:N]) and torch.equal(getattr(b_ds, name)[:N], ref), name
    assert torch.equal(b_ds.sei[:, :S], b_co.sei[:, :S]) and torch.equal(b_ds.sei[:, :S], co.super_edge_index)
    assert torch.equal(b_ds.sel.inc_idx[:2 * S], b_co.sel.inc_idx[:2 * S])
    assert torch.equal(b_ds.rei[:, :E], co.radius_edge_index)
    e1, e2 = b_ds.el, b_co.el
    assert torch.equal(e1.idx_i[:2 * E], e2.idx_i[:2 * E]) and torch.equal(e1.idx_j[:2 * E], e2.idx_j[:2 * E])
    for side in ("i", "j"):
        assert torch.equal(e1.inc[side][0][:2 * N + 1], e2.inc[side][0][:2 * N + 1]), side
        assert torch.equal(e1.inc[side][1][:2 * E], e2.inc[side][1][:2 * E]), side
    assert torch.equal(e1.mol_grp, e2.mol_grp) and torch.equal(e1.mol_grp_end, e2.mol_grp_end)
    G = int(e1.mol_grp[2 * B])
    if shared_history:
        assert torch.equal(e1.row_edge[:4 * G], e2.row_edge[:4 * G]) and torch.equal(e1.grp_atom[:G], e2.grp_atom[:G])
    mg, me = e1.mol_grp.cpu().numpy(), e1.mol_grp_end.cpu().numpy()
    live = np.zeros(G, dtype=bool)
    for m in range(2 * B):
        live[mg[m]:me[m]] = True
    live = torch.from_numpy(live).to(DEV)
    assert torch.equal(e1.grp_atom[:G][live], e2.grp_atom[:G][live])
    assert torch.equal(e1.row_edge[:4 * G].view(G, 4)[live], e2.row_edge[:4 * G].view(G, 4)[live])
    assert int(e1.status) == 0 and int(e2.status) == 0 and int(b_ds.ecap_status.word) == 0


# ------------------------------------------------------------------------------------- the device-side offsets alone
@pytest.mark.parametrize("B", [1, 63, 64, 256, 257, 300, 1000])
def test_masked_edge_offsets_is_the_exclusive_prefix(B):
    """geossl_masked_edge_offsets against numpy: e_ptr = exclusive prefix of the counts (the scan's chunks of 256 with a
    carry: B below, at and above them), dims word = views * E, status clear; a total above E_cap: every offset clamped
    to it and the status word set."""
    from geossl_amd._lib import call, ptr, stream
    rng = np.random.default_rng(B)
    cnt = rng.integers(0, 700, size=B).astype(np.int32)
    cnt[rng.random(B) < 0.3] = 0
    pre = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
    E = int(pre[-1])
    d_cnt = torch.from_numpy(cnt).to(DEV)
    for views, E_cap in ((2, E), (1, E + 64), (2, max(E // 2, 1) if E else 0)):
        e_ptr = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
        word = torch.full((3,), -7, dtype=torch.int32, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        call("geossl_masked_edge_offsets", ptr(d_cnt), B, E_cap, views, ptr(e_ptr), ptr(word[1:]), ptr(status), stream())
        assert np.array_equal(e_ptr[:B + 1].cpu().numpy(), np.minimum(pre, E_cap)) and int(e_ptr[B + 1]) == -7
        assert word.tolist() == [-7, views * min(E, E_cap), -7]
        assert int(status) == (1 if E > E_cap else 0)


# ------------------------------------------------------------------------- GPU 1: against the unmodified reference
@pytest.mark.parametrize("ratio", [0.3, 0.5])
def test_masked_bucket_fill_with_reference_kept_lists_is_the_reference_batch(ratio):
    """Fixture G16 (40 molecules of 1 .. 44 atoms, the first and fourth with one): Bucket(kind="painn").fill of the
    handle that carries the reference's kept lists writes the reference's masked batch - radius_edge_index of
    MoleculeDataset3DRadius.subgraph + collation, x, positions, batch - with the edge count and offsets made on the
    device (read here only to assert)."""
    from geossl_amd import bucket as bk
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, masking
    from geossl_amd.Geom3D.dataloaders.device_dataset import DatasetBatch
    g = load_golden("g16_masking")
    ds = DeviceDataset.from_numpy({k: g[k] for k in ("x", "positions", "sizes", "bond_index", "bond_counts")}, DEV,
                                  option="combination", radius=5.0)
    B = len(ds)
    tags = sorted(k[5:] for k in g if k.startswith("keep/") and float(k[5:].split("_")[0][1:]) == ratio)
    assert len(tags) == 2   # both seeds
    hbs = [DatasetBatch(ds, np.arange(B), masking.MaskDraw(ratio, keep=g["keep/" + tag])) for tag in tags]
    caps, E_cap, max_n = _caps(hbs, "combination", 2)
    bkt = _bucket(B, caps, E_cap, max_n)
    for tag, hb in zip(tags, hbs):
        want = g["rei/" + tag]
        N, P, S, W = bkt.fill(hb)
        assert hb._batch is None and hb.n_edges is None and bkt.real_E is None
        E = _device_E(bkt)
        assert E == want.shape[1] <= hb.n_edges_bound
        assert np.array_equal(bkt.rei[:, :E].cpu().numpy(), want), tag
        assert int(bkt.dims[bk.D_E2]) == 2 * E
        per_mol = np.bincount(g["batch/" + tag][want[0]], minlength=B)
        e_ptr = bkt.blob[bkt.off["e_ptr"]:bkt.off["e_ptr"] + B + 1].cpu().numpy()
        assert np.array_equal(e_ptr, np.concatenate([[0], np.cumsum(per_mol)]))
        assert N == int(g["kept/" + tag].sum())
        for key, got in (("x", bkt.x), ("positions", bkt.positions), ("batch", bkt.batch_vec)):
            assert np.array_equal(got[:N].cpu().numpy(), g["%s/%s" % (key, tag)]), (tag, key)
        assert int(bkt.el.status) == 0 and int(bkt.ecap_status.word) == 0


# --------------------------------------------------- GPU 2: every structure against the collated fill, bit for bit
def _handles(ds, idsets, ratio, mask_rng, seed=77):
    """Masked handles of the given id sets as a DeviceLoader makes them (device: one Philox seed; numpy: the reference's
    BFS on the host, molecule after molecule)."""
    from geossl_amd.Geom3D.dataloaders import masking
    from geossl_amd.Geom3D.dataloaders.device_dataset import DatasetBatch
    np.random.seed(seed)
    out = []
    for ids in idsets:
        keep = None
        if mask_rng == "numpy":
            keep = np.concatenate([masking.reference_bfs(int(ds.sizes[i]), ds.successors(int(i)), ratio)
                                   for i in ids]).astype(np.int32)
        out.append(DatasetBatch(ds, ids, masking.MaskDraw(ratio, seed=None if keep is not None else 1234 + seed,
                                                          keep=keep)))
    return out


def _ragged(M, seed, lo=2, hi=60, mean=22.0, sd=11.0):
    return np.clip(np.rint(np.random.default_rng(seed).normal(mean, sd, size=M)), lo, hi).astype(np.int64)


@pytest.fixture(scope="module")
def pool300():
    """300 molecules of 1 .. 60 atoms and one of 120 (more than 1024 radius edges: several 256-edge chunks of the
    gather); one-atom molecules first, last, in the middle and three in a row."""
    sizes = _ragged(300, 5)
    sizes[[0, 299, 150, 40, 41, 42]] = 1
    sizes[7] = 120
    ds = _dataset(sizes, 9)
    assert int(ds.edge_cnt[7]) > 1024
    return ds


@pytest.mark.parametrize("mask_rng", ["device", "numpy"])
@pytest.mark.parametrize("case", ["B1", "B300", "ones", "views1"])
def test_masked_handle_fill_writes_what_the_collated_fill_writes(pool300, case, mask_rng):
    """Two buckets of the same explicit capacities, one filled from the masked handle (four launches, no read-back), one
    from ds.collate of the same handle: blob, inputs, edges, two-view edge arrays, incidence lists and the group layout
    equal over the real counts.  B = 1; B = 300 (the offsets scan crosses 64 and 256; the 120-atom molecule); one-atom
    molecules first / last / in the middle / three in a row; a one-view bucket."""
    ds = pool300
    idsets = {"B1": [np.array([7]), np.array([12])],
              "B300": [np.arange(300), np.arange(300)[::-1].copy()],
              "ones": [np.array([0, 5, 40, 41, 42, 9, 150, 11, 299]), np.array([299, 7, 42, 41, 40, 3, 0, 8, 150])],
              "views1": [np.array([3, 0, 7, 20, 299, 31]), np.array([150, 9, 8, 41, 2, 6])]}[case]
    views = 1 if case == "views1" else 2
    hbs = _handles(ds, idsets, 0.3, mask_rng)
    caps, E_cap, max_n = _caps(hbs, "combination", views)
    B = len(idsets[0])
    b_ds, b_co = _bucket(B, caps, E_cap, max_n, views=views), _bucket(B, caps, E_cap, max_n, views=views)
    zero = torch.ones(100003, device=DEV)
    for hb in hbs:
        co = _twin(ds, hb)
        assert b_ds.fill(hb, zero=zero) == b_co.fill(co)
        assert hb._batch is None and hb.n_edges is None and not zero.any()
        zero.fill_(1.0)
        _assert_same_fill(b_ds, b_co, co, shared_history=True)


@pytest.mark.parametrize("mask_rng", ["device", "numpy"])
def test_masked_handle_fill_of_a_batch_without_edges(mask_rng):
    """Atoms placed 20 A apart (no radius edge, no bond): the fill runs, E = 0 on the device, every list is empty."""
    sizes = np.array([3, 2, 5, 1], dtype=np.int64)
    grid = np.stack(np.meshgrid(np.arange(3), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 3)[:11] * 20.0
    ds = _dataset(sizes, 3, positions=grid)
    assert ds.edges.size(1) == 0
    (hb,) = _handles(ds, [np.arange(4)], 0.3, mask_rng)
    assert hb.n_edges_bound == 0
    caps, E_cap, max_n = _caps([hb], "combination", 2)
    b_ds, b_co = _bucket(4, caps, E_cap, max_n), _bucket(4, caps, E_cap, max_n)
    co = _twin(ds, hb)
    assert co.radius_edge_index.size(1) == 0
    assert b_ds.fill(hb) == b_co.fill(co)
    _assert_same_fill(b_ds, b_co, co, shared_history=True)
    N = co.x.size(0)
    assert not b_ds.el.inc["i"][0][:2 * N + 1].any()


@pytest.mark.parametrize("mask_rng", ["device", "numpy"])
def test_refilled_bucket_keeps_no_stale_edge_count(pool300, mask_rng):
    """One bucket filled with many edges, then few, then many: each fill equals the fill of a FRESH bucket from the
    collated twin over the real counts (the device-side E, e_ptr and the lists' ends are rewritten every time)."""
    ds = pool300
    big, small = np.array([7, 20, 33, 64, 100, 250]), np.array([0, 41, 299, 150, 42, 12])
    hbs = _handles(ds, [big, small, big], 0.3, mask_rng)
    assert hbs[0].n_edges_bound > 8 * hbs[1].n_edges_bound
    caps, E_cap, max_n = _caps(hbs, "combination", 2)
    bkt = _bucket(6, caps, E_cap, max_n)
    seen = []
    for hb in hbs:
        co = _twin(ds, hb)
        fresh = _bucket(6, caps, E_cap, max_n)
        assert bkt.fill(hb) == fresh.fill(co)
        _assert_same_fill(bkt, fresh, co, shared_history=False)
        seen.append(_device_E(bkt))
    assert seen[1] < min(seen[0], seen[2])
    if mask_rng == "device":   # (the same seed and molecules: the same masks; the numpy stream has moved on)
        assert seen[0] == seen[2]


# ------------------------------------------------------------------------------------------------- GPU 3: the step
def _noise(N, S, B, seed):
    g = torch.Generator().manual_seed(seed)
    nz = {"pos_noise": 0.3 * torch.randn(N, 3, generator=g), "noise_level_1": torch.randint(0, 50, (B,), generator=g),
          "dist_noise_1": torch.randn(S, 1, generator=g), "noise_level_2": torch.randint(0, 50, (B,), generator=g),
          "dist_noise_2": torch.randn(S, 1, generator=g)}
    return {k: v.to(DEV) for k, v in nz.items()}


def _loader_handles(ds, B, ratio, mask_rng="device"):
    """Six masked handles from two epochs of a DeviceLoader, the largest edge bound first (capacities must not depend
    on the order of sightings)."""
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    np.random.seed(21)
    ld = DeviceLoader(ds, batch_size=B, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(6),
                      mask_ratio=ratio, mask_rng=mask_rng)
    hbs = [hb for _ in range(2) for hb in ld]
    assert len(hbs) == 6
    hbs.sort(key=lambda h: -h.n_edges_bound)
    return hbs


@pytest.fixture(scope="module")
def pool96():
    sizes = _ragged(96, 31, lo=1, hi=48, mean=20.0, sd=8.0)
    sizes[[4, 50]] = 1
    return _dataset(sizes, 31)


def test_masked_painn_handles_replay_one_bucket_graph_bit_for_bit(pool96):
    """DDMTrainer(model_3d="painn", use_graph=True) on six masked handles of two loader epochs: one capture, a bucket
    key, no handle after the first collated or counted; loss and flat gradient of every step bit-identical to the same
    launches made eagerly on a Bucket of the same capacities filled from ds.collate(h); within 2e-6 / 1e-5 of the plain
    eager step on the collated twin; a second run of the handle route repeats losses and parameters bit for bit."""
    from geossl_amd import bucket as bk
    from geossl_amd import pretrain_GeoSSL as pg
    ds, B = pool96, 32

    def trainer(use_graph):
        return pg.DDMTrainer(_painn(), product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9), lr=5e-4,
                             model_3d="painn", use_graph=use_graph)
    hbs = _loader_handles(ds, B, 0.3)
    nzs = [_noise(h.n_atoms, h.n_super, B, 500 + i) for i, h in enumerate(hbs)]
    tr = trainer(True)
    losses, grads = [], []
    for hb, nz in zip(hbs, nzs):
        losses.append(tr._graph_fwd_bwd(hb, nz).clone())
        grads.append(tr.flat.grad.clone())
    assert tr.use_graph and tr.step_graphs.captures == 1 and len(tr._graphs) == 1
    key = next(iter(tr._graphs))
    assert key[0] == "bucket"
    assert all(h._batch is None and h.n_edges is None for h in hbs[1:])
    bkt = tr._graphs[key]["bucket"]
    assert bkt.kind == "painn" and int(bkt.el.status) == 0 and int(bkt.ecap_status.word) == 0
    assert torch.isfinite(torch.stack(losses)).all()
    # ---- the same launches eagerly on a bucket of the same capacities, filled from the collated twins
    te = trainer(False)
    eb = bk.Bucket(torch.device(DEV), B, bkt.caps(), "combination", max_n=bkt.max_n, kind="painn", E_cap=bkt.E_cap)
    f32 = dict(dtype=torch.float32, device=DEV)
    sn = {"pos_noise": torch.zeros(eb.N_cap, 3, **f32), "dist_noise_1": torch.zeros(eb.S_cap, 1, **f32),
          "dist_noise_2": torch.zeros(eb.S_cap, 1, **f32), "noise_level_1": torch.zeros(B, dtype=torch.long, device=DEV),
          "noise_level_2": torch.zeros(B, dtype=torch.long, device=DEV)}
    twins = [_twin(ds, hb) for hb in hbs]
    for i, (co, nz) in enumerate(zip(twins, nzs)):
        N, P, S, W = eb.fill(co)
        sn["pos_noise"][:N].copy_(nz["pos_noise"])
        sn["dist_noise_1"][:S].copy_(nz["dist_noise_1"])
        sn["dist_noise_2"][:S].copy_(nz["dist_noise_2"])
        sn["noise_level_1"].copy_(nz["noise_level_1"])
        sn["noise_level_2"].copy_(nz["noise_level_2"])
        loss = te._fwd_bwd(eb.batch, sn)
        assert torch.equal(loss, losses[i]) and torch.equal(te.flat.grad, grads[i]), i
    # ---- the plain eager step on the collated twins themselves
    tp = trainer(False)
    for i, (co, nz) in enumerate(zip(twins, nzs)):
        loss = tp._fwd_bwd(co, nz)
        assert abs(float(loss) - float(losses[i])) <= 2e-6 * abs(float(loss)), i
        assert rel_err(tp.flat.grad, grads[i]) < 1e-5, i
    # ---- two training runs on fresh handles of the same loader
    runs = []
    for _ in range(2):
        t2 = trainer(True)
        out = [t2.step(hb, nz).clone() for hb, nz in zip(_loader_handles(ds, B, 0.3), nzs)]
        torch.cuda.synchronize()
        assert t2.step_graphs.captures == 1
        runs.append((torch.stack(out), t2.flat.flat.detach().clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0][0], losses[0])


# ------------------------------------------------------------------------------------ GPU 4: one one-view objective
def test_charge_prediction_on_masked_painn_handles_replays_one_bucket_graph():
    """test_gpu_charge's bucket-replay-against-eager pattern (numpy charge masks, 1e-6 / 1e-5) for the case its
    parametrisation stops short of: ("painn", 0.2) - masked PaiNN handles on a one-view bucket."""
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
    from geossl_amd.synthetic import add_bonds, make_molecules
    from objective_harness import assert_one_bucket, backbone, replay_vs_eager
    from test_gpu_charge import CASE
    mols = add_bonds(make_molecules(200, seed=3, mode="C"), seed=3, cut=0.3)
    ds = DeviceDataset.from_numpy(mols, DEV, option="permutation", radius=5.0)
    np.random.seed(8)
    loader = DeviceLoader(ds, batch_size=32, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(2),
                          mask_ratio=0.2, mask_rng="device")
    model = backbone("painn")
    sg = replay_vs_eager(CASE, "painn", model, CASE.heads("painn", model), [hb for _, hb in zip(range(4), loader)])
    assert_one_bucket(sg)
    (g,) = sg.graphs.values()
    assert g["bucket"].views == 1 and g["bucket"].real_E is None and int(g["bucket"].ecap_status.word) == 0


# -------------------------------------------------------------------------- GPU 5: the by-value layout is untouched
def test_edge_layout_dyn_writes_what_the_by_value_layout_writes():
    """geossl_painn_edge_layout and geossl_painn_edge_layout_dyn (the same E through device memory) on one unmasked
    batch, outputs pre-filled alike: every output array equal bit for bit, untouched slots included; an E above E_cap is
    clamped and reported."""
    from geossl_amd import _lib, ops
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd._lib import call, ptr, stream
    from geossl_amd.layout import MolLayout
    from geossl_amd.synthetic import make_batch
    sizes = np.array([18, 1, 33, 2, 60, 9, 1], dtype=np.int64)
    raw = make_batch(0, seed=31, sizes=sizes)
    raw["positions"][19 + 33:19 + 35] += np.array([[0, 0, 0], [30.0, 0, 0]], dtype=np.float32)   # the 2-atom molecule: no edge
    bt = pg.Batch.from_numpy(raw, DEV)
    e = ops.radius_graph(bt.positions, 5.0, bt.batch)
    E, N, B = int(e.size(1)), int(sizes.sum()), len(sizes)
    mol_ptr = MolLayout(bt.batch, B, sizes=list(sizes)).mol_ptr
    Ncap2, Ecap = 2 * N + 37, E + 100
    G = int(_lib.load().geossl_painn_group_capacity(2 * Ecap, Ncap2))
    i64, i32 = dict(dtype=torch.int64, device=DEV), dict(dtype=torch.int32, device=DEV)

    def outputs():
        return [torch.full((2 * Ecap,), -7, **i64), torch.full((2 * Ecap,), -7, **i64), torch.full((Ncap2 + 1,), -7, **i64),
                torch.full((2 * Ecap,), -7, **i32), torch.full((Ncap2 + 1,), -7, **i64), torch.full((2 * Ecap,), -7, **i32),
                torch.full((4 * G,), -9, **i32), torch.full((G,), -9, **i32), torch.zeros(2 * B + 1, **i32),
                torch.zeros(2 * B, **i32), torch.zeros(1, **i32)]
    by_value, dyn = outputs(), outputs()
    call("geossl_painn_edge_layout", ptr(e[0]), ptr(e[1]), E, ptr(mol_ptr), N, B, Ncap2, *[ptr(a) for a in by_value], stream())
    dE = torch.tensor([-1, E, -1], dtype=torch.int32, device=DEV)
    call("geossl_painn_edge_layout_dyn", ptr(e[0]), ptr(e[1]), Ecap, ptr(dE[1:]), ptr(mol_ptr), N, B, Ncap2,
         *[ptr(a) for a in dyn], stream())
    for k, (a, b) in enumerate(zip(by_value, dyn)):
        assert torch.equal(a, b), k
    assert int(by_value[-1]) == 0 and int(by_value[0][2 * E]) == -7 and int(by_value[8][2 * B]) == ((2 * E) >> 2) + 2 * N
    # the guard: a count above the capacity is clamped to it (no slot past the outputs is written) and reported
    short = outputs()
    call("geossl_painn_edge_layout_dyn", ptr(e[0]), ptr(e[1]), E - 8, ptr(dE[1:]), ptr(mol_ptr), N, B, Ncap2,
         *[ptr(a) for a in short], stream())
    assert int(short[-1]) == 1 and bool((short[0][2 * (E - 8):] == -7).all())


# ------------------------------------------------------------------------------------------------ GPU 6: switch off
def test_switch_off_runs_masked_painn_handles_on_their_collated_tensors(pool96, monkeypatch):
    """GEOSSL_MASKED_PAINN_BUCKETS=0: a masked PaiNN handle is materialised (counted, collated) and runs without a bucket
    graph as before; its loss agrees with the bucket route within 2e-6."""
    from geossl_amd import pretrain_GeoSSL as pg
    ds, B = pool96, 32
    losses = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("GEOSSL_MASKED_PAINN_BUCKETS", switch)
        hb = _loader_handles(ds, B, 0.3)[1]
        nz = _noise(hb.n_atoms, hb.n_super, B, 900)
        tr = pg.DDMTrainer(_painn(), product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9), lr=5e-4,
                           model_3d="painn", use_graph=True)
        losses[switch] = float(tr.step(hb, nz))
        keys = [k[0] for k in tr._graphs]
        if switch == "0":
            assert hb._batch is not None and hb.n_edges == hb.radius_edge_index.size(1) and "bucket" not in keys
        else:
            assert keys == ["bucket"] and hb.n_edges is None
    assert np.isfinite(losses["0"]) and abs(losses["0"] - losses["1"]) <= 2e-6 * abs(losses["0"]), losses
