"""GPU tests of BFS atom masking on the device loader: geossl_gather_masked_molecules with the reference's kept lists
(fixture G16) against the reference's subgraph + collation, the device draw against its CPU twin, and training on
masked handles."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import product_ncsn, product_schnet
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(hidden_channels=128, num_filters=128, num_interactions=2, num_gaussians=51, cutoff=5.0, node_class=9,
             readout="mean")


def _g16_dataset(option, radius=5.0):
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    g = load_golden("g16_masking")
    return g, DeviceDataset.from_numpy({k: g[k] for k in ("x", "positions", "sizes", "bond_index", "bond_counts")}, DEV,
                                       option=option, radius=radius)


@pytest.mark.parametrize("option", ["combination", "permutation"])
def test_masked_gather_with_reference_kept_lists_is_the_reference_batch(option):
    """Reproduction mode: the kept lists of the reference's own subgraph (G16) through geossl_gather_masked_molecules
    give x, positions, batch, super_edge_index and radius_edge_index of subgraph + AtomTupleExtractor +
    BatchAtomTuple.from_data_list element for element (one-atom molecules and isolated atoms included); the bucket's
    route (gather_into of the same handle) writes the same rows."""
    from geossl_amd.Geom3D.dataloaders import masking
    from geossl_amd.Geom3D.dataloaders.device_dataset import DatasetBatch
    g, ds = _g16_dataset(option)
    assert ds.edges is not None
    ids = np.arange(len(ds))
    for tag in sorted(k[5:] for k in g if k.startswith("keep/")):
        r = float(tag.split("_")[0][1:])
        hb = DatasetBatch(ds, ids, masking.MaskDraw(r, keep=g["keep/" + tag]))
        assert hb.n_atoms == int(g["kept/" + tag].sum())
        bt = hb.materialize()
        for key, got in (("x", bt.x), ("positions", bt.positions), ("batch", bt.batch),
                         ("rei", bt.radius_edge_index)):
            assert np.array_equal(got.cpu().numpy(), g["%s/%s" % (key, tag)]), (tag, key)
        assert np.array_equal(bt.super_edge_index.cpu().numpy(), g["sei/%s/%s" % (tag, option)]), tag
        assert hb.n_edges == g["rei/" + tag].shape[1]
        x2 = torch.empty_like(bt.x)
        p2 = torch.empty_like(bt.positions)
        mp = torch.from_numpy(np.concatenate([[0], np.cumsum(hb._sizes)]).astype(np.int32)).to(DEV)
        ds.gather_into(hb, x2, p2, mp)
        assert torch.equal(x2, bt.x) and torch.equal(p2, bt.positions)


def _bonded_dataset(M, seed, radius=None):
    from geossl_amd.Geom3D.dataloaders import DeviceDataset
    from geossl_amd.synthetic import add_bonds, make_molecules, molecule_sizes
    sizes = molecule_sizes(M, "C", np.random.default_rng(seed))
    sizes[::97] = 1
    sizes[1::89] = 2
    mols = add_bonds(make_molecules(0, seed=seed, sizes=sizes), seed=seed, cut=0.3)
    return mols, DeviceDataset.from_numpy(mols, DEV, radius=radius)


def _device_keep(ds, hb):
    """The kept lists a masked handle's device draw produces (the count launch's keep_out)."""
    from geossl_amd import _lib
    from geossl_amd._lib import call, ptr, stream
    blob, o = ds.upload_plan(hb, False)
    m, mblob = ds.mask_plan(hb)
    keep = torch.full((hb.n_atoms,), -1, dtype=torch.int32, device=DEV)
    cnt = torch.full((hb.num_graphs,), -1, dtype=torch.int32, device=DEV)
    g = _lib.Gather()
    g.src_off, g.mol_ptr = blob.data_ptr() + 4 * o["src_off"], blob.data_ptr() + 4 * o["mol_ptr"]
    m.keep_out, m.e_count = ptr(keep), ptr(cnt)
    call("geossl_gather_masked_molecules", C.byref(g), C.byref(m), hb.num_graphs, stream())
    out = keep.cpu().numpy()
    assert (cnt.cpu().numpy() == 0).all()
    del mblob
    return out


def _components(n, succ):
    comp = -np.ones(n, dtype=np.int64)
    for s in range(n):
        if comp[s] < 0:
            comp[s], todo = s, [s]
            while todo:
                a = todo.pop()
                for b in succ[a]:
                    if comp[b] < 0:
                        comp[b] = s
                        todo.append(b)
    return comp


def test_device_draw_is_its_cpu_twin_and_a_bfs():
    """Device mode: the kept lists of 1200 molecules equal the CPU twin of the documented Philox BFS bit for bit; they
    are sorted, unique, k(n) long, and BFS-shaped (per bond component: nothing, everything, or a connected part - and
    at most one component partly); the same seed repeats the masks, another epoch's seed changes them."""
    from geossl_amd.Geom3D.dataloaders import DeviceLoader, masking
    from masking_twin import device_bfs
    mols, ds = _bonded_dataset(1200, 5)
    for r in (0.3, 0.5):
        np.random.seed(3)
        hbs = list(DeviceLoader(ds, batch_size=400, shuffle=True, generator=torch.Generator().manual_seed(2),
                                mask_ratio=r))
        seed = hbs[0]._mask.seed
        for hb in hbs:
            keep = _device_keep(ds, hb)
            koff = np.concatenate([[0], np.cumsum(hb._sizes)])
            for j, i in enumerate(hb.ids.tolist()):
                n, k = int(ds.sizes[i]), int(hb._sizes[j])
                got = keep[koff[j]:koff[j + 1]]
                succ = ds.successors(i)
                assert np.array_equal(got, device_bfs(n, succ, k, i, seed)), (r, i)
                assert k == masking.kept_count(n, r) and (np.diff(got) > 0).all() and 0 <= got[0] and got[-1] < n
                comp = _components(n, succ)
                partial = 0
                for c in np.unique(comp):
                    members = set(np.nonzero(comp == c)[0].tolist())
                    kept_c = members & set(got.tolist())
                    if kept_c and kept_c != members:
                        partial += 1
                        seen, todo = {min(kept_c)}, [min(kept_c)]
                        while todo:
                            a = todo.pop()
                            for b in succ[a]:
                                if b in kept_c and b not in seen:
                                    seen.add(b)
                                    todo.append(b)
                        assert seen == kept_c, (r, i)
                assert partial <= 1, (r, i)
        assert np.array_equal(_device_keep(ds, hbs[0]), _device_keep(ds, hbs[0]))
        np.random.seed(4)
        other = next(iter(DeviceLoader(ds, batch_size=400, shuffle=True, generator=torch.Generator().manual_seed(2),
                                       mask_ratio=r)))
        assert other._mask.seed != seed and np.array_equal(other.ids, hbs[0].ids)
        assert not np.array_equal(_device_keep(ds, other), _device_keep(ds, hbs[0]))


def test_masked_gather_refusals():
    from geossl_amd import _lib
    from geossl_amd._lib import call, ptr, stream
    from geossl_amd.Geom3D.dataloaders import DeviceDataset, masking
    from geossl_amd.Geom3D.dataloaders.device_dataset import DatasetBatch
    mols, ds = _bonded_dataset(20, 8)
    hb = DatasetBatch(ds, np.arange(4), masking.MaskDraw(0.3, seed=1))
    blob, o = ds.upload_plan(hb, False)
    x = torch.empty(hb.n_atoms, 2, dtype=torch.int64, device=DEV)
    p = torch.empty(hb.n_atoms, 3, device=DEV)
    for bad in ("max_n", "csr"):
        m, mblob = ds.mask_plan(hb)
        if bad == "max_n":
            m.max_n = 2049
        else:
            m.bond_ptr = None
        g = _lib.Gather()
        g.x_src, g.pos_src, g.x_cols, g.src_off = ptr(ds.x), ptr(ds.positions), 2, blob.data_ptr() + 4 * o["src_off"]
        g.mol_ptr, g.x_dst, g.pos_dst = blob.data_ptr() + 4 * o["mol_ptr"], ptr(x), ptr(p)
        with pytest.raises(Exception):
            call("geossl_gather_masked_molecules", C.byref(g), C.byref(m), hb.num_graphs, stream())
    bi = mols["bond_index"].copy()
    bi[1, 0] = bi[0, 0]
    with pytest.raises(ValueError, match="self-loop"):
        DeviceDataset.from_numpy(dict(mols, bond_index=bi), DEV)


def test_training_on_masked_handles_is_training_on_their_collated_batches():
    """Six DDMTrainer steps on masked SchNet handles from a DeviceLoader (bucket replay, BFS + gather in the fill's one
    launch) over two epochs equal the same trainer on ds.collate() of the same handles, losses and parameters bit for
    bit, with one capture; a masked PaiNN handle trains on its collated tensors with the loss of its collated twin."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.Geom3D.dataloaders import DeviceLoader
    mols, ds = _bonded_dataset(96, 11)
    np.random.seed(21)
    torch.manual_seed(21)
    handles = [hb for _ in range(2) for hb in DeviceLoader(ds, batch_size=32, shuffle=True, drop_last=True,
                                                              mask_ratio=0.3)]
    assert len(handles) == 6 and handles[0]._mask.seed != handles[3]._mask.seed
    out = {}
    for how in ("handle", "collated"):
        tr = pg.DDMTrainer(product_schnet(SMALL, DEV), product_ncsn(128, 50, 2, DEV),
                           product_ncsn(128, 50, 2, DEV, scale=0.9), lr=5e-4, model_3d="schnet", use_graph=True)
        torch.cuda.manual_seed(99)
        losses = [tr.step(hb if how == "handle" else ds.collate(hb)).clone() for hb in handles]
        torch.cuda.synchronize()
        assert tr.step_graphs.captures == 1, how
        out[how] = (torch.stack(losses), tr.flat.flat.detach().clone())
    assert all(h._batch is None for h in handles[1:])
    assert torch.equal(out["handle"][0], out["collated"][0]) and torch.equal(out["handle"][1], out["collated"][1])
    assert torch.isfinite(out["handle"][0]).all()
    # PaiNN: the materialized path
    from geossl_amd.Geom3D.models import PaiNN
    from helpers import fill_module_
    mols, ds = _bonded_dataset(64, 12, radius=5.0)
    np.random.seed(5)
    hb = next(iter(DeviceLoader(ds, batch_size=24, shuffle=True, mask_ratio=0.3)))
    twin = ds.collate(hb)
    losses = []
    for b in (hb, twin):
        model = fill_module_(PaiNN(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1,
                                   readout="add")).to(DEV)
        tr = pg.DDMTrainer(model, product_ncsn(128, 50, 2, DEV), product_ncsn(128, 50, 2, DEV, scale=0.9), lr=5e-4,
                           model_3d="painn", use_graph=True)
        torch.cuda.manual_seed(7)
        losses.append(float(tr.step(b)))
    assert torch.equal(hb.radius_edge_index, twin.radius_edge_index) and hb.n_edges == twin.radius_edge_index.size(1)
    assert np.isfinite(losses[0]) and abs(losses[0] - losses[1]) <= 1e-5 * abs(losses[1]), losses
