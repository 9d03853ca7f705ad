"""Host side of masked PaiNN handles on capacity buckets (no GPU): the upper bound on the surviving radius edges that
sizes the bucket, the routing decision and its switch."""
import types

import numpy as np
import torch

from conftest import load_golden


def _stub(sizes, edge_cnt=None, option="combination"):
    """The host side of a DeviceDataset (what DatasetBatch / bucket.eligible read) without device arrays; edge_cnt: the
    radius edges per molecule of a dataset built with radius=..., None: a dataset without them."""
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceDataset
    sizes = np.asarray(sizes, dtype=np.int64)
    with_edges = edge_cnt is not None
    ns = types.SimpleNamespace(sizes=sizes, off=np.concatenate([[0], np.cumsum(sizes)]), pairs=sizes * (sizes - 1) // 2,
                               option=option, x_cols=2, device=torch.device("cpu"),
                               edges=object() if with_edges else None,
                               edge_cnt=np.asarray(edge_cnt, dtype=np.int64) if with_edges else None,
                               bonds=np.zeros((2, 0), np.int64))
    return type("Stub", (), dict(vars(ns), __len__=lambda self: len(sizes), check_masking=DeviceDataset.check_masking))()


def _survivors(g, tag):
    """"Both ends kept" (datasets_3D_Radius.py:43-87) restated in numpy on the whole molecules' radius edges of G16 and
    the reference's kept lists -> surviving edges per molecule."""
    sizes, kept = g["sizes"], g["kept/" + tag]
    koff = np.concatenate([[0], np.cumsum(kept)])
    eoff = np.concatenate([[0], np.cumsum(g["rei_cnt"])])
    out = []
    for m in range(len(sizes)):
        keep = np.zeros(int(sizes[m]), dtype=bool)
        keep[g["keep/" + tag][koff[m]:koff[m + 1]]] = True
        e = g["rei_src"][:, eoff[m]:eoff[m + 1]]
        out.append(int((keep[e[0]] & keep[e[1]]).sum()))
    return np.asarray(out, dtype=np.int64)


def test_edge_bound_of_a_masked_handle_covers_the_reference_survivors():
    """n_edges_bound = sum over molecules of min(edges, k (k - 1)) is at least the number of radius edges whose two ends
    the reference's own masks keep (fixture G16, every ratio and seed), molecule subsets included; it never exceeds the
    unmasked count; n_edges stays None on a masked handle."""
    from geossl_amd.Geom3D.dataloaders import masking
    from geossl_amd.Geom3D.dataloaders.device_dataset import DatasetBatch
    g = load_golden("g16_masking")
    ds = _stub(g["sizes"], g["rei_cnt"])
    tags = sorted(k[5:] for k in g if k.startswith("keep/"))
    assert len(tags) >= 4
    for tag in tags:
        r = float(tag.split("_")[0][1:])
        surv = _survivors(g, tag)
        assert surv.sum() == g["rei/" + tag].shape[1]           # (the restatement is the reference's count)
        k = masking.kept_count(g["sizes"], r)
        assert np.array_equal(k, g["kept/" + tag])
        koff = np.concatenate([[0], np.cumsum(k)])
        for ids in (np.arange(len(g["sizes"])), np.array([0, 3, 5]), np.array([11, 2, 39, 7]), np.array([3])):
            keep = np.concatenate([g["keep/" + tag][koff[i]:koff[i + 1]] for i in ids])
            hb = DatasetBatch(ds, ids, masking.MaskDraw(r, keep=keep))
            assert hb.n_edges is None
            want = int(np.minimum(g["rei_cnt"][ids], k[ids] * (k[ids] - 1)).sum())
            assert hb.n_edges_bound == want
            assert int(surv[ids].sum()) <= hb.n_edges_bound <= int(g["rei_cnt"][ids].sum())
        # a one-atom molecule keeps its atom and no edge
        assert DatasetBatch(ds, np.array([0]), masking.MaskDraw(r, seed=1)).n_edges_bound == 0
    plain = DatasetBatch(ds, np.array([4, 9]))
    assert plain.n_edges == plain.n_edges_bound == int(g["rei_cnt"][[4, 9]].sum())


def test_masked_painn_handle_is_eligible_with_edges_and_the_switch_turns_it_off(monkeypatch):
    from geossl_amd import bucket as bk
    from geossl_amd.Geom3D.dataloaders import masking
    from geossl_amd.Geom3D.dataloaders.device_dataset import DatasetBatch
    sizes = np.array([4, 18, 1, 30, 7], dtype=np.int64)
    with_e, without = _stub(sizes, sizes * (sizes - 1)), _stub(sizes)
    ids = np.array([1, 2, 3])
    monkeypatch.delenv("GEOSSL_MASKED_PAINN_BUCKETS", raising=False)
    hb = DatasetBatch(with_e, ids, masking.MaskDraw(0.3, seed=5))
    assert hb.n_edges is None and hb.n_edges_bound is not None
    assert bk.eligible(hb, "painn") and bk.eligible(hb, "schnet")
    assert bk.handle_edges(hb) == hb.n_edges_bound
    bare = DatasetBatch(without, ids, masking.MaskDraw(0.3, seed=5))   # the stub without edges still constructs
    assert bare.n_edges is None and bare.n_edges_bound is None
    assert not bk.eligible(bare, "painn") and bk.eligible(bare, "schnet")
    assert not bk.eligible(DatasetBatch(without, ids), "painn") and bk.eligible(DatasetBatch(with_e, ids), "painn")
    for value, on in (("0", False), ("1", True)):
        monkeypatch.setenv("GEOSSL_MASKED_PAINN_BUCKETS", value)
        assert bk.eligible(hb, "painn") is on
        assert bk.eligible(hb, "schnet") and bk.eligible(DatasetBatch(with_e, ids), "painn")   # (nothing else moves)


def test_step_graphs_size_a_masked_painn_bucket_by_the_bound():
    """bucket.batch_edges - what StepGraphs sizes a bucket by and Bucket.fits_batch checks - hands the bound to
    edge_capacity / Bucket.fits for a masked handle and the count otherwise."""
    from geossl_amd import bucket as bk
    from geossl_amd.Geom3D.dataloaders import masking
    from geossl_amd.Geom3D.dataloaders.device_dataset import DatasetBatch
    sizes = np.array([4, 18, 1, 30, 7], dtype=np.int64)
    ds = _stub(sizes, sizes * (sizes - 1))
    hb = DatasetBatch(ds, np.array([1, 3, 4]), masking.MaskDraw(0.5, seed=2))
    k = masking.kept_count(sizes[[1, 3, 4]], 0.5)
    assert bk.batch_edges(hb, "painn") == int((k * (k - 1)).sum()) == hb.n_edges_bound
    assert bk.batch_edges(DatasetBatch(ds, np.array([1, 3, 4])), "painn") == int((sizes * (sizes - 1))[[1, 3, 4]].sum())
    assert bk.batch_edges(hb, "schnet") is None
