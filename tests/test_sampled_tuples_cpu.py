"""Sampled atom tuples (``AtomTupleExtractor(ratio < 1)`` / ``DeviceLoader(tuple_ratio=)``) without a device: the host
half of a sampled capacity bucket against brute force, the Python twin of the device draw, the numpy-mode handles' host
lists against the host extractor under one ``np.random.seed``, the marks, the routing switch and the refusals."""
import types

import numpy as np
import pytest
import torch

import sampled_tuples_twin as tw

SIZES = [5, 1, 2, 3, 4, 33, 34, 70, 3]


class _FakeDataset:
    """What DeviceLoader / DatasetBatch read of a DeviceDataset on the host (no device memory is touched before a handle
    is materialised)."""

    triples = force = edges = bonds = None

    def __init__(self, sizes, option="combination", bonds=False):
        self.sizes, self.option = np.asarray(sizes, dtype=np.int64), option
        self.pairs = self.sizes * (self.sizes - 1) // 2
        self.device, self.x_cols = torch.device("cpu"), 2
        self.off = np.concatenate([[0], np.cumsum(self.sizes)])
        if bonds:   # a chain: atom a bonded to a + 1, both directions
            self.bonds = True
            self._succ = [[[v for v in (a - 1, a + 1) if 0 <= v < n] for a in range(n)] for n in sizes]

    def __len__(self):
        return len(self.sizes)

    def successors(self, i):
        return self._succ[i]

    def batch(self, ids):
        from geossl_amd.Geom3D.dataloaders.device_dataset import DatasetBatch
        return DatasetBatch(self, ids)

    def check_masking(self, ratio):
        pass


def _loader(ds, **kw):
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceLoader
    return DeviceLoader(ds, batch_size=len(ds), shuffle=False, **kw)


@pytest.mark.parametrize("option,ratio,kept,S,divisor", [
    ("combination", 0.3, [3, 0, 0, 0, 1, 158, 168, 724, 0], 1054, 8),
    ("permutation", 0.5, [10, 0, 1, 3, 6, 528, 561, 2415, 3], 3527, 9)])
def test_host_plan_and_image_of_a_sampled_option(option, ratio, kept, S, divisor):
    """S = sum k_m with k_m = int(M_m * ratio) counted by brute force, se_ptr their running sum, the divisor the last
    molecule that keeps a tuple + 1 (the last molecule of the 0.3 case keeps none: 8, not 9), no host inc_ptr; the blob
    carries them and the molecules' dataset ids."""
    from geossl_amd import bucket as bk
    opt = (option, ratio)
    assert tw.brute_counts(SIZES, option, ratio) == kept and sum(kept) == S
    hp = bk.host_plan(SIZES, opt, views=1)
    n = np.asarray(SIZES)
    assert hp["counts"][0] == n.sum() and hp["counts"][1] == (n * (n - 1) // 2).sum() and hp["counts"][2] == S
    assert hp["kept"].tolist() == kept and hp["divisor"] == divisor and "inc_ptr" not in hp
    assert hp["se_ptr"].tolist() == np.concatenate([[0], np.cumsum(kept)]).tolist()
    assert bk.batch_counts(SIZES, opt, 1) == hp["counts"] and bk.batch_counts(SIZES, opt, 2)[2] == S
    # the full enumeration is untouched by the new option
    full = bk.host_plan(SIZES, option, views=1)
    assert full["counts"][2] == sum(len(tw.enumeration(v, option)) for v in SIZES) and "inc_ptr" in full
    for kind in ("schnet", "painn"):
        B = len(SIZES)
        caps = bk.capacities(*hp["counts"], B=B, sizes=n)
        assert caps[2] >= S
        lay = bk.BlobLayout(B, caps, opt, kind, 1, 128)
        names = [type(p).__name__ for p in lay.parts]
        assert "_SampledTuples" in names and "_Tuples" not in names
        h = np.full(lay.words, -7, dtype=np.int32)
        ids = np.arange(B, dtype=np.int64)[::-1] + (2 ** 32 + 5)      # (the low word is what the draw counts with)
        src = (np.arange(B) * 100, np.zeros(B, np.int64), np.zeros(B, np.int64), None, None, ids)
        bk.host_image(h, lay, n, src=src)
        o = lay.off
        assert h[bk.D_S] == S and h[bk.D_N] == n.sum()
        assert h[o["se_ptr"]:o["se_ptr"] + B + 1].tolist() == hp["se_ptr"].tolist()
        assert h[o["stats"]:o["stats"] + 2].view(np.int64)[0] == divisor
        assert h[o["mol_id"]:o["mol_id"] + B].tolist() == (np.arange(B)[::-1] + 5).tolist()
        # the host writes no incidence pointer: the section is the device's
        assert (h[o["inc_ptr"]:o["inc_ptr"] + 2 * (caps[0] + 1)] == -7).all()
    # the unsampled layouts keep their sections where they were
    a, b = bk.BlobLayout(9, caps, option, "schnet", 1, 128), bk.BlobLayout(9, caps, opt, "schnet", 1, 128)
    assert all(a.off[k_] == b.off[k_] for k_ in a.off if k_ != "mol_id") and a.words + 9 == b.words


def test_kept_count_is_pythons_int_of_the_product():
    from geossl_amd.batch import kept_tuples, sampled_count
    assert sampled_count(100, 0.29) == 28 == int(100 * 0.29)          # (not 29: 100 * 0.29 is 28.999999999999996)
    for ratio in (0.29, 0.3, 0.1, 0.5, 0.7, 0.999):
        for option in ("combination", "permutation"):
            sizes = np.arange(0, 256)
            want = [int(len(range(n * (n - 1) // (2 if option == "combination" else 1))) * ratio) if n > 1 else 0
                    for n in sizes]
            assert kept_tuples(sizes, option, ratio).tolist() == want


def test_twin_draw_rule():
    """The twin on masking_twin.philox4x32_10: k slots, ascending, a function of (molecule id, seed) and not of the
    batch; ties go to the smaller slot."""
    from masking_twin import philox4x32_10
    seed = 0x1234567890ABCDEF
    w = philox4x32_10((3, 7, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    assert tw.slot_key(3, 7, seed) == (w[0] << 32) | w[1]
    got = tw.kept_slots(45, 13, 7, seed)
    assert len(got) == 13 and got == sorted(set(got)) and max(got) < 45
    keys = sorted((tw.slot_key(s, 7, seed), s) for s in range(45))
    assert got == sorted(s for _, s in keys[:13])
    assert tw.kept_slots(45, 13, 8, seed) != got and tw.kept_slots(45, 13, 7, seed + 1) != got
    sei = tw.device_tuples([5, 1, 4], [11, 12, 13], "permutation", 0.5, seed)
    assert sei.shape == (2, 10 + 0 + 6) and (sei[0] != sei[1]).all()
    assert (sei[:, :10] < 5).all() and (sei[:, 10:] >= 6).all()
    alone = tw.device_tuples([4], [13], "permutation", 0.5, seed)
    assert np.array_equal(alone + 6, sei[:, 10:])
    ptr, idx = tw.incidence(10, sei)
    assert ptr[-1] == 2 * sei.shape[1] and ptr[5] == ptr[6] == 20        # (the one-atom molecule lies on no tuple)


@pytest.mark.parametrize("mask", [False, True])
def test_numpy_mode_handles_hold_the_host_extractors_tuples(mask):
    """tuple_rng="numpy": the handle's host list is the collated super_edge_index of AtomTupleExtractor(ratio) over the
    same molecules under the same np.random.seed; with numpy masking the draws interleave per molecule, mask first."""
    from geossl_amd.Geom3D.dataloaders import masking
    from geossl_amd.Geom3D.dataloaders.dataloaders_AtomTuple import AtomTupleExtractor, BatchAtomTuple, Data
    sizes, option, ratio, mr = [5, 1, 2, 7, 12, 3], "permutation", 0.3, 0.25
    ds = _FakeDataset(sizes, option, bonds=mask)
    np.random.seed(5)
    kw = dict(mask_ratio=mr, mask_rng="numpy") if mask else {}
    (hb,) = list(_loader(ds, tuple_ratio=ratio, tuple_rng="numpy", **kw))
    np.random.seed(5)
    ext, mols, keeps = AtomTupleExtractor(ratio, option), [], []
    for i, n in enumerate(sizes):
        if mask:
            keeps.append(masking.reference_bfs(n, ds.successors(i), mr))
            n = len(keeps[-1])
        mols.append(ext(Data(x=torch.zeros(n, 2, dtype=torch.long), positions=torch.zeros(n, 3))))
    co = BatchAtomTuple.from_data_list(mols)
    assert np.array_equal(hb._tuple_draw.tuples, co.super_edge_index.numpy())
    assert hb.n_super == co.super_edge_index.size(1) and hb.tuple_counts.tolist() == [m.super_edge_index.size(1) for m in mols]
    assert list(hb._sizes) == co._sizes
    if mask:
        assert np.array_equal(hb._mask.keep, np.concatenate(keeps))
    # the marks: the same on both, distinct from _canonical (None on both), and no key of the collated batch
    assert hb._sampled == co._sampled == (option, ratio) and hb._canonical is None and co._canonical is None
    assert not any(k.startswith("_") for k in co.keys) and "super_edge_index" in co.keys
    from geossl_amd import bucket as bk
    assert bk.option_of(hb) == bk.option_of(co) == (option, ratio)


def test_marks_of_the_host_extractor():
    from geossl_amd.Geom3D.dataloaders.dataloaders_AtomTuple import AtomTupleExtractor, BatchAtomTuple, Data
    mol = lambda n: Data(x=torch.zeros(n, 2, dtype=torch.long), positions=torch.zeros(n, 3))
    full = BatchAtomTuple.from_data_list([AtomTupleExtractor(1, "combination")(mol(n)) for n in (4, 6)])
    assert full._canonical == "combination" and full._sampled is None
    np.random.seed(0)
    a, b = AtomTupleExtractor(0.5, "combination")(mol(4)), AtomTupleExtractor(0.25, "combination")(mol(6))
    mixed = BatchAtomTuple.from_data_list([a, b])
    assert mixed._canonical is None and mixed._sampled is None          # (two ratios: nobody's counts)
    plain = BatchAtomTuple.from_data_list([mol(4), AtomTupleExtractor(0.5, "combination")(mol(6))])
    assert plain._sampled is None


def test_device_mode_draws_one_more_seed_only_when_sampling():
    """An unsampled loader consumes the numpy stream exactly as before; a sampled one draws its seed after the mask's."""
    ds = _FakeDataset([4, 6, 5], bonds=True)
    np.random.seed(3)
    list(_loader(ds, mask_ratio=0.25))
    after_mask = np.random.randint(1 << 30)
    np.random.seed(3)
    (hb,) = list(_loader(ds, mask_ratio=0.25, tuple_ratio=0.5))
    after_both = np.random.randint(1 << 30)
    np.random.seed(3)
    mask_seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
    tuple_seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
    assert hb._mask.seed == mask_seed and hb._tuple_draw.seed == tuple_seed and after_both != after_mask
    assert np.random.randint(1 << 30) == after_both
    np.random.seed(3)
    (h0,) = list(_loader(ds))
    assert np.random.randint(1 << 30) == np.random.RandomState(3).randint(1 << 30)   # (nothing drawn)
    assert h0._sampled is None and h0._canonical == "combination"
    # kept counts of a masked sampled handle come from the KEPT sizes
    from geossl_amd.batch import kept_tuples
    assert hb.tuple_counts.tolist() == kept_tuples(hb._sizes, "combination", 0.5).tolist()
    assert hb.fingerprint()[0] == "sampled"


def test_sampled_handles_never_share_a_fingerprint():
    """Only the same draw shares index tensors: every sampled handle has a fingerprint of its own, also when the
    handles before it are gone and the interpreter reuses their addresses."""
    ds = _FakeDataset(list(range(4, 44)))
    from geossl_amd.Geom3D.dataloaders.device_dataset import DeviceLoader
    loader = DeviceLoader(ds, batch_size=4, shuffle=True, tuple_ratio=0.3)
    prints = [hb.fingerprint() for hb in loader]          # (each handle is freed before the next is made)
    assert len(prints) == 10 and len(set(prints)) == 10 and all(fp[0] == "sampled" for fp in prints)
    (hb,) = list(_loader(ds, tuple_ratio=0.3))
    assert hb.fingerprint() == hb.fingerprint() and hb.fingerprint() not in prints


def test_refusals():
    from geossl_amd.Geom3D.dataloaders import device_dataset as dd
    ds = _FakeDataset([4, 6, 5])
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="tuple_ratio"):
            _loader(ds, tuple_ratio=bad)
    with pytest.raises(ValueError, match="tuple_rng"):
        _loader(ds, tuple_ratio=0.5, tuple_rng="torch")
    tri = _FakeDataset([4, 6, 5])
    tri.triples = object()
    with pytest.raises(ValueError, match="triple dataset"):
        _loader(tri, tuple_ratio=0.5)
    paired = dd.PairedDeviceDataset.__new__(dd.PairedDeviceDataset)
    paired._M, paired.sizes = 2, np.asarray([4, 6, 5, 7])
    with pytest.raises(ValueError, match="paired dataset"):
        dd.DeviceLoader(paired, batch_size=2, tuple_ratio=0.5)
    with pytest.raises(ValueError, match="sparse bucket"):
        _loader(_FakeDataset([4, 256]), tuple_ratio=0.5)
    _loader(_FakeDataset([4, 256]))                                       # (unsampled: as before)


def test_routing_and_the_switch(monkeypatch):
    """Handles take the sampled bucket by default, collated batches by the recorded default; GEOSSL_SAMPLED_BUCKETS=1 /
    =0 force both ways; an unmarked batch stays ineligible."""
    from geossl_amd import bucket as bk, switches

    def fake(dtype, *shape):
        n = int(np.prod(shape))
        return types.SimpleNamespace(is_cuda=True, dtype=dtype, dim=lambda: len(shape), size=lambda i: shape[i],
                                     numel=lambda: n, is_contiguous=lambda: True, stride=lambda i: 1, _version=0)

    sizes, opt = [18, 20, 2], ("combination", 0.3)
    N, S = sum(sizes), bk.batch_counts(sizes, opt, 1)[2]

    def collated(mark, S_=S):
        return types.SimpleNamespace(_sizes=sizes, _canonical=None, _sampled=mark, positions=fake(torch.float32, N, 3),
                                     x=fake(torch.long, N, 2), batch=fake(torch.long, N),
                                     super_edge_index=fake(torch.long, 2, S_))

    (hb,) = list(_loader(_FakeDataset(sizes), tuple_ratio=0.3))
    monkeypatch.delenv("GEOSSL_SAMPLED_BUCKETS", raising=False)
    assert bk.route(hb, "schnet", 1, True, False) == opt
    assert (bk.route(collated(opt), "schnet", 1, True, False) == opt) == switches.SAMPLED_BUCKETS_COLLATED_DEFAULT
    monkeypatch.setenv("GEOSSL_SAMPLED_BUCKETS", "1")
    assert bk.route(collated(opt), "schnet", 2, True, False) == opt
    assert bk.route(collated(opt, S - 1), "schnet", 1, True, False) is None      # not int(M * ratio) columns per molecule
    assert bk.route(collated(None), "schnet", 1, True, False) is None            # no mark: nobody vouches for the counts
    assert bk.route(collated(opt), "schnet", 2, True, True) is None              # normalize under DDM: out of scope
    (same,) = list(_loader(_FakeDataset([18] * 3), tuple_ratio=0.3))
    assert bk.route(same, "schnet", 1, True, False) == opt                       # equal sizes do not share sampled tuples
    monkeypatch.setenv("GEOSSL_SAMPLED_BUCKETS", "0")
    assert bk.route(hb, "schnet", 1, True, False) is None and bk.route(collated(opt), "schnet", 1, True, False) is None
    # the bucket key carries option and ratio
    from geossl_amd.replay import StepGraphs
    monkeypatch.delenv("GEOSSL_SAMPLED_BUCKETS")
    sg = StepGraphs(lambda b, n: None, "schnet", modules=(None, None, None), views=1)
    sg._mod_ok = (tuple(switches.env(k_) for k_ in bk.MODULE_SWITCHES + bk.PAINN_SWITCHES), True)
    assert sg.bucket_key(hb) == ("bucket", 3, ("combination", 0.3))
