"""CPU tests of LEP on the sparse capacity bucket: the C ABI of the three `_dyn` entry points of csrc/pair_head.hip, the
host logic of a pair handle (Geom3D.dataloaders.PairedBatch) on a stub dataset, the host plan of its 2B fused structures,
the objective's routing flag, and the constants the other bucket kinds keep."""
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("geossl_pair_head_fwd_dyn", "geossl_pair_head_predict_dyn", "geossl_pair_head_bwd_dyn")


def test_new_abi_symbols_declared_bound_and_exported():
    from geossl_amd import _lib
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    # the `_dyn` forms take the exact forms' arguments and one device address more, before the stream
    for name in NEW_SYMBOLS:
        exact, dyn = _lib.PROTOTYPES[name[:-4]], _lib.PROTOTYPES[name]
        assert dyn[0] == exact[0] and len(dyn[1]) == len(exact[1]) + 1 and dyn[1][:len(exact[1]) - 1] == exact[1][:-1]
        assert dyn[1][-2] == dyn[1][-1] == exact[1][-1]                  # (a device address, then the stream)


class _StubPairs:
    """What a PairedBatch reads of its dataset on the host: M pairs, the sizes of the 2M structures [active | inactive]."""

    device, x_cols = "nowhere", 1

    def __init__(self, sizes_active, sizes_inactive):
        self.sizes = np.asarray(list(sizes_active) + list(sizes_inactive), dtype=np.int64)
        self._M = len(sizes_active)

    def __len__(self):
        return self._M


def test_pair_handle_host_logic(monkeypatch):
    from geossl_amd import bucket as bk
    from geossl_amd.Geom3D.dataloaders import PairedBatch
    monkeypatch.delenv("GEOSSL_SPARSE_PAIRS", raising=False)
    active, inactive = [10, 11, 12, 13, 14], [20, 21, 22, 300, 24]
    hb = PairedBatch(_StubPairs(active, inactive), [3, 0])
    assert hb.ids.tolist() == [3, 0] and hb.fused_ids.tolist() == [3, 0, 8, 5]
    assert list(hb._sizes) == [13, 10, 300, 20] and hb.num_graphs == 2 and hb.n_atoms == 343
    assert list(hb._sizes_active) == [13, 10] and list(hb._sizes_inactive) == [300, 20]
    assert bk.sparse_eligible(hb)                                        # one structure of 300 atoms
    dense = PairedBatch(_StubPairs(active, [20, 21, 22, 255, 24]), [3, 0])
    assert not bk.sparse_eligible(dense)                                 # all <= 255: today's routing
    assert not bk.sparse_eligible(PairedBatch(_StubPairs(active, [20, 21, 22, 1025, 24]), [3, 0]))
    assert bk.sparse_eligible(PairedBatch(_StubPairs(active, [20, 21, 22, 1024, 24]), [3, 0]))
    monkeypatch.setenv("GEOSSL_SPARSE_PAIRS", "1")
    assert bk.sparse_eligible(dense)
    for bad in ([], [5], [-1]):
        try:
            PairedBatch(_StubPairs(active, inactive), bad)
        except (ValueError, IndexError):
            continue
        raise AssertionError("ids %r accepted" % (bad,))


def test_host_plan_of_the_fused_structures():
    from geossl_amd import bucket as bk
    n = np.array([300, 2, 33, 257])                                      # [active 0, 1 | inactive 0, 1]
    hp = bk.host_plan(n, bk.SPARSE, views=1)
    assert hp["counts"] == (592, 0, 0, 0)
    assert np.array_equal(hp["mol_ptr"], np.concatenate([[0], np.cumsum(n)])) and hp["mol_ptr"].shape == (5,)
    assert bk.batch_counts(n, bk.SPARSE, 1) == (592, 0, 0, 0)


def test_lep_reads_no_pair_tuples():
    from geossl_amd.finetune_lep import LEP
    assert LEP.pair_tuples is False and LEP.views == 1


def test_paired_dataset_checks_before_any_upload():
    """What PairedDeviceDataset checks before anything is uploaded: the reference's position assert, one inactive
    structure and one label per pair."""
    import pytest
    import torch
    from geossl_amd.Geom3D.dataloaders import PairedDeviceDataset
    pos = torch.ones(3, 3)
    bad = pos.clone()
    bad[1] = torch.tensor([1.0, -1.0, 0.0])                              # a row that sums to 0
    x = torch.ones(3, dtype=torch.long)
    with pytest.raises(AssertionError):
        PairedDeviceDataset(x, bad, [3], x, pos, [3], [1], "cuda")
    with pytest.raises(AssertionError):
        PairedDeviceDataset(x, pos, [3], x, bad, [3], [1], "cuda")
    with pytest.raises(ValueError, match="per pair"):
        PairedDeviceDataset(x, pos, [2, 1], x, pos, [3], [1], "cuda")


def test_existing_bucket_constants_stay():
    from geossl_amd import bucket as bk
    assert bk.MAX_N == 255 and bk.MAX_N_CLASSES[-1] == 255 and bk.PAINN_MAX_N_CLASSES[-1] == 255
    assert bk.SPARSE == "sparse" and bk.SPARSE not in ("combination", "permutation", bk.TRIPLES)
    assert bk.SPARSE_MAX_N_CLASSES == (256, 512, 1024)
    assert bk.NOISE_SHAPES["target"] == ("B", (), __import__("torch").float32)
