"""The host half of ``Bucket.fill`` without a device: ``bucket.host_image`` replayed for every case and every fill of
tools/record_bucket_images.py against the blobs recorded on the MI355X (tests/golden/bucket_fill_images.npz) - header
words, pointer arrays, work list, stats, inc_ptr in its int64 view, big-atom lists, dataset / edge / triple offsets -
with the stale words a reused staging slot keeps."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import record_bucket_images as rec  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "bucket_fill_images.npz")


@pytest.fixture(scope="module")
def recorded():
    return rec.load(FIXTURE)


def test_fixture_holds_every_case_and_they_fit(recorded):
    """The fixture was recorded from the case list as it stands; every fill fits the bucket made for the first."""
    arrays, meta = recorded
    assert sorted(meta) == sorted(c["name"] for c in rec.CASES)
    for case in rec.CASES:
        m = meta[case["name"]]
        want = rec.ctor_args(case, m["fills"][0]["E"], m["fills"][0]["T"] or 0)
        assert m["ctor"] == want and len(m["fills"]) == 4
        for k in range(4):
            assert np.array_equal(arrays["%s/%d/sizes" % (case["name"], k)], rec.batch_sizes(case, k))
    assert rec.check()


@pytest.mark.parametrize("case", rec.CASES, ids=lambda c: c["name"])
def test_host_image_is_the_recorded_blob(recorded, case):
    from geossl_amd import bucket as bk
    arrays, meta = recorded
    m, name = meta[case["name"]], case["name"]
    a = m["ctor"]
    lay = bk.BlobLayout(a["B"], a["caps"], a["option"], a["kind"], a["views"], a["max_n"], a["n_rbf"])
    assert lay.off == m["off"] and lay.words == m["words"] and list(lay.big_caps) == m["big_caps"]
    ring = [np.zeros(lay.words, dtype=np.int32) for _ in range(3)]   # the bucket's three staging slots, rotated as it does
    for k, f in enumerate(m["fills"]):
        got = lambda key: arrays.get("%s/%d/%s" % (name, k, key))
        h = ring[k % 3]
        src = tuple(got(key) for key in ("src_off", "edge_off", "edge_cnt", "triple_off", "triple_cnt"))
        bk.host_image(h, lay, got("sizes"), f["counts"] if k % 2 == 0 else None, src if m["handle"] else None,
                      E=f["E"], T=f["T"], masked_edges=f["masked_edges"])
        blob = got("blob")
        same = h == blob
        if f["masked_edges"]:   # (written by geossl_masked_edge_offsets on the device)
            same[lay.off["e_ptr"]:lay.off["e_ptr"] + a["B"] + 1] = True
            same[bk.D_E2] = True
        assert same.all(), "fill %d: words %s" % (k, np.nonzero(~same)[0][:16].tolist())
