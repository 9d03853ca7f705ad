"""GPU: the cases of tools/record_bucket_images.py recorded on the tree under test against the fixture recorded before
the bucket became a list of parts (tests/golden/bucket_fill_images.npz) - the blob word for word, every other tensor
the bucket owns and the cleared buffer by digest, after each of four fills - and the launches of every fill by name."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import record_bucket_images as rec  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(HERE, "golden", "bucket_fill_images.npz")


@pytest.fixture(scope="module")
def recorded():
    return rec.load(FIXTURE)


def launches_of(case, T):
    """The entry points one fill passes to `call`, in order: one gather (a masked handle: the masked gather; a masked
    PaiNN handle: count pass, edge offsets, gather), a handle's triples, PaiNN's edge layout.  (A collated triple batch's
    two `copy_` are not launches of the library.)"""
    painn = case["kind"] == "painn"
    if case["masked"]:
        seq = ["geossl_gather_masked_molecules"]
        if painn:
            seq += ["geossl_masked_edge_offsets", "geossl_gather_masked_molecules"]
    else:
        seq = ["geossl_gather_molecules"]
    if case["option"] == "triples" and case["source"] == "handle" and T:
        seq.append("geossl_gather_triples")
    if painn:
        seq.append("geossl_painn_edge_layout_dyn" if case["masked"] else "geossl_painn_edge_layout")
    return seq


@pytest.mark.parametrize("case", rec.CASES, ids=lambda c: c["name"])
def test_fills_match_the_recording_and_launch_what_they_did(recorded, case, monkeypatch):
    from geossl_amd import _lib, bucket as bk
    names, real_call = [], _lib.call

    def counted(name, *args):
        names.append(name)
        return real_call(name, *args)
    # (`_lib.call` wrapped under the name `Bucket.fill` and its parts launch through: what builds the datasets and the
    # collated twins of the handles is not counted)
    monkeypatch.setattr(bk, "call", counted)
    arrays, meta = rec.record_case(case, DEV)
    want_arrays, want_meta = recorded
    name = case["name"]
    d = rec.diff((arrays, {name: meta}), ({k: v for k, v in want_arrays.items() if k.startswith(name + "/")},
                                          {name: want_meta[name]}))
    assert not d, "\n".join(d)
    assert names == [n_ for f in meta["fills"] for n_ in launches_of(case, f["T"])]
