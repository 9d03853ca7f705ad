"""The numpy twin of the incidence-list entry (tests/painn_inc_twin.py: a stable sort by key within each structure, how
csrc/painn_inc.hip is built) against the plain-Python restatement of layout.EdgeLayout's definition.  No GPU: what the
GPU test compares the kernel with is checked here first."""
import numpy as np
import pytest

import painn_inc_twin as tw

SIZES_A = (300, 2, 64, 1)


def random_edges(sizes, per_atom, seed, empty=()):
    """[2, E] int64: per structure about per_atom * n edges with both ends drawn inside it (duplicates and self edges
    included: the layout does not care), neither row sorted; structures in `empty` get none."""
    rng = np.random.default_rng(seed)
    cols, a0 = [], 0
    for m, n in enumerate(sizes):
        if m not in empty:
            k = min(per_atom * n, 33 * n)
            cols.append(a0 + rng.integers(0, n, size=(2, k)))
        a0 += n
    return np.concatenate(cols, axis=1).astype(np.int64) if cols else np.zeros((2, 0), np.int64)


def check(ei, sizes, want_status):
    lists, status = tw.edge_layout_definition(ei, sizes)
    iptr_i, ilist_i, iptr_j, ilist_j, st = tw.layout_twin(ei, sizes)
    assert status == st == want_status
    N = sum(sizes)
    for side, iptr, ilist in (("i", iptr_i, ilist_i), ("j", iptr_j, ilist_j)):
        assert iptr.shape == (N + 1,) and iptr[-1] == ei.shape[1] and np.all(np.diff(iptr) >= 0)
        kept = [len(r) for r in lists[side]]
        assert tw.lists_of(iptr, ilist, sizes, kept) == lists[side]
        if not want_status:   # nothing left out: the lists are EdgeLayout's arrays themselves
            assert np.array_equal(iptr, np.concatenate([[0], np.cumsum(kept)]))
            assert np.array_equal(ilist, np.concatenate([np.asarray(r, np.int32) for r in lists[side]]))


def test_twin_is_the_definition_on_the_size_set():
    check(random_edges(SIZES_A, 12, 1), SIZES_A, 0)


def test_a_structure_without_edges():
    ei = random_edges(SIZES_A, 12, 2, empty=(1,))
    check(ei, SIZES_A, 0)
    check(random_edges(SIZES_A, 12, 3, empty=(0, 3)), SIZES_A, 0)
    check(np.zeros((2, 0), np.int64), SIZES_A, 0)


def test_an_edge_that_leaves_its_structure_is_dropped_and_reported():
    ei = random_edges(SIZES_A, 12, 4)
    e = 1000                                  # an edge of structure 0 ...
    assert ei[0, e] < 300
    ei[1, e] = 301                            # ... whose other end is in structure 1
    lists, status = tw.edge_layout_definition(ei, SIZES_A)
    assert status == 1 and all(e not in r for side in "ij" for r in lists[side])
    check(ei, SIZES_A, 1)


def test_structures_in_the_wrong_order_are_reported():
    ei = random_edges(SIZES_A, 12, 5)
    first = int(np.sum(ei[0] < 300))
    swapped = np.concatenate([ei[:, first:], ei[:, :first]], axis=1)
    assert tw.layout_twin(swapped, SIZES_A)[4] == 1


def test_capacity_form():
    ei = random_edges(SIZES_A, 12, 6)
    E, N = ei.shape[1], sum(SIZES_A)
    padded = np.concatenate([ei, np.full((2, 50), 7, np.int64)], axis=1)
    exact, cap = tw.layout_twin(ei, SIZES_A), tw.layout_twin(padded, SIZES_A, E=E, N_cap=N + 30)
    for k in (0, 2):
        assert np.array_equal(cap[k][:N + 1], exact[k]) and np.all(cap[k][N:] == E)
        assert np.array_equal(cap[k + 1], exact[k + 1])


# ---------------------------------------------------------------------------- the host plan of the sparse PaiNN bucket
def _handle(sizes, n_edges=1000, mask=None):
    """What bucket.route reads of a DeviceLoader handle, without a device."""
    import types
    return types.SimpleNamespace(_sizes=np.asarray(sizes, dtype=np.int64), _dataset=object(), _mask=mask, _triples=False,
                                 _canonical="combination", n_edges=n_edges, n_edges_bound=n_edges)


def test_host_plan_of_the_sparse_painn_bucket():
    from geossl_amd import bucket as bk
    sizes = np.asarray(SIZES_A, dtype=np.int64)
    B, N, E = len(sizes), int(sizes.sum()), 4321
    caps = bk.sparse_capacities(N, B, sizes=sizes)
    E_cap = bk.edge_capacity(E, B, sizes=sizes)
    assert caps[0] >= N and caps[0] % 32 == 0 and E_cap >= E + 64 and E_cap % 64 == 0
    assert bk.edge_capacity(E, B, prev=E_cap, sizes=sizes) >= E_cap          # (nothing shrinks)
    lay = bk.BlobLayout(B, caps, bk.SPARSE, kind="painn", views=1, max_n=512)
    assert [type(p).__name__ for p in lay.parts] == ["_Atoms", "_SparseEdgesPart"] and lay.big_caps == ()
    o = lay.off
    # one running sum: dims, mol_ptr / pair_ptr (2B + 1 each), se_ptr, no work list, stats on an even word, no inc_ptr,
    # no big lists, then src_off, e_src_off, e_ptr
    assert o["dims"] == 0 and o["mol_ptr"] == bk.DIMS_WORDS and o["pair_ptr"] == o["mol_ptr"] + 2 * B + 1
    assert o["stats"] % 2 == 0 and o["inc_ptr"] == o["stats"] + 4 == o["big0"] == o["big1"] == o["src_off"]
    assert o["e_src_off"] == o["src_off"] + B and o["e_ptr"] == o["e_src_off"] + B
    assert lay.words == o["e_ptr"] + B + 1 == o["t_src_off"] == o["t_ptr"]
    # SchNet's sparse bucket has no edge sections; the dense PaiNN bucket keeps its part
    assert [type(p).__name__ for p in bk.BlobLayout(B, caps, bk.SPARSE, views=1).parts] == ["_Atoms"]
    # the host image of a handle: counts, mol_ptr, where the structures and their edges start in the dataset
    h = np.full(lay.words, -9, dtype=np.int32)
    src_off, e_off = np.asarray([700, 0, 302, 366]), np.asarray([9000, 0, 4000, 4400])
    e_cnt = np.asarray([4000, 2, 319, 0])
    bk.host_image(h, lay, sizes, src=(src_off, e_off, e_cnt, None, None), E=E)
    assert list(h[0:8]) == [N, N, 0, 0, 0, B, 3 * N, E]
    assert list(h[o["mol_ptr"]:o["mol_ptr"] + B + 1]) == [0, 300, 302, 366, 367]
    assert list(h[o["src_off"]:o["src_off"] + B]) == list(src_off)
    assert list(h[o["e_src_off"]:o["e_src_off"] + B]) == list(e_off)
    assert list(h[o["e_ptr"]:o["e_ptr"] + B + 1]) == [0, 4000, 4002, 4321, 4321]
    # a collated batch: the edge sections are the device's (left as they are)
    h2 = np.full(lay.words, -9, dtype=np.int32)
    bk.host_image(h2, lay, sizes, E=E)
    assert h2[bk.D_E2] == E and np.all(h2[o["e_src_off"]:] == -9)


def test_fits_checks_the_edges():
    import types
    from geossl_amd import bucket as bk
    b = types.SimpleNamespace(caps=lambda: (1024, 33 * 1024, 0, 0), max_n=512, kind="painn", E_cap=5000, option=bk.SPARSE,
                              T_cap=0)
    fits = lambda counts, hi, E: bk.Bucket.fits(b, counts, hi, E)
    assert fits((1000, 0, 0, 0), 400, 5000)
    assert not fits((1000, 0, 0, 0), 400, 5001)         # the edges outgrow it
    assert not fits((1025, 0, 0, 0), 400, 10)           # the atoms
    assert not fits((1000, 0, 0, 0), 513, 10)           # the largest structure
    b.kind = "schnet"
    assert fits((1000, 0, 0, 0), 400, 5001)             # (SchNet's sparse bucket has no edge capacity)


def test_eligibility_and_the_three_switch_values(monkeypatch):
    from geossl_amd import bucket as bk
    from geossl_amd import switches
    for k in ("GEOSSL_PAINN_SPARSE_BUCKETS", "GEOSSL_SPARSE_BUCKETS", "GEOSSL_SPARSE_PAIRS", "GEOSSL_PAINN_TILE",
              "GEOSSL_PAINN_VECTOR"):
        monkeypatch.delenv(k, raising=False)
    hb = _handle(SIZES_A)
    route = lambda b, kind="painn", views=1, pair_tuples=False: bk.route(b, kind, views, pair_tuples, False)
    # unset: handles by the measurement's outcome
    assert switches.painn_sparse_buckets(False) is False
    assert switches.painn_sparse_buckets(True) is switches.PAINN_SPARSE_BUCKETS_DEFAULT
    assert route(hb) == (bk.SPARSE if switches.PAINN_SPARSE_BUCKETS_DEFAULT else None)
    monkeypatch.setenv("GEOSSL_SPARSE_BUCKETS", "1")     # SchNet's switch alone leaves PaiNN out ...
    monkeypatch.setenv("GEOSSL_PAINN_SPARSE_BUCKETS", "0")
    assert route(hb) is None and route(hb, "schnet") == bk.SPARSE
    monkeypatch.setenv("GEOSSL_SPARSE_BUCKETS", "0")     # ... and PaiNN's switch leaves SchNet's bucket alone
    monkeypatch.setenv("GEOSSL_PAINN_SPARSE_BUCKETS", "1")
    assert route(hb) == bk.SPARSE and route(hb, "schnet") is None
    assert switches.painn_sparse_buckets(False) and switches.painn_sparse_buckets(True)
    # what is not eligible: a step that reads pair tuples or has two views, no radius edges, a masked handle, a
    # structure above 1024 atoms, an empty structure, a dense layout, no atom-tile route
    assert route(hb, pair_tuples=True) is None and route(hb, views=2) is None
    assert route(_handle(SIZES_A, n_edges=None)) is None
    assert route(_handle(SIZES_A, mask=object())) is None
    assert route(_handle((300, 1025))) is None and route(_handle((300, 0))) is None
    assert route(_handle((255, 40))) == "combination"    # (a dense layout keeps the dense PaiNN bucket)
    monkeypatch.setenv("GEOSSL_SPARSE_PAIRS", "1")
    assert route(_handle((255, 40))) == bk.SPARSE
    monkeypatch.setenv("GEOSSL_PAINN_TILE", "0")
    assert route(hb) is None
    monkeypatch.delenv("GEOSSL_PAINN_TILE")
    monkeypatch.setenv("GEOSSL_PAINN_VECTOR", "1")
    assert route(hb) is None
