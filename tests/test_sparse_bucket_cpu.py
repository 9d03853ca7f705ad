"""CPU tests of the sparse capacity bucket (geossl_amd/bucket.py, option "sparse"): the C ABI of the two `_dyn` entry
points of csrc/sparse_pairs.hip, the capacity logic on random size sequences, the host plan, and the constants the
other bucket kinds keep."""
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("geossl_sparse_pairs_build_dyn", "geossl_cfconv_aggregate_sparse_dyn")


def test_new_abi_symbols_declared_bound_and_exported():
    from geossl_amd import _lib
    h = open(os.path.join(REPO, "include", "geossl_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _lib.PROTOTYPES, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    # the `_dyn` forms take the exact forms' arguments and one device address more
    for name in NEW_SYMBOLS:
        exact, dyn = _lib.PROTOTYPES[name[:-4]], _lib.PROTOTYPES[name]
        assert dyn[0] == exact[0] and len(dyn[1]) == len(exact[1]) + 1 and dyn[1][:len(exact[1]) - 1] == exact[1][:-1]


def _random_sizes(rng, B, hi):
    n = rng.integers(1, hi + 1, size=B)
    n[rng.integers(0, B)] = hi
    return n


def test_capacities_hold_every_batch_that_fits_the_atoms():
    from geossl_amd import bucket as bk
    from geossl_amd.layout import SPARSE_MAX_N, sparse_pair_capacity
    rng = np.random.default_rng(0)
    for trial in range(200):
        B = int(rng.integers(1, 33))
        hi = int(rng.integers(2, SPARSE_MAX_N + 1))
        first = _random_sizes(rng, B, hi)
        N_cap, P_cap, S_cap, W_cap = bk.sparse_capacities(int(first.sum()), B, sizes=first)
        assert N_cap >= first.sum() and P_cap == 33 * N_cap and S_cap == 0 and W_cap == 0
        assert bk.batch_counts(first, bk.SPARSE, 1) == (int(first.sum()), 0, 0, 0)
        # any sequence of B' molecules with sum <= N_cap: its list fits P_cap
        for _ in range(20):
            other = _random_sizes(rng, B, int(rng.integers(1, SPARSE_MAX_N + 1)))
            while other.sum() > N_cap:
                other = np.maximum(other // 2, 1)
            assert sparse_pair_capacity(other) <= P_cap, (first, other)
    # the worst case: every molecule at the 33-rows-per-atom bound
    assert sparse_pair_capacity([1024] * 4) == 33 * 4096 <= bk.sparse_capacities(4096, 4)[1]


def test_max_n_class_bounds():
    from geossl_amd import bucket as bk
    from geossl_amd.layout import SPARSE_MAX_N
    assert bk.SPARSE_MAX_N_CLASSES[-1] == SPARSE_MAX_N == 1024
    for hi in range(1, SPARSE_MAX_N + 1):
        c = bk.sparse_max_n_class(hi)
        assert hi <= c <= 1024 and c in bk.SPARSE_MAX_N_CLASSES
        for prev in bk.SPARSE_MAX_N_CLASSES:
            c2 = bk.sparse_max_n_class(hi, prev)
            assert c2 >= max(hi, prev) and c2 <= 1024
    assert [bk.sparse_max_n_class(h) for h in (2, 256, 257, 300, 512, 513, 1024)] == [256, 256, 512, 512, 512, 1024, 1024]


def test_previous_capacities_are_never_undercut():
    from geossl_amd import bucket as bk
    rng = np.random.default_rng(1)
    for trial in range(100):
        B = int(rng.integers(1, 17))
        a, b = _random_sizes(rng, B, int(rng.integers(2, 1025))), _random_sizes(rng, B, int(rng.integers(2, 1025)))
        prev = bk.sparse_capacities(int(a.sum()), B, sizes=a)
        nxt = bk.sparse_capacities(int(b.sum()), B, prev=prev, sizes=b)
        assert all(n_ >= p_ for n_, p_ in zip(nxt, prev)) and nxt[0] >= b.sum() and nxt[1] == 33 * nxt[0]


def test_host_plan_of_the_sparse_option():
    from geossl_amd import bucket as bk
    n = np.array([300, 2, 64, 1])
    hp = bk.host_plan(n, bk.SPARSE, views=1)
    assert hp["counts"] == (367, 0, 0, 0)
    assert np.array_equal(hp["mol_ptr"], np.concatenate([[0], np.cumsum(n)]))
    # no pair, tuple or work entries
    assert set(hp) == {"counts", "mol_ptr"}


def test_existing_bucket_constants_stay():
    from geossl_amd import bucket as bk
    assert bk.MAX_N == 255 and bk.MAX_N_CLASSES[-1] == 255 and bk.PAINN_MAX_N_CLASSES[-1] == 255
    assert bk.SPARSE == "sparse" and bk.SPARSE not in ("combination", "permutation", bk.TRIPLES)


def test_switch_values(monkeypatch):
    """Unset: DeviceLoader handles take the sparse bucket, collated batches do not; 1: both; 0: neither."""
    from geossl_amd import switches
    monkeypatch.delenv("GEOSSL_SPARSE_BUCKETS", raising=False)
    assert switches.sparse_buckets(True) and not switches.sparse_buckets(False)
    monkeypatch.setenv("GEOSSL_SPARSE_BUCKETS", "1")
    assert switches.sparse_buckets(True) and switches.sparse_buckets(False)
    monkeypatch.setenv("GEOSSL_SPARSE_BUCKETS", "0")
    assert not switches.sparse_buckets(True) and not switches.sparse_buckets(False)


def test_eligibility_from_host_sizes(monkeypatch):
    """sparse_eligible needs host sizes in 1 .. 1024 and a layout that would be sparse; a dataset handle needs no
    tensors."""
    import types
    from geossl_amd import bucket as bk
    monkeypatch.delenv("GEOSSL_SPARSE_PAIRS", raising=False)
    handle = lambda sizes: types.SimpleNamespace(_sizes=np.asarray(sizes), _dataset=object(), _mask=None, _triples=False)
    assert bk.sparse_eligible(handle([300, 2, 64, 1])) and bk.sparse_eligible(handle([1024]))
    assert not bk.sparse_eligible(handle([255, 17]))          # a dense layout: today's routing
    assert not bk.sparse_eligible(handle([1025, 3]))
    assert not bk.sparse_eligible(types.SimpleNamespace(_sizes=None))
    monkeypatch.setenv("GEOSSL_SPARSE_PAIRS", "1")
    assert bk.sparse_eligible(handle([5, 17, 2, 33]))
    monkeypatch.setenv("GEOSSL_SPARSE_PAIRS", "0")
    assert not bk.sparse_eligible(handle([300, 2]))
