"""Python twin of the device-side draw of sampled atom tuples (geossl_sampled_tuples), written from the rule in
include/geossl_hip.h, and brute-force forms of what a sampled bucket holds, for the sampled-tuple tests."""
import itertools

import numpy as np

from masking_twin import M32, philox4x32_10


def enumeration(n, option):
    """The extractor's tuples of an n-atom molecule in slot order (dataloaders_AtomTuple.py:19-24) as a list of pairs."""
    it = itertools.permutations(range(n), 2) if option == "permutation" else itertools.combinations(range(n), 2)
    return list(it)


def slot_key(s, mol_id, seed):
    """(w0 << 32) | w1 of Philox-4x32-10 on the counter (s, mol_id, 0, 0) under (seed low, seed high)."""
    w = philox4x32_10((s, mol_id & M32, 0, 0), (seed & M32, (seed >> 32) & M32))
    return (w[0] << 32) | w[1]


def kept_slots(M, k, mol_id, seed):
    """The k slots of M with the smallest (key, slot), ascending."""
    order = sorted(range(M), key=lambda s: (slot_key(s, mol_id, seed), s))
    return sorted(order[:k])


def brute_counts(sizes, option, ratio):
    """int(M * ratio) per molecule, M counted by enumerating."""
    return [int(len(enumeration(int(n), option)) * ratio) for n in sizes]


def device_tuples(sizes, ids, option, ratio, seed):
    """super_edge_index [2, S] of the batch under the device rule: per molecule the kept slots in ascending order,
    unranked, with the batch's atom offset added."""
    cols, at = [], 0
    for n, i in zip(sizes, ids):
        tup = enumeration(int(n), option)
        k = int(len(tup) * ratio)
        cols += [(at + tup[s][0], at + tup[s][1]) for s in kept_slots(len(tup), k, int(i), seed)]
        at += int(n)
    return np.asarray(cols, dtype=np.int64).reshape(-1, 2).T


def incidence(N, sei):
    """(inc_ptr [N + 1], inc_idx [2 S]): every atom's tuple ids, ascending (the u side before the v side of one tuple)."""
    lists = [[] for _ in range(N)]
    for s, (u, v) in enumerate(sei.T.tolist()):
        lists[u].append(s)
        lists[v].append(s)
    ptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum([len(l_) for l_ in lists], out=ptr[1:])
    return ptr, np.asarray([s for l_ in lists for s in l_], dtype=np.int32)
