"""Pocket-sized test structures for the tests of the sparse pair list and of LBA fine-tuning (and for the maker of
fixture G24): atoms by rejection sampling in a cube at density 0.08 per cubic Angstrom with a minimum separation of 1 A,
``np.random.default_rng(100 * seed + k)`` for molecule k, cast to float32.  ``first_seed`` searches range(64) for the
first seed whose batch has no same-molecule pair within 1e-4 A of the cutoff (force_twin.cutoff_margin): closer than that,
fp32 and fp64 may build different radius graphs."""
import functools

import numpy as np

DENSITY = 0.08      # atoms per cubic Angstrom
MIN_SEP = 1.0       # Angstrom
MARGIN = 1e-4       # Angstrom


def molecule(n, seed, k):
    rng = np.random.default_rng(100 * seed + k)
    side = (n / DENSITY) ** (1.0 / 3.0)
    pts = np.empty((n, 3), dtype=np.float64)
    have = 0
    while have < n:
        p = rng.uniform(0.0, side, size=3)
        if have == 0 or np.min(np.sum((pts[:have] - p) ** 2, axis=1)) >= MIN_SEP * MIN_SEP:
            pts[have] = p
            have += 1
    return pts.astype(np.float32)


def structures(sizes, seed):
    """-> dict(positions [N, 3] f32, batch [N] i64, x [N] i64 atom types in 1 .. 8, sizes)."""
    pos = np.concatenate([molecule(int(n), seed, k) for k, n in enumerate(sizes)])
    batch = np.repeat(np.arange(len(sizes), dtype=np.int64), np.asarray(sizes, dtype=np.int64))
    N = pos.shape[0]
    x = ((np.arange(N, dtype=np.int64) * 7 + batch * 3) % 8) + 1
    return dict(positions=pos, batch=batch, x=x, sizes=[int(n) for n in sizes])


@functools.lru_cache(maxsize=None)
def first_seed(sizes, cutoff):
    """(seed, margin) of the first seed in range(64) whose structures keep every pair MARGIN away from the cutoff."""
    from force_twin import cutoff_margin
    for seed in range(64):
        s = structures(sizes, seed)
        m = cutoff_margin(s["positions"], s["batch"], cutoff)
        if m >= MARGIN:
            return seed, m
    raise AssertionError("no seed in range(64) keeps sizes %r %.0e A away from cutoff %g" % (sizes, MARGIN, cutoff))


def checked(sizes, cutoff):
    """The structures of first_seed(sizes, cutoff), with the seed and the margin."""
    seed, margin = first_seed(tuple(int(n) for n in sizes), float(cutoff))
    return dict(structures(sizes, seed), seed=seed, margin=margin)


def pair_capacity(sizes):
    """layout.sparse_pair_capacity, restated: sum_m min(n (n - 1) / 2, 33 n)."""
    return sum(min(n * (n - 1) // 2, 33 * n) for n in (int(k) for k in sizes))
