#!/usr/bin/env python3
"""Host count of what the atom-window logic of k_filter_bwd_h (filter_bwd.hip: decide()) does on a batch: per tile height
and window capacity the share of tiles that keep the window (sticky), get a fresh one, or take the unstaged fallback.
    python tools/filter_bwd_window_share.py [mols=1024] [set=B] [cutoff=5.0] [layers=6]
Pair slots as the step's filter launches see them: lexicographic i < j inside a molecule, the slots without an edge
(d >= cutoff) dropped (the live-pair list), the clean view of the molecules bench.py times.  No GPU needed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def pair_list(mols, molset, cutoff):
    from geossl_amd.synthetic import make_molecules
    m = make_molecules(mols, seed=1000, mode=molset)
    pos, first = m["positions"].astype(np.float64), 0
    pi, pj = [], []
    for n in (int(n) for n in m["sizes"]):
        i, j = np.triu_indices(n, k=1)
        live = np.linalg.norm(pos[first + i] - pos[first + j], axis=1) < cutoff
        pi.append(first + i[live])
        pj.append(first + j[live])
        first += n
    return np.concatenate(pi), np.concatenate(pj)


def simulate(pair_i, pair_j, tr, cap, layers):
    """decide() tile by tile over the contiguous tile range of every block (256 / layers blocks per layer)."""
    P = pair_i.size
    ntiles = (P + tr - 1) // tr
    nb = max(1, min(256 // max(layers, 1), ntiles))
    per = (ntiles + nb - 1) // nb
    sticky = fresh = fallback = 0
    for b in range(nb):
        have, walo = False, 0
        for t in range(b * per, min(ntiles, (b + 1) * per)):
            alo = int(pair_i[t * tr])
            amax = int(pair_j[t * tr:min(P, (t + 1) * tr)].max()) + 1
            if have and alo >= walo and amax - walo <= cap:
                sticky += 1
            elif amax - alo <= cap:
                fresh += 1
                have, walo = True, alo
            else:
                fallback += 1
    return ntiles, sticky, fresh, fallback


def main():
    mols = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    molset = sys.argv[2] if len(sys.argv) > 2 else "B"
    cutoff = float(sys.argv[3]) if len(sys.argv) > 3 else 5.0
    layers = int(sys.argv[4]) if len(sys.argv) > 4 else 6
    pi, pj = pair_list(mols, molset, cutoff)
    print("set %s, %d molecules, %.1f A: %d live pair slots" % (molset, mols, cutoff, pi.size))
    print("%4s %4s %8s %8s %8s %9s   %s" % ("TR", "cap", "tiles", "sticky", "fresh", "fallback", "fresh windows per 1024 rows"))
    for tr, cap in ((32, 40), (64, 40), (64, 48), (64, 56), (64, 64)):
        n, s, f, fb = simulate(pi, pj, tr, cap, layers)
        print("%4d %4d %8d %8.4f %8.4f %9.5f   %.2f" % (tr, cap, n, s / n, f / n, fb / n, 1024.0 * f / (n * tr)))


if __name__ == "__main__":
    main()
