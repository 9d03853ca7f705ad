"""numpy / Python twins of the device-side atom masking (geossl_gather_masked_molecules), written from the rule in
include/geossl_hip.h and DESIGN 2, and of the masked gather, for the masking tests."""
import numpy as np

M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox-4x32-10 of four 32-bit counter words under two key words (Salmon et al., SC'11)."""
    c0, c1, c2, c3 = (int(v) & M32 for v in ctr)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw(mol_id, t, seed, m):
    """An integer below m: (word 0 of Philox(counter (mol_id, t, 0, 0), key (seed low, seed high)) * m) >> 32."""
    w = philox4x32_10((mol_id, t, 0, 0), (seed & M32, (seed >> 32) & M32))[0]
    return (w * m) >> 32


def device_bfs(n, succ, k, mol_id, seed):
    """The kept atoms of one molecule (ascending) under the device rule: t = 0 picks the start below n; each later step
    t picks the draw(|frontier|)-th frontier atom in ascending order, or - frontier empty - the draw(n - t)-th unvisited
    atom; frontier = (frontier | successors(new)) - visited."""
    atom = draw(mol_id, 0, seed, n)
    vis = {atom}
    fr = set(succ[atom]) - vis
    for t in range(1, k):
        cand = sorted(fr) if fr else sorted(set(range(n)) - vis)
        atom = cand[draw(mol_id, t, seed, len(cand))]
        vis.add(atom)
        fr = (fr | set(succ[atom])) - vis
    return np.asarray(sorted(vis), dtype=np.int64)


def masked_collate(x, positions, sizes, keep, kept, rei_src=None, rei_cnt=None):
    """What the masked gather writes for molecules taken in order: rows keep of every molecule, the batch vector and -
    from the molecules' own radius edges (local indices, concatenated, rei_cnt per molecule) - the edges with both ends
    kept, renumbered by rank and offset to the batch."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    koff = np.concatenate([[0], np.cumsum(kept)])
    rows = np.concatenate([off[m] + keep[koff[m]:koff[m + 1]] for m in range(len(sizes))])
    out = {"x": x[rows], "positions": positions[rows], "batch": np.repeat(np.arange(len(sizes)), kept)}
    if rei_src is not None:
        eoff = np.concatenate([[0], np.cumsum(rei_cnt)])
        es = []
        for m in range(len(sizes)):
            rank = np.full(sizes[m], -1, dtype=np.int64)
            rank[keep[koff[m]:koff[m + 1]]] = np.arange(kept[m])
            e = rank[rei_src[:, eoff[m]:eoff[m + 1]]]
            es.append(e[:, (e >= 0).all(axis=0)] + koff[m])
        out["rei"] = np.concatenate(es, axis=1)
    return out
