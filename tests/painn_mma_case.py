"""The hand-made edge list of the matrix-pipe PaiNN forward's tests (csrc/painn_mma.hip), its group layout restated in
numpy (geossl_amd/layout.py: EdgeLayout.groups) and the kernel's summation order emulated in fp32: a plain module, no
GPU.  tests/test_painn_forms_cpu.py checks the emulation against the fp64 twin, tests/test_gpu_painn_mma.py runs the
kernel on the same edges and checks this module's layout against the device's."""
import numpy as np

SIZES = (44, 1, 2, 44, 7)
# in-degrees of the first molecule's atoms.  Groups of four rows: 43 -> 11 groups (groups 0 .. 10: the run crosses the end
# of the first tile, a tile being eight groups); 0, 1, 3, 4, 1 -> one group each, the last of them is group 15, the last
# group of the second tile; 5, 8 -> two groups; 28, 29, 32, 33 -> 7, 8, 8, 9 groups; then small degrees.
HEAD_DEGREES = (43, 0, 1, 3, 4, 1, 5, 8, 28, 29, 32, 33)
REQUIRED_DEGREES = (0, 1, 3, 4, 5, 8, 28, 29, 32, 33, 43)
MAX_DEGREE = 43


def degrees():
    rng = np.random.default_rng(44)
    d0 = list(HEAD_DEGREES) + [(5 * a) % 7 for a in range(len(HEAD_DEGREES), SIZES[0])]
    d3 = [int(v) for v in rng.integers(0, 44, size=SIZES[3])]
    return [d0, [0], [3, 1], d3, [4, 4, 4, 4, 4, 4, 8]]       # (the last molecule: 6 + 2 = 8 groups; the second: 1)


def edges():
    """-> edge_index [2, E] int64 (row 0 the target), batch [N] int64: per molecule, atom a is the target of degree(a)
    edges whose sources are drawn inside the molecule with duplicates (self loops included); the edges of a molecule are
    shuffled among themselves (the layout asks for molecules in batch order, not for more)."""
    rng = np.random.default_rng(45)
    tgt, src, a0 = [], [], 0
    for n, deg in zip(SIZES, degrees()):
        assert len(deg) == n
        t_ = np.repeat(np.arange(a0, a0 + n), deg)
        s_ = rng.integers(a0, a0 + n, size=t_.size)
        order = rng.permutation(t_.size)
        tgt.append(t_[order])
        src.append(s_[order])
        a0 += n
    batch = np.repeat(np.arange(len(SIZES)), SIZES)
    return np.stack([np.concatenate(tgt), np.concatenate(src)]).astype(np.int64), batch.astype(np.int64)


def groups_np(edge_index, sizes):
    """EdgeLayout.groups("i", mol_ptr) in numpy: (row_edge [4 G], grp_code [G], grp_ptr [N + 1], mol_grp [B + 1]) with G
    the number of groups in use (the device arrays are longer and hold -1 behind them)."""
    tgt = edge_index[0]
    N = int(sum(sizes))
    order = np.argsort(tgt, kind="stable")                     # an atom's edges in ascending edge order
    deg = np.bincount(tgt, minlength=N)
    iptr = np.concatenate([[0], np.cumsum(deg)])
    ng = np.maximum((deg + 3) // 4, 1)
    grp_ptr = np.concatenate([[0], np.cumsum(ng)])
    G = int(grp_ptr[-1])
    row_edge = np.full(4 * G, -1, dtype=np.int64)
    grp_code = np.zeros(G, dtype=np.int64)
    for a in range(N):
        row_edge[4 * grp_ptr[a]:4 * grp_ptr[a] + deg[a]] = order[iptr[a]:iptr[a + 1]]
        grp_code[grp_ptr[a]:grp_ptr[a + 1]] = 2 * a
        grp_code[grp_ptr[a + 1] - 1] += 1
    mol_ptr = np.concatenate([[0], np.cumsum(sizes)])
    return row_edge, grp_code, grp_ptr, grp_ptr[mol_ptr]


def emulate_fwd_mma(q, mu, xc, edge_index, sizes, phi, fcut, dirv, Wf, bf):
    """The forward in fp32 in the kernel's order of additions (numpy float32 arrays in, q_out [N, F], mu_out [N, 3, F]
    float32 out): per molecule the tiles of eight groups; a group's four rows are added in row order, the group sums to the
    atom's running sums in group order - across the end of a tile - and the residual last.  The filter is a plain fp32
    dot product with the bias as the last term (R + 1 roundings of u / 4: inside the 9 u the matrix-pipe form is given)."""
    f32 = np.float32
    N, F = q.shape
    row_edge, code, _, mol_grp = groups_np(edge_index, sizes)
    src = edge_index[1]
    q_out, mu_out = np.full((N, F), np.nan, f32), np.full((N, 3, F), np.nan, f32)
    for m in range(len(sizes)):
        t = np.zeros((4, F), f32)                              # q, mu x, mu y, mu z of the current target atom
        for gb in range(int(mol_grp[m]), int(mol_grp[m + 1]), 8):
            for g in range(gb, min(gb + 8, int(mol_grp[m + 1]))):
                s = np.zeros((4, F), f32)
                for e in row_edge[4 * g:4 * g + 4]:
                    if e < 0:
                        continue                               # (a padding row adds an exact zero)
                    W = np.zeros(3 * F, f32)
                    for k in range(phi.shape[1]):
                        W = (W + f32(phi[e, k]) * Wf[:, k]).astype(f32)
                    W = ((W + bf).astype(f32) * f32(fcut[e])).astype(f32)
                    x = (W * xc[src[e]]).astype(f32)
                    s[0] = s[0] + x[:F]
                    for d in range(3):
                        s[1 + d] = s[1 + d] + ((x[F:2 * F] * f32(dirv[e, d])).astype(f32) + (x[2 * F:] * mu[src[e], d]).astype(f32))
                t = t + s
                if code[g] & 1:
                    a = int(code[g] >> 1)
                    q_out[a] = q[a] + t[0]
                    mu_out[a] = mu[a] + t[1:]
                    t = np.zeros((4, F), f32)
    return q_out, mu_out
