"""Which test covers each kernel that holds a packed-fp32 instruction whose LOW result reads a source's HIGH half, and at
what occupancy that test launches it.

Why: the mu-zero form of k_painn_fwd_mma dropped one term in lanes 48-63 only when two waves shared a SIMD (DESIGN 7,
round 6); its instruction was `v_pk_mul_f32 .. op_sel:[0,1]`.  Every kernel whose code object still holds such a form
(tools/scan_packed_opsel.py: lo_select_forms) is listed here with the full-occupancy fp64 test that covers it and the
launch that test makes: block size, dynamic LDS (restated from the kernel's launcher in geossl_amd/csrc) and grid.
tests/test_packed_opsel_cpu.py checks, without a GPU, that the list is complete and that each recorded launch reaches
the stated waves per SIMD on the built code object.  A plain module, no tests of its own.
"""
import re

GPU_MODULE = "test_gpu_packed_kernels"

# ---- the shapes the GPU tests launch at (test_gpu_packed_kernels.py imports them)
BENCH_MOLS = 1024           # bench.py's batch: 1024 molecules, set A (18 atoms each)
SET_A_MAX_N = 18
SET_B_MAX_N = 33            # synthetic.molecule_sizes(mode="B"): at most 33 atoms (the tests assert it)
FILTER_L = 2                # layers per filter-backward launch: grid (256 // L, L) = 256 blocks, one per CU
NCSN_S = BENCH_MOLS * 18 * 17 // 2        # super-edges of the bench batch ("combination": n (n - 1) / 2 per molecule)
PAINN_F = 128
PAINN_EDGES_MIN = 200000    # radius edges of the bench batch at 5 A (the test asserts its batch has at least these)
TAPE_N = 1 << 24            # elements per element-wise map launch
ATOMS = BENCH_MOLS * 18

CUS = 256
HUGE_GRID = 1 << 30         # "as many blocks as the CUs take": the resource limit alone


def _ceil4(x):
    return (x + 3) // 4 * 4


# ---- dynamic LDS of each launcher, in bytes (restated; the registry test recomputes occupancy from these)
def filter_bwd_h_lds(F):        # filter_bwd.hip: BwdLdsH<F>::bytes()
    KC, CB, AS = F // 16, F // 32, F + 4
    stage = 2 * 40 * AS + 32 + 4 * 32 + 4 + 8
    return (KC * 2 + CB * 4 + 8) * 1024 + 32 + 256 + 2 * stage * 4


def filter_bwd_lds(F):          # filter_bwd.hip: BwdLds<F>::bytes()
    KC, CB, AS = F // 16, F // 32, F + 4
    stage = 2 * 40 * AS + 32 + 4 * 32 + 4
    return (KC * 3 + CB * 6 + 12) * 1024 + 2 * stage * 4


def filter_bwd_grid(L=FILTER_L, ntiles=HUGE_GRID):   # filter_bwd.hip: blocks_per_layer x L
    return min(max(256 // L, 1), ntiles) * L


def ncsn_fwd_lds(F):            # ncsn_rows.hip: geossl_ddm_loss_fwd / _fwd2
    NMB, H, KS = F // 32, F // 2, F // 16
    HMB = (H + 31) // 32
    return (NMB + HMB) * KS * 3 * 1024 + (5 * F + 2 * 32 * HMB + 8) * 4


def ncsn_fwd_grid(S=NCSN_S):    # ncsn_rows.hip: row_blocks_grid
    return min(((S + 31) // 32 + 7) // 8, 256)


def ncsn_fwd2_grid(S=NCSN_S):   # (row_blocks_grid + 1) / 2 blocks per head, two heads
    return (ncsn_fwd_grid(S) + 1) // 2 * 2


def painn_fwd_mol_lds(max_n, R, F=PAINN_F):        # painn.hip: geossl_painn_interaction_fwd_mol
    return (max_n * 6 * F + (4 * F // 64) * 16 * _ceil4(R + 5)) * 4


def painn_fwd_mol_grid(B, lds):
    return min(B, 256 * (2 if 2 * lds <= 160 * 1024 else 1))


def painn_bwd_mol_lds(max_n, R, F=PAINN_F):        # painn.hip: geossl_painn_interaction_bwd_mol
    stage = max_n * 4 * F + (4 * F // 64) * 16 * _ceil4(R + 5)
    return max(stage, 3 * F * (R + 1)) * 4


def painn_bwd_grid(N=ATOMS):   # painn.hip: GEOSSL_PAINN_BWD_BLOCKS
    return min(N, 1536)


def painn_edge_grads_lds(R, F=PAINN_F):            # painn_force.hip
    return (3 * F * (R + 1) + 3 * F) * 4


def painn_edge_grads_grid(E=PAINN_EDGES_MIN):      # painn_force.hip: grid_for(E, 4 waves * 8, 4096)
    return max(1, min((E + 31) // 32, 4096))


def tape_grid(n=TAPE_N):        # tape.hip: tape_grid((n + 3) / 4, 256) on 16-byte aligned tensors
    return max(1, min(((n + 3) // 4 + 255) // 256, 8192))


def painn_mma_lds(max_n):       # painn_mma.hip: painn_mma_lds
    return (max_n * 7 * 128 + 4 * 160 + 8) * 4


def painn_mma_grid(B, lds):
    return min(B, 256 * (2 if 2 * lds <= 160 * 1024 else 1))


ONE_BLOCK_PER_CU = "the launcher fixes one block per CU and the block has %d threads (%d waves over 4 SIMDs)"
MMA_SET_B = "33 atoms of set B take 119 KB of LDS: one 256-thread block per CU (the product's set-B occupancy)"

# ---- the registry: one entry per instantiation.  `symbol`: a regex on the mangled name; `tests`: GPU test functions of
# GPU_MODULE (or "module::function" elsewhere); `launches`: (label, block threads, dynamic LDS bytes, blocks in grid,
# waves per SIMD that launch reaches, why it is 1 if it is) - the launches the tests make.
ENTRIES = []


def _add(family, symbol, tests, launches):
    ENTRIES.append(dict(family=family, symbol=symbol, tests=list(tests), launches=list(launches)))


_FILTER_TEST = ["test_filter_backward_at_full_occupancy_vs_fp64"]
for _nw in (1, 2, 4):
    _F = 32 * _nw
    _w, _cap = (2, None) if _nw == 4 else (1, ONE_BLOCK_PER_CU % (128 * _nw, 2 * _nw))
    for _recomp in (0, 1):   # k_filter_bwd_h<NW, T == NULL>
        _add("k_filter_bwd_h", r"k_filter_bwd_hILi%dELb%dE" % (_nw, _recomp), _FILTER_TEST,
             [("F=%d %s" % (_F, "recompute" if _recomp else "saved"), 128 * _nw, filter_bwd_h_lds(_F), filter_bwd_grid(),
               _w, _cap)])
    _add("k_filter_bwd", r"k_filter_bwdILi%dE" % _nw, _FILTER_TEST,          # GEOSSL_FILTER_BWD_BF16X3
         [("F=%d bf16x3" % _F, 128 * _nw, filter_bwd_lds(_F), filter_bwd_grid(), _w, _cap)])

for _nmb in (1, 2, 4):
    _add("k_ncsn_fwd", r"k_ncsn_fwdILi%dE" % _nmb, ["test_ncsn_head_forward_at_full_occupancy_vs_fp64"],
         [("F=%d" % (32 * _nmb), 512, ncsn_fwd_lds(32 * _nmb), ncsn_fwd_grid(), 2, None)])
    _add("k_ncsn_fwd2", r"k_ncsn_fwd2ILi%dE" % _nmb, ["test_ncsn_head_forward_at_full_occupancy_vs_fp64"],
         [("F=%d two heads" % (32 * _nmb), 512, ncsn_fwd_lds(32 * _nmb), ncsn_fwd2_grid(), 2, None)])


def _mol_launches(label, block, lds_of, grid_of, waves):
    return [("%s set %s" % (label, s), block, lds_of(n), grid_of(lds_of(n)), w, c)
            for (s, n), (w, c) in zip((("A", SET_A_MAX_N), ("B", SET_B_MAX_N)), waves)]


for _r in (8, 16, 20, 32):
    # set B (33 atoms) needs more than half the LDS: one block per CU, its 8 waves give 2 per SIMD
    _add("k_painn_interaction_fwd_mol", r"k_painn_interaction_fwd_molILi%dE" % _r,
         ["test_painn_interaction_forward_at_full_occupancy_vs_fp64"],
         _mol_launches("R=%d" % _r, 512, lambda n, r=_r: painn_fwd_mol_lds(n, r), lambda l: painn_fwd_mol_grid(BENCH_MOLS, l),
                       [(2 if _r == 32 else 4, None), (2, None)]))
    _add("k_painn_interaction_bwd", r"k_painn_interaction_bwdILi%dE" % _r,
         ["test_painn_interaction_backward_at_full_occupancy_vs_fp64"],
         [("R=%d per atom" % _r, 128, 0, painn_bwd_grid(), {8: 3, 16: 2, 20: 2, 32: 1}[_r],
           "320 VGPR+AGPR per lane: one wave per SIMD by registers" if _r == 32 else None)])
    _add("k_painn_edge_grads", r"k_painn_edge_gradsILi%dE" % _r, ["test_painn_edge_grads_at_full_occupancy_vs_fp64"],
         [("R=%d" % _r, 256, painn_edge_grads_lds(_r), painn_edge_grads_grid(), {8: 4, 16: 3, 20: 2, 32: 2}[_r], None)])
for _r in (8, 16, 20):
    for _mz in (0, 1):
        _add("k_painn_interaction_bwd_mol", r"k_painn_interaction_bwd_molILi%dELb%dE" % (_r, _mz),
             ["test_painn_interaction_backward_at_full_occupancy_vs_fp64"],
             _mol_launches("R=%d %s" % (_r, "mu0" if _mz else "general"), 512, lambda n, r=_r: painn_bwd_mol_lds(n, r),
                           lambda l: min(BENCH_MOLS, 256), [(2, None), (2, None)]))
    for _mz in (0, 1):   # the family of the round-6 finding: now built without packed fp32 ops, registered all the same
        # (the general form, Lb0, by the test that runs it with LIVE mu; the two round-6 tests zero mu: they cover Lb1)
        _add("k_painn_fwd_mma", r"k_painn_fwd_mmaILi%dELb%dE" % (_r, _mz),
             ["test_gpu_round6::test_painn_first_interaction_with_mu_null_is_the_general_kernel_bit_for_bit",
              "test_gpu_round6::test_painn_first_interaction_with_mu_null_at_more_batch_shapes"] if _mz else
             ["test_gpu_painn_mma::test_forward_with_live_mu_at_full_occupancy_vs_fp64"],
             _mol_launches("R=%d" % _r, 256, painn_mma_lds, lambda l: painn_mma_grid(BENCH_MOLS, l),
                           [(2, None), (1, MMA_SET_B)]))

_add("k_tape_unary", r"k_tape_unaryE", ["test_tape_unary_maps_at_full_occupancy_vs_fp64"],
     [("n=2^24", 256, 0, tape_grid(), 8, None)])


def entries_for(kernel):
    return [e for e in ENTRIES if re.search(e["symbol"], kernel)]


def launch(symbol, label):
    """The recorded launch `label` of the entry `symbol`: (block, dynamic LDS, grid, waves)."""
    for e in ENTRIES:
        if e["symbol"] == symbol:
            for l in e["launches"]:
                if l[0] == label:
                    return l[1:5]
    raise KeyError((symbol, label))
