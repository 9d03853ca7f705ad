/* C ABI of libgeossl_hip.so — the MI355X (gfx950) hot path of GeoSSL's SchNet/PaiNN + DDM step.
 *
 * The reference (chao1224/GeoSSL) is pure Python: it has no FFI, the "interface" this library sits behind is
 * the set of ATen / torch_geometric / torch_scatter / torch_cluster calls its hot path makes.  Every entry
 * point below names the reference call site(s) it replaces (paths relative to the reference root).
 *
 * Conventions (all functions):
 *   - raw DEVICE pointers, explicit sizes, scalars by value, trailing hipStream_t;
 *   - return value is a hipError_t as int (0 = success); nothing throws, allocates or synchronises;
 *   - the caller owns every buffer, pre-allocates outputs / workspaces and keeps inputs alive until the
 *     stream reaches the call; re-entrant, no global state.
 *   - fp32 everywhere; "i64" index tensors are the reference's int64 tensors, internal indices are int32.
 */
#ifndef GEOSSL_HIP_H
#define GEOSSL_HIP_H
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
typedef struct ihipStream_t* hipStream_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define GEOSSL_ABI_VERSION 1
#define GEOSSL_MAX_L 12 /* max interaction blocks handled by the batched-by-layer kernels */
#define GEOSSL_TN_MAX 32 /* max problems in one batched weight-gradient launch */
#define GEOSSL_LOSS_PARTIALS 256 /* block partials of the per-row loss that geossl_ddm_loss_fwd leaves in its workspace */

/* epilogue flags of geossl_linear */
#define GEOSSL_EPI_BIAS 1      /* + bias[n] */
#define GEOSSL_EPI_SSP 2       /* ShiftedSoftplus (schnet.py:210-216) */
#define GEOSSL_EPI_RESIDUAL 4  /* + res[r][n]   (h = h + block(h), schnet.py:97) */
#define GEOSSL_EPI_MUL_DSSP 8  /* * d ssp/dx recovered from the saved ssp OUTPUT tprev[r][n] (backward) */
#define GEOSSL_CHAIN_NEW_INPUT 32  /* geossl_linear_chain, F = 128: the stage reads its own input `xin` (a Linear over a
                                      wide input = several F-wide passes in one launch) */
#define GEOSSL_CHAIN_ADD_PREV 64   /* ... and adds the result of the stage before it (kept in registers) */
#define GEOSSL_EPI_SILU 128       /* geossl_linear_chain, F = 128: Y = X W^T + b goes to `out` as it is (the backward needs the
                                    pre-activation), silu(Y) to `out_act` (may be NULL) and into the next stage -
                                    Dense(F, F, silu) + the Dense behind it, painn_utils.py:27-35 */
#define GEOSSL_EPI_MUL_DSILU 256  /* ... with tprev: * silu'(tprev), tprev = the saved PRE-activation (backward) */
#define GEOSSL_CHAIN_SAME_INPUT 16 /* geossl_linear_chain, F = 128: the stage takes the input of the stage before it
                                      (several F -> F blocks of one wide Linear in one launch) instead of its result */

int geossl_abi_version(void);

/* ---- batch layout (position independent; built once per collated batch) -------------------------------
 * Replaces the index bookkeeping of BatchAtomTuple.from_data_list (Geom3D/dataloaders/dataloaders_AtomTuple.py:57-73)
 * and the `batch[-1].item()+1` of num_graphs (:75-78).  `batch` must be sorted ascending (collated batches are).
 *   mol_ptr[B+1]  : atom offsets; pair_ptr[B+1] : offsets of the n(n-1)/2 "pair slots" (i<j, lexicographic —
 *                   the same enumeration as AtomTupleExtractor "combination", :22-23)
 *   stats[4]      : {max atoms per molecule, total pair slots P, 1 if batch is not sorted / out of range, 0}
 *   pair_i/pair_j : atom ids (global) of every pair slot                                                   */
int geossl_layout_build(const int64_t* batch, int64_t N, int64_t B, int32_t* mol_ptr, int32_t* pair_ptr,
                        int64_t* stats, hipStream_t stream);
/* Device-side AtomTupleExtractor (dataloaders_AtomTuple.py:15-37 with ratio = 1) including the node offset of the
 * collate (:64-65): super_edge_index rows out0 / out1.  option 0 = "combination" (i<j, itertools.combinations
 * order), 1 = "permutation" (i != j, itertools.permutations order).  tuple_ptr[B+1] (int64): exclusive prefix sum
 * of the per-molecule tuple counts n(n-1)/2 or n(n-1).                                                        */
int geossl_atom_tuples(const int32_t* mol_ptr, const int64_t* tuple_ptr, int64_t B, int option, int64_t* out0,
                       int64_t* out1, hipStream_t stream);
int geossl_pair_index_fill(const int32_t* mol_ptr, const int32_t* pair_ptr, int64_t B, int32_t* pair_i,
                           int32_t* pair_j, hipStream_t stream);

/* ---- radius graph (K1) — torch_cluster.radius_graph via torch_geometric (schnet.py:91;
 * datasets_3D_Radius.py:120) + the edge length of schnet.py:93.
 * Semantics: per molecule, per target i scan sources j ascending, hit when fl32(dx^2+dy^2+dz^2) < r2 (strict,
 * no FMA), stop after `cap` hits (cap = max_num_neighbors + 1, the self hit counts), drop j == i.
 *   _count : deg[N] = in-degree of every target
 *   _fill  : edge_ptr[N+1] = exclusive scan of deg (caller); writes edge_index as two int64 rows
 *            (src = source j, dst = target i; target-major, sources ascending) and edge_weight[E]
 *   geossl_pair_geometry : the same graph in pair-slot form for the fused SchNet path:
 *            pair_d[P] = |x_i - x_j|, pair_c[P] = 0.5*(cos(d*pi/cutoff)+1) (the CFConv envelope, schnet.py:186),
 *            pair_flag[P] bit0 = edge (j -> i) present, bit1 = edge (i -> j) present, for slot (i<j).       */
int geossl_radius_graph_count(const float* pos, const int32_t* mol_ptr, int64_t B, int max_n, float r2, int cap,
                              int32_t* deg, hipStream_t stream);
int geossl_radius_graph_fill(const float* pos, const int32_t* mol_ptr, int64_t B, int max_n, float r2, int cap,
                             const int64_t* edge_ptr, int64_t* edge_src, int64_t* edge_dst, float* edge_weight,
                             hipStream_t stream);
int geossl_pair_geometry(const float* pos, const int32_t* mol_ptr, const int32_t* pair_ptr, int64_t B, int max_n,
                         float r2, int cap, float cutoff, float* pair_d, float* pair_c, uint8_t* pair_flag,
                         hipStream_t stream);

/* ---- Gaussian smearing (K2) — GaussianSmearing.forward, schnet.py:205-207: out[e][g] = exp(coeff*(d-off_g)^2) */
int geossl_rbf_fwd(const float* d, int64_t E, const float* offset, int G, float coeff, float* out,
                   hipStream_t stream);

/* ---- ShiftedSoftplus as a stand-alone op — ShiftedSoftplus.forward, schnet.py:210-216 (the module is usable on its
 * own in the reference; inside the hot path it is fused into the GEMM epilogues):  y = softplus(x) - log 2;
 * backward from the saved OUTPUT: dx = dy * sigmoid(x) = dy * (1 - 0.5 exp(-y)).                                 */
int geossl_ssp_fwd(const float* x, int64_t n, float* y, hipStream_t stream);
int geossl_ssp_bwd(const float* y, const float* dy, int64_t n, float* dx, hipStream_t stream);

/* ---- continuous-filter network for all interaction blocks (K3) — InteractionBlock.mlp applied in
 * CFConv.forward, schnet.py:141-145,186-187:  Wf_l[p] = (ssp(rbf(d_p) A1_l^T + b1_l) A2_l^T + b2_l) * C(d_p),
 * C(d) = 0.5*(cos(d*pi/cutoff)+1).  One launch covers every layer l < L and every pair slot p < P.
 *   T (optional, training) : saved hidden activation ssp(.) [L][P][F];  Wf : [L][P][F]                      */
typedef struct {
  const float* w1[GEOSSL_MAX_L]; /* mlp.0.weight [F][G] */
  const float* b1[GEOSSL_MAX_L]; /* mlp.0.bias   [F]    */
  const float* w2[GEOSSL_MAX_L]; /* mlp.2.weight [F][F] */
  const float* b2[GEOSSL_MAX_L]; /* mlp.2.bias   [F]    */
} GeosslFilterWeights;
int geossl_cfconv_filter_fwd(const float* pair_d, const float* pair_c, int64_t P, const GeosslFilterWeights* w, int L,
                             int F, int G, const float* offset, float coeff, float* T, float* Wf, hipStream_t stream);

/* Backward of K3 with respect to the filter-network weights, all blocks at once (positions carry no gradient on
 * the DDM path).  The upstream gradient dWf[p] = flag0*dagg[i]*x[j] + flag1*dagg[j]*x[i] is never materialised: it is
 * rebuilt from the per-layer atom tensors x_l = conv.lin1(h) and dagg_l = dL/d(aggregate) (both [N][F]) staged in LDS.
 *   dA2_l = sum_p dO^T T,  db2_l = sum_p dO,  dU = ((dO) A2_l) * ssp'(.),  dA1_l = sum_p dU^T rbf(d),  db1_l = sum_p dU
 * with dO = dWf * C(d).  Deterministic (per-wave / per-block partials + fixed-order reduction).                 */
typedef struct {
  const float* x[GEOSSL_MAX_L];    /* [N][F] */
  const float* dagg[GEOSSL_MAX_L]; /* [N][F] */
} GeosslFilterGradIn;
typedef struct {
  float* dw1[GEOSSL_MAX_L];
  float* db1[GEOSSL_MAX_L];
  float* dw2[GEOSSL_MAX_L];
  float* db2[GEOSSL_MAX_L];
} GeosslFilterGradOut;
int64_t geossl_cfconv_filter_bwd_workspace_floats(int64_t P, int L, int F, int G);
int geossl_cfconv_filter_bwd(const float* pair_d, const float* pair_c, const uint8_t* pair_flag, const int32_t* pair_i,
                             const int32_t* pair_j, int64_t P, int64_t N, const GeosslFilterWeights* w,
                             const GeosslFilterGradIn* g, int L, int F, int G, const float* offset, float coeff,
                             const float* T, const GeosslFilterGradOut* out, float* workspace, int accumulate,
                             hipStream_t stream);

/* ---- position gradient through K1-K4 (first order) — the d/d pos of finetune_md17.py:46 through
 * schnet.py:91-93 (edge length), :186-187 (cosine envelope) and :205-207 (Gaussian smearing); SURVEY 8(f) N3.
 * Same inputs as geossl_cfconv_filter_bwd plus the filter rows Wf; dd[l][p] = dL/dd_p contributed by block l:
 *   sum_c (flag0*dagg[i][c]*x[j][c] + flag1*dagg[j][c]*x[i][c]) * dWf[p][c]/dd,
 *   dWf/dd = C(d) * W2 (ssp'(.) * (W1 rbf'(d)))  +  C'(d)/C(d) * Wf        (the filter row differentiated forward).
 * geossl_pair_position_grad sums dd over l and applies d|pos_a - pos_b|/d pos to both atoms of every pair slot:
 *   dpos[a] = sum_b (sum_l dd[l][slot(a,b)]) * (pos[a] - pos[b]) / d(a,b)        (fixed order, no atomics).   */
int geossl_cfconv_filter_dpos(const float* pair_d, const float* pair_c, const uint8_t* pair_flag, const int32_t* pair_i,
                              const int32_t* pair_j, int64_t P, const GeosslFilterWeights* w,
                              const GeosslFilterGradIn* g, int L, int F, int G, const float* offset, float coeff,
                              float cutoff, const float* T, const float* Wf, float* dd, hipStream_t stream);
int geossl_pair_position_grad(const float* pos, const float* pair_d, const float* dd, const int32_t* mol_ptr,
                              const int32_t* pair_ptr, int64_t B, int64_t P, int L, float* dpos, hipStream_t stream);

/* ---- neighbour aggregation (K4) — MessagePassing.propagate(aggr="add") with message x_j * W
 * (schnet.py:190,194-195): out[i] = sum over edges (j -> i), j ascending, of x[j] * Wf[slot(i,j)].
 * swap = 1 runs the transposed graph (backward w.r.t. x): out[j] = sum over edges (j -> i) of x[i]*Wf.
 * order (may be NULL): a permutation of the molecules, the sequence in which they are started (largest first for
 * ragged batches; it does not change any result).                                                              */
int geossl_cfconv_aggregate(const float* x, const float* Wf, const uint8_t* pair_flag, const int32_t* mol_ptr,
                            const int32_t* pair_ptr, const int32_t* order, int64_t B, int max_n, int F, int swap,
                            float* out, hipStream_t stream);
/* The same aggregation from a host-built work list (ragged batches): work entries molecule | part << 24 (molecule < 2^24,
 * part 0 .. 254; -1 = padding) in EIGHT queues of nwork / 8 entries each, one per XCD (workgroup b takes entry b / 8 of
 * queue b mod 8: the items of one molecule, which read each other's filter rows, share an L2), largest molecules first
 * within a queue.  A molecule of n atoms has geossl_aggregate_parts(n) entries
 * (1, 2 or 4 up to 33 atoms: the 27..33-atom molecules are shared by that many waves, one group of target atoms each; n
 * above 33 atoms - Molecule3D with hydrogens, datasets_Molecule3D.py:65 - where a wave sums ONE target atom without a
 * size class) - every sum is still formed by one wave in the order of geossl_cfconv_aggregate, bit for bit.
 * max_n <= 255, 32 < F <= 128.                                                                                      */
int geossl_aggregate_parts(int n);
/* ... and with ONE work item per target atom for every molecule (work[i] = molecule | target << 24, all atoms of the
 * launch): small batches, where a launch is bound by its longest walk (a chain of memory round trips) and not by
 * bytes - every filter row is read by both of its atoms.  Same sums, bit for bit.                                      */
int geossl_cfconv_aggregate_targets_dyn(const float* x, const float* Wf, const uint8_t* pair_flag, const int32_t* mol_ptr,
                                        const int32_t* pair_ptr, const int32_t* work, int64_t nwork, int max_n, int F,
                                        int swap, float* out, const int32_t* dyn_nwork, hipStream_t stream);
int geossl_cfconv_aggregate_work(const float* x, const float* Wf, const uint8_t* pair_flag, const int32_t* mol_ptr,
                                 const int32_t* pair_ptr, const int32_t* work, int64_t nwork, int max_n, int F,
                                 int swap, float* out, hipStream_t stream);

/* Gradient of geossl_cfconv_aggregate with respect to the filter rows, as a tensor:
 * out[p][c] = f0 a[i][c] b[j][c] + f1 a[j][c] b[i][c] for pair slot p = (i < j) with edge flags f0 (j -> i), f1 (i -> j)
 * (exchanged when swap = 1).  The first-order path never materialises it (geossl_cfconv_filter_bwd); the second-order
 * path (training on forces, finetune_md17.py:46-54) keeps it differentiable.                                      */
int geossl_pair_product(const float* a, const float* b, const int32_t* pair_i, const int32_t* pair_j,
                        const uint8_t* pair_flag, int64_t P, int F, int swap, float* out, hipStream_t stream);

/* ---- atom-row Linear — ATen Linear at schnet.py:99,101,166,189,191 and its autograd.
 * Y[r][n] = epi(sum_k X[r][k] * Bm[k][n]); transB=1: W is torch layout [NO][K] (forward);
 * transB=0: W is [K][NO] (backward w.r.t. input: dX = dY W).  K % 8 == 0, K,NO <= 256.  ldx / ldy: row strides of
 * X and of Y (res and tprev share ldy), so column slices of wider tensors can be read / written in place.
 * R > INT_MAX is refused (hipErrorInvalidValue, nothing launched): the kernels count rows in 32 bits.        */
int geossl_linear(const float* X, int ldx, const float* W, const float* bias, const float* res, const float* tprev,
                  float* Y, int ldy, int64_t R, int K, int NO, int transB, int flags, hipStream_t stream);

/* Prepared weights.  geossl_linear re-shapes W into its MFMA operand image (bf16 pieces in fragment order) in every
 * block of every launch; a weight that is used by several launches between two optimiser steps (forward, backward,
 * both views) can be converted once instead: geossl_linear_prepare builds the images of up to GEOSSL_PREPARE_MAX
 * weights of one shape in a single launch, geossl_linear_prepared is geossl_linear reading such an image
 * (same arithmetic, bit-identical results).  geossl_linear_image_words: size of one image in 32-bit words, 0 if the
 * shape has no prepared path (K not in {32, 64, 128}).                                                       */
#define GEOSSL_PREPARE_MAX 64 /* weights in one geossl_linear_prepare / geossl_chain_prepare launch */
typedef struct {
  const float* W[GEOSSL_PREPARE_MAX];
  uint32_t* image[GEOSSL_PREPARE_MAX];
  int ldw[GEOSSL_PREPARE_MAX]; /* row stride of W in floats (a multiple of 4), 0 = dense; geossl_chain_prepare only: a column
                             block of a wider weight (PaiNN's Dense(2F, F), painn.py:87) is converted where it lies */
  int tb[GEOSSL_PREPARE_MAX];  /* geossl_chain_prepare only: 0 = the call's transB, 1 = transB 1, 2 = transB 0 for this weight
                                  (the forward and the backward image of a weight from one launch) */
} GeosslPrepareBatch;
int64_t geossl_linear_image_words(int K, int NO);
int geossl_linear_prepare(const GeosslPrepareBatch* batch, int nprob, int K, int NO, int transB, hipStream_t stream);
int geossl_linear_prepared(const float* X, int ldx, const uint32_t* image, const float* bias, const float* res,
                           const float* tprev, float* Y, int ldy, int64_t R, int K, int NO, int flags,
                           hipStream_t stream);

/* Chains of square atom-row Linear layers in one launch.  Between two neighbour aggregations the reference applies
 * three row-local layers back to back - conv.lin2 (schnet.py:191), act + lin + residual (:165-166,97), the next
 * block's conv.lin1 (:189); after the last block lin2, lin and the head (:99-101) - and autograd walks the same chains
 * backwards.  Stage s: Y_s = epi_s(X_s W_s^T + b_s), X_{s+1} = Y_s, with geossl_linear's epilogue (flags:
 * GEOSSL_EPI_SSP; tprev != NULL: * ssp'(tprev); res != NULL: + res) and Y_s stored to `out` when it is not NULL
 * (row stride ld, shared with res / tprev).  Every stage is F -> F, F in {32, 64, 128}.  `image`: operand image of the
 * stage's weight from geossl_chain_prepare (transB as in geossl_linear: 1 = W is [NO][K] (forward), 0 = W is [K][NO]
 * (dX = dY W)), geossl_chain_image_words(F) 32-bit words each.  The image is opaque: MFMA operand fragments of W split
 * into 16-bit pieces (F = 128: two fp16 pieces of W scaled by a power of two per 32-column output block, the four
 * exponents stored behind the fragments; F = 64 / 32: three bf16 pieces); results carry fp32-GEMM accuracy.        */
#define GEOSSL_CHAIN_MAX 5 /* F = 128; the F = 64 / 32 forms take up to 3 stages */
typedef struct {
  const uint32_t* image;
  const float* bias;  /* may be NULL */
  const float* res;   /* may be NULL */
  const float* tprev; /* may be NULL */
  float* out;         /* may be NULL: the stage's result is only consumed by the next stage */
  int ld;
  int flags;
  const float* xin;   /* GEOSSL_CHAIN_NEW_INPUT: the stage's own input rows [R][F] (row stride ldxin), else NULL */
  int ldxin;
  int pad_;
  float* out_act;     /* GEOSSL_EPI_SILU: silu of the stage's result (row stride ld), may be NULL */
} GeosslChainStage;
typedef struct {
  int nstage;
  GeosslChainStage st[GEOSSL_CHAIN_MAX];
} GeosslChain;
int64_t geossl_chain_image_words(int F);
int geossl_chain_prepare(const GeosslPrepareBatch* batch, int nprob, int F, int transB, hipStream_t stream);
int geossl_linear_chain(const float* X, int ldx, const GeosslChain* chain, int64_t R, int F, hipStream_t stream);

/* The layer loop of the SchNet backbone in one launch (schnet.py:95-101 between the filter network and the heads, and
 * its backward): a list of operations that each block of the launch applies, in order, to the rows of the molecules it
 * owns - kind 0: the chain of geossl_linear_chain over those rows (plain stages: dense [N][F] operands, at most three),
 * kind 1: geossl_cfconv_aggregate for those molecules (x = X, filter rows Wf, destination out; swap as there).  `plan`
 * [nblocks][4] int32 = {first row, end row, first molecule, end molecule} of a block (at most 96 rows; consecutive
 * blocks cover the batch).  uniform != 0: every molecule has max_n atoms.  stagger: the second half of the grid starts
 * that many sleeps late (0 = in step; for experiments).  F = 128 and uniform batches of at most 20 atoms per molecule;
 * anything else returns hipErrorInvalidValue and the caller launches the operations one by one.  Same arithmetic as
 * the separate launches: results bit-identical. */
#define GEOSSL_LOOP_MAX_OPS 14
typedef struct {
  int kind; /* 0 = chain, 1 = aggregation */
  int swap;
  const float* X;
  const float* Wf;
  float* out;
  GeosslChain chain;
} GeosslLoopOp;
int geossl_schnet_layer_loop(const GeosslLoopOp* ops, int nops, const int32_t* plan, int nblocks, const int32_t* mol_ptr,
                             const int32_t* pair_ptr, const uint8_t* pair_flag, int max_n, int uniform, int64_t N, int F,
                             int stagger, hipStream_t stream);
/* The same loop over RAGGED molecules (1 .. 33 atoms each) of a SMALL batch: block b owns `mols_per_block` (1 or 2)
 * consecutive molecules, found from mol_ptr on the device - no host plan, so the launch also serves a capacity bucket
 * (the `_dyn` section below), whose index structures are device data; every wave takes the unrolled walk of its
 * molecule's size class.  B molecules in at most 1024 blocks.  N = rows of the atom tensors (a capacity is fine: no row
 * past mol_ptr[B] is touched).  Results bit-identical to the separate launches. */
int geossl_schnet_layer_loop_ragged(const GeosslLoopOp* ops, int nops, const int32_t* mol_ptr, const int32_t* pair_ptr,
                                    const uint8_t* pair_flag, int64_t B, int mols_per_block, int64_t N, int F,
                                    hipStream_t stream);

/* batched weight gradients: dW_z[m][n] (+)= sum_r A_z[r][m]*B_z[r][n], db_z[m] (+)= sum_r A_z[r][m];
 * lda / ldb / ldw: row strides of A_z, B_z, dW_z (M, N <= 128 per problem: wider layers are tiled by the caller)  */
typedef struct {
  const float* A[GEOSSL_TN_MAX];
  const float* B[GEOSSL_TN_MAX];
  float* dW[GEOSSL_TN_MAX];
  float* db[GEOSSL_TN_MAX]; /* may be NULL */
} GeosslTnBatch;
typedef struct {
  float* out[GEOSSL_TN_MAX];
} GeosslReduceBatch;
void geossl_tn_plan(int64_t R, int nprob, int* chunk, int* nblk);
int64_t geossl_tn_workspace_floats(int64_t R, int M, int N, int nprob);
int geossl_linear_wgrad(const GeosslTnBatch* batch, int nprob, int64_t R, int M, int N, int lda, int ldb, int ldw,
                        float* workspace, int accumulate, hipStream_t stream);

/* ---- embedding — torch.nn.Embedding at schnet.py:89 (z is a strided int64 view x[:,0])                     */
int geossl_embedding_fwd(const int64_t* z, int64_t z_stride, const float* table, int num_classes, int64_t N, int F,
                         float* out, int32_t* status, hipStream_t stream);
int64_t geossl_embedding_bwd_workspace_floats(int num_classes, int F);
int geossl_embedding_bwd(const int64_t* z, int64_t z_stride, const float* dh, int num_classes, int64_t N, int F,
                         float* dtable, float* workspace, int accumulate, hipStream_t stream);

/* ---- readout — torch_scatter.scatter(h, batch, dim=0, reduce) at schnet.py:115 / painn.py:266
 * mean = sum / max(count,1).  _bwd: dh[a] = dout[batch[a]] (/count).                                          */
int geossl_segment_reduce_fwd(const float* h, const int32_t* mol_ptr, int64_t B, int F, int mean, float* out,
                              hipStream_t stream);
/* F.normalize(h, dim=-1) of the optional --normalize branch of do_DDM (pretrain_GeoSSL.py:193-195):
 * y = h / max(||h||_2, eps) per row; norm[N] (may be NULL in inference) is kept for the backward
 * dh = (g - y (g . y)) / max(||h||, eps).                                                                     */
int geossl_row_normalize_fwd(const float* h, int64_t N, int F, float eps, float* y, float* norm, hipStream_t stream);
int geossl_row_normalize_bwd(const float* g, const float* y, const float* norm, int64_t N, int F, float eps,
                             float* dh, hipStream_t stream);
int geossl_segment_reduce_bwd(const float* dout, const int32_t* mol_ptr, int64_t B, int F, int mean, float* dh,
                              int accumulate, hipStream_t stream);

/* ---- DDM pieces — examples/pretrain_GeoSSL.py:68-74,199-205 and examples/NCSN.py:183-220 ----------------- */
/* perturb (:72): out = pos + noise */
int geossl_axpy(const float* a, const float* b, float alpha, int64_t n, float* out, hipStream_t stream);
/* super-edge length (:199-205): out[s] = sqrt(sum((pos[u]-pos[v])^2)) */
int geossl_pair_distance(const float* pos, const int64_t* sei0, const int64_t* sei1, int64_t S, float* out,
                         hipStream_t stream);
/* batch.to(device)-side plumbing of a replayed step (:248): two device-to-device copies (atom types and positions of
 * the next batch into a captured graph's input buffers) as one launch; byte counts, multiples of 4 */
int geossl_copy2(void* dst0, const void* src0, int64_t bytes0, void* dst1, const void* src1, int64_t bytes1,
                 hipStream_t stream);
/* The five random draws of a DDM step (perturb :72: N(mu, sigma) per coordinate, n_pos = 3 N values; per head a noise
 * level in [0, K) per molecule NCSN.py:190 and N(0, 1) per super-edge :194) in one launch, for a caller that owns its
 * random stream (DDMTrainer with device noise): Philox4x32-10 keyed by the 64-bit *seed on the device.  The reference's
 * own loop keeps torch's calls (do_DDM: same generator, same values). */
int geossl_ddm_noise(const int64_t* seed, float mu, float sigma, int64_t n_pos, int64_t S, int64_t B, int K1, int K2,
                     float* pos_noise, int64_t* noise_level_1, float* distance_noise_1, int64_t* noise_level_2,
                     float* distance_noise_2, hipStream_t stream);
/* the same with the 64-bit Philox key passed by value (a caller that derives it on the host - from torch's generator
 * state - saves the launch that draws it on the device) */
int geossl_ddm_noise_seeded(uint64_t seed, float mu, float sigma, int64_t n_pos, int64_t S, int64_t B, int K1, int K2,
                            float* pos_noise, int64_t* noise_level_1, float* distance_noise_1, int64_t* noise_level_2,
                            float* distance_noise_2, hipStream_t stream);
/* both views at once (:68-74 and :199-205 for a fused two-view batch): pos2 [2N][3] = [pos ; pos + noise], d01 / d02 [S] =
 * super-edge lengths in the clean / perturbed view - geossl_axpy, the concatenation and two geossl_pair_distance calls
 * in one launch, same arithmetic; z2 != NULL: also z2 [2N] = the atom types z[i * z_stride] of the N atoms, twice */
int geossl_ddm_views(const float* pos, const float* noise, const int64_t* sei0, const int64_t* sei1, int64_t N, int64_t S,
                     float* pos2, float* d01, float* d02, const int64_t* z, int64_t z_stride, int64_t* z2,
                     hipStream_t stream);
/* per-batch bookkeeping for the NCSN head: se_ptr[B+1] = first super-edge of every molecule (needs
 * batch[sei0] non-decreasing and both ends in one molecule: true for collated batches),
 * stats = {max(edge2graph)+1 (the divisor of NCSN.py:212), 1 if the ordering assumption fails}; and the
 * atom -> incident (super-)edge lists (inc_ptr from an exclusive scan of inc_cnt by the caller); sides bit0 /
 * bit1 select matches on row 0 / row 1 of the index (3 = both, the NCSN case; 1 or 2 = PaiNN's per-target /
 * per-source edge lists).                                                                                     */
int geossl_super_edge_ptr(const int64_t* batch, const int64_t* sei0, const int64_t* sei1, int64_t S, int64_t B,
                          int32_t* se_ptr, int64_t* stats, hipStream_t stream);
int geossl_incidence_count(const int64_t* batch, const int64_t* sei0, const int64_t* sei1, const int32_t* se_ptr,
                           int64_t N, int sides, int32_t* inc_cnt, hipStream_t stream);
int geossl_incidence_fill(const int64_t* batch, const int64_t* sei0, const int64_t* sei1, const int32_t* se_ptr,
                          int64_t N, int sides, const int64_t* inc_ptr, int32_t* inc_idx, hipStream_t stream);

typedef struct {
  const float* in_w1; /* input_distance_mlp.layers.0.weight [F][1] */
  const float* in_b1; /* [F] */
  const float* in_w2; /* input_distance_mlp.layers.1.weight [1][F] */
  const float* in_b2; /* [1] */
  const float* o1_w;  /* output_mlp.layers.0.weight [F][F+1] */
  const float* o1_b;  /* [F] */
  const float* o2_w;  /* output_mlp.layers.1.weight [F/2][F] */
  const float* o2_b;  /* [F/2] */
  const float* o3_w;  /* output_mlp.layers.2.weight [1][F/2] */
  const float* o3_b;  /* [1] */
  const float* sigmas; /* [K] */
} GeosslNcsnWeights;
typedef struct {
  float* in_w1; float* in_b1; float* in_w2; float* in_b2;
  float* o1_w; float* o1_b; float* o2_w; float* o2_b; float* o3_w; float* o3_b;
} GeosslNcsnGrads;
/* Saved per-row state of the head (training): a1 [S][F], a2 [S][F/2] (post-relu), pd[S] (perturbed distance),
 * emb[S], gscale[S] = d loss_e / d(output_mlp out).                                                         */
typedef struct {
  float* a1; float* a2; float* pd; float* emb; float* gscale;
} GeosslNcsnSaved;
/* K5 forward: loss_e[S] (NCSN.py:209) from node features h [N][F], distances d[S], the two random draws
 * noise_level[B] (i64, :190) and distance_noise[S] (:194) given as inputs.                                   */
/* workspace (GEOSSL_LOSS_PARTIALS floats, may be NULL): receives one partial sum of loss_e per block of the launch, zeros
 * behind them - geossl_loss_reduce_partials finishes the sum without another pass over loss_e */
int64_t geossl_ddm_loss_fwd_workspace_floats(int F);
int geossl_ddm_loss_fwd(const float* h, const int64_t* batch, const int64_t* sei0, const int64_t* sei1, int64_t S,
                        const float* distance, const int64_t* noise_level, const float* distance_noise,
                        const GeosslNcsnWeights* w, int F, float anneal_power, float* loss_e,
                        const GeosslNcsnSaved* saved, float* workspace, hipStream_t stream);
/* loss = sum_s loss_e[s] / divisor (NCSN.py:210-212), fixed-order two-stage sum; out_scale multiplies the result
 * (0.5 for the (l1+l2)/2 of pretrain_GeoSSL.py:210) and accumulate adds to *loss.                            */
int64_t geossl_loss_reduce_workspace_floats(int64_t S);
int geossl_loss_reduce(const float* loss_e, int64_t S, const int64_t* stats_divisor, float out_scale, float* loss,
                       float* workspace, int accumulate, hipStream_t stream);
/* The two heads of a DDM step (pretrain_GeoSSL.py:207-208: same super-edges, each head its own view, weights and noise)
 * in the SAME launches - at the reference's batch size one head's row pass fills a quarter of the chip.
 * geossl_ddm_loss_fwd2: both row passes (workspace as in geossl_ddm_loss_fwd); geossl_loss_reduce_partials2: loss =
 * scale0 * mean_0 + scale1 * mean_1 from the two workspaces; geossl_ddm_loss_bwd_fused2: both one-pass backwards, their
 * reductions, and dh of both heads (geossl_incidence_gather) - 3 launches where the single-head calls make 8. */
typedef struct {
  const float* h;              /* [N][F] node features of the head's view */
  const float* distance;       /* [S] */
  const int64_t* noise_level;  /* [B] */
  const float* distance_noise; /* [S] */
  GeosslNcsnWeights w;
  GeosslNcsnSaved saved;       /* all NULL: nothing kept for a backward */
  float anneal_power;
  float pad_;
  float* loss_e;               /* [S] */
  float* workspace;            /* GEOSSL_LOSS_PARTIALS floats */
} GeosslNcsnHeadFwd;
typedef struct {
  const float* h;
  GeosslNcsnWeights w;
  GeosslNcsnSaved saved;
  float out_scale;
  float pad_;
  float* dfeat;                /* [S][F] */
  float* demb;                 /* [S] */
  float* grow;                 /* [S] */
  GeosslNcsnGrads grads;
  float* workspace;            /* geossl_ddm_loss_bwd_fused_workspace_floats(S, F) */
  float* dh;                   /* [N][F], may be NULL */
} GeosslNcsnHeadBwd;
int geossl_ddm_loss_fwd2(const GeosslNcsnHeadFwd* heads, const int64_t* batch, const int64_t* sei0, const int64_t* sei1,
                         int64_t S, int F, hipStream_t stream);
int geossl_loss_reduce_partials2(const float* partial0, const float* partial1, const int64_t* stats_divisor, float scale0,
                                 float scale1, float* loss, hipStream_t stream);
int geossl_ddm_loss_bwd_fused2(const GeosslNcsnHeadBwd* heads, const int64_t* sei0, const int64_t* sei1, int64_t S,
                               int64_t N, int F, const int64_t* stats_divisor, const float* gout, const int64_t* inc_ptr,
                               const int32_t* inc_idx, int accumulate, hipStream_t stream);
/* the same loss from the block partials geossl_ddm_loss_fwd left in its workspace (fixed order: blocks in sequence) */
int geossl_loss_reduce_partials(const float* partial, const int64_t* stats_divisor, float out_scale, float* loss,
                                int accumulate, hipStream_t stream);
/* K5 backward.  gout = upstream gradient of the head's scalar loss (device scalar, may be NULL = 1),
 * row pass: dz1 [S][F] (grad at output_mlp hidden 1 pre-activation), dfeat [S][F] (grad w.r.t. h_u + h_v),
 * demb[S]; then weight gradients; then dh[a] (+)= sum of dfeat over incident super-edges (fixed order).      */
int geossl_ddm_loss_bwd_rows(const GeosslNcsnWeights* w, const GeosslNcsnSaved* saved, int64_t S, int F,
                             const int64_t* stats_divisor, float out_scale, const float* gout, float* dz1,
                             float* dfeat, float* demb, float* grow, hipStream_t stream);
int64_t geossl_ddm_loss_bwd_workspace_floats(int64_t S, int F);
int geossl_ddm_loss_bwd_weights(const float* h, const int64_t* sei0, const int64_t* sei1, int64_t S, int F,
                                const GeosslNcsnWeights* w, const GeosslNcsnSaved* saved, const float* dz1,
                                const float* demb, const float* grow, const GeosslNcsnGrads* grads,
                                float* workspace, int accumulate, hipStream_t stream);
/* The same backward in one pass over the rows (ncsn_bwd.hip): row gradients dfeat / demb / grow AND every weight
 * gradient of the head (all members of `grads`), nothing per-row re-read and no dz1 in HBM.  h [N][F] is the head's
 * input (its rows are gathered again for the layers.0 weight gradient).                                        */
int64_t geossl_ddm_loss_bwd_fused_workspace_floats(int64_t S, int F);
int geossl_ddm_loss_bwd_fused(const float* h, const int64_t* sei0, const int64_t* sei1, int64_t S, int64_t N, int F,
                              const GeosslNcsnWeights* w, const GeosslNcsnSaved* saved, const int64_t* stats_divisor,
                              float out_scale, const float* gout, float* dfeat, float* demb, float* grow,
                              const GeosslNcsnGrads* grads, float* workspace, int accumulate, hipStream_t stream);
int geossl_incidence_gather(const float* dfeat, const int64_t* inc_ptr, const int32_t* inc_idx, int64_t N, int F,
                            float* dh, int accumulate, hipStream_t stream);

/* ---- PaiNN (BASELINE config 5) — Geom3D/models/painn.py:32-66,91-114,216-269 -------------------------------
 * idx_i / idx_j are rows 0 / 1 of radius_edge_index (int64).  Edge geometry (painn.py:232-239): dir[E][3] = r_ij/d,
 * fcut[E] = cosine cutoff * [d < cutoff] (painn_utils.py:152-154), phi[E][R] = Gaussian RBF (painn_utils.py:99-103).
 * interaction_fwd (painn.py:54-64): inc_ptr/inc_idx = edges grouped by idx_i (geossl_incidence_*, sides = 1);
 * xc = interatomic_context_net(q) [N][3F]; Wf/bf = the layer's 3F rows of filter_net; q [N][F], mu [N][3][F].
 * interaction_bwd: edges grouped by idx_j (sides = 2); returns d xc, d mu (incl. the residual) and the
 * filter_net gradient rows of the layer.  mix_* are the element-wise parts of PaiNNMixing (painn.py:100-113):
 * mm = mu_channel_mix(mu) [N][3][2F], ctx = [q, |mu_V|] [N][2F], dot = sum_xyz mu_V*mu_W, xx = context net out.  */
int geossl_painn_edge_geom(const float* pos, const int64_t* idx_i, const int64_t* idx_j, int64_t E, float cutoff,
                           const float* offsets, const float* widths, int R, float* dir, float* fcut, float* phi,
                           hipStream_t stream);
int geossl_silu_fwd(const float* u, int64_t n, float* y, hipStream_t stream);
int geossl_silu_bwd(const float* u, const float* dy, int64_t n, float* du, hipStream_t stream);
int geossl_painn_interaction_fwd(const float* q, const float* mu, const float* xc, const int64_t* idx_j,
                                 const int64_t* inc_ptr, const int32_t* inc_idx, const float* phi, const float* fcut,
                                 const float* dir, const float* Wf, const float* bf, int64_t N, int F, int R,
                                 float* q_out, float* mu_out, hipStream_t stream);
int64_t geossl_painn_interaction_bwd_workspace_floats(int64_t N, int F, int R);
int geossl_painn_interaction_bwd(const float* dq_out, const float* dmu_out, const float* mu, const float* xc,
                                 const int64_t* idx_i, const int64_t* inc_ptr, const int32_t* inc_idx, const float* phi,
                                 const float* fcut, const float* dir, const float* Wf, const float* bf, int64_t N, int F,
                                 int R, float* dxc, float* dmu_in, float* dWf, float* dbf, float* workspace,
                                 int accumulate, hipStream_t stream);
/* The forward pass with the filter on the matrix pipe (F = 128, n_rbf in {8, 16, 20}): W = phi' Wf'^T as one small GEMM
 * per tile of 32 edge rows (the bias as a column of the contraction, the cutoff applied to the product as in the
 * reference, Geom3D/models/painn.py:54-58), the message arithmetic (:59-64) on the vector unit, a team
 * of four waves per molecule.  Rows are laid out in groups of four that share their target atom (the edges of an atom
 * in incidence order, padded to a multiple of four): row_edge [4 G] int32 (-1 = padding), grp_atom [G] int32 =
 * 2 * atom + (the group is the last one of its atom), mol_grp [B + 1] int32 = first group of a molecule; an atom
 * without edges has one group of padding rows.  Same sums as geossl_painn_interaction_fwd in another (fixed) order.
 * mu == NULL (round 6): mu is identically zero - the FIRST interaction (painn.py:249) - no row of it is staged or gathered;
 * likewise geossl_painn_interaction_bwd_mol[_skip] with mu == NULL and dmu_in == NULL (both or neither): the dmumu third of
 * the filter is not evaluated, its outputs are the exact zeros the general form computes, dmu_in is not written. */
int geossl_painn_interaction_fwd_mma(const float* q, const float* mu, const float* xc, const int64_t* idx_j,
                                     const int32_t* row_edge, const int32_t* grp_atom, const int32_t* mol_grp,
                                     const float* phi, const float* fcut, const float* dir, const float* Wf,
                                     const float* bf, const int32_t* mol_ptr, int64_t B, int max_n, int64_t N, int F, int R,
                                     float* q_out, float* mu_out, hipStream_t stream);
/* The same two passes with the molecule layout (mol_ptr [B+1] int32, max_n atoms in the largest molecule): one block
 * per molecule, the rows every edge of the molecule reads staged in LDS once (results identical bit for bit; falls back
 * to the per-atom kernels when F is not 64 / 128 or a molecule's rows do not fit the LDS).                      */
int geossl_painn_interaction_fwd_mol(const float* q, const float* mu, const float* xc, const int64_t* idx_j,
                                     const int64_t* inc_ptr, const int32_t* inc_idx, const float* phi, const float* fcut,
                                     const float* dir, const float* Wf, const float* bf, const int32_t* mol_ptr,
                                     int64_t B, int max_n, int64_t N, int F, int R, float* q_out, float* mu_out,
                                     hipStream_t stream);
int64_t geossl_painn_interaction_bwd_mol_workspace_floats(int64_t N, int64_t B, int F, int R);
int geossl_painn_interaction_bwd_mol(const float* dq_out, const float* dmu_out, const float* mu, const float* xc,
                                     const int64_t* idx_i, const int64_t* inc_ptr, const int32_t* inc_idx,
                                     const float* phi, const float* fcut, const float* dir, const float* Wf,
                                     const float* bf, const int32_t* mol_ptr, int64_t B, int max_n, int64_t N, int F,
                                     int R, float* dxc, float* dmu_in, float* dWf, float* dbf, float* workspace,
                                     int accumulate, hipStream_t stream);
int geossl_painn_mix_pre_fwd(const float* q, const float* mm, int64_t N, int F, float eps, float* ctx, float* dot,
                             hipStream_t stream);
/* mu_out == NULL (mix_post_fwd) / dmu_new == NULL (mix_post_bwd): the LAST block of the backbone - its mu' is nobody's
 * input (the representation is q, painn.py:262-269), so it is not formed and its gradient is the zero it is. */
int geossl_painn_mix_post_fwd(const float* q, const float* mu, const float* mm, const float* xx, const float* dot,
                              int64_t N, int F, float* q_out, float* mu_out, hipStream_t stream);
int geossl_painn_mix_post_bwd(const float* dq_new, const float* dmu_new, const float* mm, const float* xx,
                              const float* dot, int64_t N, int F, float* dxx, float* dmm, hipStream_t stream);
int geossl_painn_mix_pre_bwd(const float* dq_new, const float* dctx, const float* ctx, const float* mm, int64_t N, int F,
                             float* dq_in, float* dmm, hipStream_t stream);
int geossl_add(const float* a, const float* b, int64_t n, float* out, hipStream_t stream);

/* ---- PaiNN position gradient, first order — examples/finetune_md17.py:46 (grad(energy, positions)) through
 * Geom3D/models/painn.py:232-241,54-64.  edge_grads (one call per interaction block, in the backward's order, the first
 * with accumulate = 0): dphi [E][R], dfcut [E], ddir [E][3] += the block's dL/d(phi, fcut, dir) given the gradient at
 * the block's output (dq_out [N][F], dmu_out [N][3][F]), its inputs mu [N][3][F], xc [N][3F] and its filter_net rows
 * Wf [3F][R] / bf [3F].  edge_geom_bwd: dr [E][3] = dL/d r_ij (r_ij = pos[idx_i] - pos[idx_j]).  position_grad:
 * dpos [N][3] = sum of dr over the edges by idx_i minus the sum over the edges by idx_j (the two incidence lists of
 * geossl_incidence_*, sides = 1 and 2), fixed order. */
int geossl_painn_edge_grads(const float* dq_out, const float* dmu_out, const float* mu, const float* xc,
                            const int64_t* idx_i, const int64_t* idx_j, const float* phi, const float* fcut,
                            const float* dir, const float* Wf, const float* bf, int64_t E, int F, int R, float* dphi,
                            float* dfcut, float* ddir, int accumulate, hipStream_t stream);
int geossl_painn_edge_geom_bwd(const float* pos, const int64_t* idx_i, const int64_t* idx_j, int64_t E, float cutoff,
                               const float* offsets, const float* widths, int R, const float* dphi, const float* dfcut,
                               const float* ddir, float* dr, hipStream_t stream);
int geossl_painn_position_grad(const float* dr, const int64_t* inc_i_ptr, const int32_t* inc_i_idx,
                               const int64_t* inc_j_ptr, const int32_t* inc_j_idx, int64_t N, float* dpos,
                               hipStream_t stream);

/* ---- Adam — torch.optim.Adam step at pretrain_GeoSSL.py:258-260,343 over one flat fp32 buffer
 * (amsgrad off; weight_decay added to the gradient as torch does).  step_count is the 1-based step.  The
 * hyperparameters are the DOUBLES Python holds: torch forms 1 - beta, lr / bias_correction1 and sqrt(bias_correction2) in
 * double and rounds once; the update is torch's default (foreach) device arithmetic bit for bit
 * (tools/probes/adam_probe.hip).                                                                              */
int geossl_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                     double beta1, double beta2, double eps, double weight_decay, int64_t step_count, float grad_scale,
                     hipStream_t stream);

/* ---- Capacity launches: the `_dyn` entry points --------------------------------------------------------------------
 * The reference's loader is DataLoaderAtomTuple(dataset, batch_size, shuffle=True) over ragged molecules
 * (examples/pretrain_GeoSSL.py:301, Geom3D/dataloaders/dataloaders_AtomTuple.py:81-88): the atom, pair-slot and
 * super-edge counts of a batch change every step, while a captured HIP graph fixes every launch's grid and by-value
 * arguments.  A `_dyn` entry point is its namesake with the row count(s) ALSO readable from device memory: the by-value
 * count is the CAPACITY (it sizes the grid, the workspaces and the layer stride of [L][P][F] tensors), `dyn_*` (nullable;
 * NULL = the namesake's behaviour) points at an int32 holding the batch's real count, written before the launch reaches
 * the stream.  Rows at and past the real count do not exist: never read, never written; their blocks leave zero partial
 * sums.  Real counts must be >= 1.  The index structures a launch walks (mol_ptr, pair_ptr, work lists, incidence lists,
 * super_edge_index) are device data anyway.  geossl_amd.pretrain_GeoSSL.StepGraphs replays ONE graph per
 * (molecules per batch, capacity) on batches of any size sequence this way.
 *
 * dyn_view (the two NCSN entry points): both heads were handed the base address of ONE [view 0 ; view 1] feature /
 * gradient tensor; head 1's rows start *dyn_view rows (the real atom count of a view) behind head 0's.            */
#define GEOSSL_COPY_MAX 8
typedef struct GeosslCopyBatch {
  void* dst[GEOSSL_COPY_MAX];
  const void* src[GEOSSL_COPY_MAX];
  int64_t bytes[GEOSSL_COPY_MAX]; /* multiples of 4; buffers 4-byte aligned; src[i] == NULL: dst[i] is filled with zeros */
} GeosslCopyBatch;
/* batch.to(device) into the static inputs of a replayed graph (:248): n <= GEOSSL_COPY_MAX device copies, one launch */
int geossl_copy_n(const GeosslCopyBatch* batch, int n, hipStream_t stream);
/* perturb + both views + both super-edge length sets (:68-74,199-205); view 1 starts at row *dyn_N of pos2 / z2 */
int geossl_ddm_views_dyn(const float* pos, const float* noise, const int64_t* sei0, const int64_t* sei1, int64_t N,
                         int64_t S, float* pos2, float* d01, float* d02, const int64_t* z, int64_t z_stride, int64_t* z2,
                         const int32_t* dyn_N, const int32_t* dyn_S, hipStream_t stream);
int geossl_embedding_fwd_dyn(const int64_t* z, int64_t z_stride, const float* table, int num_classes, int64_t N, int F,
                             float* out, int32_t* status, const int32_t* dyn_N, hipStream_t stream);
int geossl_embedding_bwd_dyn(const int64_t* z, int64_t z_stride, const float* dh, int num_classes, int64_t N, int F,
                             float* dtable, float* workspace, int accumulate, const int32_t* dyn_N, hipStream_t stream);
int geossl_cfconv_filter_fwd_dyn(const float* pair_d, const float* pair_c, int64_t P, const GeosslFilterWeights* w, int L,
                                 int F, int G, const float* offset, float coeff, float* T, float* Wf,
                                 const int32_t* dyn_P, hipStream_t stream);
int geossl_cfconv_filter_bwd_dyn(const float* pair_d, const float* pair_c, const uint8_t* pair_flag,
                                 const int32_t* pair_i, const int32_t* pair_j, int64_t P, int64_t N,
                                 const GeosslFilterWeights* w, const GeosslFilterGradIn* g, int L, int F, int G,
                                 const float* offset, float coeff, const float* T, const GeosslFilterGradOut* out,
                                 float* workspace, int accumulate, const int32_t* dyn_P, const int32_t* dyn_N,
                                 hipStream_t stream);
/* The Gaussian-smearing fragments of the filter backward's dW1 product as a per-step image (csrc/rbf_frag.h): for every
 * 32-row tile of the pair list the words the kernel otherwise builds in LDS for every layer again -
 * [tile][gb 2][ks 2][piece 2][64 lanes] of 16-byte words, 8 KB per tile, geossl_rbf_fragments_bytes(P) in all.  They
 * depend on the row's distance, offset / coeff and G only.  P is the list's CAPACITY: every tile of it is written (rows at
 * and past the real count *dyn_P with the last real row's distance, as the kernel's tile build substitutes), so no
 * word of the image is ever unwritten.  geossl_cfconv_filter_bwd_frag(_dyn): geossl_cfconv_filter_bwd(_dyn) copying
 * the fragments from `image` (built from the same pair_d, P, G, offset, coeff, dyn_P) - the same bits.  The forms
 * that keep their own Gaussians (three bf16 pieces, T == NULL) ignore the image.                                   */
int64_t geossl_rbf_fragments_bytes(int64_t P);
int geossl_rbf_fragments(const float* pair_d, int64_t P, int G, const float* offset, float coeff, void* image,
                         hipStream_t stream);
int geossl_rbf_fragments_dyn(const float* pair_d, int64_t P, int G, const float* offset, float coeff, void* image,
                             const int32_t* dyn_P, hipStream_t stream);
/* (for tests) the same items in plain order, [tile][item 256][piece 2] of 16-byte words, geossl_rbf_fragments_bytes(P);
 * item it = (gb * 2 + ks) * 64 + lane sits at word (it >> 6) * 128 + piece * 64 + (it & 63) of its tile in the image */
int geossl_rbf_fragment_items(const float* pair_d, int64_t P, int G, const float* offset, float coeff, void* items,
                              const int32_t* dyn_P, hipStream_t stream);
int geossl_cfconv_filter_bwd_frag(const float* pair_d, const float* pair_c, const uint8_t* pair_flag,
                                  const int32_t* pair_i, const int32_t* pair_j, int64_t P, int64_t N,
                                  const GeosslFilterWeights* w, const GeosslFilterGradIn* g, int L, int F, int G,
                                  const float* offset, float coeff, const float* T, const GeosslFilterGradOut* out,
                                  float* workspace, int accumulate, const void* image, hipStream_t stream);
int geossl_cfconv_filter_bwd_frag_dyn(const float* pair_d, const float* pair_c, const uint8_t* pair_flag,
                                      const int32_t* pair_i, const int32_t* pair_j, int64_t P, int64_t N,
                                      const GeosslFilterWeights* w, const GeosslFilterGradIn* g, int L, int F, int G,
                                      const float* offset, float coeff, const float* T, const GeosslFilterGradOut* out,
                                      float* workspace, int accumulate, const int32_t* dyn_P, const int32_t* dyn_N,
                                      const void* image, hipStream_t stream);
/* work items [0, *dyn_nwork) of the list */
int geossl_cfconv_aggregate_work_dyn(const float* x, const float* Wf, const uint8_t* pair_flag, const int32_t* mol_ptr,
                                     const int32_t* pair_ptr, const int32_t* work, int64_t nwork, int max_n, int F,
                                     int swap, float* out, const int32_t* dyn_nwork, hipStream_t stream);
/* F = 128 (the weight-stationary chain kernel) only */
int geossl_linear_chain_dyn(const float* X, int ldx, const GeosslChain* chain, int64_t R, int F, const int32_t* dyn_R,
                            hipStream_t stream);
int geossl_linear_wgrad_dyn(const GeosslTnBatch* batch, int nprob, int64_t R, int M, int N, int lda, int ldb, int ldw,
                            float* workspace, int accumulate, const int32_t* dyn_R, hipStream_t stream);
int geossl_ddm_loss_fwd2_dyn(const GeosslNcsnHeadFwd* heads, const int64_t* batch, const int64_t* sei0,
                             const int64_t* sei1, int64_t S, int F, const int32_t* dyn_S, const int32_t* dyn_view,
                             hipStream_t stream);
int geossl_ddm_loss_bwd_fused2_dyn(const GeosslNcsnHeadBwd* heads, const int64_t* sei0, const int64_t* sei1, int64_t S,
                                   int64_t N, int F, const int64_t* stats_divisor, const float* gout,
                                   const int64_t* inc_ptr, const int32_t* inc_idx, int accumulate, const int32_t* dyn_S,
                                   const int32_t* dyn_view, hipStream_t stream);

/* ---- PaiNN on a capacity bucket (round 5): the precomputed radius_edge_index of a batch is geometry-dependent
 * (datasets_3D_Radius.py:120), so a replayed PaiNN step reads every edge structure from static buffers that ONE launch
 * rewrites per step.
 * geossl_painn_edge_layout: from the collated one-view edge list (rows src_i = radius_edge_index[0], src_j = [1], E edges
 * grouped by molecule in batch order, both ends in one molecule; dataloaders_AtomTuple.py:64-65) and the one-view
 * molecule CSR (mol_ptr [B + 1], N atoms) to the structures of the fused (clean | perturbed) 2B-molecule batch - the
 * perturbed view keeps the clean view's graph (pretrain_GeoSSL.py:190-191), its atoms start at N, its edges at E:
 *   idx_i2 / idx_j2 [2E]; incidence lists by idx_i (iptr_i [N2cap + 1], ilist_i [2E]) and by idx_j, an atom's edges in
 *   ascending edge order; atoms [2N, N2cap] get empty lists; the four-row group layout of the matrix-pipe forward
 *   (row_edge [4 G], grp_atom [G], G = geossl_painn_group_capacity(2 E_cap, N2cap)) with the groups of molecule m in
 *   [mol_grp[m], mol_grp_end[m]); *status is set to 1 on an edge that leaves its molecule (or a molecule above 256
 *   atoms) - such edges are left out.  Molecules of at most 256 atoms.
 * geossl_painn_edge_layout_dyn: the namesake with the edge count read from device memory (*dyn_E, one view's edges; a
 *   masked batch of a device-resident dataset, whose surviving edges are counted on the device:
 *   geossl_masked_edge_offsets): the same kernel body - the offset of view 1, the end 2E of the lists, mol_grp[2B], the
 *   bound of the search for a molecule's edge range and the check that the molecules' ranges tile [0, E) all use the
 *   device value - with outputs sized for E_cap edges per view.  The host-side range check is on E_cap; *dyn_E outside
 *   [0, E_cap] is clamped into it and sets *status.  Given the same E through memory it writes what the by-value entry
 *   point writes, bit for bit.
 * geossl_painn_interaction_fwd_mma_dyn: the namesake with mol_grp_end (NULL: groups lie back to back).
 * The element-wise launches take the real row / edge count from device memory like the other `_dyn` entry points.   */
int64_t geossl_painn_group_capacity(int64_t E2, int64_t N2);
int geossl_painn_edge_layout(const int64_t* src_i, const int64_t* src_j, int64_t E, const int32_t* mol_ptr, int64_t N,
                             int64_t B, int64_t N2cap, int64_t* idx_i2, int64_t* idx_j2, int64_t* iptr_i,
                             int32_t* ilist_i, int64_t* iptr_j, int32_t* ilist_j, int32_t* row_edge, int32_t* grp_atom,
                             int32_t* mol_grp, int32_t* mol_grp_end, int32_t* status, hipStream_t stream);
int geossl_painn_edge_layout_dyn(const int64_t* src_i, const int64_t* src_j, int64_t E_cap, const int32_t* dyn_E,
                                 const int32_t* mol_ptr, int64_t N, int64_t B, int64_t N2cap, int64_t* idx_i2,
                                 int64_t* idx_j2, int64_t* iptr_i, int32_t* ilist_i, int64_t* iptr_j, int32_t* ilist_j,
                                 int32_t* row_edge, int32_t* grp_atom, int32_t* mol_grp, int32_t* mol_grp_end,
                                 int32_t* status, hipStream_t stream);
int geossl_painn_edge_geom_dyn(const float* pos, const int64_t* idx_i, const int64_t* idx_j, int64_t E, float cutoff,
                               const float* offsets, const float* widths, int R, float* dir, float* fcut, float* phi,
                               const int32_t* dyn_E, hipStream_t stream);
int geossl_painn_interaction_fwd_mma_dyn(const float* q, const float* mu, const float* xc, const int64_t* idx_j,
                                         const int32_t* row_edge, const int32_t* grp_atom, const int32_t* mol_grp,
                                         const float* phi, const float* fcut, const float* dir, const float* Wf,
                                         const float* bf, const int32_t* mol_ptr, int64_t B, int max_n, int64_t N, int F,
                                         int R, float* q_out, float* mu_out, const int32_t* mol_grp_end,
                                         hipStream_t stream);
/* Molecules above the LDS rows of a molecule-staged interaction launch (geossl_painn_stage_cap: kind 0 = matrix-pipe
 * forward, 1 = vector forward, 2 = backward; atoms) - Molecule3D with hydrogens has them - no longer send the whole
 * batch to the per-atom kernels: geossl_painn_interaction_fwd_mma_dyn and geossl_painn_interaction_bwd_mol_skip SKIP
 * such molecules, and the per-atom kernels cover a LIST of atoms (min(nlist, *dyn_nlist) entries of atom_list; the
 * backward with accumulate = 1 adds its filter-gradient partials to what the molecule-staged launch left in dWf / dbf;
 * workspace: geossl_painn_interaction_bwd_workspace_floats(nlist, F, R)).                                              */
int geossl_painn_stage_cap(int kind, int F, int R);
int geossl_painn_interaction_fwd_atoms(const float* q, const float* mu, const float* xc, const int64_t* idx_j,
                                       const int64_t* inc_ptr, const int32_t* inc_idx, const float* phi,
                                       const float* fcut, const float* dir, const float* Wf, const float* bf,
                                       const int32_t* atom_list, int64_t nlist, const int32_t* dyn_nlist, int F, int R,
                                       float* q_out, float* mu_out, hipStream_t stream);
int geossl_painn_interaction_bwd_atoms(const float* dq_out, const float* dmu_out, const float* mu, const float* xc,
                                       const int64_t* idx_i, const int64_t* inc_ptr, const int32_t* inc_idx,
                                       const float* phi, const float* fcut, const float* dir, const float* Wf,
                                       const float* bf, const int32_t* atom_list, int64_t nlist,
                                       const int32_t* dyn_nlist, int F, int R, float* dxc, float* dmu_in, float* dWf,
                                       float* dbf, float* workspace, int accumulate, hipStream_t stream);
int geossl_painn_interaction_bwd_mol_skip(const float* dq_out, const float* dmu_out, const float* mu, const float* xc,
                                          const int64_t* idx_i, const int64_t* inc_ptr, const int32_t* inc_idx,
                                          const float* phi, const float* fcut, const float* dir, const float* Wf,
                                          const float* bf, const int32_t* mol_ptr, int64_t B, int max_n, int64_t N, int F,
                                          int R, float* dxc, float* dmu_in, float* dWf, float* dbf, float* workspace,
                                          int accumulate, hipStream_t stream);
int geossl_painn_mix_pre_fwd_dyn(const float* q, const float* mm, int64_t N, int F, float eps, float* ctx, float* dot,
                                 const int32_t* dyn_N, hipStream_t stream);
int geossl_painn_mix_post_fwd_dyn(const float* q, const float* mu, const float* mm, const float* xx, const float* dot,
                                  int64_t N, int F, float* q_out, float* mu_out, const int32_t* dyn_N,
                                  hipStream_t stream);
int geossl_painn_mix_post_bwd_dyn(const float* dq_new, const float* dmu_new, const float* mm, const float* xx,
                                  const float* dot, int64_t N, int F, float* dxx, float* dmm, const int32_t* dyn_N,
                                  hipStream_t stream);
int geossl_painn_mix_pre_bwd_dyn(const float* dq_new, const float* dctx, const float* ctx, const float* mm, int64_t N,
                                 int F, float* dq_in, float* dmm, const int32_t* dyn_N, hipStream_t stream);

/* ---- PaiNN interaction on atom tiles (painn_tile.hip): structures of hundreds of atoms -------------------------------
 * The filter on the matrix pipe with no molecule in LDS: an atom's incidence list is walked in tiles of 32 rows (one
 * MFMA tile), the rows of the atoms at the other end come from L2.  F = 128, R in {8, 16, 20} (geossl_painn_tile_ok;
 * anything else: hipErrorInvalidValue).  The argument lists are those of geossl_painn_interaction_fwd_atoms /
 * _bwd_atoms, with two extensions: atom_list == NULL means atoms 0 .. nlist-1, and mu == NULL means mu is identically
 * zero (the first interaction: no mu rows are gathered; the backward then requires dmu_in == NULL).  min(nlist,
 * *dyn_nlist) entries are real when dyn_nlist is given; the grid depends on nlist alone.  Bit-reproducible, and an
 * atom's outputs do not depend on its place in the list.  The backward leaves one filter-gradient partial per block
 * in `workspace` (geossl_painn_interaction_bwd_tile_workspace_floats(nlist, F, R)) and sums them in block order into
 * dWf / dbf (accumulate = 1: onto what is there).                                                                        */
int geossl_painn_tile_ok(int F, int R);
int geossl_painn_interaction_fwd_tile(const float* q, const float* mu, const float* xc, const int64_t* idx_j,
                                      const int64_t* inc_ptr, const int32_t* inc_idx, const float* phi,
                                      const float* fcut, const float* dir, const float* Wf, const float* bf,
                                      const int32_t* atom_list, int64_t nlist, const int32_t* dyn_nlist, int F, int R,
                                      float* q_out, float* mu_out, hipStream_t stream);
int64_t geossl_painn_interaction_bwd_tile_workspace_floats(int64_t nlist, int F, int R);
int geossl_painn_interaction_bwd_tile(const float* dq_out, const float* dmu_out, const float* mu, const float* xc,
                                      const int64_t* idx_i, const int64_t* inc_ptr, const int32_t* inc_idx,
                                      const float* phi, const float* fcut, const float* dir, const float* Wf,
                                      const float* bf, const int32_t* atom_list, int64_t nlist,
                                      const int32_t* dyn_nlist, int F, int R, float* dxc, float* dmu_in, float* dWf,
                                      float* dbf, float* workspace, int accumulate, hipStream_t stream);

/* ---- Incidence lists of a collated edge list, structures of up to 1024 atoms (painn_inc.hip) -------------------------
 * What the atom-tile kernels above read as inc_ptr / inc_idx, for both sides, in ONE launch whose grid depends on
 * (N, B, max_n) alone - what layout.EdgeLayout builds with five launches, two torch cumsums and a read-back per batch
 * object.
 * From the one-view edge list (rows src_i = radius_edge_index[0], src_j = [1], E edges grouped by structure in batch
 * order, both ends in one structure) and the structure CSR (mol_ptr [B + 1], N atoms): iptr_i [N + 1] / ilist_i [E] =
 * the edges by src_i, iptr_j / ilist_j = by src_j, an atom's edges in ascending edge order.  No two-view copies, no
 * group layout.  max_n: the largest structure as a HOST integer (1 .. GEOSSL_PAINN_INC_MAX_N; anything else, E or N
 * above INT_MAX: hipErrorInvalidValue) - the host cannot see mol_ptr, so it sizes the grid by max_n and refuses by it;
 * a structure that has more atoms all the same gets no edges and sets *status.
 * *status is set to 1 (never reset) on an edge that leaves its structure, on a list that is not grouped by structure
 * in batch order and on a mol_ptr that does not end at N.  Such edges are left out; the lists are then not to be used
 * (the slots left free hold an edge id of the same structure, so a kernel queued before the status is read stays inside
 * the edge arrays).  Integer work only, bit-reproducible.
 * geossl_painn_incidence_layout_dyn: the namesake with both counts read from device memory, outputs sized for
 *   (E_cap, N_cap): atoms [*dyn_N, N_cap] get iptr = *dyn_E (empty lists), no list entry at or beyond *dyn_E is
 *   written; a count outside [0, capacity] is clamped into it and sets *status.  Given the same counts through memory
 *   it writes what the by-value entry writes, bit for bit.
 * `workspace`: geossl_painn_incidence_layout_workspace_bytes(E_cap, N_cap, B) bytes - 0 with the present one-launch
 *   decomposition (NULL is accepted).                                                                                  */
#define GEOSSL_PAINN_INC_MAX_N 1024
int64_t geossl_painn_incidence_layout_workspace_bytes(int64_t E_cap, int64_t N_cap, int64_t B);
int geossl_painn_incidence_layout(const int64_t* src_i, const int64_t* src_j, int64_t E, const int32_t* mol_ptr,
                                  int64_t N, int64_t B, int max_n, int64_t* iptr_i, int32_t* ilist_i, int64_t* iptr_j,
                                  int32_t* ilist_j, int32_t* status, void* workspace, hipStream_t stream);
int geossl_painn_incidence_layout_dyn(const int64_t* src_i, const int64_t* src_j, int64_t E_cap, const int32_t* dyn_E,
                                      const int32_t* mol_ptr, int64_t N_cap, int64_t B, int max_n, int64_t* iptr_i,
                                      int32_t* ilist_i, int64_t* iptr_j, int32_t* ilist_j, int32_t* status,
                                      const int32_t* dyn_N, void* workspace, hipStream_t stream);

/* ---- Second-order route (training on forces): the primitives of geossl_amd/tape.py that are not dense products --------
 * Replaces, on the route that differentiates a force again (examples/finetune_md17.py:46-54: pred_force =
 * -grad(E, pos, create_graph=True); loss.backward()), the ATen element-wise / index kernels autograd would launch for
 * Geom3D/models/schnet.py:93,186,205-207,213-216 (distance, cosine envelope, Gaussian smearing, shifted softplus) and
 * Geom3D/models/painn.py:54-64,100-113, painn_utils.py:99-103,152-154 (gathers, index_add, split / cat, the xyz
 * broadcasts).  fp32, row-major [R][D]; PaiNN's [n][3][F] is the matrix [3 n][F].  No atomics: fixed summation order.
 * geossl_tape_unary:  y = f(alpha x + beta); kind: 0 affine, 1 exp, 2 cos, 3 sin, 4 shifted softplus, 5 sigmoid,
 *   6 s(1-s), 7 s(1-s)(1-2s), 8 reciprocal, 9 sqrt, 10 silu, 11 silu', 12 silu'', 13 exp(alpha x^2), 14 and 15 its first
 *   and second derivative in x, 16 (x < alpha), 17 |t|, 18 sign(t), 19 -1/t^2, 20 2/t^3,
 *   21 t^-1/2, 22 t^-3/2.
 * geossl_tape_binary: y[r][c] = scale * (A op B), op: 0 add, 1 sub, 2 mul, 3 A alone (a broadcast written out);
 *   operand modes: 0 [R][D], 1 [R] (per row), 2 [D] (per column), 3 [R/3][D] (the row r / 3; R a multiple of 3).
 * geossl_tape_reduce: the adjoints of those broadcasts: kind 1 row sums -> [R], 2 column sums -> [D] (workspace of
 *   geossl_tape_colsum_workspace_floats(R, D) floats), 3 sums over the xyz triple -> [R/3][D].
 * geossl_tape_gather_rows: out[e] = src[idx[e]] (idx int64 when idx64, else int32); geossl_tape_scatter_rows: its
 *   adjoint over a sorted incidence list: out[n] = sum of src[perm[k]], k in [ptr[n], ptr[n+1]) in ascending k (ptr
 *   int64 when ptr64, else int32 - the incidence lists of a PaiNN edge layout are taken as they are).
 * geossl_tape_copy2d: dst[r][c] = src[r][c] for an R x C block of two row-major matrices with row strides ld_*;
 * geossl_tape_fill: dst[i] = value.                                                                                  */
int geossl_tape_unary(int kind, const float* x, int64_t n, float alpha, float beta, float* y, hipStream_t stream);
int geossl_tape_binary(int op, const float* a, int amode, const float* b, int bmode, int64_t R, int D, float scale,
                       float* y, hipStream_t stream);
int64_t geossl_tape_colsum_workspace_floats(int64_t R, int D);
int geossl_tape_reduce(int kind, const float* x, int64_t R, int D, float* y, float* workspace, hipStream_t stream);
int geossl_tape_gather_rows(const float* src, const void* idx, int idx64, int64_t E, int D, float* out,
                            hipStream_t stream);
int geossl_tape_scatter_rows(const float* src, const void* ptr, int ptr64, const int32_t* perm, int64_t N, int D,
                             float* out, hipStream_t stream);
int geossl_tape_copy2d(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int64_t R, int C,
                       hipStream_t stream);
int geossl_tape_fill(float* dst, int64_t n, float value, hipStream_t stream);

/* ---- batch assembly from a device-resident dataset (round 6) -------------------------------------------------------
 * Replaces, for molecules that already live in HBM, the per-step host collation of the reference's loader:
 * DataLoaderAtomTuple(dataset, batch_size, shuffle=True) (examples/pretrain_GeoSSL.py:295-301) ->
 * BatchAtomTuple.from_data_list (Geom3D/dataloaders/dataloaders_AtomTuple.py:46-73) over molecules that went through
 * AtomTupleExtractor (:15-37) and, for PaiNN, carry the radius_edge_index of datasets_3D_Radius.py:105-131.
 * One block per chosen molecule m (B of them, in batch order):
 *   x_dst / pos_dst rows [mol_ptr[m], mol_ptr[m+1]) = rows [src_off[m], ...) of x_src [*, x_cols] / pos_src [*, 3];
 *   batch_dst[row] = m (:61; NULL: skipped);
 *   sei0 / sei1 columns [se_ptr[m], se_ptr[m+1]) = the molecule's atom tuples + mol_ptr[m] (:64-65), option 0 =
 *     "combination" (itertools.combinations order), 1 = "permutation" (NULL: skipped);
 *   pair_i / pair_j = the pair-slot atoms of the TWO-VIEW batch (what geossl_pair_index_fill writes for the [2B+1]
 *     arrays [mol_ptr ; mol_ptr[1:] + N], pair_ptr2; N = mol_ptr[B]) (NULL: skipped);
 *   inc_idx entries [inc_ptr[a], inc_ptr[a+1]) of every atom a = its incident super-edges in ascending order (what
 *     geossl_incidence_fill(sides = 3) finds for the enumerations above) (NULL: skipped);
 *   e0_dst / e1_dst columns [e_ptr[m], e_ptr[m+1]) = columns [e_src_off[m], ...) of e0_src / e1_src with the node offset
 *     changed from src_off[m] to mol_ptr[m] (:64-65) (NULL: skipped).
 * zero (nullable): zero_count floats cleared by the same launch.  A collated batch is the special case src_off = mol_ptr.
 * Every pointer array is device memory written before the launch reaches the stream; nothing is read back.           */
typedef struct GeosslGather {
  const int64_t* x_src;
  const float* pos_src;
  const int32_t* src_off;   /* [B] */
  const int32_t* mol_ptr;   /* [B+1] */
  int64_t* x_dst;
  float* pos_dst;
  int64_t* batch_dst;
  const int32_t* se_ptr;    /* [B+1] */
  int64_t* sei0;
  int64_t* sei1;
  const int32_t* pair_ptr2; /* [2B+1] */
  int32_t* pair_i;
  int32_t* pair_j;
  const int64_t* inc_ptr;   /* [N+1] */
  int32_t* inc_idx;
  const int64_t* e0_src;
  const int64_t* e1_src;
  const int32_t* e_src_off; /* [B] */
  const int32_t* e_ptr;     /* [B+1] */
  int64_t* e0_dst;
  int64_t* e1_dst;
  float* zero;
  int64_t zero_count;
  int32_t x_cols;
  int32_t option;
} GeosslGather;
int geossl_gather_molecules(const GeosslGather* g, int64_t B, hipStream_t stream);

/* ---- masked batch assembly: BFS atom masking (Molecule3DDataset.subgraph, Geom3D/datasets/datasets_3D.py:24-67;
 * MoleculeDataset3DRadius.subgraph, datasets_3D_Radius.py:43-87).  `g` as for geossl_gather_molecules, except that
 * mol_ptr / se_ptr / pair_ptr2 / inc_ptr / e_ptr describe the MASKED molecules (k kept atoms of molecule m:
 * k = mol_ptr[m+1] - mol_ptr[m], a function of n alone: int(n (1 - ratio)) + 1) while src_off / e_src_off point at the
 * whole molecule in the dataset.  Destination row mol_ptr[m] + i reads source row src_off[m] + keep[i]; the structures
 * that depend on k only are those of a k-atom molecule; a radius edge survives when both its ends are kept, in edge
 * order, its ends renumbered by their rank among the kept atoms (torch_geometric.utils.subgraph(relabel_nodes=True)).
 * One block per molecule.  The kept list `keep` (ascending local indices) comes from keep_in, or - keep_in == NULL - is
 * drawn by the block's first wave: a BFS over the bond graph with Philox-4x32-10, key = (seed low, seed high word),
 * counter = (mol_id[m], t, 0, 0), word 0; an integer below c is (w * c) >> 32 (64-bit product).  t = 0 picks the start
 * atom below n; step t = 1 .. k-1 picks, when the frontier (bond successors of the visited atoms, minus the visited) is
 * empty, the draw(n - t)-th unvisited atom in ascending order, else the draw(|frontier|)-th frontier atom in ascending
 * order.  With e_count != NULL the launch only decides the kept lists, writes keep_out (required then) and counts the
 * surviving radius edges of every molecule into e_count - the survivor count depends on the draw, so a gather with
 * radius edges is a count launch, a read-back of B counts (the caller's e_ptr; or geossl_masked_edge_offsets, which
 * makes e_ptr on the device) and a gather launch with keep_in = the count launch's keep_out.  Refused (hipErrorInvalidValue): max_n > 2048, bond_ptr / bond_dst NULL when drawing.
 * Molecules with n > 2048 or k outside [1, n] are skipped; kept atoms of keep_in outside [0, n) read atom 0.          */
typedef struct GeosslMask {
  const int32_t* bond_ptr;  /* [Ntot+1] over DATASET atoms: the successors of atom s are bond_dst[bond_ptr[s] ..
                               bond_ptr[s+1]) (the edge_index of the molecule; no self-loops) */
  const int32_t* bond_dst;  /* local atom indices 0 .. n-1 */
  const int32_t* src_n;     /* [B] atoms of each molecule before masking */
  const int64_t* mol_id;    /* [B] dataset molecule ids (the first counter word of the draw) */
  const int32_t* keep_in;   /* [mol_ptr[B]] kept atoms, laid out by mol_ptr (NULL: drawn on the device) */
  int32_t* keep_out;        /* [mol_ptr[B]] the kept lists (NULL: not written) */
  const int32_t* e_src_cnt; /* [B] radius edges of each molecule in the dataset (with e0_src / e1_src / e_src_off) */
  int32_t* e_count;         /* [B] non-NULL: the count launch */
  uint64_t seed;
  int32_t max_n;            /* largest n of the batch */
  int32_t pad_;
} GeosslMask;
int geossl_gather_masked_molecules(const GeosslGather* g, const GeosslMask* mask, int64_t B, hipStream_t stream);

/* geossl_masked_edge_offsets: the read-back of the B counts done on the device instead (a masked PaiNN batch on a
 * capacity bucket, whose captured step reads its edge count from device memory).  From e_count [B] (the count launch's
 * survivors per molecule) one block writes e_ptr [B + 1] = their exclusive prefix (e_ptr[B] = E, the edges of one
 * view: what the gather launch takes as g->e_ptr and geossl_painn_edge_layout_dyn as dyn_E) and *dyn_E2 = views * E
 * (views 1 or 2: the edge count of the batch the backbone sees).  B is scanned in chunks of the block's threads with a
 * carry.  Every offset is clamped to E_cap, so the launches behind it stay inside buffers of that capacity; *status
 * (nullable) is set to 1 when the total exceeds E_cap or a count is negative.  Integer work, plain stores, no atomics.
 * Refused (hipErrorInvalidValue): B outside [1, 2^24], 2 E_cap >= 2^30, views other than 1 or 2, a NULL array.     */
int geossl_masked_edge_offsets(const int32_t* e_count, int64_t B, int64_t E_cap, int views, int32_t* e_ptr,
                               int32_t* dyn_E2, int32_t* status, hipStream_t stream);

/* ---- contrastive heads: pretrain_GeoSSL.py --GeoSSL_option=InfoNCE / EBM_NCE (:103-176) -----------------------------
 * X, Y [B][F]: the readouts of the two views (row-major fp32).  No atomics: the same inputs give the same bits.
 * InfoNCE (:141-176), S = X Y^T * inv_t (inv_t = 1 / args.T), loss = (CE(S, arange(B)) + CE(S^T, arange(B))) / 2:
 *   stats [5B] (out) = {max m of every row [B] and column [B], l = log1p(sum of exp(S - m) over all but the first
 *   maximum) of every row [B] and column [B], diagonal S_ii [B]}: lse = m + l; amax [2B] (out) first-index argmax of
 *   every row and column - both the backward's input; loss [1]; counts [2] = {rows with argmax i, columns with argmax
 *   j} (the reference's acc = (counts[0] / B + counts[1] / B) / 2).
 *   Backward: G = exp(S - lse_row) + exp(S - lse_col) - 2 I; dX = G Y, dY = G^T X, both * gout[0] * inv_t / (2B). */
int geossl_infonce_fwd(const float* X, const float* Y, int64_t B, int F, float inv_t, float* stats, int32_t* amax,
                       float* loss, int32_t* counts, hipStream_t stream);
int geossl_infonce_bwd(const float* X, const float* Y, const float* stats, const int32_t* amax, int64_t B, int F,
                       float inv_t, const float* gout, float* dX, float* dY, hipStream_t stream);
/* EBM-NCE (:103-138, cycle_index examples/util.py:19-22), 1 <= num_neg <= B: pred [B][1 + num_neg] (out, the backward's
 * input) = <x_i, y_i>, <x_i, y_{(i+k) mod B}> in fp32; BCEWithLogits in fp64: terms [B], hits [2B] workspaces;
 * loss [1] (double) = (mean softplus(-pos) + num_neg mean softplus(neg)) / (1 + num_neg); counts [2] = {pos > 0, neg < 0}.
 * Backward with the fp64 upstream gradient gout[0]: dpred cast to fp32, dX / dY gathered from the neighbour rows. */
int geossl_ebm_nce_fwd(const float* X, const float* Y, int64_t B, int F, int num_neg, float* pred, double* terms,
                       int32_t* hits, double* loss, int32_t* counts, hipStream_t stream);
int geossl_ebm_nce_bwd(const float* X, const float* Y, const float* pred, int64_t B, int F, int num_neg,
                       const double* gout, float* dX, float* dY, hipStream_t stream);

/* ---- distance-prediction head: examples/pretrain_DistancePrediction.py:15-25,66-79 (csrc/distance_head.hip) ----------
 * h [N][F] node features (F = 64, 128, 256 or 512: geossl_distance_head_width_ok), W [2F] = predictor.weight = [w_u | w_v],
 * bias [1], pos [N][3], super-edges (sei0[e], sei1[e]) = (u_e, v_e), e < S.  No atomics: the same inputs give the same bits.
 * Forward: proj [N][2] (out) = (w_u . h_i, w_v . h_i); pred [S] (out) = (a_{u_e} + b_{v_e}) + bias; target_e =
 *   sqrtf((dx*dx + dy*dy) + dz*dz) of pos_u - pos_v; sgn [S] (out, the backward's input) = sign(pred_e - target_e) (0 on a
 *   tie); loss [1] = mean |pred - target| (fp64 sums in a fixed order, NaN for S = 0).  workspace:
 *   geossl_distance_head_fwd_workspace_floats(S) floats, 8-byte aligned.
 * Backward with the upstream gradient gout[0]: d pred_e = (gout / S) sgn_e; dA_i / dB_i = the sums of d pred over the
 *   super-edges with u_e = i / v_e = i in ascending edge order on the atom's incidence list (inc_ptr / inc_idx of
 *   geossl_incidence_fill with sides = 3); dh [N][F] = dA_i w_u + dB_i w_v; dW [2F] (+)= [sum dA_i h_i | sum dB_i h_i],
 *   db [1] (+)= sum dA_i, from per-block partials added in block order.  accumulate: dW / db (+)= instead of =.  workspace:
 *   geossl_distance_head_bwd_workspace_floats(N, F) floats.
 * `_dyn`: N and S are capacities (grids, workspaces); dyn_N / dyn_S (nullable) point at the real counts - the mean
 *   divides by the real S, atoms and super-edges past the real counts are neither read nor written. */
int geossl_distance_head_width_ok(int F);
int64_t geossl_distance_head_fwd_workspace_floats(int64_t S);
int64_t geossl_distance_head_bwd_workspace_floats(int64_t N, int F);
int geossl_distance_head_fwd(const float* h, int64_t N, int F, const float* W, const float* bias, const float* pos,
                             const int64_t* sei0, const int64_t* sei1, int64_t S, float* proj, float* pred, float* sgn,
                             float* workspace, float* loss, hipStream_t stream);
int geossl_distance_head_fwd_dyn(const float* h, int64_t N, int F, const float* W, const float* bias, const float* pos,
                                 const int64_t* sei0, const int64_t* sei1, int64_t S, float* proj, float* pred,
                                 float* sgn, float* workspace, float* loss, const int32_t* dyn_N, const int32_t* dyn_S,
                                 hipStream_t stream);
int geossl_distance_head_bwd(const float* h, int64_t N, int F, const float* W, const int64_t* sei0, int64_t S,
                             const float* sgn, const int64_t* inc_ptr, const int32_t* inc_idx, const float* gout,
                             float* dh, float* dW, float* db, float* workspace, int accumulate, hipStream_t stream);
int geossl_distance_head_bwd_dyn(const float* h, int64_t N, int F, const float* W, const int64_t* sei0, int64_t S,
                                 const float* sgn, const int64_t* inc_ptr, const int32_t* inc_idx, const float* gout,
                                 float* dh, float* dW, float* db, float* workspace, int accumulate,
                                 const int32_t* dyn_N, const int32_t* dyn_S, hipStream_t stream);

/* ---- charge prediction: examples/pretrain_ChargePrediction.py:15-25,61-81 (csrc/charge_head.hip) ---------------------
 * Mask draw and apply (geossl_charge_mask[_dyn], one block): x [N][x_cols] int64 atom features (column 0: the type);
 * k (out, [1]) = trunc((double)N * ratio) - Python's int(M * ratio), geossl_charge_mask_count(N, ratio) on the host.
 * Exactly one of seed / given is non-NULL:
 *   seed: the k atoms are drawn on the device.  Atom i gets the 64-bit key (w0 << 32) | w1 of Philox-4x32-10 with
 *     key = (seed[0] low, seed[0] high word), counter = (i, 0, 0, 0); the k atoms with the smallest (key, i) are taken
 *     (a uniform k-subset: a radix select over the keys, equal keys by ascending i), written to idx [k] in ascending
 *     atom order; then seed[0] += 1 (a replayed graph draws a fresh mask, the same seed value the same mask).
 *   given: idx [k] = given[0 .. k) as it is (a host draw, np.random.choice(M, k, replace=False)).
 * labels [k] (out) = x[idx[j]][0] before any write (-1 for an index outside [0, N)); then x[idx[j]][0] = C - 1 (the
 * mask token) for every listed atom.  2 <= C <= 16, 0 <= ratio <= 1.
 * Head (geossl_charge_head_*): h [N][F] node features (F = 64, 128, 256 or 512 and 2 <= C <= 16:
 * geossl_charge_head_width_ok), W [C][F], bias [C], idx / labels [K] with k = k_dev[0] (NULL: k = K) real rows.
 * Forward: logits_j = h[idx_j] W^T + bias, a max-subtracted log-softmax in fp32; prob [K][C] (out) = softmax rows;
 *   loss [1] = mean_j (lse_j - logit_j[labels_j]) (fp64 sums in a fixed order; NaN for k = 0).  A row with idx outside
 *   [0, N) or a label outside [0, C) reads nothing, adds NaN, gets a zero prob row and sets bit 0 of status[0].
 *   workspace: geossl_charge_head_fwd_workspace_floats(K) floats, 8-byte aligned.
 * Backward with the upstream gradient gout[0]: d_j = (prob_j - onehot(labels_j)) (gout / k); dh [N][F] (out) = 0 on
 *   every row, d_j W on the rows idx_j (indices are distinct); dW [C][F] / db [C] (+)= sum_j d_j^T h[idx_j] / sum_j d_j
 *   from per-block partials added in block order.  accumulate: dW / db (+)= instead of =.  k = 0: all zero.
 *   workspace: geossl_charge_head_bwd_workspace_floats(K, F, C) floats.
 * `_dyn`: N is a capacity and dyn_N (nullable) points at the real atom count; with k_dev, K is a capacity too.  Rows
 *   past the real counts are neither read nor written.  No atomics beyond integer counts: the same bits every launch. */
int64_t geossl_charge_mask_count(int64_t N, double ratio);
int geossl_charge_mask(int64_t* x, int x_cols, int64_t N, double ratio, int C, int64_t* seed, const int64_t* given,
                       int64_t* idx, int64_t* labels, int32_t* k, hipStream_t stream);
int geossl_charge_mask_dyn(int64_t* x, int x_cols, int64_t N, double ratio, int C, int64_t* seed, const int64_t* given,
                           int64_t* idx, int64_t* labels, int32_t* k, const int32_t* dyn_N, hipStream_t stream);
int geossl_charge_head_width_ok(int F, int C);
int64_t geossl_charge_head_fwd_workspace_floats(int64_t K);
int64_t geossl_charge_head_bwd_workspace_floats(int64_t K, int F, int C);
int geossl_charge_head_fwd(const float* h, int64_t N, int F, const float* W, const float* bias, int C,
                           const int64_t* idx, const int64_t* labels, int64_t K, const int32_t* k_dev, float* prob,
                           float* workspace, float* loss, int32_t* status, hipStream_t stream);
int geossl_charge_head_fwd_dyn(const float* h, int64_t N, int F, const float* W, const float* bias, int C,
                               const int64_t* idx, const int64_t* labels, int64_t K, const int32_t* k_dev, float* prob,
                               float* workspace, float* loss, int32_t* status, const int32_t* dyn_N,
                               hipStream_t stream);
int geossl_charge_head_bwd(const float* h, int64_t N, int F, const float* W, int C, const int64_t* idx,
                           const int64_t* labels, int64_t K, const int32_t* k_dev, const float* prob, const float* gout,
                           float* dh, float* dW, float* db, float* workspace, int accumulate, hipStream_t stream);
int geossl_charge_head_bwd_dyn(const float* h, int64_t N, int F, const float* W, int C, const int64_t* idx,
                               const int64_t* labels, int64_t K, const int32_t* k_dev, const float* prob,
                               const float* gout, float* dh, float* dW, float* db, float* workspace, int accumulate,
                               const int32_t* dyn_N, hipStream_t stream);

/* ---- 3D InfoGraph: examples/pretrain_3DInfoGraph.py:19-31,56-76 (csrc/infograph_head.hip) ---------------------------
 * x [N][F] node features (F = 64, 128 or 256: geossl_infograph_width_ok), W [F][F] the Discriminator's weight,
 * mol_ptr [B + 1] int32 offsets of the B >= 1 molecules (atoms sorted by molecule).  readout: 0 "add", 1 "mean"
 * (sum / max(n_b, 1), the arithmetic of geossl_segment_reduce_fwd) of the rows of x, or 2: the caller's m_in [B][F]
 * (m_in non-NULL exactly for 2).
 * Forward: s [B][F] (out) = sigmoid(m), h [B][F] (out) = s W; scores [2][N] (out): pos_i = <x_i, h_b> at [i],
 *   neg_i = <x_i, h_{(b+1) mod B}> at [N + i] for atom i of molecule b; loss [1] = mean_i softplus(-pos_i) +
 *   mean_i softplus(neg_i) (BCEWithLogits against 1 and 0; fp64 sums in a fixed order, stored as fp32; no atoms: NaN);
 *   counts [2] int32 = #(pos_i > 0), #(neg_i < 0).  workspace: geossl_infograph_fwd_workspace_floats(B) floats, 8-byte
 *   aligned.
 * Backward with the upstream gradient gout[0] and c = gout[0] / N: g_pos_i = (sigmoid(pos_i) - 1) c,
 *   g_neg_i = sigmoid(neg_i) c; dh [B][F] (out) = sum_{i in b} g_pos_i x_i + sum_{i in (b-1) mod B} g_neg_i x_i;
 *   dm_b = (dh_b W^T) s_b (1 - s_b); dx [N][F] (out) = g_pos_i h_b + g_neg_i h_{(b+1) mod B} plus the readout's backward
 *   dm_b (/ max(n_b, 1) for "mean"), or, for readout 2, dm [B][F] (out; non-NULL exactly for 2) and no readout term.
 *   dW = s^T dh is left to the caller (geossl_linear_wgrad).
 * `_dyn`: N is a capacity (the row stride of scores) and dyn_N (nullable) points at the real atom count; mol_ptr holds
 *   the real offsets.  Rows past the real count are neither read nor written.  No atomics: the same bits every launch. */
int geossl_infograph_width_ok(int F);
int64_t geossl_infograph_fwd_workspace_floats(int64_t B);
int geossl_infograph_fwd(const float* x, int64_t N, int F, const float* W, const int32_t* mol_ptr, int64_t B,
                         int readout, const float* m_in, float* s, float* h, float* scores, float* workspace,
                         float* loss, int32_t* counts, hipStream_t stream);
int geossl_infograph_fwd_dyn(const float* x, int64_t N, int F, const float* W, const int32_t* mol_ptr, int64_t B,
                             int readout, const float* m_in, float* s, float* h, float* scores, float* workspace,
                             float* loss, int32_t* counts, const int32_t* dyn_N, hipStream_t stream);
int geossl_infograph_bwd(const float* x, int64_t N, int F, const float* W, const int32_t* mol_ptr, int64_t B,
                         int readout, const float* s, const float* h, const float* scores, const float* gout,
                         float* dx, float* dm, float* dh, hipStream_t stream);
int geossl_infograph_bwd_dyn(const float* x, int64_t N, int F, const float* W, const int32_t* mol_ptr, int64_t B,
                             int readout, const float* s, const float* h, const float* scores, const float* gout,
                             float* dx, float* dm, float* dh, const int32_t* dyn_N, hipStream_t stream);

/* ---- Supervised property head: examples/pretrain_Supervised.py:79-104, finetune_qm9.py:163-384 (csrc/property_head.hip)
 * h [N][F] per-atom latent (F = 64, 128 or 256: geossl_property_width_ok), mol_ptr [B + 1] int32 offsets of the B >= 1
 * molecules (atoms sorted by molecule).  readout: 0 "add", 1 "mean" (sum / max(n_b, 1), the arithmetic of
 * geossl_segment_reduce_fwd).  head 0: Linear(F, 1), W1 = w [F], b1 = b [1], W2 = b2 = NULL; head 1: Dense(F, F/2, silu)
 * then Dense(F/2, 1), W1 [F/2][F], b1 [F/2], W2 = w2 [F/2], b2 [1].  stats [2] = (mean, std) in device memory.
 * y: target of molecule b at y[b * y_stride].  loss_kind: 0 L1, 1 MSE.
 * Forward: m [B][F] (out) = readout; z [B][F/2] (out, head 1) = pre-activation; pred [B] (out); t_b = (y_b - mean) / std
 *   (fp32, two roundings); loss [1] = mean_b |pred_b - t_b| or mean_b (pred_b - t_b)^2 (fp64 sum in a fixed order,
 *   stored as fp32).  workspace: geossl_property_workspace_floats(B) floats, 8-byte aligned.
 * Predict: pred [B] (out) = pred_b * std + mean (eval()); no loss, no m / z.
 * Backward with gout[0]: dpred_b = sign(pred_b - t_b) gout / B (sign(0) = 0) or (2 / B) (pred_b - t_b) gout;
 *   dh [N][F] (out) = dm_b (/ max(n_b, 1) for "mean") on every atom of b, dm_b = dpred_b w (head 0) or
 *   dz_b W1 with dz [B][F/2] (out, head 1) = dpred_b w2 silu'(z_b);  dw / db (nullable; head 0: dL/dw [F], dL/db [1];
 *   head 1: dL/dw2 [F/2], dL/db2 [1]) written, or added to with accumulate = 1.  Head 1's dW1 = dz^T m and db1 are left to
 *   the caller (geossl_linear_wgrad).
 * `_dyn`: N is a capacity and dyn_N (nullable) points at the real atom count; mol_ptr holds the real offsets.  No atom
 *   row at or past the real count is read or written.  No atomics: the same bits every launch.
 * geossl_property_targets: out[b] = y[m * T + task_id] for the dataset molecule m whose first atom is src_off[b]
 *   (mol_off [M + 1] int64, strictly increasing; NaN when no molecule starts there). */
int geossl_property_width_ok(int F);
int64_t geossl_property_workspace_floats(int64_t B);
int geossl_property_fwd(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, int head,
                        const float* W1, const float* b1, const float* W2, const float* b2, const float* y,
                        int64_t y_stride, const float* stats, int loss_kind, float* m, float* z, float* pred,
                        float* workspace, float* loss, hipStream_t stream);
int geossl_property_fwd_dyn(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, int head,
                            const float* W1, const float* b1, const float* W2, const float* b2, const float* y,
                            int64_t y_stride, const float* stats, int loss_kind, float* m, float* z, float* pred,
                            float* workspace, float* loss, const int32_t* dyn_N, hipStream_t stream);
int geossl_property_predict(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, int head,
                            const float* W1, const float* b1, const float* W2, const float* b2, const float* stats,
                            float* pred, hipStream_t stream);
int geossl_property_predict_dyn(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout,
                                int head, const float* W1, const float* b1, const float* W2, const float* b2,
                                const float* stats, float* pred, const int32_t* dyn_N, hipStream_t stream);
int geossl_property_bwd(int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, int head, const float* W1,
                        const float* W2, const float* m, const float* z, const float* pred, const float* y,
                        int64_t y_stride, const float* stats, int loss_kind, const float* gout, float* dh, float* dz,
                        float* dw, float* db, float* workspace, int accumulate, hipStream_t stream);
int geossl_property_bwd_dyn(int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, int head, const float* W1,
                            const float* W2, const float* m, const float* z, const float* pred, const float* y,
                            int64_t y_stride, const float* stats, int loss_kind, const float* gout, float* dh, float* dz,
                            float* dw, float* db, float* workspace, int accumulate, const int32_t* dyn_N,
                            hipStream_t stream);
int geossl_property_targets(const float* y, int64_t M, int T, int task_id, const int64_t* mol_off,
                            const int32_t* src_off, int64_t B, float* out, hipStream_t stream);

/* ---- LEP pair head: examples/finetune_lep.py:33-45 (train), :77-90 (eval) (csrc/pair_head.hip)
 * h [N][F] per-atom latent (F = 32, 64 or 128: geossl_pair_head_width_ok) of a batch of 2B structures
 * [active 0 .. B-1 | inactive 0 .. B-1], mol_ptr [2B + 1] int32 atom offsets (atoms sorted by structure), B >= 1 pairs.
 * readout: 0 "add", 1 "mean" (sum / max(n_s, 1), the arithmetic of geossl_segment_reduce_fwd).  w [2F], b [1]: the
 * parameters of Linear(2F, 1); y [B] float32 labels.  No atomics: the same inputs give the same bits.
 * Forward: m [2B][F] (out) the readouts, z [B] (out) = b + <w[0:F], m_b> + <w[F:2F], m_{B+b}>, loss [1] (out) = mean_b of
 *   max(z_b, 0) - z_b y_b + log1p(exp(-|z_b|)) (fp64 terms added in pair order, stored as fp32).
 *   workspace: geossl_pair_head_workspace_floats(B) floats, 8-byte aligned.
 * Predict: z [B] only.
 * Backward with gout[0]: dz_b = gout (sigmoid(z_b) - y_b) / B; dh [N][F] (out) = dz_b w[side F + j] (/ max(n_s, 1) for
 *   "mean") on every atom row of both structures of pair b, each written once; dw [2F] / db [1] (out; NULL: skipped) =
 *   sum_b dz_b m[side B + b][j] / sum_b dz_b in pair order, added to what is there when accumulate != 0.
 * `_dyn`: N is a capacity and dyn_N (nullable) points at the real atom count; mol_ptr [2B + 1] holds the real offsets
 *   (B is exact).  No atom row of h / dh at or past the real count is read or written; the arithmetic and the order of
 *   every sum are those of the exact forms (the same inputs give the same bits as they do). */
int geossl_pair_head_width_ok(int F);
int64_t geossl_pair_head_workspace_floats(int64_t B);
int geossl_pair_head_fwd(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, const float* w,
                         const float* b, const float* y, float* m, float* z, float* workspace, float* loss,
                         hipStream_t stream);
int geossl_pair_head_predict(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout,
                             const float* w, const float* b, float* z, hipStream_t stream);
int geossl_pair_head_bwd(int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, const float* w, const float* m,
                         const float* z, const float* y, const float* gout, float* dh, float* dw, float* db,
                         float* workspace, int accumulate, hipStream_t stream);
int geossl_pair_head_fwd_dyn(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout,
                             const float* w, const float* b, const float* y, float* m, float* z, float* workspace,
                             float* loss, const int32_t* dyn_N, hipStream_t stream);
int geossl_pair_head_predict_dyn(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout,
                                 const float* w, const float* b, float* z, const int32_t* dyn_N, hipStream_t stream);
int geossl_pair_head_bwd_dyn(int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, const float* w,
                             const float* m, const float* z, const float* y, const float* gout, float* dh, float* dw,
                             float* db, float* workspace, int accumulate, const int32_t* dyn_N, hipStream_t stream);

/* ---- angle prediction on atom triples: examples/pretrain_TorsionAnglePrediction.py:16-27,64-78 (csrc/torsion_head.hip)
 * h [N][F] node features (F = 64, 128, 256 or 512: geossl_torsion_head_width_ok), W [3F] = predictor.weight =
 * [w_u | w_v | w_w], bias [1], triples (tri0[t], tri1[t], tri2[t]) = (u_t, v_t, w_t), t < T (batch atom ids), angle [T] the
 * targets (batch.super_edge_angle).  No atomics: the same inputs give the same bits.
 * Forward: proj [N][3] (out) = (w_u . h_i, w_v . h_i, w_w . h_i); pred [T] (out) = ((a_u + b_v) + c_w) + bias; res [T]
 *   (out, the backward's input) = pred - angle; loss [1] = mean res^2 (fp64 sums in a fixed order, NaN for T = 0).  A
 *   triple with an atom outside [0, N) reads nothing: pred = res = NaN.  workspace:
 *   geossl_torsion_head_fwd_workspace_floats(T) floats, 8-byte aligned.
 * Backward with the upstream gradient gout[0]: d pred_t = (2 gout / T) res_t; dA_i / dB_i / dC_i = the sums of d pred over
 *   the triples with u_t = i / v_t = i / w_t = i in ascending triple order; dh [N][F] = dA_i w_u + dB_i w_v + dC_i w_w;
 *   dW [3F] (+)= [sum dA_i h_i | sum dB_i h_i | sum dC_i h_i], db [1] (+)= sum dA_i, from per-block partials added in block
 *   order.  accumulate: dW / db (+)= instead of =.  The triples must be grouped by molecule in batch order with their three
 *   atoms in one molecule (collated AtomTripleExtractor output is): mol_ptr [B + 1] int32 are the atom offsets of the
 *   B >= 1 molecules, and molecule m's triples are the run whose u lies in [mol_ptr[m], mol_ptr[m + 1]) (one block per
 *   molecule scans it; a triple that breaks the grouping is dropped from the sums).  workspace:
 *   geossl_torsion_head_bwd_workspace_floats(N, F) floats.
 * `_dyn`: N and T are capacities (grids, workspaces); dyn_N / dyn_T (nullable) point at the real counts - the mean divides
 *   by the real T, atoms and triples past the real counts are neither read nor written; mol_ptr holds the real offsets.
 * geossl_triple_angles: angle [T] (out) = the angle at the MIDDLE atom of each triple, atan2f(|a x b|, a . b) with
 *   a = pos_u - pos_v, b = pos_w - pos_v, in [0, pi], 0 when a or b is zero (NaN for an atom outside [0, N)).  This is
 *   this library's definition of super_edge_angle: the reference tree holds no code that fills it.
 * geossl_gather_triples (one block per molecule m of the batch, B of them): columns [t_ptr[m], t_ptr[m + 1]) of
 *   tri0 / tri1 / tri2 = columns [t_src_off[m], ...) of the dataset's tri_src [3][stride] (int32, local atom indices)
 *   + mol_ptr[m] (dataloaders_AtomTriple.py:58-59); angle_dst likewise from angle_src. */
int geossl_torsion_head_width_ok(int F);
int64_t geossl_torsion_head_fwd_workspace_floats(int64_t T);
int64_t geossl_torsion_head_bwd_workspace_floats(int64_t N, int F);
int geossl_torsion_head_fwd(const float* h, int64_t N, int F, const float* W, const float* bias, const int64_t* tri0,
                            const int64_t* tri1, const int64_t* tri2, const float* angle, int64_t T, float* proj,
                            float* pred, float* res, float* workspace, float* loss, hipStream_t stream);
int geossl_torsion_head_fwd_dyn(const float* h, int64_t N, int F, const float* W, const float* bias, const int64_t* tri0,
                                const int64_t* tri1, const int64_t* tri2, const float* angle, int64_t T, float* proj,
                                float* pred, float* res, float* workspace, float* loss, const int32_t* dyn_N,
                                const int32_t* dyn_T, hipStream_t stream);
int geossl_torsion_head_bwd(const float* h, int64_t N, int F, const float* W, const int64_t* tri0, const int64_t* tri1,
                            const int64_t* tri2, int64_t T, const float* res, const int32_t* mol_ptr, int64_t B,
                            const float* gout, float* dh, float* dW, float* db, float* workspace, int accumulate,
                            hipStream_t stream);
int geossl_torsion_head_bwd_dyn(const float* h, int64_t N, int F, const float* W, const int64_t* tri0,
                                const int64_t* tri1, const int64_t* tri2, int64_t T, const float* res,
                                const int32_t* mol_ptr, int64_t B, const float* gout, float* dh, float* dW, float* db,
                                float* workspace, int accumulate, const int32_t* dyn_N, const int32_t* dyn_T,
                                hipStream_t stream);
int geossl_triple_angles(const float* pos, int64_t N, const int64_t* tri0, const int64_t* tri1, const int64_t* tri2,
                         int64_t T, float* angle, hipStream_t stream);
int geossl_gather_triples(const int32_t* tri_src, int64_t stride, const float* angle_src, const int32_t* t_src_off,
                          const int32_t* t_ptr, const int32_t* mol_ptr, int64_t B, int64_t* tri0, int64_t* tri1,
                          int64_t* tri2, float* angle_dst, hipStream_t stream);

/* ---- sparse pair list (csrc/sparse_pairs.hip): SchNet on structures of up to 1024 atoms ----------------------------
 * The radius graph of geossl_pair_geometry as a compacted list: per molecule in batch order the pairs (a < b) with an
 * edge in at least one direction, lexicographic, as int32 global atom ids; pair_d / pair_c / pair_flag as in the dense
 * form (same fp32 arithmetic, op by op).  Nothing is read back: every array has `capacity` rows (the caller's bound
 * sum_m min(n_m (n_m - 1) / 2, (cap) n_m), cap = max_num_neighbors + 1), n_pairs[0] receives the real number of rows
 * (the dyn_P of the filter kernels) and the rows past it are rewritten on every call as flag 0, pair_i = pair_j = 0,
 * pair_c = 0, pair_d = cutoff.  Incidence lists: inc_ptr[N + 1], and for atom t the entries [inc_ptr[t], inc_ptr[t+1])
 * in ascending partner order (pair_j == t first, then pair_i == t): inc_pair = row of the pair, inc_src = partner |
 * (edge partner -> t) << 30 | (edge t -> partner) << 31; inc_pair / inc_src hold 2 * capacity entries.
 * Work arrays: mol_cnt[B], up_cnt[N], lo_cnt[N].  1 <= max_n <= 1024, else hipErrorInvalidValue.                    */
int geossl_sparse_pairs_build(const float* pos, const int32_t* mol_ptr, int64_t B, int64_t N, int max_n, float r2,
                              int cap, float cutoff, int64_t capacity, int32_t* mol_cnt, int32_t* up_cnt,
                              int32_t* lo_cnt, int32_t* pair_i, int32_t* pair_j, float* pair_d, float* pair_c,
                              uint8_t* pair_flag, int32_t* inc_ptr, int32_t* inc_pair, uint32_t* inc_src,
                              int32_t* n_pairs, hipStream_t stream);
/* The build for a capacity bucket: N is the CAPACITY of the per-atom arrays (up_cnt / lo_cnt [N], inc_ptr [N + 1]) and
 * dyn_N (device, not null) the batch's real atom count; mol_ptr holds the B real offsets (B is exact).  No atom row at
 * or past the real count is read; inc_ptr[0 .. N_real] is written; max_n is a bound on the largest molecule that only
 * sizes LDS (the list does not depend on it).  Everything else as geossl_sparse_pairs_build, bit for bit.          */
int geossl_sparse_pairs_build_dyn(const float* pos, const int32_t* mol_ptr, int64_t B, int64_t N, int max_n, float r2,
                                  int cap, float cutoff, int64_t capacity, int32_t* mol_cnt, int32_t* up_cnt,
                                  int32_t* lo_cnt, int32_t* pair_i, int32_t* pair_j, float* pair_d, float* pair_c,
                                  uint8_t* pair_flag, int32_t* inc_ptr, int32_t* inc_pair, uint32_t* inc_src,
                                  int32_t* n_pairs, const int32_t* dyn_N, hipStream_t stream);

/* ---- live-pair list of a dense layout (csrc/sparse_pairs.hip, csrc/graph.hip) -------------------------------------
 * The filter network has work only for the pair slots that carry an edge (pair_flag != 0).
 *   geossl_pair_geometry_live : geossl_pair_geometry, and mol_live[B] (nullable) = live slots per molecule.
 *   geossl_live_pairs_build   : the live slots in slot order (stable: pair_i still ascends), packed back to back into
 *            live_d / live_c / live_flag / live_i / live_j; row_slot[r] = dense slot of row r; n_live[0] = the number
 *            of rows, on the device (the dyn_P of the filter kernels).  Every output has P rows (the capacity: nothing is
 *            sized by a read-back); rows past n_live are rewritten on every call as flag 0, pair_i = pair_j = 0,
 *            pair_c = 0, pair_d = cutoff, row_slot = 0.  dyn_P (nullable): the real slot count of a capacity bucket.
 *            One launch, no atomics, deterministic.
 *   geossl_cfconv_filter_fwd_rows : geossl_cfconv_filter_fwd_dyn on such a list: row r stores its hidden row at T row r
 *            and its filter row at Wf row row_slot[r] (row_slot == NULL: row r, the plain call); Wf rows of dead slots are
 *            not written.  The values of a row do not depend on where it stands in the list.
 *   geossl_gather_live_rows : dst[l][r][:] = src[l][row_slot[r]][:] for r < n_live, l < L ([L][P][F] tensors, F a multiple
 *            of 4): hidden rows stored per dense slot regrouped to the list's rows.                                   */
int geossl_pair_geometry_live(const float* pos, const int32_t* mol_ptr, const int32_t* pair_ptr, int64_t B, int max_n,
                              float r2, int cap, float cutoff, float* pair_d, float* pair_c, uint8_t* pair_flag,
                              int32_t* mol_live, hipStream_t stream);
int geossl_live_pairs_build(const float* pair_d, const float* pair_c, const uint8_t* pair_flag, const int32_t* pair_i,
                            const int32_t* pair_j, const int32_t* mol_ptr, const int32_t* pair_ptr,
                            const int32_t* mol_live, int64_t B, int64_t P, float cutoff, const int32_t* dyn_P,
                            float* live_d, float* live_c, uint8_t* live_flag, int32_t* live_i, int32_t* live_j,
                            int32_t* row_slot, int32_t* n_live, hipStream_t stream);
int geossl_cfconv_filter_fwd_rows(const float* pair_d, const float* pair_c, int64_t P, const GeosslFilterWeights* w, int L,
                                  int F, int G, const float* offset, float coeff, float* T, float* Wf,
                                  const int32_t* dyn_P, const int32_t* row_slot, hipStream_t stream);
int geossl_gather_live_rows(const float* src, const int32_t* row_slot, const int32_t* n_live, int64_t P, int L, int F,
                            float* dst, hipStream_t stream);

/* out[t] = sum over t's incidence entries with the edge partner -> t (swap = 1: t -> partner, the transposed graph) of
 * x[partner] * Wf[row], ascending partner, separate multiply and add (the rounding sequence of geossl_cfconv_aggregate);
 * F in {32, 64, 128}; no atomics; every row of out is written (zeros for an atom without such pairs).               */
int geossl_cfconv_aggregate_sparse(const float* x, const float* Wf, const int32_t* inc_ptr, const int32_t* inc_pair,
                                   const uint32_t* inc_src, int64_t N, int F, int swap, float* out,
                                   hipStream_t stream);
/* The same launch at a capacity: the grid comes from N, a wave whose atom is at or past *dyn_N (device, not null)
 * returns - those rows of x and out are neither read nor written.  Same arithmetic, bit for bit.                    */
int geossl_cfconv_aggregate_sparse_dyn(const float* x, const float* Wf, const int32_t* inc_ptr,
                                       const int32_t* inc_pair, const uint32_t* inc_src, int64_t N, int F, int swap,
                                       float* out, const int32_t* dyn_N, hipStream_t stream);
/* geossl_pair_position_grad through the incidence lists: dd is [L, P] (P = capacity) from geossl_cfconv_filter_dpos. */
int geossl_pair_position_grad_sparse(const float* pos, const float* pair_d, const float* dd, const int32_t* inc_ptr,
                                     const int32_t* inc_pair, const uint32_t* inc_src, int64_t N, int64_t P, int L,
                                     float* dpos, hipStream_t stream);

/* ---- MD17 evaluation: energy head with its seed, error sums, per-atom targets (csrc/force_head.hip) ----------------
 * geossl_energy_head_fwd : energy[B] = head(readout(h)) and seed[N][F] = d(sum_b energy_b)/dh in one launch, for the two
 *   heads and the widths of geossl_property_fwd (geossl_property_width_ok; head 0: W1 = w [F], b1 = b [1], W2 = b2 = NULL;
 *   head 1: W1 [F/2][F], b1 [F/2], W2 = w2 [F/2], b2 [1]) with its arithmetic; readout 0 = add, 1 = mean.  mol_ptr [B + 1]
 *   are atom offsets in [0, N]; the seed rows of every molecule are written.  Deterministic, no atomics.
 * geossl_force_metrics_accumulate : acc = [sum |pred_energy - y| (f64), sum |-dE_dpos - force_target| (f64), B (i64),
 *   counted force elements (i64)] (32 bytes, 8-byte aligned) has this call's sums ADDED onto it: the caller zeroes it
 *   and reads it once per epoch.  pred_energy, y [B]; dE_dpos, force_target [N][3].  Differences in fp32, sums in fp64 in
 *   a fixed order; an element whose dE_dpos is NaN is skipped on both sides and not counted; energies are never skipped.
 *   One block; calls on one stream are ordered, and a captured graph may hold the launch (acc is its only state).
 * geossl_gather_atom_rows : dst rows [mol_ptr[b], mol_ptr[b + 1]) = src rows [src_off[b], ...) for b < B; src [n_src][C],
 *   dst [N][C] float32.  A molecule whose offsets leave either array is not copied.                                  */
int geossl_energy_head_fwd(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, int head,
                           const float* W1, const float* b1, const float* W2, const float* b2, float* energy,
                           float* seed, hipStream_t stream);
int geossl_force_metrics_accumulate(const float* pred_energy, const float* y, int64_t B, const float* dE_dpos,
                                    const float* force_target, int64_t N, void* acc, hipStream_t stream);
int geossl_gather_atom_rows(const float* src, int64_t n_src, int C, const int32_t* src_off, const int32_t* mol_ptr,
                            int64_t B, int64_t N, float* dst, hipStream_t stream);

/* ---- evaluation passes: error sums and result rows of one batch (csrc/eval_collect.hip) -----------------------------
 * geossl_eval_collect : acc = [sum a (f64), sum s (f64), rows (i64), unused (i64)] (32 bytes, 8-byte aligned) has this
 *   batch's sums and B ADDED onto it: the caller zeroes it before a pass and reads it once behind it.  Per row, in fp32:
 *   kind 0 (regression) d = pred - target, a = |d|, s = d d; kind 1 (BCE with logits, z = pred, y = target)
 *   a = max(z, 0) - z y + log1p(exp(-|z|)), s = 0; the sums in fp64 in a fixed order, no atomics.  out_pred[offset + b] =
 *   pred[b] and out_true[offset + b] = target[b] for b < B; either output may be NULL (the sums alone).  offset is a host
 *   value (the launch is made eagerly behind a replay).  One block; B = 0 returns 0 without a launch.                  */
int geossl_eval_collect(const float* pred, const float* target, int64_t B, int kind, int64_t offset, float* out_pred,
                        float* out_true, void* acc, hipStream_t stream);

/* ---- sampled atom tuples of a batch: AtomTupleExtractor(ratio < 1) on the device (csrc/sampled_tuples.hip) ------------
 * One block per molecule m < B (n = mol_ptr[m + 1] - mol_ptr[m] <= 255 atoms from batch row a0 = mol_ptr[m] on), launched
 * behind the gather of a capacity bucket.  The molecule owns the k = se_ptr[m + 1] - se_ptr[m] columns of sei0 / sei1 from
 * se_ptr[m] on.  k is NEVER computed here: it is the host's int(M * ratio) (Python float arithmetic, batch.kept_tuples),
 * M = n (n - 1) / 2 slots of itertools.combinations order (option 0) or n (n - 1) of itertools.permutations (option 1).
 * draw != 0: slot s gets the 64-bit key (w0 << 32) | w1, (w0, w1, ., .) = Philox-4x32-10 of the counter
 *   (s, mol_id[m], 0, 0) under the key words (seed & 0xffffffff, seed >> 32).  The k slots with the smallest (key, s) are
 *   kept (k > M: refused), unranked and written in ASCENDING SLOT ORDER with a0 added.  mol_id [B] int32: what
 *   identifies the molecule in its dataset (the low word of its id), so a molecule's draw does not depend on its batch.
 * draw == 0: sei0 / sei1 already hold the batch's tuples (a collated batch's tensor, a host-drawn list); mol_id and seed
 *   are not read.
 * Both: a tuple whose ends do not both lie in [a0, a0 + n) or are the same atom sets status[0] = 1 (nullable; nothing
 *   resets it) and is left out of the lists below.  inc_ptr (nullable; int64 [N + 1]): inc_ptr[a0 + i] = 2 se_ptr[m] + the
 *   exclusive scan of the molecule's atom degrees (both ends count); the last molecule also writes inc_ptr[a0 + n] =
 *   2 se_ptr[B].  inc_idx (nullable; int32 [2 S]): for every atom the ids of the tuples it lies on, ascending - exactly
 *   what geossl_incidence_count + an exclusive scan + geossl_incidence_fill (sides = 3) give for the same list.
 * Integer work only: LDS counters, no floating atomics; the same inputs give the same bits.  N_cap / S_cap: rows of the
 * atom arrays / columns of sei (2 S_cap < 2^31); a molecule whose offsets leave them (or n > 255) sets the status word
 * and writes nothing. */
int geossl_sampled_tuples(const int32_t* mol_ptr, const int32_t* se_ptr, int64_t B, int option, const int32_t* mol_id,
                          int draw, uint64_t seed, int64_t N_cap, int64_t S_cap, int64_t* sei0, int64_t* sei1,
                          int64_t* inc_ptr, int32_t* inc_idx, int32_t* status, hipStream_t stream);

/* ---- GeoSSL-RR: the two AutoEncoder heads of examples/pretrain_GeoSSL.py:77-100 (csrc/rr_head.hip) ---------------------
 * The AutoEncoder is THIS PROJECT'S definition (geossl_amd/Geom3D/models/autoencoder.py): p = Linear2(relu(BatchNorm1d(
 * Linear1(x)))) and a loss of p against y: kind 0 "l1" mean |p - y|, 1 "l2" mean (p - y)^2, 2 "cosine" - mean over the rows
 * of <p, y> / (max(|p|, 1e-8) max(|y|, 1e-8)).  Both heads run in the same launches: head 0 on (X, Y), head 1 on (Y, X);
 * X, Y [B][F] fp32, F = 128 (geossl_rr_head_width_ok), 2 <= B <= 2^20 (an exact count on every route).
 * params / grads: HOST arrays of 12 device pointers, per head W1 [F][F], b1 [F], gamma [F], beta [F], W2 [F][F], b2 [F];
 * buffers: host array of 6 device pointers, per head running_mean [F], running_var [F], num_batches_tracked (int64 [1]).
 * Forward: Z = a W1^T + b1; per column the batch mean and the biased variance over the B rows; zhat [2][B][F] (out) =
 *   (Z - mean) istd with istd [2][F] (out) = 1 / sqrt(var + eps_h); act [2][B][F] (out) = relu(gamma zhat + beta);
 *   p [2][B][F] (out) = act W2^T + b2; loss [1] = (loss_0 + loss_1) / 2 (fp64 sums in a fixed order, stored as fp32).  The
 *   same pass updates the buffers IN PLACE: running = (1 - momentum_h) running + momentum_h (mean | var B / (B - 1)),
 *   num_batches_tracked + 1.  workspace: geossl_rr_head_workspace_floats(B) floats, 8-byte aligned.  5 launches.
 * Backward from the upstream gradient gout[0]: dp [2][B][F] (scratch), dz [2][B][F] (scratch; ends as the gradient of Z),
 *   dt [2][B][F] (scratch: the gradients of the heads' targets; non-NULL exactly when detach_target == 0); the 12
 *   parameter gradients written, or added to with accumulate = 1 (the four weight and bias pairs through
 *   geossl_linear_wgrad, tn_workspace: geossl_tn_workspace_floats(B, F, F, 4) floats); dxy [2B][F] (out): rows [0, B) the
 *   gradient of X = head 0's input gradient (+ head 1's target gradient), rows [B, 2B) that of Y.  l1: sign(0) = 0.
 *   6 launches.  The two dense products of each pass run on the matrix pipe with three-way split operands; no atomics:
 *   the same bits every launch. */
int geossl_rr_head_width_ok(int F);
int64_t geossl_rr_head_workspace_floats(int64_t B);
int geossl_rr_head_fwd(const float* X, const float* Y, int64_t B, int F, int loss_kind, const float* const* params,
                       float* const* buffers, float eps0, float momentum0, float eps1, float momentum1, float* zhat,
                       float* istd, float* act, float* p, float* workspace, float* loss, hipStream_t stream);
int geossl_rr_head_bwd(const float* X, const float* Y, int64_t B, int F, int loss_kind, int detach_target,
                       const float* const* params, const float* zhat, const float* istd, const float* act,
                       const float* p, const float* gout, float* dp, float* dz, float* dt, float* const* grads,
                       int accumulate, float* dxy, float* tn_workspace, hipStream_t stream);

/* ---- molecular dynamics on a force field: the integrator around the force pass (csrc/md_integrate.hip) ----------------
 * An MD step of B independent replicas is geossl_md_advance, the force pass on pos, geossl_md_finish.  Device state:
 * pos, vel, grad [N][3] and energy [B] fp32; cinv_mass [N] = ACCEL / m and rsqrt_mass [N] = m^-1/2 fp32; ke_coef [N] =
 * m / (2 ACCEL) fp64; params [4] fp32 = (dt, c1 = exp(-gamma dt), sigma_T = sqrt(1 - c1^2) sqrt(KB T ACCEL), unused);
 * state [8] int64 = (steps completed, step in flight + 1, Philox seed, record_every, step of trajectory slot 0,
 * thermostat 0 NVE / 1 Langevin, unused, unused).  Parameters and state are read from the device by every launch: a
 * captured graph of these launches follows their changes.
 * geossl_md_advance : a = (-grad) cinv_mass, vh = fma(dt/2, a, v); NVE x = fma(dt, vh, x), vel = vh; Langevin
 *   x = fma(dt/2, vh, x), vo = fma(c1, vh, (sigma_T rsqrt_mass) xi), x = fma(dt/2, vo, x), vel = vo.  xi: the normals of
 *   geossl_md_normals at (seed, step = state[0]).  Writes state[1] = state[0] + 1.
 * geossl_md_finish : v = fma(dt/2, (-grad_new) cinv_mass, vel); grad = grad_new and energy = energy_new (either may BE
 *   the other buffer); per molecule KE = sum ke_coef |v|^2 in fp64 in a fixed order, no atomics.  With s = state[1] and
 *   d = s - state[4]: when d >= 0, d % record_every == 0 and d / record_every < frames, slot d / record_every of traj_pos
 *   / traj_vel [frames][N][3] fp32, traj_pot [frames][B] fp32 (energy_new) and traj_kin [frames][B] fp64 is written.
 *   Writes state[0] = s.  record_only != 0: no kick, no step word written, slot 0 written (frames >= 1).  mol_ptr
 *   [B + 1] are atom offsets in [0, N]; frames = 0: nothing is recorded and the traj pointers may be NULL.
 * geossl_md_normals : out [N][3] = the first three normals of Philox-4x32-10 at the counter (atom, step & 0xffffffff,
 *   step >> 32, 0) under the key (seed & 0xffffffff, seed >> 32), Box-Muller - what geossl_md_advance draws.           */
int geossl_md_advance(float* pos, float* vel, const float* grad, const float* cinv_mass, const float* rsqrt_mass,
                      const float* params, int64_t* state, int64_t N, hipStream_t stream);
int geossl_md_finish(const float* pos, float* vel, const float* grad_new, const float* energy_new, float* grad,
                     float* energy, const float* cinv_mass, const double* ke_coef, const int32_t* mol_ptr, int64_t B,
                     int64_t N, const float* params, int64_t* state, int record_only, int64_t frames, float* traj_pos,
                     float* traj_vel, float* traj_pot, double* traj_kin, hipStream_t stream);
int geossl_md_normals(uint64_t seed, uint64_t step, int64_t N, float* out, hipStream_t stream);

/* ---- structure relaxation on a force field: FIRE around the force pass (csrc/relax.hip) -----------------------------
 * A step of B independent replicas is the force pass on pos, then geossl_fire_step.  Device state: pos, vel, grad [N][3]
 * and energy [B] fp32; cinv_mass [N] = ACCEL / m fp32; params [8] fp32 = (ftol, dt_max, dt_min, max_step, f_inc, f_dec,
 * alpha_start, f_alpha); iparams [4] int64 = (n_min, record_every, call counter of trajectory slot 0, unused); per
 * molecule mol_dt, mol_alpha [B] fp32 and mol_state [B][4] int32 = (npos, done, nsteps, calls).  All of it is read from
 * the device by every launch: a captured graph of these launches follows its changes.
 * geossl_fire_step : per molecule, with F = -grad_new and fp64 reductions in a fixed order (no atomics): converged =
 *   done or max_i |F_i| < ftol.  A converged molecule is latched (done = 1) and only its call counter moves.  Otherwise
 *   P = sum F.v > 0 or v = 0: v = (1 - alpha) v + alpha sqrt(vv / ff) F, and after more than n_min such steps in a row
 *   dt = min(dt f_inc, dt_max), alpha = alpha f_alpha; else v = 0, alpha = alpha_start, dt = max(dt f_dec, dt_min).
 *   Then v += dt F cinv_mass, dr = dt v, pos += min(1, max_step / max_i |dr_i|) dr.  The fp32 rounding sequence is stated
 *   in csrc/relax.hip.  grad = grad_new and energy = energy_new are kept (either may BE the other buffer).  With d =
 *   calls - iparams[2]: when d >= 0, d % record_every == 0 and d / record_every < frames, slot d / record_every of traj_pos
 *   / traj_vel [frames][N][3] and traj_energy / traj_fmax / traj_dt / traj_alpha fp32, traj_npos / traj_done int32
 *   [frames][B] receives the state AS THE STEP FOUND IT (done: after the test at these positions).  evaluate_only != 0:
 *   the test and the frame into slot 0 (frames >= 1), nothing else is written.  mol_ptr [B + 1] are atom offsets in
 *   [0, N]; frames = 0: nothing is recorded and the traj pointers may be NULL.
 * geossl_fire_active : active[0] = the number of molecules with done == 0 (one block, fixed order).                   */
int geossl_fire_step(float* pos, float* vel, const float* grad_new, const float* energy_new, float* grad, float* energy,
                     const float* cinv_mass, const int32_t* mol_ptr, int64_t B, int64_t N, const float* params,
                     const int64_t* iparams, float* mol_dt, float* mol_alpha, int32_t* mol_state, int evaluate_only,
                     int64_t frames, float* traj_pos, float* traj_vel, float* traj_energy, float* traj_fmax,
                     float* traj_dt, float* traj_alpha, int32_t* traj_npos, int32_t* traj_done, hipStream_t stream);
int geossl_fire_active(const int32_t* mol_state, int64_t B, int32_t* active, hipStream_t stream);

/* ---- normal-mode analysis on a force field: central-difference Hessian, finishing pass, Jacobi (csrc/vibrations.hip) ---
 * A round of B molecules (N atoms, mol_ptr [B + 1]) is geossl_hessian_displace, the force pass on the image batch,
 * geossl_hessian_collect.  Device state: x0 [N][3] fp32, the reference geometry; img [2 C][N][3] fp32, the image batch
 * (image 2 c is (c, +), image 2 c + 1 is (c, -)); grad [2 C][N][3] and energy_img [2 C][B] fp32, the pass's results;
 * delta [1] fp32; state [4] int64 = (round, round in flight, unused, unused).  All of it is read from the device by every
 * launch: a captured graph of these launches follows its changes.
 * geossl_hessian_displace : with r = state[0] and k = r C + c, every image is x0 except local coordinate k of each
 *   molecule with k < 3 n_b, which is fl32(x0_k + delta) in image (c, +) and fl32(x0_k - delta) in (c, -).  Writes
 *   state[1] = r.
 * geossl_hessian_collect : with r = state[1] and k = r C + c: for r < R and k < 3 n_b, hessian[b][k][t] = (g+[t] - g-[t]) /
 *   (x+_k - x-_k) for t < 3 n_b, in fp64 from the fp32 gradients and the two fp32 coordinates the images hold; other rows
 *   are not touched.  r == R: energy[b] = energy_img[0][b], fmax[b] = max_i |g_i| of image 0 (fp64).  Writes state[0] = r + 1.
 *   hessian [B][M][M] fp64 with M >= 3 n_max (M <= 765).
 * geossl_hessian_finish : per molecule, fp64, in a fixed order (no atomics): asymmetry = max |H - H^T|, H = (H + H^T) / 2,
 *   D_ij = H_ij / sqrt(m_i m_j) (both zero outside the 3 n_b block); project 1: the three translations, 2: also the three
 *   rotations about the centre of mass, mass-weighted, orthonormalised by modified Gram-Schmidt, a vector dropped when its
 *   remaining norm is not above 1e-5 of its own; n_projected = the survivors; D = P D P, P = I - sum v v^T.  masses [N]
 *   fp64; workspace: geossl_hessian_finish_workspace(B, M) doubles.
 * geossl_sym_eig_jacobi : A [B][M][M] fp64 (the upper triangle of the leading dims[b] x dims[b] block is read), M <= 99.
 *   One block per matrix: cyclic Jacobi in round-robin order, the disjoint rotations of a round computed first and then
 *   applied; stop when max off-diagonal <= 2^-50 |A|_F (tested once per sweep) or after max_sweeps sweeps.  eigenvalues
 *   [B][M] ascending (NaN past dims[b]), modes [B][M][M] with the eigenvectors in the columns (zero outside the block),
 *   sweeps [B] and converged [B] int32.  The rotation formula and the skip rule are stated in csrc/vibrations.hip.       */
int geossl_hessian_displace(const float* x0, const int32_t* mol_ptr, const float* delta, int64_t* state, int64_t B,
                            int64_t N, int64_t C, float* img, hipStream_t stream);
int geossl_hessian_collect(const float* img, const float* grad, const float* energy_img, const int32_t* mol_ptr,
                           int64_t* state, int64_t B, int64_t N, int64_t C, int64_t R, int64_t M, double* hessian,
                           double* energy, double* fmax, hipStream_t stream);
int64_t geossl_hessian_finish_workspace(int64_t B, int64_t M);
int geossl_hessian_finish(double* hessian, const float* x0, const double* masses, const int32_t* mol_ptr, int64_t B,
                          int64_t N, int64_t M, int project, double* D, double* asymmetry, int32_t* n_projected,
                          double* workspace, hipStream_t stream);
int geossl_sym_eig_jacobi(const double* A, const int32_t* dims, int64_t B, int64_t M, int max_sweeps, double* eigenvalues,
                          double* modes, int32_t* sweeps, int32_t* converged, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GEOSSL_HIP_H */
