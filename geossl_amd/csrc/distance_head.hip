// Distance-prediction head of examples/pretrain_DistancePrediction.py:15-25,66-79: pred_e = Linear(2F, 1)(cat(h_u, h_v)),
// target_e = |pos_u - pos_v|, loss = L1Loss(pred, target) = mean_e |pred_e - target_e|, forward and backward.
//
// A linear layer on a concatenation splits into two per-atom projections: with W = [w_u | w_v],
//   a_i = w_u . h_i,  b_i = w_v . h_i,  pred_e = (a_{u_e} + b_{v_e}) + bias,
// so the [S][2F] edge features of the reference are never formed.  Forward: one wave per atom computes (a_i, b_i)
// (k_cat_project<V, 2> of head_common.h), then one pass over the super-edges computes target, pred, sgn(pred - target) and
// per-block sums of |pred - target| (k_dist_edges), and one block adds the block sums in order and divides by S
// (k_head_loss).
// Backward, with d pred_e = (gout / S) sgn_e (L1Loss's mean and abs backward; sgn(0) = 0):
//   dA_i = sum of d pred_e over the super-edges with u_e = i, dB_i over those with v_e = i, each in ascending edge
//   order on the atom's incidence list (k_dist_atom_grads: one thread per atom);
//   dh_i = dA_i w_u + dB_i w_v (written), and per block of atoms the partials of dW = [sum dA_i h_i | sum dB_i h_i] and of
//   db = sum dA_i (k_cat_dh<2>); one launch adds the block partials in block order (k_cat_wgrad<2>).
// Every sum has a fixed order and there are no atomics: two launches on the same inputs give the same bits.
// Capacity launches (`_dyn`): N and S are capacities that size the grids; the real counts are read from dyn_N / dyn_S.
// Atoms and super-edges at and past them are never read or written, and the mean divides by the real S.
#include "geossl_hip.h"
#include "head_common.h"

using namespace geossl;

namespace {

constexpr int kEdgeBlock = 256;
constexpr int kEdgesPerThread = 4;
constexpr int kEdgesPerBlock = kEdgeBlock * kEdgesPerThread;
constexpr int kAtomBlock = 256;

// Block k owns super-edges [k kEdgesPerBlock, (k + 1) kEdgesPerBlock); partial[k] = the sum of their |pred - target| in
// fp64 (per thread in edge order, then a tree over the block).  Blocks at and past the real S write nothing.
__global__ __launch_bounds__(kEdgeBlock) void k_dist_edges(const float* __restrict__ proj, const float* __restrict__ bias,
                                                           const float* __restrict__ pos, const int64_t* __restrict__ sei0,
                                                           const int64_t* __restrict__ sei1, int S_cap,
                                                           const int32_t* __restrict__ dyn_S, float* __restrict__ pred,
                                                           float* __restrict__ sgn, double* __restrict__ partial) {
  const int S = dyn_count(S_cap, dyn_S);
  const int e0 = blockIdx.x * kEdgesPerBlock;
  if (e0 >= S) return;
  const float b0 = bias[0];
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < kEdgesPerThread; ++k) {
    const int e = e0 + k * kEdgeBlock + threadIdx.x;
    if (e < S) {
      const int64_t u = sei0[e], v = sei1[e];
      // torch.sqrt(torch.sum((u_pos - v_pos) ** 2, dim=1)): fl(fl(fl(dx^2) + fl(dy^2)) + fl(dz^2)), a correctly
      // rounded square root
      const float dx = pos[3 * u] - pos[3 * v];
      const float dy = pos[3 * u + 1] - pos[3 * v + 1];
      const float dz = pos[3 * u + 2] - pos[3 * v + 2];
      const float target = sqrtf(norm2_rn(dx, dy, dz));
      const float p = add_rn(add_rn(proj[2 * u], proj[2 * v + 1]), b0);
      const float r = p - target;
      pred[e] = p;
      sgn[e] = r > 0.f ? 1.f : (r < 0.f ? -1.f : (r == 0.f ? 0.f : r));   // (NaN stays NaN)
      acc += fabs((double)r);
    }
  }
  const double sum = block_sum_f64<kEdgeBlock>(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// dAB[i] = (dA_i, dB_i): the atom's incidence list (every super-edge with u = i or v = i, ascending) walked in order,
// d pred_e = (gout / S) sgn_e.
__global__ __launch_bounds__(kAtomBlock) void k_dist_atom_grads(const int64_t* __restrict__ sei0,
                                                                const float* __restrict__ sgn,
                                                                const int64_t* __restrict__ inc_ptr,
                                                                const int32_t* __restrict__ inc_idx, int N_cap, int S_cap,
                                                                const int32_t* __restrict__ dyn_N,
                                                                const int32_t* __restrict__ dyn_S,
                                                                const float* __restrict__ gout, float* __restrict__ dAB) {
  const int N = dyn_count(N_cap, dyn_N);
  const int i = blockIdx.x * kAtomBlock + threadIdx.x;
  if (i >= N) return;
  const int S = dyn_count(S_cap, dyn_S);
  const float c = gout[0] / (float)S;   // MeanBackward: grad / numel
  float dA = 0.f, dB = 0.f;
  const int64_t k1 = inc_ptr[i + 1];
  for (int64_t k = inc_ptr[i]; k < k1; ++k) {
    const int e = inc_idx[k];
    const float g = mul_rn(c, sgn[e]);
    if (sei0[e] == i)
      dA += g;
    else
      dB += g;
  }
  dAB[2 * (int64_t)i] = dA;
  dAB[2 * (int64_t)i + 1] = dB;
}

inline int64_t edge_blocks(int64_t S) { return std::max<int64_t>(1, (S + kEdgesPerBlock - 1) / kEdgesPerBlock); }
inline bool width_ok(int F) { return wave_row_width_ok(F); }

}  // namespace

extern "C" int geossl_distance_head_width_ok(int F) { return width_ok(F) ? 1 : 0; }

extern "C" int64_t geossl_distance_head_fwd_workspace_floats(int64_t S) { return 2 * edge_blocks(S); }

extern "C" int64_t geossl_distance_head_bwd_workspace_floats(int64_t N, int F) {
  return 2 * std::max<int64_t>(N, 1) + atom_blocks(N) * (2 * (int64_t)F + 1);
}

extern "C" int geossl_distance_head_fwd_dyn(const float* h, int64_t N, int F, const float* W, const float* bias,
                                            const float* pos, const int64_t* sei0, const int64_t* sei1, int64_t S,
                                            float* proj, float* pred, float* sgn, float* workspace, float* loss,
                                            const int32_t* dyn_N, const int32_t* dyn_S, hipStream_t stream) {
  if (N < 0 || S < 0 || N >= (1 << 30) || S >= (1 << 30) || !width_ok(F)) return (int)hipErrorInvalidValue;
  if (N > 0) {
    const int e = launch_cat_project<2>(h, N, F, W, dyn_N, proj, stream);
    if (e != 0) return e;
  }
  double* partial = reinterpret_cast<double*>(workspace);
  if (S > 0) {
    hipLaunchKernelGGL(k_dist_edges, dim3((unsigned)edge_blocks(S)), dim3(kEdgeBlock), 0, stream, proj, bias, pos, sei0,
                       sei1, (int)S, dyn_S, pred, sgn, partial);
    GEOSSL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_head_loss<kEdgesPerBlock>, dim3(1), dim3(kLossBlock), 0, stream, partial, 0, (int)S, dyn_S, loss);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_distance_head_fwd(const float* h, int64_t N, int F, const float* W, const float* bias,
                                        const float* pos, const int64_t* sei0, const int64_t* sei1, int64_t S,
                                        float* proj, float* pred, float* sgn, float* workspace, float* loss,
                                        hipStream_t stream) {
  return geossl_distance_head_fwd_dyn(h, N, F, W, bias, pos, sei0, sei1, S, proj, pred, sgn, workspace, loss, nullptr,
                                      nullptr, stream);
}

extern "C" int geossl_distance_head_bwd_dyn(const float* h, int64_t N, int F, const float* W, const int64_t* sei0,
                                            int64_t S, const float* sgn, const int64_t* inc_ptr, const int32_t* inc_idx,
                                            const float* gout, float* dh, float* dW, float* db, float* workspace,
                                            int accumulate, const int32_t* dyn_N, const int32_t* dyn_S,
                                            hipStream_t stream) {
  if (N < 0 || S < 0 || N >= (1 << 30) || S >= (1 << 30) || !width_ok(F)) return (int)hipErrorInvalidValue;
  float* dAB = workspace;
  float* part = workspace + 2 * std::max<int64_t>(N, 1);
  if (N > 0) {
    hipLaunchKernelGGL(k_dist_atom_grads, dim3((unsigned)((N + kAtomBlock - 1) / kAtomBlock)), dim3(kAtomBlock), 0,
                       stream, sei0, sgn, inc_ptr, inc_idx, (int)N, (int)S, dyn_N, dyn_S, gout, dAB);
    GEOSSL_CHECK_LAUNCH();
  }
  return launch_cat_bwd<2>(h, N, F, W, dAB, part, dyn_N, dh, dW, db, accumulate, stream);
}

extern "C" int geossl_distance_head_bwd(const float* h, int64_t N, int F, const float* W, const int64_t* sei0, int64_t S,
                                        const float* sgn, const int64_t* inc_ptr, const int32_t* inc_idx,
                                        const float* gout, float* dh, float* dW, float* db, float* workspace,
                                        int accumulate, hipStream_t stream) {
  return geossl_distance_head_bwd_dyn(h, N, F, W, sei0, S, sgn, inc_ptr, inc_idx, gout, dh, dW, db, workspace,
                                      accumulate, nullptr, nullptr, stream);
}
