// Distance-prediction head of examples/pretrain_DistancePrediction.py:15-25,66-79: pred_e = Linear(2F, 1)(cat(h_u, h_v)),
// target_e = |pos_u - pos_v|, loss = L1Loss(pred, target) = mean_e |pred_e - target_e|, forward and backward.
//
// A linear layer on a concatenation splits into two per-atom projections: with W = [w_u | w_v],
//   a_i = w_u . h_i,  b_i = w_v . h_i,  pred_e = (a_{u_e} + b_{v_e}) + bias,
// so the [S][2F] edge features of the reference are never formed.  Forward: one wave per atom computes (a_i, b_i)
// (k_dist_project), then one pass over the super-edges computes target, pred, sgn(pred - target) and per-block sums of
// |pred - target| (k_dist_edges), and one block adds the block sums in order and divides by S (k_dist_loss).
// Backward, with d pred_e = (gout / S) sgn_e (L1Loss's mean and abs backward; sgn(0) = 0):
//   dA_i = sum of d pred_e over the super-edges with u_e = i, dB_i over those with v_e = i, each in ascending edge
//   order on the atom's incidence list (k_dist_atom_grads: one thread per atom);
//   dh_i = dA_i w_u + dB_i w_v (written), and per block of atoms the partials of dW = [sum dA_i h_i | sum dB_i h_i] and of
//   db = sum dA_i (k_dist_dh); one launch adds the block partials in block order (k_dist_wgrad).
// Every sum has a fixed order and there are no atomics: two launches on the same inputs give the same bits.
// Capacity launches (`_dyn`): N and S are capacities that size the grids; the real counts are read from dyn_N / dyn_S.
// Atoms and super-edges at and past them are never read or written, and the mean divides by the real S.
#include "common.h"
#include "geossl_hip.h"

using namespace geossl;

namespace {

constexpr int kProjBlock = 256;               // 4 waves, one atom per wave at a time
constexpr int kEdgeBlock = 256;
constexpr int kEdgesPerThread = 4;
constexpr int kEdgesPerBlock = kEdgeBlock * kEdgesPerThread;
constexpr int kAtomsPerBlock = 32;            // k_dist_dh: atoms per block (one partial row of dW / db per block)
constexpr int kAtomBlock = 256;

// (a_i, b_i) = (w_u . h_i, w_v . h_i): lane l holds features [l V, l V + V) of the row (F = 64 V), a butterfly over the
// wave adds the 64 lane sums in a fixed order.
template <int V>
__global__ __launch_bounds__(kProjBlock) void k_dist_project(const float* __restrict__ h, int N_cap,
                                                              const float* __restrict__ W, const int32_t* __restrict__ dyn_N,
                                                              float* __restrict__ proj) {
  constexpr int F = 64 * V;
  const int N = dyn_count(N_cap, dyn_N);
  const int l = threadIdx.x & 63;
  float wu[V], wv[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    wu[k] = W[l * V + k];
    wv[k] = W[F + l * V + k];
  }
  const int waves = gridDim.x * (kProjBlock / 64);
  for (int i = blockIdx.x * (kProjBlock / 64) + (threadIdx.x >> 6); i < N; i += waves) {
    const float* row = h + (int64_t)i * F + l * V;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float x = row[k];
      a = fmaf(wu[k], x, a);
      b = fmaf(wv[k], x, b);
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (l == 0) {
      proj[2 * (int64_t)i] = a;
      proj[2 * (int64_t)i + 1] = b;
    }
  }
}

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
  __shared__ double red[kEdgeBlock];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = kEdgeBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// One block: loss = (sum of the block partials, in block order per thread, then a tree) / S.  S = 0: 0 / 0 = NaN, the
// mean of an empty tensor.
__global__ __launch_bounds__(256) void k_dist_loss(const double* __restrict__ partial, int S_cap,
                                                   const int32_t* __restrict__ dyn_S, float* __restrict__ loss) {
  const int S = dyn_count(S_cap, dyn_S);
  const int nblk = (S + kEdgesPerBlock - 1) / kEdgesPerBlock;
  double acc = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 256) acc += partial[k];
  __shared__ double red[256];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] / (double)S);
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

// Block k owns atoms [k kAtomsPerBlock, ...): dh_i = dA_i w_u + dB_i w_v and the partial row
// part[k] = [sum dA_i h_i (F) | sum dB_i h_i (F) | sum dA_i (1)] over its atoms in ascending order.  Thread t: columns
// t, t + blockDim.x, ...
__global__ void k_dist_dh(const float* __restrict__ h, int N_cap, int F, const float* __restrict__ W,
                          const float* __restrict__ dAB, const int32_t* __restrict__ dyn_N, float* __restrict__ dh,
                          float* __restrict__ part) {
  const int N = dyn_count(N_cap, dyn_N);
  const int i0 = blockIdx.x * kAtomsPerBlock;
  if (i0 >= N) return;
  const int i1 = min(N, i0 + kAtomsPerBlock);
  float* prow = part + (int64_t)blockIdx.x * (2 * F + 1);
  for (int f = threadIdx.x; f < F; f += blockDim.x) {
    const float wu = W[f], wv = W[F + f];
    float su = 0.f, sv = 0.f;
    for (int i = i0; i < i1; ++i) {
      const float dA = dAB[2 * (int64_t)i], dB = dAB[2 * (int64_t)i + 1];
      const float x = h[(int64_t)i * F + f];
      const float g = fmaf(dB, wv, mul_rn(dA, wu));
      dh[(int64_t)i * F + f] = g;
      su = fmaf(dA, x, su);
      sv = fmaf(dB, x, sv);
    }
    prow[f] = su;
    prow[F + f] = sv;
  }
  if (threadIdx.x == 0) {
    float sb = 0.f;
    for (int i = i0; i < i1; ++i) sb += dAB[2 * (int64_t)i];
    prow[2 * F] = sb;
  }
}

// dW[c] / db (+)= the partials of column c summed over the real blocks in block order (compensated).
__global__ __launch_bounds__(256) void k_dist_wgrad(const float* __restrict__ part, int N_cap, int F,
                                                    const int32_t* __restrict__ dyn_N, float* __restrict__ dW,
                                                    float* __restrict__ db, int accumulate) {
  const int N = dyn_count(N_cap, dyn_N);
  const int nblk = (N + kAtomsPerBlock - 1) / kAtomsPerBlock;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c > 2 * F) return;
  const float s = kahan_sum_strided(part + c, 0, nblk, 2 * F + 1);
  float* o = c < 2 * F ? dW + c : db;
  *o = accumulate ? *o + s : s;
}

inline int proj_blocks(int64_t N) {
  const int64_t need = (N + kProjBlock / 64 - 1) / (kProjBlock / 64);
  return (int)std::max<int64_t>(1, std::min<int64_t>(need, 2048));
}

inline int64_t edge_blocks(int64_t S) { return std::max<int64_t>(1, (S + kEdgesPerBlock - 1) / kEdgesPerBlock); }
inline int64_t atom_blocks(int64_t N) { return std::max<int64_t>(1, (N + kAtomsPerBlock - 1) / kAtomsPerBlock); }

inline bool width_ok(int F) { return F == 64 || F == 128 || F == 256 || F == 512; }

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
    const dim3 grid(proj_blocks(N));
    switch (F) {
      case 64: hipLaunchKernelGGL(k_dist_project<1>, grid, dim3(kProjBlock), 0, stream, h, (int)N, W, dyn_N, proj); break;
      case 128: hipLaunchKernelGGL(k_dist_project<2>, grid, dim3(kProjBlock), 0, stream, h, (int)N, W, dyn_N, proj); break;
      case 256: hipLaunchKernelGGL(k_dist_project<4>, grid, dim3(kProjBlock), 0, stream, h, (int)N, W, dyn_N, proj); break;
      default: hipLaunchKernelGGL(k_dist_project<8>, grid, dim3(kProjBlock), 0, stream, h, (int)N, W, dyn_N, proj); break;
    }
    GEOSSL_CHECK_LAUNCH();
  }
  double* partial = reinterpret_cast<double*>(workspace);
  if (S > 0) {
    hipLaunchKernelGGL(k_dist_edges, dim3((unsigned)edge_blocks(S)), dim3(kEdgeBlock), 0, stream, proj, bias, pos, sei0,
                       sei1, (int)S, dyn_S, pred, sgn, partial);
    GEOSSL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_dist_loss, dim3(1), dim3(256), 0, stream, partial, (int)S, dyn_S, loss);
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
    hipLaunchKernelGGL(k_dist_dh, dim3((unsigned)atom_blocks(N)), dim3(std::min(F, 256)), 0, stream, h, (int)N, F, W,
                       dAB, dyn_N, dh, part);
    GEOSSL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_dist_wgrad, dim3((unsigned)((2 * F + 1 + 255) / 256)), dim3(256), 0, stream, part, (int)N, F,
                     dyn_N, dW, db, accumulate);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_distance_head_bwd(const float* h, int64_t N, int F, const float* W, const int64_t* sei0, int64_t S,
                                        const float* sgn, const int64_t* inc_ptr, const int32_t* inc_idx,
                                        const float* gout, float* dh, float* dW, float* db, float* workspace,
                                        int accumulate, hipStream_t stream) {
  return geossl_distance_head_bwd_dyn(h, N, F, W, sei0, S, sgn, inc_ptr, inc_idx, gout, dh, dW, db, workspace,
                                      accumulate, nullptr, nullptr, stream);
}
