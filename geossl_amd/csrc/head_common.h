// Building blocks shared by the fused loss heads (distance_head.hip, torsion_head.hip, charge_head.hip,
// infograph_head.hip, property_head.hip, pair_head.hip).  The heads' numerical contract is "fixed order, no atomics, same
// bits"; every order that more than one head uses is written down here once:
//   block_sum / k_head_loss                 the fp64 tree over a block, and the one-block loss step on top of it;
//   k_cat_project / k_cat_dh / k_cat_wgrad  Linear(K F, 1) on a concatenation of K atom rows as K per-atom projections
//                                           (distance: K = 2, torsion: K = 3), forward and backward;
//   k_head_vgrad                            per-column sums over the molecules for the gradients of a last layer;
//   dispatch_int                            a runtime width to a template argument.
// The readout (readout_col, scatter_readout_col) and the scalar functions live in common.h: the backbone uses them too.
#pragma once
#include "common.h"

#include <algorithm>
#include <type_traits>

namespace geossl {

constexpr int kProjBlock = 256;       // k_cat_project: 4 waves, one atom per wave at a time
constexpr int kAtomsPerBlock = 32;    // k_cat_dh: atoms per block (one partial row of dW / db per block)
constexpr int kLossBlock = 256;       // k_head_loss: one block of this many threads

// Sum of v over a block of T threads through red [T] in LDS: store, barrier, then red[t] += red[t + o] for
// o = T/2 ... 1.  V: double, or a struct of several sums with operator+= (one tree for all of them).
template <int T, class V>
__device__ __forceinline__ V block_sum(V v, V* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}
template <int T>
__device__ __forceinline__ double block_sum_f64(double v) {
  __shared__ double red[T];
  return block_sum<T>(v, red);
}

// One block: loss = (sum of the fp64 slots) / count, stored as fp32; count = the real row count (`dyn`, else `cap`).
// Thread t adds the slots t, t + kLossBlock, ... in order, then the tree.  count = 0: 0 / 0 = NaN, the mean of an empty
// tensor.  PER_SLOT > 0: every slot is a block partial over PER_SLOT rows, so the ceil(count / PER_SLOT) slots of the
// real rows are added (PER_SLOT = 1: a slot per row); PER_SLOT = 0: `nslots` slots.
template <int PER_SLOT>
__global__ __launch_bounds__(kLossBlock) void k_head_loss(const double* __restrict__ slots, int nslots, int cap,
                                                          const int32_t* __restrict__ dyn, float* __restrict__ loss) {
  const int count = dyn_count(cap, dyn);
  const int n = PER_SLOT > 0 ? (count + PER_SLOT - 1) / PER_SLOT : nslots;
  double acc = 0.0;
  for (int k = threadIdx.x; k < n; k += kLossBlock) acc += slots[k];
  const double s = block_sum_f64<kLossBlock>(acc);
  if (threadIdx.x == 0) loss[0] = (float)(s / (double)count);
}

// proj[i] = (w_0 . h_i, ..., w_{K-1} . h_i), W = [w_0 | ... | w_{K-1}]: lane l holds features [l V, l V + V) of the row
// (F = 64 V), a butterfly over the wave adds the 64 lane sums in a fixed order.
template <int V, int K>
__global__ __launch_bounds__(kProjBlock) void k_cat_project(const float* __restrict__ h, int N_cap,
                                                             const float* __restrict__ W, const int32_t* __restrict__ dyn_N,
                                                             float* __restrict__ proj) {
  constexpr int F = 64 * V;
  const int N = dyn_count(N_cap, dyn_N);
  const int l = threadIdx.x & 63;
  float w[K][V];
#pragma unroll
  for (int k = 0; k < V; ++k)
#pragma unroll
    for (int s = 0; s < K; ++s) w[s][k] = W[s * F + l * V + k];
  const int waves = gridDim.x * (kProjBlock / 64);
  for (int i = blockIdx.x * (kProjBlock / 64) + (threadIdx.x >> 6); i < N; i += waves) {
    const float* row = h + (int64_t)i * F + l * V;
    float a[K];
#pragma unroll
    for (int s = 0; s < K; ++s) a[s] = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float x = row[k];
#pragma unroll
      for (int s = 0; s < K; ++s) a[s] = fmaf(w[s][k], x, a[s]);
    }
#pragma unroll
    for (int s = 0; s < K; ++s) a[s] = wave_sum(a[s]);
    if (l == 0) {
#pragma unroll
      for (int s = 0; s < K; ++s) proj[K * (int64_t)i + s] = a[s];
    }
  }
}

// Block k owns atoms [k kAtomsPerBlock, ...); d [N][K] holds the atoms' gradients of the K projections.
// dh_i = sum_s d_is w_s (a product for s = 0, then an fma per side in side order) and the partial row
// part[k] = [sum_i d_i0 h_i (F) | ... | sum_i d_i,K-1 h_i (F) | sum_i d_i0 (1)] over its atoms in ascending order.
// Thread t: columns t, t + blockDim.x, ...
template <int K>
__global__ void k_cat_dh(const float* __restrict__ h, int N_cap, int F, const float* __restrict__ W,
                         const float* __restrict__ d, const int32_t* __restrict__ dyn_N, float* __restrict__ dh,
                         float* __restrict__ part) {
  const int N = dyn_count(N_cap, dyn_N);
  const int i0 = blockIdx.x * kAtomsPerBlock;
  if (i0 >= N) return;
  const int i1 = min(N, i0 + kAtomsPerBlock);
  float* prow = part + (int64_t)blockIdx.x * (K * F + 1);
  for (int f = threadIdx.x; f < F; f += blockDim.x) {
    float w[K], acc[K];
#pragma unroll
    for (int s = 0; s < K; ++s) {
      w[s] = W[s * F + f];
      acc[s] = 0.f;
    }
    for (int i = i0; i < i1; ++i) {
      float di[K];
#pragma unroll
      for (int s = 0; s < K; ++s) di[s] = d[K * (int64_t)i + s];
      const float x = h[(int64_t)i * F + f];
      float g = mul_rn(di[0], w[0]);
#pragma unroll
      for (int s = 1; s < K; ++s) g = fmaf(di[s], w[s], g);
      dh[(int64_t)i * F + f] = g;
#pragma unroll
      for (int s = 0; s < K; ++s) acc[s] = fmaf(di[s], x, acc[s]);
    }
#pragma unroll
    for (int s = 0; s < K; ++s) prow[s * F + f] = acc[s];
  }
  if (threadIdx.x == 0) {
    float sb = 0.f;
    for (int i = i0; i < i1; ++i) sb += d[K * (int64_t)i];
    prow[K * F] = sb;
  }
}

// dW[c] / db (+)= the partials of column c summed over the real blocks in block order (compensated).
template <int K>
__global__ __launch_bounds__(256) void k_cat_wgrad(const float* __restrict__ part, int N_cap, int F,
                                                   const int32_t* __restrict__ dyn_N, float* __restrict__ dW,
                                                   float* __restrict__ db, int accumulate) {
  const int N = dyn_count(N_cap, dyn_N);
  const int nblk = (N + kAtomsPerBlock - 1) / kAtomsPerBlock;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c > K * F) return;
  const float s = kahan_sum_strided(part + c, 0, nblk, K * F + 1);
  float* o = c < K * F ? dW + c : db;
  *o = accumulate ? *o + s : s;
}

// Vector gradients of a last layer, one thread per column.  Column c < cols: dw[c] (+)= sum_b dpred_b v_b[c] in b order,
// where v is `cols / width` stacked [B][width] blocks and column c is column c % width of block c / width (SILU:
// silu(v) in its place); column `cols`: db (+)= sum_b dpred_b.  A null dw / db is skipped.
template <bool SILU>
__global__ __launch_bounds__(256) void k_head_vgrad(const float* __restrict__ v, int cols, int width, int B,
                                                    const float* __restrict__ dpred, float* __restrict__ dw,
                                                    float* __restrict__ db, int accumulate) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c > cols) return;
  float* out = c < cols ? dw : db;
  if (out == nullptr) return;
  float acc = 0.0f;
  if (c < cols) {
    const float* col = v + (size_t)(c / width) * B * width + (c % width);
#pragma unroll 8
    for (int b = 0; b < B; ++b) {
      const float x = col[(size_t)b * width];
      acc = fmaf(dpred[b], SILU ? siluf_(x) : x, acc);
    }
  } else {
    for (int b = 0; b < B; ++b) acc += dpred[b];
  }
  const int o = c < cols ? c : 0;
  out[o] = accumulate ? out[o] + acc : acc;
}

// fn(std::integral_constant<int, X>) for the X of Xs that equals x (a width, or V = F / 64, as a template argument of
// the launch inside fn); false when x is none of them.
template <int... Xs, class Fn>
inline bool dispatch_int(int x, Fn&& fn) {
  return ((x == Xs ? (fn(std::integral_constant<int, Xs>{}), true) : false) || ...);
}

inline int proj_blocks(int64_t N) {
  const int64_t need = (N + kProjBlock / 64 - 1) / (kProjBlock / 64);
  return (int)std::max<int64_t>(1, std::min<int64_t>(need, 2048));
}
inline int64_t atom_blocks(int64_t N) { return std::max<int64_t>(1, (N + kAtomsPerBlock - 1) / kAtomsPerBlock); }

// F = 64 V with V in (1, 2, 4, 8): a wave holds one row
inline bool wave_row_width_ok(int F) { return F == 64 || F == 128 || F == 256 || F == 512; }

// The three launches of the backward of a K-sided head after its own kernel has filled d [N][K] (workspace: d, then the
// partial rows of k_cat_dh).
template <int K>
inline int launch_cat_bwd(const float* h, int64_t N, int F, const float* W, const float* d, float* part,
                          const int32_t* dyn_N, float* dh, float* dW, float* db, int accumulate, hipStream_t stream) {
  if (N > 0) {
    hipLaunchKernelGGL(k_cat_dh<K>, dim3((unsigned)atom_blocks(N)), dim3(std::min(F, 256)), 0, stream, h, (int)N, F, W, d,
                       dyn_N, dh, part);
    GEOSSL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_cat_wgrad<K>, dim3((unsigned)((K * F + 1 + 255) / 256)), dim3(256), 0, stream, part, (int)N, F,
                     dyn_N, dW, db, accumulate);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

template <int K>
inline int launch_cat_project(const float* h, int64_t N, int F, const float* W, const int32_t* dyn_N, float* proj,
                              hipStream_t stream) {
  dispatch_int<1, 2, 4, 8>(F / 64, [&](auto v) {
    hipLaunchKernelGGL((k_cat_project<decltype(v)::value, K>), dim3(proj_blocks(N)), dim3(kProjBlock), 0, stream, h,
                       (int)N, W, dyn_N, proj);
  });
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

}  // namespace geossl
