// Supervised property head of examples/pretrain_Supervised.py:79-104 and examples/finetune_qm9.py:163-275 (train) /
// :278-384 (eval): the backbone's readout, graph_pred_linear, the normalised target and the L1 / MSE mean, forward and
// backward.
//
// Heads: 0 = SchNet's Linear(F, 1) (w [F], b [1]); 1 = PaiNN's create_output_layers() at its defaults,
// Dense(F, F/2, silu) then Dense(F/2, 1) (W1 [F/2][F], b1 [F/2], w2 [F/2], b2 [1]).
//
// Forward, k_prop_fwd (kTile molecules per block, thread j = feature j):
//   m_b = readout of the atom rows of molecule b ("add": a sum in atom order, "mean": that sum / max(n_b, 1) -
//     readout_col of common.h, the function k_segment_reduce_fwd calls, so the head's readout has the backbone's bits);
//   head 1: z_bk = b1_k + sum_j W1_kj m_bj (fp32 fma chain in j order), a_bk = silu(z_bk);
//   pred_b = bias + <w, m_b> (head 0) or b2 + <w2, a_b> (head 1): lane products, a fixed xor tree per wave, the waves
//     added in order;
//   t_b = (y_b - mean) / std (fp32, a subtract then a divide, the two roundings ATen does); per molecule |pred_b - t_b|
//     (L1) or (pred_b - t_b)^2 (MSE) into an fp64 slot.  Predict mode writes pred_b * std + mean instead (eval()).
//   k_head_loss<1> (head_common.h, one block): the B slots added in a fixed order, / B, stored as fp32.
// Backward, c = gout[0] / B: dpred_b = c sign(pred_b - t_b) (sign(0) = 0, torch's sgn) or (2 / B) (pred_b - t_b) gout[0].
//   k_prop_bwd (kTile molecules per block): dm_b = dpred_b w (head 0), or dz_bk = dpred_b w2_k silu'(z_bk) and
//     dm_bj = sum_k dz_bk W1_kj (head 1); dh_i = dm_b (/ max(n_b, 1) for "mean") for every atom i of molecule b.
//   k_head_vgrad (head_common.h, one thread per column): dw = sum_b dpred_b m_b, db = sum_b dpred_b (head 0);
//     dw2 = sum_b dpred_b a_b, db2 = sum_b dpred_b (head 1), in molecule order.  dW1 = dz^T m and db1 are the caller's
//     (geossl_linear_wgrad).
// Every sum has a fixed order and there are no atomics: the same inputs give the same bits.
// mean and std are read from stats [2] in device memory, so a replayed graph picks up new values.
// Capacity launches (`_dyn`): N is a capacity and the real atom count is read from dyn_N; mol_ptr [B + 1] holds the real
// offsets (B is exact).  No atom row at or past the real count is read or written.
#include "geossl_hip.h"
#include "head_common.h"

using namespace geossl;

namespace {

constexpr int kTile = 4;   // molecules per block of k_prop_fwd / k_prop_bwd

enum Head { kLinear = 0, kMlp = 1 };
enum Mode { kL1 = 0, kMse = 1, kPredict = 2 };

// t_b = (y_b - mean) / std with ATen's two roundings
__device__ __forceinline__ float norm_target(float y, float mean, float sd) { return sub_rn(y, mean) / sd; }

__device__ __forceinline__ float dpred_of(float d, int mode, float gout, int B) {
  if (mode == kL1) {
    const float c = gout / (float)B;
    return d > 0.0f ? c : (d < 0.0f ? -c : 0.0f);
  }
  return mul_rn(mul_rn((float)(2.0 / (double)B), d), gout);
}

template <int F, bool MLP>
__global__ __launch_bounds__(F) void k_prop_fwd(const float* __restrict__ h, int N_cap, const int32_t* __restrict__ dyn_N,
                                                const int32_t* __restrict__ mol_ptr, int B, int readout,
                                                const float* __restrict__ W1, const float* __restrict__ b1,
                                                const float* __restrict__ W2, const float* __restrict__ b2,
                                                const float* __restrict__ y, int64_t y_stride,
                                                const float* __restrict__ stats, int mode, float* __restrict__ m_out,
                                                float* __restrict__ z_out, float* __restrict__ pred,
                                                double* __restrict__ part) {
  constexpr int K = MLP ? F / 2 : F;   // inputs of the last layer
  constexpr int W = F / 64;            // waves per block
  __shared__ float sm[kTile][F];
  __shared__ float sa[kTile][MLP ? F / 2 : 1];
  __shared__ float red[kTile][W];
  const int j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const int b0 = blockIdx.x * kTile;
  const int n_real = dyn_count(N_cap, dyn_N);
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    const int b = b0 + t;
    float v = 0.0f;
    if (b < B) {
      const int a0 = min(mol_ptr[b], n_real), a1 = min(mol_ptr[b + 1], n_real);
      v = readout_col(h, F, j, a0, a1, readout == kMean);
      if (m_out != nullptr) m_out[(size_t)b * F + j] = v;
    }
    sm[t][j] = v;
  }
  __syncthreads();
  float prod[kTile];
  if constexpr (MLP) {
    if (j < K) {
      float acc[kTile];
      const float bk = b1[j];
#pragma unroll
      for (int t = 0; t < kTile; ++t) acc[t] = bk;
      // (scalar loads: a parameter of a flat buffer has no 16-byte alignment to rely on)
      const float* wrow = W1 + (size_t)j * F;
#pragma unroll 8
      for (int q = 0; q < F; ++q) {
        const float w = wrow[q];
#pragma unroll
        for (int t = 0; t < kTile; ++t) acc[t] = fmaf(w, sm[t][q], acc[t]);
      }
      const float w2 = W2[j];
#pragma unroll
      for (int t = 0; t < kTile; ++t) {
        if (b0 + t < B && z_out != nullptr) z_out[(size_t)(b0 + t) * K + j] = acc[t];
        prod[t] = mul_rn(w2, siluf_(acc[t]));
      }
    } else {
#pragma unroll
      for (int t = 0; t < kTile; ++t) prod[t] = 0.0f;
    }
  } else {
    const float wj = W1[j];
#pragma unroll
    for (int t = 0; t < kTile; ++t) prod[t] = mul_rn(wj, sm[t][j]);
  }
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    const float s = wave_sum(prod[t]);
    if (lane == 0) red[t][wave] = s;
  }
  __syncthreads();
  if (j < kTile) {
    const int b = b0 + j;
    if (b < B) {
      float s = 0.0f;
#pragma unroll
      for (int w = 0; w < W; ++w) s += red[j][w];
      const float p = s + (MLP ? b2[0] : b1[0]);
      const float mean = stats[0], sd = stats[1];
      if (mode == kPredict) {
        pred[b] = add_rn(mul_rn(p, sd), mean);
      } else {
        pred[b] = p;
        const float d = sub_rn(p, norm_target(y[(size_t)b * y_stride], mean, sd));
        part[b] = mode == kL1 ? (double)fabsf(d) : (double)mul_rn(d, d);
      }
    }
  }
}

template <int F, bool MLP>
__global__ __launch_bounds__(F) void k_prop_bwd(int N_cap, const int32_t* __restrict__ dyn_N,
                                                const int32_t* __restrict__ mol_ptr, int B, int readout,
                                                const float* __restrict__ W1, const float* __restrict__ W2,
                                                const float* __restrict__ z, const float* __restrict__ pred,
                                                const float* __restrict__ y, int64_t y_stride,
                                                const float* __restrict__ stats, int mode,
                                                const float* __restrict__ gout, float* __restrict__ dh,
                                                float* __restrict__ dz_out, float* __restrict__ dpred_out) {
  constexpr int K = F / 2;
  __shared__ float sdz[kTile][MLP ? F / 2 : 1];
  const int j = threadIdx.x;
  const int b0 = blockIdx.x * kTile;
  const int n_real = dyn_count(N_cap, dyn_N);
  const float g = gout[0], mean = stats[0], sd = stats[1];
  float dp[kTile];
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    const int b = b0 + t;
    dp[t] = 0.0f;
    if (b < B) {
      const float d = sub_rn(pred[b], norm_target(y[(size_t)b * y_stride], mean, sd));
      dp[t] = dpred_of(d, mode, g, B);
      if (j == 0) dpred_out[b] = dp[t];
    }
  }
  float dm[kTile];
  if constexpr (MLP) {
    if (j < K) {
      const float w2 = W2[j];
#pragma unroll
      for (int t = 0; t < kTile; ++t) {
        const int b = b0 + t;
        float v = 0.0f;
        if (b < B) {
          const float zk = z[(size_t)b * K + j];
          const float s = sigmoidf_(zk);
          v = mul_rn(mul_rn(dp[t], w2), s * (1.0f + zk * (1.0f - s)));
          dz_out[(size_t)b * K + j] = v;
        }
        sdz[t][j] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kTile; ++t) dm[t] = 0.0f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const float w = W1[(size_t)k * F + j];
#pragma unroll
      for (int t = 0; t < kTile; ++t) dm[t] = fmaf(sdz[t][k], w, dm[t]);
    }
  } else {
    const float wj = W1[j];
#pragma unroll
    for (int t = 0; t < kTile; ++t) dm[t] = mul_rn(dp[t], wj);
  }
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    const int b = b0 + t;
    if (b >= B) break;
    const int a0 = min(mol_ptr[b], n_real), a1 = min(mol_ptr[b + 1], n_real);
    scatter_readout_col(dh, F, j, a0, a1, dm[t], readout == kMean);
  }
}

__global__ __launch_bounds__(256) void k_prop_targets(const float* __restrict__ y, int64_t M, int T, int task,
                                                      const int64_t* __restrict__ off, const int32_t* __restrict__ src_off,
                                                      int B, float* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int64_t s = src_off[b];
  int64_t lo = 0, hi = M;   // the molecule m with off[m] == s: off is strictly increasing (every molecule has atoms)
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= s) lo = mid; else hi = mid;
  }
  out[b] = (M > 0 && off[lo] == s) ? y[lo * T + task] : __int_as_float(0x7fc00000);
}

inline bool width_ok(int F) { return F == 64 || F == 128 || F == 256; }

inline bool args_ok(int64_t N, int F, int64_t B, int readout, int head, int mode) {
  return N >= 0 && N < (1 << 30) && B >= 1 && B < (1 << 24) && width_ok(F) && (readout == kAdd || readout == kMean) &&
         (head == kLinear || head == kMlp) && mode >= kL1 && mode <= kPredict;
}

template <int F>
void launch_fwd(int head, dim3 grid, hipStream_t stream, const float* h, int N, const int32_t* dyn_N,
                const int32_t* mol_ptr, int B, int readout, const float* W1, const float* b1, const float* W2,
                const float* b2, const float* y, int64_t ys, const float* stats, int mode, float* m, float* z,
                float* pred, double* part) {
  if (head == kMlp)
    hipLaunchKernelGGL((k_prop_fwd<F, true>), grid, dim3(F), 0, stream, h, N, dyn_N, mol_ptr, B, readout, W1, b1, W2,
                       b2, y, ys, stats, mode, m, z, pred, part);
  else
    hipLaunchKernelGGL((k_prop_fwd<F, false>), grid, dim3(F), 0, stream, h, N, dyn_N, mol_ptr, B, readout, W1, b1, W2,
                       b2, y, ys, stats, mode, m, z, pred, part);
}

template <int F>
void launch_bwd(int head, dim3 grid, hipStream_t stream, int N, const int32_t* dyn_N, const int32_t* mol_ptr, int B,
                int readout, const float* W1, const float* W2, const float* z, const float* pred, const float* y,
                int64_t ys, const float* stats, int mode, const float* gout, float* dh, float* dz, float* dpred) {
  if (head == kMlp)
    hipLaunchKernelGGL((k_prop_bwd<F, true>), grid, dim3(F), 0, stream, N, dyn_N, mol_ptr, B, readout, W1, W2, z, pred,
                       y, ys, stats, mode, gout, dh, dz, dpred);
  else
    hipLaunchKernelGGL((k_prop_bwd<F, false>), grid, dim3(F), 0, stream, N, dyn_N, mol_ptr, B, readout, W1, W2, z, pred,
                       y, ys, stats, mode, gout, dh, dz, dpred);
}

int fwd_impl(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, int head,
             const float* W1, const float* b1, const float* W2, const float* b2, const float* y, int64_t y_stride,
             const float* stats, int mode, float* m, float* z, float* pred, float* workspace, float* loss,
             const int32_t* dyn_N, hipStream_t stream) {
  if (!args_ok(N, F, B, readout, head, mode) || W1 == nullptr || b1 == nullptr || stats == nullptr || pred == nullptr ||
      (head == kMlp && (W2 == nullptr || b2 == nullptr)) ||
      (mode != kPredict && (y == nullptr || y_stride < 1 || workspace == nullptr || loss == nullptr)))
    return (int)hipErrorInvalidValue;
  double* part = reinterpret_cast<double*>(workspace);
  const dim3 tiles((unsigned)((B + kTile - 1) / kTile));
  dispatch_int<64, 128, 256>(F, [&](auto f) {
    launch_fwd<decltype(f)::value>(head, tiles, stream, h, (int)N, dyn_N, mol_ptr, (int)B, readout, W1, b1, W2, b2, y,
                                   y_stride, stats, mode, m, z, pred, part);
  });
  GEOSSL_CHECK_LAUNCH();
  if (mode != kPredict) {
    hipLaunchKernelGGL(k_head_loss<1>, dim3(1), dim3(kLossBlock), 0, stream, part, 0, (int)B, nullptr, loss);
    GEOSSL_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" int geossl_property_width_ok(int F) { return width_ok(F) ? 1 : 0; }

extern "C" int64_t geossl_property_workspace_floats(int64_t B) { return 2 * (B > 0 ? B : 1); }

extern "C" int geossl_property_fwd_dyn(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout,
                                       int head, const float* W1, const float* b1, const float* W2, const float* b2,
                                       const float* y, int64_t y_stride, const float* stats, int loss_kind, float* m,
                                       float* z, float* pred, float* workspace, float* loss, const int32_t* dyn_N,
                                       hipStream_t stream) {
  if (loss_kind != kL1 && loss_kind != kMse) return (int)hipErrorInvalidValue;
  if (m == nullptr || (head == kMlp && z == nullptr)) return (int)hipErrorInvalidValue;
  return fwd_impl(h, N, F, mol_ptr, B, readout, head, W1, b1, W2, b2, y, y_stride, stats, loss_kind, m, z, pred,
                  workspace, loss, dyn_N, stream);
}

extern "C" int geossl_property_fwd(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout,
                                   int head, const float* W1, const float* b1, const float* W2, const float* b2,
                                   const float* y, int64_t y_stride, const float* stats, int loss_kind, float* m, float* z,
                                   float* pred, float* workspace, float* loss, hipStream_t stream) {
  return geossl_property_fwd_dyn(h, N, F, mol_ptr, B, readout, head, W1, b1, W2, b2, y, y_stride, stats, loss_kind, m,
                                 z, pred, workspace, loss, nullptr, stream);
}

extern "C" int geossl_property_predict_dyn(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B,
                                           int readout, int head, const float* W1, const float* b1, const float* W2,
                                           const float* b2, const float* stats, float* pred, const int32_t* dyn_N,
                                           hipStream_t stream) {
  return fwd_impl(h, N, F, mol_ptr, B, readout, head, W1, b1, W2, b2, nullptr, 0, stats, kPredict, nullptr, nullptr,
                  pred, nullptr, nullptr, dyn_N, stream);
}

extern "C" int geossl_property_predict(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout,
                                       int head, const float* W1, const float* b1, const float* W2, const float* b2,
                                       const float* stats, float* pred, hipStream_t stream) {
  return geossl_property_predict_dyn(h, N, F, mol_ptr, B, readout, head, W1, b1, W2, b2, stats, pred, nullptr, stream);
}

extern "C" int geossl_property_bwd_dyn(int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, int head,
                                       const float* W1, const float* W2, const float* m, const float* z,
                                       const float* pred, const float* y, int64_t y_stride, const float* stats,
                                       int loss_kind, const float* gout, float* dh, float* dz, float* dw, float* db,
                                       float* workspace, int accumulate, const int32_t* dyn_N, hipStream_t stream) {
  if (!args_ok(N, F, B, readout, head, loss_kind) || loss_kind == kPredict || W1 == nullptr || m == nullptr ||
      pred == nullptr || y == nullptr || y_stride < 1 || stats == nullptr || gout == nullptr || dh == nullptr ||
      workspace == nullptr || (head == kMlp && (W2 == nullptr || z == nullptr || dz == nullptr)))
    return (int)hipErrorInvalidValue;
  const dim3 tiles((unsigned)((B + kTile - 1) / kTile));
  float* dpred = workspace;
  dispatch_int<64, 128, 256>(F, [&](auto f) {
    launch_bwd<decltype(f)::value>(head, tiles, stream, (int)N, dyn_N, mol_ptr, (int)B, readout, W1, W2, z, pred, y,
                                   y_stride, stats, loss_kind, gout, dh, dz, dpred);
  });
  GEOSSL_CHECK_LAUNCH();
  if (dw != nullptr || db != nullptr) {
    const int K = head == kMlp ? F / 2 : F;
    const dim3 cols((unsigned)((K + 1 + 255) / 256));
    // v = silu(z) for head 1, m for head 0: one [B][K] block
    if (head == kMlp)
      hipLaunchKernelGGL(k_head_vgrad<true>, cols, dim3(256), 0, stream, z, K, K, (int)B, dpred, dw, db, accumulate);
    else
      hipLaunchKernelGGL(k_head_vgrad<false>, cols, dim3(256), 0, stream, m, K, K, (int)B, dpred, dw, db, accumulate);
    GEOSSL_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int geossl_property_bwd(int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, int head,
                                   const float* W1, const float* W2, const float* m, const float* z, const float* pred,
                                   const float* y, int64_t y_stride, const float* stats, int loss_kind,
                                   const float* gout, float* dh, float* dz, float* dw, float* db, float* workspace,
                                   int accumulate, hipStream_t stream) {
  return geossl_property_bwd_dyn(N, F, mol_ptr, B, readout, head, W1, W2, m, z, pred, y, y_stride, stats, loss_kind,
                                 gout, dh, dz, dw, db, workspace, accumulate, nullptr, stream);
}

extern "C" int geossl_property_targets(const float* y, int64_t M, int T, int task_id, const int64_t* mol_off,
                                       const int32_t* src_off, int64_t B, float* out, hipStream_t stream) {
  if (y == nullptr || mol_off == nullptr || src_off == nullptr || out == nullptr || M < 0 || T < 1 || task_id < 0 ||
      task_id >= T || B < 0 || B >= (1 << 24))
    return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  hipLaunchKernelGGL(k_prop_targets, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, y, M, T, task_id, mol_off,
                     src_off, (int)B, out);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
