// Pair head of examples/finetune_lep.py:33-45 (train) / :77-90 (eval): the backbone's readout of the active and the
// inactive conformation of every protein-ligand pair, torch.cat(dim=1), graph_pred_linear = Linear(2F, 1), squeeze and
// BCEWithLogitsLoss (mean), forward and backward.
//
// The 2B structures of the batch are [active 0 .. B-1 | inactive 0 .. B-1]: pair b is the structures b and B + b, and
// mol_ptr [2B + 1] holds their atom offsets.  w [2F] is the head's weight row (w[0:F] meets the active readout,
// w[F:2F] the inactive one), b [1] its bias, y [B] the labels as float32.
//
// Forward, k_pair_fwd (kTile pairs per block, thread j = feature j; F = 32 runs in a 64-thread block whose upper
// lanes add zeros):
//   m_s = readout of the atom rows of structure s ("add": a sum in atom order, "mean": that sum / max(n_s, 1) -
//     readout_col of common.h, the function k_segment_reduce_fwd calls, so the head's readout has the backbone's bits);
//   z_b = (sum over the waves of <w[0:F], m_b>, then of <w[F:2F], m_{B+b}>) + b: lane products, a fixed xor tree per
//     wave, the waves added in order, the active side first;
//   per pair the BCE-with-logits term in the overflow-safe form max(z, 0) - z y + log1p(exp(-|z|)), evaluated in fp64
//     from the fp32 logit, into an fp64 slot.  Predict mode writes z only.
//   k_head_loss<1> (head_common.h, one block; the property head's): the B slots added in a fixed order, / B, stored as
//     fp32.
// Backward: dz_b = gout[0] (sigmoid(z_b) - y_b) / B.
//   k_pair_bwd (kTile pairs per block): dh_i = dz_b w[side F + j] (/ max(n_s, 1) for "mean") for every atom i of the
//     two structures of pair b - every atom row is written exactly once.
//   k_head_vgrad (head_common.h, one thread per column): dw[side F + j] = sum_b dz_b m[side B + b][j], db = sum_b dz_b,
//     in pair order.
// Every sum has a fixed order and there are no atomics: the same inputs give the same bits.
// Capacity launches (`_dyn`): N is a capacity and the real atom count is read from dyn_N; mol_ptr [2B + 1] holds the real
// offsets (B is exact).  No atom row at or past the real count is read or written.  The exact forms are the same kernels
// with dyn_N = nullptr: the clamp is to N, as before.
#include "geossl_hip.h"
#include "head_common.h"

using namespace geossl;

namespace {

constexpr int kTile = 4;   // pairs per block of k_pair_fwd / k_pair_bwd

template <int F>
__global__ __launch_bounds__(F < 64 ? 64 : F) void k_pair_fwd(const float* __restrict__ h, int N_cap,
                                                              const int32_t* __restrict__ dyn_N,
                                                              const int32_t* __restrict__ mol_ptr, int B, int readout,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              const float* __restrict__ y, float* __restrict__ m_out,
                                                              float* __restrict__ z_out, double* __restrict__ part) {
  constexpr int T = F < 64 ? 64 : F;   // threads per block
  constexpr int W = T / 64;            // waves per block
  __shared__ float red[kTile][2][W];
  const int j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const int b0 = blockIdx.x * kTile;
  const bool live = j < F;
  const int N = dyn_count(N_cap, dyn_N);
  const float w0 = live ? w[j] : 0.0f, w1 = live ? w[F + j] : 0.0f;
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    const int b = b0 + t;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      float v = 0.0f;
      if (b < B && live) {
        const int s = side * B + b;
        const int a0 = min(mol_ptr[s], N), a1 = min(mol_ptr[s + 1], N);
        v = readout_col(h, F, j, a0, a1, readout == kMean);
        if (m_out != nullptr) m_out[(size_t)s * F + j] = v;
      }
      const float p = wave_sum(mul_rn(side == 0 ? w0 : w1, v));
      if (lane == 0) red[t][side][wave] = p;
    }
  }
  __syncthreads();
  if (j < kTile) {
    const int b = b0 + j;
    if (b < B) {
      float s = 0.0f;
#pragma unroll
      for (int side = 0; side < 2; ++side)
#pragma unroll
        for (int q = 0; q < W; ++q) s += red[j][side][q];
      const float z = s + bias[0];
      z_out[b] = z;
      if (part != nullptr) {
        const double zd = (double)z, yd = (double)y[b];
        part[b] = fmax(zd, 0.0) - zd * yd + log1p(exp(-fabs(zd)));
      }
    }
  }
}

template <int F>
__global__ __launch_bounds__(F < 64 ? 64 : F) void k_pair_bwd(int N_cap, const int32_t* __restrict__ dyn_N,
                                                              const int32_t* __restrict__ mol_ptr, int B,
                                                              int readout, const float* __restrict__ w,
                                                              const float* __restrict__ z, const float* __restrict__ y,
                                                              const float* __restrict__ gout, float* __restrict__ dh,
                                                              float* __restrict__ dz_out) {
  const int j = threadIdx.x;
  const int b0 = blockIdx.x * kTile;
  const int N = dyn_count(N_cap, dyn_N);
  const float g = gout[0];
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    const int b = b0 + t;
    if (b >= B) break;
    const float dz = g * (sigmoidf_(z[b]) - y[b]) / (float)B;
    if (j == 0) dz_out[b] = dz;
    if (j >= F) continue;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int s = side * B + b;
      const int a0 = min(mol_ptr[s], N), a1 = min(mol_ptr[s + 1], N);
      scatter_readout_col(dh, F, j, a0, a1, mul_rn(dz, w[side * F + j]), readout == kMean);
    }
  }
}

inline bool width_ok(int F) { return F == 32 || F == 64 || F == 128; }

inline bool args_ok(int64_t N, int F, int64_t B, int readout) {
  return N >= 0 && N < (1 << 30) && B >= 1 && B < (1 << 23) && width_ok(F) && (readout == kAdd || readout == kMean);
}

int fwd_impl(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, const float* w,
             const float* b, const float* y, float* m, float* z, float* workspace, float* loss, bool predict,
             const int32_t* dyn_N, hipStream_t stream) {
  if (!args_ok(N, F, B, readout) || mol_ptr == nullptr || w == nullptr || b == nullptr || z == nullptr ||
      (N > 0 && h == nullptr) || (!predict && (y == nullptr || m == nullptr || workspace == nullptr || loss == nullptr)))
    return (int)hipErrorInvalidValue;
  double* part = predict ? nullptr : reinterpret_cast<double*>(workspace);
  const dim3 tiles((unsigned)((B + kTile - 1) / kTile));
  dispatch_int<32, 64, 128>(F, [&](auto f) {
    hipLaunchKernelGGL(k_pair_fwd<decltype(f)::value>, tiles, dim3(std::max(F, 64)), 0, stream, h, (int)N, dyn_N, mol_ptr,
                       (int)B, readout, w, b, y, m, z, part);
  });
  GEOSSL_CHECK_LAUNCH();
  if (!predict) {
    hipLaunchKernelGGL(k_head_loss<1>, dim3(1), dim3(kLossBlock), 0, stream, part, 0, (int)B, nullptr, loss);
    GEOSSL_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

extern "C" int geossl_pair_head_width_ok(int F) { return width_ok(F) ? 1 : 0; }

extern "C" int64_t geossl_pair_head_workspace_floats(int64_t B) { return 2 * (B > 0 ? B : 1); }

extern "C" int geossl_pair_head_fwd_dyn(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout,
                                        const float* w, const float* b, const float* y, float* m, float* z,
                                        float* workspace, float* loss, const int32_t* dyn_N, hipStream_t stream) {
  return fwd_impl(h, N, F, mol_ptr, B, readout, w, b, y, m, z, workspace, loss, false, dyn_N, stream);
}

extern "C" int geossl_pair_head_fwd(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout,
                                    const float* w, const float* b, const float* y, float* m, float* z,
                                    float* workspace, float* loss, hipStream_t stream) {
  return geossl_pair_head_fwd_dyn(h, N, F, mol_ptr, B, readout, w, b, y, m, z, workspace, loss, nullptr, stream);
}

extern "C" int geossl_pair_head_predict_dyn(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B,
                                            int readout, const float* w, const float* b, float* z,
                                            const int32_t* dyn_N, hipStream_t stream) {
  return fwd_impl(h, N, F, mol_ptr, B, readout, w, b, nullptr, nullptr, z, nullptr, nullptr, true, dyn_N, stream);
}

extern "C" int geossl_pair_head_predict(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B,
                                        int readout, const float* w, const float* b, float* z, hipStream_t stream) {
  return geossl_pair_head_predict_dyn(h, N, F, mol_ptr, B, readout, w, b, z, nullptr, stream);
}

extern "C" int geossl_pair_head_bwd_dyn(int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, const float* w,
                                        const float* m, const float* z, const float* y, const float* gout, float* dh,
                                        float* dw, float* db, float* workspace, int accumulate, const int32_t* dyn_N,
                                        hipStream_t stream) {
  if (!args_ok(N, F, B, readout) || mol_ptr == nullptr || w == nullptr || m == nullptr || z == nullptr ||
      y == nullptr || gout == nullptr || (N > 0 && dh == nullptr) || workspace == nullptr)
    return (int)hipErrorInvalidValue;
  const dim3 tiles((unsigned)((B + kTile - 1) / kTile));
  float* dz = workspace;
  dispatch_int<32, 64, 128>(F, [&](auto f) {
    hipLaunchKernelGGL(k_pair_bwd<decltype(f)::value>, tiles, dim3(std::max(F, 64)), 0, stream, (int)N, dyn_N, mol_ptr,
                       (int)B, readout, w, z, y, gout, dh, dz);
  });
  GEOSSL_CHECK_LAUNCH();
  if (dw != nullptr || db != nullptr) {
    // column c < 2F is column c % F of the [B][F] readouts of side c / F
    hipLaunchKernelGGL(k_head_vgrad<false>, dim3((unsigned)((2 * F + 1 + 255) / 256)), dim3(256), 0, stream, m, 2 * F, F,
                       (int)B, dz, dw, db, accumulate);
    GEOSSL_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int geossl_pair_head_bwd(int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout, const float* w,
                                    const float* m, const float* z, const float* y, const float* gout, float* dh,
                                    float* dw, float* db, float* workspace, int accumulate, hipStream_t stream) {
  return geossl_pair_head_bwd_dyn(N, F, mol_ptr, B, readout, w, m, z, y, gout, dh, dw, db, workspace, accumulate, nullptr,
                                  stream);
}
