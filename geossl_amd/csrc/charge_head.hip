// Charge Prediction of examples/pretrain_ChargePrediction.py:15-25,61-81: the masked-atom draw and its write into the
// atom types, and the head loss = CrossEntropyLoss(Linear(F, C)(node_repr[masked]), charge_actual[masked]), forward and
// backward.
//
// Mask (k_charge_mask, one block): k = trunc((double)N * ratio), Python's int(M * ratio).  The k atoms are either
//   * drawn on the device: atom i gets the 64-bit key (w0 << 32) | w1 of Philox-4x32-10 under the 64-bit seed
//     seed[0] with counter (i, 0, 0, 0), and the k atoms with the smallest (key, i) are taken (a radix select over the
//     keys, 8 bits per pass from the top, that stops as soon as the taken set is decided; equal keys go by index).
//     A uniform k-subset; the list is written in ascending atom order and seed[0] is advanced by one, so a replayed
//     graph draws a fresh mask;
//   * or given: a host-drawn list (np.random.choice) used as it is, in its own order.
// The labels are the atoms' original types x[i, 0]; then x[i, 0] = C - 1 (the mask token) for every listed atom.
//
// Head forward (k_charge_fwd: one wave per masked row, W in LDS): logits = h[idx_j] W^T + b, a max-subtracted
//   log-softmax, term_j = lse_j - logit_j[y_j]; the softmax rows are kept for the backward; per-block fp64 sums of the
//   terms in row order, then one block adds them in block order and divides by k (k_head_loss of head_common.h; k = 0:
//   0 / 0 = NaN, the mean of an empty tensor).  A row whose atom index is outside [0, N) or whose label is outside [0, C) reads nothing, its term is
//   NaN, its softmax row 0, and bit 0 of the status word is set (nn.CrossEntropyLoss raises for such a label).
// Head backward, with g = gout[0] / k (fp32): d_j = (p_j - onehot(y_j)) g;
//   dh = 0 on every atom row, then dh[idx_j] = d_j W for the masked rows (k_charge_bwd_rows);
//   per block of masked rows the partials of dW = sum_j d_j^T h[idx_j] and db = sum_j d_j, added in block order with
//   a compensated sum (k_charge_wgrad).  k = 0: dh, dW and db are exactly zero.
// Every sum has a fixed order and the only atomics count into LDS histograms (integer adds: the same counts in any
// order), so the same inputs and seed give the same bits.
// Capacity launches (`_dyn`): N and K are capacities that size grids and buffers; the real N is read from dyn_N and
// the real k from k_dev (written by the mask launch).  Rows at and past them are neither read nor written.
#include "geossl_hip.h"
#include "head_common.h"

using namespace geossl;

namespace {

constexpr int kMaskThreads = 1024;   // k_charge_mask: one block, thread t owns a contiguous run of atoms
constexpr int kMaskWaves = kMaskThreads / 64;
constexpr int kFwdBlock = 256;       // 4 waves, one masked row per wave at a time
constexpr int kFwdMaxBlocks = 1024;
constexpr int kBwdBlock = 256;
constexpr int kBwdMaxBlocks = 256;   // row blocks of the backward (and partial rows of dW / db)
constexpr int kBwdChunk = 32;        // masked rows staged in LDS at a time
constexpr int kMaxC = 16;
constexpr int kMaxCols = kMaxC * (512 + 1);
constexpr int kColsPerThread = (kMaxCols + kBwdBlock - 1) / kBwdBlock;

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return c;
}

__device__ __forceinline__ uint64_t atom_key(int i, uint2 key) {
  const uint4 r = philox4x32_10(make_uint4((uint32_t)i, 0u, 0u, 0u), key);
  return ((uint64_t)r.x << 32) | r.y;
}

__device__ __forceinline__ int wave_incl_scan_i(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// exclusive prefix of v over the block's threads in thread order; *total = the block's sum.  sh: kMaskWaves ints.
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int* total) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int incl = wave_incl_scan_i(v);
  if (lane == 63) sh[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kMaskWaves; ++w) {
    const int s = sh[w];
    base += w < wave ? s : 0;
    tot += s;
  }
  __syncthreads();   // (sh is reused by the next scan)
  *total = tot;
  return base + incl - v;
}

__device__ __forceinline__ int mask_k(int N, double ratio) {
  const int k = (int)((double)N * ratio);   // truncation toward zero: Python's int()
  return k < 0 ? 0 : (k > N ? N : k);
}

__global__ __launch_bounds__(kMaskThreads) void k_charge_mask(int64_t* __restrict__ x, int x_cols, int N_cap,
                                                              const int32_t* __restrict__ dyn_N, double ratio, int C,
                                                              int64_t* __restrict__ seed,
                                                              const int64_t* __restrict__ given,
                                                              int64_t* __restrict__ idx, int64_t* __restrict__ labels,
                                                              int32_t* __restrict__ k_out) {
  __shared__ int hist[256];
  __shared__ int scan_sh[kMaskWaves];
  __shared__ int pick[3];            // digit, count below it, count in it
  __shared__ uint64_t seed_sh;
  const int N = dyn_count(N_cap, dyn_N);
  const int k = mask_k(N, ratio);
  const int t = threadIdx.x;
  if (t == 0) k_out[0] = k;
  const int64_t token = C - 1;
  if (given != nullptr) {
    // the host's list as it is: labels first (every read before any write: a listed atom twice would otherwise read
    // its own token), then the token
    for (int j = t; j < k; j += kMaskThreads) {
      const int64_t i = given[j];
      idx[j] = i;
      labels[j] = (i >= 0 && i < N) ? x[i * x_cols] : -1;   // (-1: the head reports it)
    }
    __syncthreads();
    for (int j = t; j < k; j += kMaskThreads) {
      const int64_t i = given[j];
      if (i >= 0 && i < N) x[i * x_cols] = token;
    }
    return;
  }
  if (t == 0) seed_sh = (uint64_t)seed[0];
  __syncthreads();
  const uint64_t sd = seed_sh;
  if (t == 0) seed[0] = (int64_t)(sd + 1);   // (every thread holds sd already)
  const uint2 key = make_uint2((uint32_t)sd, (uint32_t)(sd >> 32));
  const int per = (N + kMaskThreads - 1) / kMaskThreads;
  const int a0 = min(N, t * per), a1 = min(N, a0 + per);
  // ---- the k smallest keys: prefix P of the resolved top bits M, `need` of the atoms with (key & M) == P still to take
  uint64_t P = 0, M = 0;
  int need = k;
  bool all_ties = true;   // every atom with (key & M) == P is taken (else: the first `need` of them in index order)
  if (k > 0 && k < N) {
    all_ties = false;
    for (int shift = 56; shift >= 0; shift -= 8) {
      for (int b = t; b < 256; b += kMaskThreads) hist[b] = 0;
      __syncthreads();
      for (int i = a0; i < a1; ++i) {
        const uint64_t kv = atom_key(i, key);
        if ((kv & M) == P) atomicAdd(&hist[(int)((kv >> shift) & 255)], 1);
      }
      __syncthreads();
      if (t < 64) {   // wave 0: the digit whose bin holds the need-th candidate
        const int c0 = hist[4 * t], c1 = hist[4 * t + 1], c2 = hist[4 * t + 2], c3 = hist[4 * t + 3];
        const int incl = wave_incl_scan_i(c0 + c1 + c2 + c3);
        const int excl = incl - (c0 + c1 + c2 + c3);
        if (excl < need && need <= incl) {
          int below = excl, d = 4 * t;
          const int c[4] = {c0, c1, c2, c3};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (below + c[q] >= need) {
              d = 4 * t + q;
              break;
            }
            below += c[q];
          }
          pick[0] = d;
          pick[1] = below;
          pick[2] = hist[d];
        }
      }
      __syncthreads();
      const int d = pick[0];
      need -= pick[1];
      P |= (uint64_t)d << shift;
      M |= (uint64_t)255 << shift;
      const int cnt = pick[2];
      __syncthreads();   // (pick / hist are rewritten by the next pass)
      if (cnt == need) {
        all_ties = true;
        break;
      }
    }
  }
  // ---- compaction in ascending atom order: taken = key < P, or (key & M) == P and among the first `need` such atoms
  int ties = 0;
  if (!all_ties) {
    for (int i = a0; i < a1; ++i) ties += (atom_key(i, key) & M) == P;
  }
  int tot;
  int tie_rank = block_excl_scan(ties, scan_sh, &tot);
  auto taken = [&](int i, int& rank) -> bool {
    if (k == 0) return false;
    if (k == N) return true;
    const uint64_t kv = atom_key(i, key);
    if ((kv & M) == P) {
      if (all_ties) return true;
      return rank++ < need;
    }
    return kv < P;
  };
  int cnt = 0, r = tie_rank;
  for (int i = a0; i < a1; ++i) cnt += taken(i, r);
  int pos = block_excl_scan(cnt, scan_sh, &tot);
  r = tie_rank;
  for (int i = a0; i < a1; ++i) {
    if (taken(i, r)) {
      int64_t* xi = x + (int64_t)i * x_cols;
      idx[pos] = i;
      labels[pos] = xi[0];
      xi[0] = token;
      ++pos;
    }
  }
}

// One wave per masked row j (rows j = wave, wave + waves, ... < k): lane l holds features [l V, l V + V) of h[idx_j].
template <int V>
__global__ __launch_bounds__(kFwdBlock) void k_charge_fwd(const float* __restrict__ h, int N_cap,
                                                         const int32_t* __restrict__ dyn_N,
                                                         const float* __restrict__ W, const float* __restrict__ bias,
                                                         int C, const int64_t* __restrict__ idx,
                                                         const int64_t* __restrict__ labels, int K_cap,
                                                         const int32_t* __restrict__ k_dev, float* __restrict__ prob,
                                                         double* __restrict__ partial, int32_t* __restrict__ status) {
  constexpr int F = 64 * V;
  __shared__ float Ws[kMaxC * F];
  __shared__ float bs[kMaxC];
  __shared__ double wsum[kFwdBlock / 64];
  const int N = dyn_count(N_cap, dyn_N);
  const int k = dyn_count(K_cap, k_dev);
  for (int q = threadIdx.x; q < C * F; q += kFwdBlock) Ws[q] = W[q];
  if (threadIdx.x < C) bs[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int waves = gridDim.x * (kFwdBlock / 64);
  double acc = 0.0;   // (lane 0: this wave's terms in row order)
  for (int j = blockIdx.x * (kFwdBlock / 64) + wave; j < k; j += waves) {
    const int64_t i = idx[j], y = labels[j];
    const bool ok = i >= 0 && i < N && y >= 0 && y < C;   // (uniform over the wave)
    if (!ok) {
      if (l < C) prob[(int64_t)j * C + l] = 0.f;
      if (l == 0) {
        atomicOr(status, 1);   // (a flag: the same word in any order)
        acc += (double)NAN;
      }
      continue;
    }
    float hv[V];
    const float* row = h + i * F + l * V;
#pragma unroll
    for (int v = 0; v < V; ++v) hv[v] = row[v];
    float logit[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) {
      if (c < C) {
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < V; ++v) s = fmaf(hv[v], Ws[c * F + l * V + v], s);
        logit[c] = wave_sum(s) + bs[c];
      }
    }
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) m = fmaxf(m, logit[c]);
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) se += expf(logit[c] - m);
    const float lse = m + logf(se);
    float mine = 0.f, ly = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) {
      if (c < C) {
        if (c == l) mine = logit[c];
        if (c == (int)y) ly = logit[c];
      }
    }
    if (l < C) prob[(int64_t)j * C + l] = expf(mine - lse);
    if (l == 0) acc += (double)(lse - ly);
  }
  if (l == 0) wsum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kFwdBlock / 64; ++w) s += wsum[w];
    partial[blockIdx.x] = s;
  }
}

__global__ void k_charge_zero_rows(float* __restrict__ dh, int N_cap, int F, const int32_t* __restrict__ dyn_N) {
  const int64_t n = (int64_t)dyn_count(N_cap, dyn_N) * F / 4;   // (F is a multiple of 64)
  float4* p = reinterpret_cast<float4*>(dh);
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x)
    p[q] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// Block b owns masked rows [b R, min(k, (b + 1) R)), R = ceil(k / gridDim.x): dh[idx_j] = d_j W, and the partial row
// part[b] = [c][F + 1]: (sum_j d_j[c] h[idx_j][f])_f, sum_j d_j[c], rows in ascending order.
__global__ __launch_bounds__(kBwdBlock) void k_charge_bwd_rows(const float* __restrict__ h, int N_cap, int F,
                                                               const int32_t* __restrict__ dyn_N,
                                                               const float* __restrict__ W, int C,
                                                               const int64_t* __restrict__ idx,
                                                               const int64_t* __restrict__ labels, int K_cap,
                                                               const int32_t* __restrict__ k_dev,
                                                               const float* __restrict__ prob,
                                                               const float* __restrict__ gout, float* __restrict__ dh,
                                                               float* __restrict__ part) {
  extern __shared__ float lds[];
  float* Ws = lds;                                 // [C][F]
  float* ds = Ws + C * F;                          // [kBwdChunk][C]
  __shared__ int64_t rows[kBwdChunk];
  const int N = dyn_count(N_cap, dyn_N);
  const int k = dyn_count(K_cap, k_dev);
  const int R = (k + gridDim.x - 1) / gridDim.x;
  const int j0 = blockIdx.x * R;
  if (R == 0 || j0 >= k) return;
  const int j1 = min(k, j0 + R);
  const float g = gout[0] / (float)k;
  for (int q = threadIdx.x; q < C * F; q += kBwdBlock) Ws[q] = W[q];
  const int cols = C * (F + 1);
  float acc[kColsPerThread];
#pragma unroll
  for (int q = 0; q < kColsPerThread; ++q) acc[q] = 0.f;
  for (int jc = j0; jc < j1; jc += kBwdChunk) {
    const int nr = min(kBwdChunk, j1 - jc);
    __syncthreads();   // (Ws loaded / the previous chunk's ds and rows consumed)
    for (int q = threadIdx.x; q < nr * C; q += kBwdBlock) {
      const int r = q / C, c = q - r * C, j = jc + r;
      const int64_t i = idx[j], y = labels[j];
      const bool ok = i >= 0 && i < N && y >= 0 && y < C;
      ds[q] = ok ? (prob[(int64_t)j * C + c] - (c == (int)y ? 1.f : 0.f)) * g : 0.f;
      if (c == 0) rows[r] = ok ? i : -1;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nr * F; q += kBwdBlock) {
      const int r = q / F, f = q - r * F;
      const int64_t i = rows[r];
      if (i < 0) continue;
      float s = 0.f;
      for (int c = 0; c < C; ++c) s = fmaf(ds[r * C + c], Ws[c * F + f], s);
      dh[i * F + f] = s;
    }
#pragma unroll
    for (int q = 0; q < kColsPerThread; ++q) {
      const int col = q * kBwdBlock + threadIdx.x;
      if (col < cols) {
        const int c = col / (F + 1), f = col - c * (F + 1);
        float s = acc[q];
        for (int r = 0; r < nr; ++r) {
          const int64_t i = rows[r];
          const float hv = f == F ? 1.f : (i >= 0 ? h[i * F + f] : 0.f);
          s = fmaf(ds[r * C + c], hv, s);
        }
        acc[q] = s;
      }
    }
  }
  float* prow = part + (int64_t)blockIdx.x * cols;
#pragma unroll
  for (int q = 0; q < kColsPerThread; ++q) {
    const int col = q * kBwdBlock + threadIdx.x;
    if (col < cols) prow[col] = acc[q];
  }
}

// dW[c][f] / db[c] (+)= the partial rows of the blocks that own masked rows, added in block order (compensated).
__global__ __launch_bounds__(256) void k_charge_wgrad(const float* __restrict__ part, int F, int C, int nblk_cap,
                                                      int K_cap, const int32_t* __restrict__ k_dev,
                                                      float* __restrict__ dW, float* __restrict__ db, int accumulate) {
  const int k = dyn_count(K_cap, k_dev);
  const int R = (k + nblk_cap - 1) / nblk_cap;
  const int nblk = R == 0 ? 0 : (k + R - 1) / R;
  const int cols = C * (F + 1);
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= cols) return;
  const float s = kahan_sum_strided(part + col, 0, nblk, cols);
  const int c = col / (F + 1), f = col - c * (F + 1);
  float* o = f == F ? db + c : dW + c * F + f;
  *o = accumulate ? *o + s : s;
}

inline bool width_ok(int F, int C) { return wave_row_width_ok(F) && C >= 2 && C <= kMaxC; }
inline int fwd_blocks(int64_t K) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((K + kFwdBlock / 64 - 1) / (kFwdBlock / 64), kFwdMaxBlocks));
}
inline int bwd_blocks(int64_t K) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((K + kBwdChunk - 1) / kBwdChunk, kBwdMaxBlocks));
}

}  // namespace

extern "C" int64_t geossl_charge_mask_count(int64_t N, double ratio) {
  const int64_t k = (int64_t)((double)N * ratio);
  return k < 0 ? 0 : (k > N ? N : k);
}

extern "C" int geossl_charge_mask_dyn(int64_t* x, int x_cols, int64_t N, double ratio, int C, int64_t* seed,
                                      const int64_t* given, int64_t* idx, int64_t* labels, int32_t* k,
                                      const int32_t* dyn_N, hipStream_t stream) {
  if (N < 0 || N >= (1 << 30) || x_cols < 1 || !(ratio >= 0.0 && ratio <= 1.0) || C < 2 || C > kMaxC ||
      (seed == nullptr) == (given == nullptr))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_charge_mask, dim3(1), dim3(kMaskThreads), 0, stream, x, x_cols, (int)N, dyn_N, ratio, C, seed,
                     given, idx, labels, k);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_charge_mask(int64_t* x, int x_cols, int64_t N, double ratio, int C, int64_t* seed,
                                  const int64_t* given, int64_t* idx, int64_t* labels, int32_t* k,
                                  hipStream_t stream) {
  return geossl_charge_mask_dyn(x, x_cols, N, ratio, C, seed, given, idx, labels, k, nullptr, stream);
}

extern "C" int geossl_charge_head_width_ok(int F, int C) { return width_ok(F, C) ? 1 : 0; }

extern "C" int64_t geossl_charge_head_fwd_workspace_floats(int64_t K) { return 2 * (int64_t)fwd_blocks(K); }

extern "C" int64_t geossl_charge_head_bwd_workspace_floats(int64_t K, int F, int C) {
  return (int64_t)bwd_blocks(K) * C * ((int64_t)F + 1);
}

extern "C" int geossl_charge_head_fwd_dyn(const float* h, int64_t N, int F, const float* W, const float* bias, int C,
                                          const int64_t* idx, const int64_t* labels, int64_t K, const int32_t* k_dev,
                                          float* prob, float* workspace, float* loss, int32_t* status,
                                          const int32_t* dyn_N, hipStream_t stream) {
  if (N < 0 || K < 0 || N >= (1 << 30) || K > N || !width_ok(F, C) || status == nullptr)
    return (int)hipErrorInvalidValue;
  double* partial = reinterpret_cast<double*>(workspace);
  const int nb = fwd_blocks(K);
  if (K > 0) {
    dispatch_int<1, 2, 4, 8>(F / 64, [&](auto v) {
      hipLaunchKernelGGL(k_charge_fwd<decltype(v)::value>, dim3(nb), dim3(kFwdBlock), 0, stream, h, (int)N, dyn_N, W, bias,
                         C, idx, labels, (int)K, k_dev, prob, partial, status);
    });
    GEOSSL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_head_loss<0>, dim3(1), dim3(kLossBlock), 0, stream, partial, K > 0 ? nb : 0, (int)K, k_dev, loss);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_charge_head_fwd(const float* h, int64_t N, int F, const float* W, const float* bias, int C,
                                      const int64_t* idx, const int64_t* labels, int64_t K, const int32_t* k_dev,
                                      float* prob, float* workspace, float* loss, int32_t* status,
                                      hipStream_t stream) {
  return geossl_charge_head_fwd_dyn(h, N, F, W, bias, C, idx, labels, K, k_dev, prob, workspace, loss, status, nullptr,
                                    stream);
}

extern "C" int geossl_charge_head_bwd_dyn(const float* h, int64_t N, int F, const float* W, int C, const int64_t* idx,
                                          const int64_t* labels, int64_t K, const int32_t* k_dev, const float* prob,
                                          const float* gout, float* dh, float* dW, float* db, float* workspace,
                                          int accumulate, const int32_t* dyn_N, hipStream_t stream) {
  if (N < 0 || K < 0 || N >= (1 << 30) || K > N || !width_ok(F, C)) return (int)hipErrorInvalidValue;
  if (N > 0) {
    const int64_t n4 = N * F / 4;
    hipLaunchKernelGGL(k_charge_zero_rows, dim3((unsigned)std::min<int64_t>((n4 + 255) / 256, 2048)), dim3(256), 0,
                       stream, dh, (int)N, F, dyn_N);
    GEOSSL_CHECK_LAUNCH();
  }
  const int nb = bwd_blocks(K);
  if (K > 0) {
    const size_t lds = ((size_t)C * F + (size_t)kBwdChunk * C) * sizeof(float);
    hipLaunchKernelGGL(k_charge_bwd_rows, dim3(nb), dim3(kBwdBlock), lds, stream, h, (int)N, F, dyn_N, W, C, idx,
                       labels, (int)K, k_dev, prob, gout, dh, workspace);
    GEOSSL_CHECK_LAUNCH();
  }
  const int cols = C * (F + 1);
  hipLaunchKernelGGL(k_charge_wgrad, dim3((cols + 255) / 256), dim3(256), 0, stream, workspace, F, C, nb,
                     (int)K, K > 0 ? k_dev : nullptr, dW, db, accumulate);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_charge_head_bwd(const float* h, int64_t N, int F, const float* W, int C, const int64_t* idx,
                                      const int64_t* labels, int64_t K, const int32_t* k_dev, const float* prob,
                                      const float* gout, float* dh, float* dW, float* db, float* workspace,
                                      int accumulate, hipStream_t stream) {
  return geossl_charge_head_bwd_dyn(h, N, F, W, C, idx, labels, K, k_dev, prob, gout, dh, dW, db, workspace,
                                    accumulate, nullptr, stream);
}
