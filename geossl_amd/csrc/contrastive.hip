// Contrastive heads of pretrain_GeoSSL.py --GeoSSL_option=InfoNCE / EBM_NCE (examples/pretrain_GeoSSL.py:103-176):
// the loss of two views' readouts X, Y [B][F] and its gradient with respect to both, forward and backward.
//
// InfoNCE (:141-176): S = X Y^T / T, loss = (CE(S, arange) + CE(S^T, arange)) / 2.  A block of four waves owns a 32-row
// strip of S (role 0) or of S^T (role 1) and walks the 32-column tiles of the other index, wave w the tiles w, w+4, ...
// A tile is one chain of f32-input MFMAs (v_mfma_f32_32x32x2_f32: exact fp32, a k-ordered fma chain); S is never stored.
// The k assignment of a step puts lane half h on k = h*ceil(F/2) + s, so a lane reads contiguous features of its row.
// Because fma(a, b, c) = fma(b, a, c), the tile of S^T computed with the operands swapped holds the same bits as S:
// forward and backward, row and column role, all see one S.  Forward: per row an online (max, sum of exp, first
// argmax) over the row's tiles, the four waves' partials merged in wave order (equal maxima: the smaller index, torch's
// first-maximum rule), then one block reduces the rows in a fixed order.  Backward: the tile of S is recomputed, turned
// into G = exp(S - lse_row) + exp(S - lse_col) - 2 delta in place, and G * (other matrix) accumulated on the same MFMA;
// the four waves' partial strips are added in wave order through LDS.  S * (1/T) is rounded on its own (mul_rn): a
// product contracted into the fma of the exponent's argument would leave the forward's and the backward's exponents
// different by the product's rounding error (G of a lone molecule would not be exactly 0).  No atomics anywhere: two
// launches on the same inputs give the same bits.
// Accuracy: a row's log-sum-exp is kept as (max m, l = log1p(r)) with r = the sum of exp(S - m) over every entry but the
// first maximum, never as m + log(1 + r) in one float.  A row whose diagonal dominates has a loss (m - d) + l = l far
// below m and a diagonal softmax term p - 1 = expm1(-l) far below 1: both come out to fp32's relative precision, where
// m + log(s) and exp(S - lse) - 1 would lose everything below ulp(m) (1e-3 relative at a loss of 1e-5).
//
// EBM-NCE (:103-138): a wave per molecule; the B (1 + num_neg) dot products in fp32 in a fixed order (lane-strided
// partial sums, then a butterfly), softplus / sigmoid and the loss in fp64 like the reference's `.double()` criterion;
// the backward casts d pred back to fp32 before it scales the neighbour rows (what `.double()`'s backward does).
#include "common.h"
#include "geossl_hip.h"

using namespace geossl;

namespace {

constexpr int kWaves = 4;
constexpr int kBlock = 64 * kWaves;
constexpr int kFGroup = 128;   // backward: output columns per pass (4 accumulator tiles of 32)

// The 32 x 32 tile A[i0 .. i0+31] . Bm[j0 .. j0+31]^T of two row-major [B][F] matrices (rows >= B read as zero).
// Lane l: row i0 + (l&31) of A and j0 + (l&31) of Bm, k = h*half + s with h = l>>5.
template <bool VEC>
__device__ __forceinline__ f32x16 s_tile(const float* __restrict__ A, int ia, const float* __restrict__ Bm, int jb,
                                         int B, int F) {
  const int l = threadIdx.x & 63, h = l >> 5;
  const int half = (F + 1) >> 1;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const bool va = ia < B, vb = jb < B;
  const float* pa = A + (int64_t)(va ? ia : 0) * F + h * half;
  const float* pb = Bm + (int64_t)(vb ? jb : 0) * F + h * half;
  if (VEC) {   // F % 8 == 0: half % 4 == 0, every row 32-byte aligned
    for (int s = 0; s < half; s += 4) {
      f32x4 a = va ? *reinterpret_cast<const f32x4*>(pa + s) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 b = vb ? *reinterpret_cast<const f32x4*>(pb + s) : f32x4{0.f, 0.f, 0.f, 0.f};
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], acc, 0, 0, 0);
    }
  } else {
    for (int s = 0; s < half; ++s) {
      const bool kin = h * half + s < F;
      const float a = (va && kin) ? pa[s] : 0.f;
      const float b = (vb && kin) ? pb[s] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
  }
  return acc;
}

__device__ __forceinline__ int acc_row(int r, int l) { return (r & 3) + 8 * (r >> 2) + 4 * (l >> 5); }

// grid (strips, 2): blockIdx.y = 0 rows of S (A = X, Bm = Y), 1 rows of S^T (A = Y, Bm = X).
// stats = {m [2B] (row, column), l [2B], diag [B] (role 0)}, amax[2B].
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_infonce_fwd(const float* __restrict__ X, const float* __restrict__ Y, int B,
                                                        int F, float inv_t, float* __restrict__ stats,
                                                        int32_t* __restrict__ amax) {
  const int role = blockIdx.y;
  const float* A = role ? Y : X;
  const float* Bm = role ? X : Y;
  const int i0 = blockIdx.x * 32;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __shared__ float tile[kWaves][32][33];
  __shared__ float sm[kWaves][32], ss[kWaves][32], sd[32];
  __shared__ int sa[kWaves][32];
  float m = -INFINITY, s = 0.f;   // s: the sum of exp(v - m) over the entries seen except the first maximum
  int am = -1;
  const int ntile = (B + 31) >> 5;
  const int gi = i0 + (l & 31);
  for (int t0 = 0; t0 < ntile; t0 += kWaves) {
    const int t = t0 + w;
    if (t < ntile) {
      const f32x16 acc = s_tile<VEC>(A, i0 + (l & 31), Bm, t * 32 + (l & 31), B, F);
#pragma unroll
      for (int r = 0; r < 16; ++r) tile[w][acc_row(r, l)][l & 31] = acc[r];
    }
    __syncthreads();
    if (t < ntile && l < 32) {
      const int c_end = min(32, B - t * 32);
      for (int c = 0; c < c_end; ++c) {
        const int j = t * 32 + c;
        const float v = mul_rn(tile[w][l][c], inv_t);   // (rounded once: backward recomputes the same bits)
        if (j == gi) sd[l] = v;
        if (v > m) {
          s = am < 0 ? 0.f : (s + 1.f) * expf(m - v);
          m = v;
          am = j;
        } else {
          s += expf(v - m);
        }
      }
    }
    __syncthreads();
  }
  if (l < 32) {
    sm[w][l] = m;
    ss[w][l] = s;
    sa[w][l] = am;
  }
  __syncthreads();
  if (w == 0 && l < 32 && gi < B) {
    float M = sm[0][l], S = ss[0][l];   // (wave 0 always holds column 0)
    int Am = sa[0][l];
    for (int v = 1; v < kWaves; ++v) {
      const float mv = sm[v][l], sv = ss[v][l];
      const int av = sa[v][l];
      if (av < 0) continue;             // no column in this wave
      if (mv > M) {
        S = sv + (S + 1.f) * expf(M - mv);
        M = mv;
        Am = av;
      } else if (mv == M) {             // equal maxima: the smaller index stays the first maximum, the other joins S
        S = S + sv + 1.f;
        Am = min(Am, av);
      } else {
        S = S + (sv + 1.f) * expf(mv - M);
      }
    }
    stats[role * B + gi] = M;
    stats[2 * B + role * B + gi] = log1pf(S);
    amax[role * B + gi] = Am;
    if (role == 0) stats[4 * B + gi] = sd[l];
  }
}

// One block: loss = sum_i ((m_row - d) + l_row + (m_col - d) + l_col) / (2B) (fp64 accumulation, fixed order), the
// two hit counts.
__global__ __launch_bounds__(256) void k_infonce_reduce(const float* __restrict__ stats,
                                                        const int32_t* __restrict__ amax, int B, float* __restrict__ loss,
                                                        int32_t* __restrict__ counts) {
  __shared__ double sacc[256];
  __shared__ int shr[256], shc[256];
  double acc = 0.0;
  int hr = 0, hc = 0;
  for (int i = threadIdx.x; i < B; i += 256) {
    const double d = stats[4 * B + i];
    acc += ((double)stats[i] - d) + (double)stats[2 * B + i] + ((double)stats[B + i] - d) + (double)stats[3 * B + i];
    hr += amax[i] == i;
    hc += amax[B + i] == i;
  }
  sacc[threadIdx.x] = acc;
  shr[threadIdx.x] = hr;
  shc[threadIdx.x] = hc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sacc[threadIdx.x] += sacc[threadIdx.x + o];
      shr[threadIdx.x] += shr[threadIdx.x + o];
      shc[threadIdx.x] += shc[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss[0] = (float)(sacc[0] / (2.0 * (double)B));
    counts[0] = shr[0];
    counts[1] = shc[0];
  }
}

// grid (strips, 2): role 0 writes the strip of dX = G Y, role 1 the strip of dY = G^T X, both * gout / (2BT).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_infonce_bwd(const float* __restrict__ X, const float* __restrict__ Y,
                                                        const float* __restrict__ stats,
                                                        const int32_t* __restrict__ amax, int B, int F, float inv_t,
                                                        const float* __restrict__ gout, float* __restrict__ dX,
                                                        float* __restrict__ dY) {
  const int role = blockIdx.y;
  const float* own = role ? Y : X;
  const float* oth = role ? X : Y;
  const float* m_own = stats + (role ? B : 0);
  const float* m_oth = stats + (role ? 0 : B);
  const float* l_own = stats + 2 * B + (role ? B : 0);
  const float* l_oth = stats + 2 * B + (role ? 0 : B);
  const int32_t* a_own = amax + (role ? B : 0);
  const int32_t* a_oth = amax + (role ? 0 : B);
  float* out = role ? dY : dX;
  const int i0 = blockIdx.x * 32;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __shared__ float tile[kWaves][32][33];
  __shared__ float red[32][kFGroup + 1];
  const float scale = gout[0] * inv_t / (2.f * (float)B);
  const int ntile = (B + 31) >> 5;
  for (int fg = 0; fg < F; fg += kFGroup) {
    const int nft = min(4, (F - fg + 31) >> 5);
    f32x16 o[4];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[ft][r] = 0.f;
    for (int t0 = 0; t0 < ntile; t0 += kWaves) {
      const int t = t0 + w;
      if (t < ntile) {
        const f32x16 acc = s_tile<VEC>(own, i0 + (l & 31), oth, t * 32 + (l & 31), B, F);
        const int j = t * 32 + (l & 31);
        const float mo = j < B ? m_oth[j] : 0.f, lo = j < B ? l_oth[j] : 0.f;
        const bool jmax = j < B && a_oth[j] == j;   // the column's first maximum is its diagonal
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = acc_row(r, l), i = i0 + row;
          float g = 0.f;
          if (i < B && j < B) {
            const float v = mul_rn(acc[r], inv_t);
            if (i != j) {
              g = expf((v - m_own[i]) - l_own[i]) + expf((v - mo) - lo);
            } else {   // p - 1 per direction; at the first maximum (v = m) that is expm1(-l), exact to fp32 precision
              const float lr = l_own[i];
              g = (a_own[i] == i ? expm1f(-lr) : expf((v - m_own[i]) - lr) - 1.f) +
                  (jmax ? expm1f(-lo) : expf((v - mo) - lo) - 1.f);
            }
          }
          tile[w][row][l & 31] = g;
        }
      }
      __syncthreads();
      if (t < ntile) {
#pragma unroll 4
        for (int q = 0; q < 16; ++q) {
          const int k = 2 * q + (l >> 5);
          const float a = tile[w][l & 31][k];   // A[i][k] = G[i][j0 + k]
          const int j = t * 32 + k;
#pragma unroll
          for (int ft = 0; ft < 4; ++ft) {
            if (ft < nft) {
              const int f = fg + ft * 32 + (l & 31);
              const float b = (j < B && f < F) ? oth[(int64_t)j * F + f] : 0.f;
              o[ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, o[ft], 0, 0, 0);
            }
          }
        }
      }
      __syncthreads();
    }
    // the four partial strips in wave order: ((o0 + o1) + o2) + o3
    for (int v = 0; v < kWaves; ++v) {
      if (w == v) {
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
          if (ft < nft) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              float& d = red[acc_row(r, l)][ft * 32 + (l & 31)];
              d = v == 0 ? o[ft][r] : d + o[ft][r];
            }
          }
        }
      }
      __syncthreads();
    }
    for (int idx = threadIdx.x; idx < 32 * kFGroup; idx += kBlock) {
      const int row = idx / kFGroup, col = idx % kFGroup;
      const int i = i0 + row, f = fg + col;
      if (i < B && f < F && col < nft * 32) out[(int64_t)i * F + f] = red[row][col] * scale;
    }
    __syncthreads();
  }
}

// ---- EBM-NCE ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_dot(const float* __restrict__ a, const float* __restrict__ b, int F) {
  const int l = threadIdx.x & 63;
  float p = 0.f;
  for (int f = l; f < F; f += 64) p = fmaf(a[f], b[f], p);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
  return p;
}

__device__ __forceinline__ int wrap(int64_t v, int B) { return (int)(((v % B) + B) % B); }

// a wave per molecule i: pred[i][0] = <x_i, y_i>, pred[i][k] = <x_i, y_{(i+k) mod B}> (cycle_index, examples/util.py:19-22)
__global__ __launch_bounds__(kBlock) void k_ebm_nce_fwd(const float* __restrict__ X, const float* __restrict__ Y, int B,
                                                        int F, int K, float* __restrict__ pred,
                                                        double* __restrict__ terms, int32_t* __restrict__ hits) {
  const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i >= B) return;
  const float* xi = X + (int64_t)i * F;
  double term = 0.0;
  int hp = 0, hn = 0;
  for (int k = 0; k <= K; ++k) {
    const int j = wrap((int64_t)i + k, B);
    const float p = wave_dot(xi, Y + (int64_t)j * F, F);
    if (k == 0) {
      term += softplus_d(-(double)p);   // BCE(p, 1)
      hp += p > 0.f;
    } else {
      term += softplus_d((double)p);    // BCE(p, 0)
      hn += p < 0.f;
    }
    if ((threadIdx.x & 63) == 0) pred[(int64_t)i * (K + 1) + k] = p;
  }
  if ((threadIdx.x & 63) == 0) {
    terms[i] = term;
    hits[i] = hp;
    hits[B + i] = hn;
  }
}

__global__ __launch_bounds__(256) void k_ebm_nce_reduce(const double* __restrict__ terms,
                                                        const int32_t* __restrict__ hits, int B, int K,
                                                        double* __restrict__ loss, int32_t* __restrict__ counts) {
  __shared__ double sacc[256];
  __shared__ int shp[256], shn[256];
  double acc = 0.0;
  int hp = 0, hn = 0;
  for (int i = threadIdx.x; i < B; i += 256) {
    acc += terms[i];
    hp += hits[i];
    hn += hits[B + i];
  }
  sacc[threadIdx.x] = acc;
  shp[threadIdx.x] = hp;
  shn[threadIdx.x] = hn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sacc[threadIdx.x] += sacc[threadIdx.x + o];
      shp[threadIdx.x] += shp[threadIdx.x + o];
      shn[threadIdx.x] += shn[threadIdx.x + o];
    }
    __syncthreads();
  }
  // (loss_pos + K loss_neg) / (1 + K) with loss_pos = mean over B, loss_neg = mean over B K
  if (threadIdx.x == 0) {
    loss[0] = sacc[0] / ((double)B * (double)(K + 1));
    counts[0] = shp[0];
    counts[1] = shn[0];
  }
}

// d pred (fp64, cast to fp32) = gout (sigmoid(p) - [k == 0]) / (B (1 + K));
// dx_i = sum_k dpred[i][k] y_{(i+k) mod B},  dy_i = sum_k dpred[(i-k) mod B][k] x_{(i-k) mod B}  (k = 0 first)
__global__ __launch_bounds__(kBlock) void k_ebm_nce_bwd(const float* __restrict__ X, const float* __restrict__ Y,
                                                        const float* __restrict__ pred, int B, int F, int K,
                                                        const double* __restrict__ gout, float* __restrict__ dX,
                                                        float* __restrict__ dY) {
  const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i >= B) return;
  const int l = threadIdx.x & 63;
  const double coef = gout[0] / ((double)B * (double)(K + 1));
  for (int f0 = 0; f0 < F; f0 += 64) {
    const int f = f0 + l;
    if (f >= F) break;
    float gx = 0.f, gy = 0.f;
    for (int k = 0; k <= K; ++k) {
      const int jx = wrap((int64_t)i + k, B);        // partner of x_i in pair k
      const int iy = wrap((int64_t)i - k, B);        // molecule whose pair k uses y_i
      const double sx = sigmoid_d((double)pred[(int64_t)i * (K + 1) + k]) - (k == 0 ? 1.0 : 0.0);
      const double sy = sigmoid_d((double)pred[(int64_t)iy * (K + 1) + k]) - (k == 0 ? 1.0 : 0.0);
      const float dpx = (float)(coef * sx), dpy = (float)(coef * sy);
      gx = fmaf(dpx, Y[(int64_t)jx * F + f], gx);
      gy = fmaf(dpy, X[(int64_t)iy * F + f], gy);
    }
    dX[(int64_t)i * F + f] = gx;
    dY[(int64_t)i * F + f] = gy;
  }
}

inline bool vec_ok(const float* a, const float* b, int F) {
  return F % 8 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

}  // namespace

extern "C" int geossl_infonce_fwd(const float* X, const float* Y, int64_t B, int F, float inv_t, float* stats,
                                  int32_t* amax, float* loss, int32_t* counts, hipStream_t stream) {
  if (B <= 0 || F <= 0) return (int)hipErrorInvalidValue;
  if (B > (1 << 24)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((B + 31) / 32), 2);
  if (vec_ok(X, Y, F))
    hipLaunchKernelGGL(k_infonce_fwd<true>, grid, dim3(kBlock), 0, stream, X, Y, (int)B, F, inv_t, stats, amax);
  else
    hipLaunchKernelGGL(k_infonce_fwd<false>, grid, dim3(kBlock), 0, stream, X, Y, (int)B, F, inv_t, stats, amax);
  GEOSSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_infonce_reduce, dim3(1), dim3(256), 0, stream, stats, amax, (int)B, loss, counts);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_infonce_bwd(const float* X, const float* Y, const float* stats, const int32_t* amax, int64_t B,
                                  int F, float inv_t, const float* gout, float* dX, float* dY, hipStream_t stream) {
  if (B <= 0 || F <= 0) return (int)hipErrorInvalidValue;
  if (B > (1 << 24)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)((B + 31) / 32), 2);
  if (vec_ok(X, Y, F))
    hipLaunchKernelGGL(k_infonce_bwd<true>, grid, dim3(kBlock), 0, stream, X, Y, stats, amax, (int)B, F, inv_t, gout, dX,
                       dY);
  else
    hipLaunchKernelGGL(k_infonce_bwd<false>, grid, dim3(kBlock), 0, stream, X, Y, stats, amax, (int)B, F, inv_t, gout, dX,
                       dY);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_ebm_nce_fwd(const float* X, const float* Y, int64_t B, int F, int num_neg, float* pred,
                                  double* terms, int32_t* hits, double* loss, int32_t* counts, hipStream_t stream) {
  if (B <= 0 || F <= 0 || num_neg < 1 || num_neg > B) return (int)hipErrorInvalidValue;
  if (B > (1 << 24)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ebm_nce_fwd, dim3((unsigned)((B + kWaves - 1) / kWaves)), dim3(kBlock), 0, stream, X, Y, (int)B,
                     F, num_neg, pred, terms, hits);
  GEOSSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_ebm_nce_reduce, dim3(1), dim3(256), 0, stream, terms, hits, (int)B, num_neg, loss, counts);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_ebm_nce_bwd(const float* X, const float* Y, const float* pred, int64_t B, int F, int num_neg,
                                  const double* gout, float* dX, float* dY, hipStream_t stream) {
  if (B <= 0 || F <= 0 || num_neg < 1 || num_neg > B) return (int)hipErrorInvalidValue;
  if (B > (1 << 24)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ebm_nce_bwd, dim3((unsigned)((B + kWaves - 1) / kWaves)), dim3(kBlock), 0, stream, X, Y, pred,
                     (int)B, F, num_neg, gout, dX, dY);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
