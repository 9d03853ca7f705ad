// GeoSSL-RR (representation reconstruction, examples/pretrain_GeoSSL.py:77-100): the two AutoEncoder heads of a step,
// forward and backward, BOTH HEADS IN THE SAME LAUNCHES (gridDim.z / gridDim.y = head).  The AutoEncoder is this
// project's own definition (geossl_amd/Geom3D/models/autoencoder.py; the reference tree has no such class):
//     p = Linear2(relu(BatchNorm1d(Linear1(x)))),   loss(p, y) of kind l1 / l2 / cosine,
// head 0 on (X, Y), head 1 on (Y, X), the step's loss (loss_0 + loss_1) / 2.  F = 128 only.
//
//   forward (5 launches)                              backward (6 launches)
//   k_rr_gemm<NT>      Z = a W1^T + b1                k_rr_dp           dp (and the targets' gradients) per loss kind
//   k_rr_bn_fwd        batch statistics, zhat, A,     k_rr_gemm<NN>     dz = (dp W2) . [A > 0]
//                      running statistics in place    k_rr_bn_bwd       dgamma, dbeta, dZ in place of dz
//   k_rr_gemm<NT>      p = A W2^T + b2                geossl_linear_wgrad   dW2, db2, dW1, db1 of both heads (2 launches)
//   k_rr_loss_rows     one fp64 slot per row          k_rr_gemm<NN>     dX / dY = dZ W1 (+ the other head's target
//   k_rr_loss          the two means, (l0 + l1) / 2                     gradient), into the [2B][F] gradient
//
// The launch count does not depend on B.  The dense products run on the bf16 matrix pipe with both operands split three
// ways (split.h: mma6); a wave owns a 32 x 32 tile of the output and walks the 128 contraction indices in 8 steps.  The
// statistics are fp32 sums in a fixed order (16 row groups per column, combined in group order), the loss a fixed fp64
// tree over the per-row slots (head_common.h: block_sum).  No atomics anywhere: the same bits every launch.
#include "geossl_hip.h"
#include "head_common.h"
#include "split.h"

namespace geossl {
namespace {

constexpr int kF = 128;          // the one width served
constexpr int kBnCols = 16;      // k_rr_bn_*: columns per block
constexpr int kBnGroups = 16;    // ... and row groups (kBnCols * kBnGroups threads)
constexpr int kRowsPerBlock = 4; // k_rr_loss_rows / k_rr_dp: a wave per row
constexpr float kCosEps = 1e-8f; // F.cosine_similarity's eps

enum LossKind { kL1 = 0, kL2 = 1, kCosine = 2 };

struct HeadPtrs {  // one pointer per head
  const float* p[2];
};
struct HeadOut {
  float* p[2];
};

// out_h [B][128] = in_h (x) W_h (+ bias_h) for both heads; TRANSB: out[r][n] = sum_k in[r][k] W[n][k] (a Linear's forward),
// else out[r][k] = sum_n in[r][n] W[n][k] (its input gradient).  Epilogue: + bias[col]; zero where mask[r][col] <= 0
// (ReLU's backward on the saved activation); + add[r][col] (the other head's target gradient).  Rows past B: loads are
// clamped to row B - 1, nothing is stored.
template <bool TRANSB>
__global__ __launch_bounds__(64) void k_rr_gemm(HeadPtrs in, HeadPtrs W, HeadPtrs bias, HeadPtrs mask, HeadPtrs add,
                                                 HeadOut out, int B) {
  const int head = blockIdx.z;
  const int lane = threadIdx.x, j = lane & 31, kh = lane >> 5;
  const int r0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  const float* __restrict__ a = in.p[head] + (size_t)min(r0 + j, B - 1) * kF;
  const float* __restrict__ w = W.p[head];
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
  for (int s = 0; s < kF / 16; ++s) {
    const int k0 = 16 * s + 8 * kh;
    float av[8], bv[8];
    const float4 a0 = *reinterpret_cast<const float4*>(a + k0), a1 = *reinterpret_cast<const float4*>(a + k0 + 4);
    av[0] = a0.x, av[1] = a0.y, av[2] = a0.z, av[3] = a0.w, av[4] = a1.x, av[5] = a1.y, av[6] = a1.z, av[7] = a1.w;
    if (TRANSB) {
      const float* wr = w + (size_t)(n0 + j) * kF + k0;
      const float4 b0 = *reinterpret_cast<const float4*>(wr), b1 = *reinterpret_cast<const float4*>(wr + 4);
      bv[0] = b0.x, bv[1] = b0.y, bv[2] = b0.z, bv[3] = b0.w, bv[4] = b1.x, bv[5] = b1.y, bv[6] = b1.z, bv[7] = b1.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) bv[e] = w[(size_t)(k0 + e) * kF + n0 + j];
    }
    mma6(acc, split8(av), split8(bv));
  }
  const int col = n0 + j;
  const float bc = bias.p[head] != nullptr ? bias.p[head][col] : 0.0f;
  const float* __restrict__ mk = mask.p[head];
  const float* __restrict__ ad = add.p[head];
  float* __restrict__ o = out.p[head];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = r0 + c_row(r, lane);
    if (row >= B) continue;
    const size_t at = (size_t)row * kF + col;
    float v = acc[r] + bc;
    if (mk != nullptr) v = mk[at] > 0.0f ? v : 0.0f;
    if (ad != nullptr) v = v + ad[at];
    o[at] = v;
  }
}

// sum over the block's 16 row groups of one column's partials, in group order; every thread of the column gets the sum
__device__ __forceinline__ float groups_sum(float v, float (*red)[kBnCols], int g, int c) {
  __syncthreads();  // (the previous tree's reads)
  red[g][c] = v;
  __syncthreads();
  float s = red[0][c];
#pragma unroll
  for (int k = 1; k < kBnGroups; ++k) s += red[k][c];
  return s;
}

struct BnFwd {
  float* z[2];             // [B][128] in: Linear1's output; out: zhat
  const float* gamma[2];
  const float* beta[2];
  float* run_mean[2];
  float* run_var[2];
  int64_t* batches[2];
  float* istd[2];          // [128] out
  float* act[2];           // [B][128] out: relu(gamma zhat + beta)
  float eps[2], momentum[2];
};

// Training-mode BatchNorm1d + ReLU of both heads.  Block (x, head): columns [16 x, 16 x + 16); thread (g, c) adds rows
// g, g + 16, ... of column c in order, the 16 group sums are added in group order.  mean, then the biased variance as the
// mean of (z - mean)^2 (two passes: no cancellation), zhat in place of z, the activation, and the module's buffers in
// place: running = (1 - m) running + m (mean | variance B / (B - 1)), num_batches_tracked + 1.
__global__ __launch_bounds__(kBnCols* kBnGroups) void k_rr_bn_fwd(BnFwd a, int B) {
  __shared__ float red[kBnGroups][kBnCols];
  const int head = blockIdx.y;
  const int c = threadIdx.x % kBnCols, g = threadIdx.x / kBnCols;
  const int col = blockIdx.x * kBnCols + c;
  float* __restrict__ z = a.z[head];
  float s = 0.0f;
  for (int r = g; r < B; r += kBnGroups) s += z[(size_t)r * kF + col];
  const float mean = groups_sum(s, red, g, c) / (float)B;
  float q = 0.0f;
  for (int r = g; r < B; r += kBnGroups) {
    const float d = z[(size_t)r * kF + col] - mean;
    q = fmaf(d, d, q);
  }
  const float var = groups_sum(q, red, g, c) / (float)B;
  const float istd = 1.0f / sqrtf(var + a.eps[head]);
  const float ga = a.gamma[head][col], be = a.beta[head][col];
  float* __restrict__ act = a.act[head];
  for (int r = g; r < B; r += kBnGroups) {
    const size_t at = (size_t)r * kF + col;
    const float zh = (z[at] - mean) * istd;
    z[at] = zh;
    act[at] = fmaxf(fmaf(ga, zh, be), 0.0f);
  }
  if (g == 0) {
    a.istd[head][col] = istd;
    const float m = a.momentum[head];
    const float unbiased = var * ((float)B / (float)(B - 1));
    a.run_mean[head][col] = (1.0f - m) * a.run_mean[head][col] + m * mean;
    a.run_var[head][col] = (1.0f - m) * a.run_var[head][col] + m * unbiased;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.batches[head][0] += 1;
}

struct BnBwd {
  float* dz[2];            // [B][128] in: the gradient of gamma zhat + beta; out: the gradient of Linear1's output
  const float* zhat[2];
  const float* gamma[2];
  const float* istd[2];
  float* dgamma[2];
  float* dbeta[2];
  float* db1[2];
};

// BatchNorm1d's backward with batch statistics: s1 = sum_r dz, s2 = sum_r dz zhat per column (the order of k_rr_bn_fwd),
// dbeta (+)= s1, dgamma (+)= s2, dZ = gamma istd (dz - s1 / B - zhat s2 / B).  The gradient of Linear1's bias is the
// column sum of dZ, which is ZERO for every input (the normalisation subtracts the column mean: a shift of Z by b1 does
// not reach the loss): written as 0 (+= 0), where a summation of the rounded dZ would leave noise of order 1e-9.
__global__ __launch_bounds__(kBnCols* kBnGroups) void k_rr_bn_bwd(BnBwd a, int B, int accumulate) {
  __shared__ float red[kBnGroups][kBnCols];
  const int head = blockIdx.y;
  const int c = threadIdx.x % kBnCols, g = threadIdx.x / kBnCols;
  const int col = blockIdx.x * kBnCols + c;
  float* __restrict__ dz = a.dz[head];
  const float* __restrict__ zh = a.zhat[head];
  float s1 = 0.0f, s2 = 0.0f;
  for (int r = g; r < B; r += kBnGroups) {
    const size_t at = (size_t)r * kF + col;
    const float d = dz[at];
    s1 += d;
    s2 = fmaf(d, zh[at], s2);
  }
  s1 = groups_sum(s1, red, g, c);
  s2 = groups_sum(s2, red, g, c);
  if (g == 0) {
    float* dg = a.dgamma[head] + col;
    float* db = a.dbeta[head] + col;
    *dg = accumulate ? *dg + s2 : s2;
    *db = accumulate ? *db + s1 : s1;
    if (!accumulate) a.db1[head][col] = 0.0f;
  }
  const float k = a.gamma[head][col] * a.istd[head][col];
  const float m1 = s1 / (float)B, m2 = s2 / (float)B;
  for (int r = g; r < B; r += kBnGroups) {
    const size_t at = (size_t)r * kF + col;
    dz[at] = k * ((dz[at] - m1) - zh[at] * m2);
  }
}

struct RowSums {
  float dot, pp, yy;
};
// lane l of the row's wave holds columns l and l + 64
__device__ __forceinline__ RowSums cosine_sums(float p0, float p1, float y0, float y1) {
  RowSums s;
  s.dot = wave_sum(fmaf(p1, y1, p0 * y0));
  s.pp = wave_sum(fmaf(p1, p1, p0 * p0));
  s.yy = wave_sum(fmaf(y1, y1, y0 * y0));
  return s;
}

// slot[head][r] (fp64) = the row's loss term: sum_c |p - y|, sum_c (p - y)^2, or cos(p_r, y_r) = <p, y> /
// (max(|p|, eps) max(|y|, eps)); a wave per row, the 64 lane sums added by wave_sum's butterfly.
__global__ __launch_bounds__(64 * kRowsPerBlock) void k_rr_loss_rows(HeadPtrs p, HeadPtrs target, int B, int kind,
                                                                      double* __restrict__ slots) {
  const int head = blockIdx.y;
  const int l = threadIdx.x & 63;
  const int r = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= B) return;
  const float* pr = p.p[head] + (size_t)r * kF;
  const float* yr = target.p[head] + (size_t)r * kF;
  const float p0 = pr[l], p1 = pr[l + 64], y0 = yr[l], y1 = yr[l + 64];
  float v;
  if (kind == kCosine) {
    const RowSums s = cosine_sums(p0, p1, y0, y1);
    v = s.dot / (fmaxf(sqrtf(s.pp), kCosEps) * fmaxf(sqrtf(s.yy), kCosEps));
  } else {
    const float d0 = p0 - y0, d1 = p1 - y1;
    v = wave_sum(kind == kL1 ? fabsf(d0) + fabsf(d1) : fmaf(d1, d1, d0 * d0));
  }
  if (l == 0) slots[(size_t)head * B + r] = (double)v;
}

// loss = (mean_0 + mean_1) / 2: each head's slots added in fp64 (thread t: slots t, t + 256, ... in order, then the tree),
// head 0 before head 1; l1 / l2: / (B 128), cosine: - / B.
__global__ __launch_bounds__(kLossBlock) void k_rr_loss(const double* __restrict__ slots, int B, int kind,
                                                        float* __restrict__ loss) {
  double m[2];
  for (int head = 0; head < 2; ++head) {
    double acc = 0.0;
    for (int k = threadIdx.x; k < B; k += kLossBlock) acc += slots[(size_t)head * B + k];
    const double s = block_sum_f64<kLossBlock>(acc);
    m[head] = kind == kCosine ? -s / (double)B : s / ((double)B * kF);
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)((m[0] + m[1]) * 0.5);
}

// dp_h [B][128] = d loss / d p_h from the upstream gout[0]; with dt non-null also the gradient of head h's target (rows of
// the OTHER view).  l1: c sign(p - y) with sign(0) = 0, c = gout / (2 B 128); l2: 2 c (p - y); cosine, c = -gout / (2 B),
// np = max(|p|, eps), ny likewise: dp = c (y / (np ny) - cos p / np^2), dt = c (p / (np ny) - cos y / ny^2).
__global__ __launch_bounds__(64 * kRowsPerBlock) void k_rr_dp(HeadPtrs p, HeadPtrs target, int B, int kind,
                                                               const float* __restrict__ gout, HeadOut dp, HeadOut dt) {
  const int head = blockIdx.y;
  const int l = threadIdx.x & 63;
  const int r = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= B) return;
  const size_t at = (size_t)r * kF + l;
  const float* pr = p.p[head] + at;
  const float* yr = target.p[head] + at;
  const float p0 = pr[0], p1 = pr[64], y0 = yr[0], y1 = yr[64];
  const float g = gout[0];
  float g0, g1, t0, t1;
  if (kind == kCosine) {
    const float c = -g / (2.0f * (float)B);
    const RowSums s = cosine_sums(p0, p1, y0, y1);
    const float np = fmaxf(sqrtf(s.pp), kCosEps), ny = fmaxf(sqrtf(s.yy), kCosEps);
    const float inv = 1.0f / (np * ny), cs = s.dot * inv;
    const float kp = cs / (np * np), ky = cs / (ny * ny);
    g0 = c * (y0 * inv - kp * p0), g1 = c * (y1 * inv - kp * p1);
    t0 = c * (p0 * inv - ky * y0), t1 = c * (p1 * inv - ky * y1);
  } else {
    const float c = g / (2.0f * (float)B * (float)kF);
    const float d0 = p0 - y0, d1 = p1 - y1;
    if (kind == kL1) {
      g0 = c * (float)((d0 > 0.0f) - (d0 < 0.0f)), g1 = c * (float)((d1 > 0.0f) - (d1 < 0.0f));
    } else {
      g0 = 2.0f * c * d0, g1 = 2.0f * c * d1;
    }
    t0 = -g0, t1 = -g1;
  }
  dp.p[head][at] = g0;
  dp.p[head][at + 64] = g1;
  if (dt.p[head] != nullptr) {
    dt.p[head][at] = t0;
    dt.p[head][at + 64] = t1;
  }
}

inline bool width_ok(int F) { return F == kF; }
inline bool shape_ok(int64_t B, int F, int kind) {
  return width_ok(F) && B >= 2 && B <= (1 << 20) && kind >= kL1 && kind <= kCosine;
}
inline dim3 gemm_grid(int64_t B) { return dim3((unsigned)((B + 31) / 32), kF / 32, 2); }
inline dim3 row_grid(int64_t B) { return dim3((unsigned)((B + kRowsPerBlock - 1) / kRowsPerBlock), 2); }

}  // namespace
}  // namespace geossl

using namespace geossl;

extern "C" int geossl_rr_head_width_ok(int F) { return width_ok(F) ? 1 : 0; }

// the fp64 row slots of both heads, in floats
extern "C" int64_t geossl_rr_head_workspace_floats(int64_t B) { return 4 * (B > 0 ? B : 1); }

extern "C" int geossl_rr_head_fwd(const float* X, const float* Y, int64_t B, int F, int loss_kind,
                                  const float* const* params, float* const* buffers, float eps0, float momentum0,
                                  float eps1, float momentum1, float* zhat, float* istd, float* act, float* p,
                                  float* workspace, float* loss, hipStream_t stream) {
  if (!shape_ok(B, F, loss_kind)) return (int)hipErrorInvalidValue;
  const size_t BF = (size_t)B * kF;
  const HeadPtrs none{{nullptr, nullptr}};
  // params: per head W1, b1, gamma, beta, W2, b2; buffers: per head running_mean, running_var, num_batches_tracked
  hipLaunchKernelGGL(k_rr_gemm<true>, gemm_grid(B), dim3(64), 0, stream, HeadPtrs{{X, Y}},
                     HeadPtrs{{params[0], params[6]}}, HeadPtrs{{params[1], params[7]}}, none, none,
                     HeadOut{{zhat, zhat + BF}}, (int)B);
  GEOSSL_CHECK_LAUNCH();
  BnFwd bn;
  for (int h = 0; h < 2; ++h) {
    bn.z[h] = zhat + h * BF;
    bn.gamma[h] = params[6 * h + 2];
    bn.beta[h] = params[6 * h + 3];
    bn.run_mean[h] = buffers[3 * h];
    bn.run_var[h] = buffers[3 * h + 1];
    bn.batches[h] = reinterpret_cast<int64_t*>(buffers[3 * h + 2]);
    bn.istd[h] = istd + h * kF;
    bn.act[h] = act + h * BF;
  }
  bn.eps[0] = eps0, bn.eps[1] = eps1, bn.momentum[0] = momentum0, bn.momentum[1] = momentum1;
  hipLaunchKernelGGL(k_rr_bn_fwd, dim3(kF / kBnCols, 2), dim3(kBnCols * kBnGroups), 0, stream, bn, (int)B);
  GEOSSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_rr_gemm<true>, gemm_grid(B), dim3(64), 0, stream, HeadPtrs{{act, act + BF}},
                     HeadPtrs{{params[4], params[10]}}, HeadPtrs{{params[5], params[11]}}, none, none,
                     HeadOut{{p, p + BF}}, (int)B);
  GEOSSL_CHECK_LAUNCH();
  double* slots = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(k_rr_loss_rows, row_grid(B), dim3(64 * kRowsPerBlock), 0, stream, HeadPtrs{{p, p + BF}},
                     HeadPtrs{{Y, X}}, (int)B, loss_kind, slots);
  GEOSSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_rr_loss, dim3(1), dim3(kLossBlock), 0, stream, slots, (int)B, loss_kind, loss);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_rr_head_bwd(const float* X, const float* Y, int64_t B, int F, int loss_kind, int detach_target,
                                  const float* const* params, const float* zhat, const float* istd, const float* act,
                                  const float* p, const float* gout, float* dp, float* dz, float* dt,
                                  float* const* grads, int accumulate, float* dxy, float* tn_workspace,
                                  hipStream_t stream) {
  if (!shape_ok(B, F, loss_kind) || (detach_target == 0) != (dt != nullptr)) return (int)hipErrorInvalidValue;
  const size_t BF = (size_t)B * kF;
  const HeadPtrs none{{nullptr, nullptr}};
  hipLaunchKernelGGL(k_rr_dp, row_grid(B), dim3(64 * kRowsPerBlock), 0, stream, HeadPtrs{{p, p + BF}}, HeadPtrs{{Y, X}},
                     (int)B, loss_kind, gout, HeadOut{{dp, dp + BF}},
                     HeadOut{{dt, dt != nullptr ? dt + BF : nullptr}});
  GEOSSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_rr_gemm<false>, gemm_grid(B), dim3(64), 0, stream, HeadPtrs{{dp, dp + BF}},
                     HeadPtrs{{params[4], params[10]}}, none, HeadPtrs{{act, act + BF}}, none, HeadOut{{dz, dz + BF}},
                     (int)B);
  GEOSSL_CHECK_LAUNCH();
  BnBwd bn;
  for (int h = 0; h < 2; ++h) {
    bn.dz[h] = dz + h * BF;
    bn.zhat[h] = zhat + h * BF;
    bn.gamma[h] = params[6 * h + 2];
    bn.istd[h] = istd + h * kF;
    bn.dgamma[h] = grads[6 * h + 2];
    bn.dbeta[h] = grads[6 * h + 3];
    bn.db1[h] = grads[6 * h + 1];
  }
  hipLaunchKernelGGL(k_rr_bn_bwd, dim3(kF / kBnCols, 2), dim3(kBnCols * kBnGroups), 0, stream, bn, (int)B, accumulate);
  GEOSSL_CHECK_LAUNCH();
  // dW2 = dp^T A, db2 = sum_r dp; dW1 = dZ^T x (db1: k_rr_bn_bwd) - the four problems in one batched launch + its reduction
  GeosslTnBatch tb = {};
  for (int h = 0; h < 2; ++h) {
    tb.A[h] = dp + h * BF, tb.B[h] = act + h * BF, tb.dW[h] = grads[6 * h + 4], tb.db[h] = grads[6 * h + 5];
    tb.A[2 + h] = dz + h * BF, tb.B[2 + h] = h == 0 ? X : Y, tb.dW[2 + h] = grads[6 * h], tb.db[2 + h] = nullptr;
  }
  const int rc = geossl_linear_wgrad(&tb, 4, B, kF, kF, kF, kF, kF, tn_workspace, accumulate, stream);
  if (rc != 0) return rc;
  // dX = dZ_0 W1_0 (+ head 1's target gradient), dY = dZ_1 W1_1 (+ head 0's)
  hipLaunchKernelGGL(k_rr_gemm<false>, gemm_grid(B), dim3(64), 0, stream, HeadPtrs{{dz, dz + BF}},
                     HeadPtrs{{params[0], params[6]}}, none, none,
                     HeadPtrs{{dt != nullptr ? dt + BF : nullptr, dt}}, HeadOut{{dxy, dxy + BF}}, (int)B);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
