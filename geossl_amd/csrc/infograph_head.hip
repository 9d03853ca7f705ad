// 3D InfoGraph of examples/pretrain_3DInfoGraph.py:19-31,56-76: the backbone's readout, the Discriminator
// (h = sigmoid(readout) @ W, score = <node_repr, h[molecule]>) on every atom against its own molecule (positive) and the
// next one, (b + 1) mod B (negative, cycle_index(B, 1) of examples/util.py:19-22), BCEWithLogitsLoss of both, forward
// and backward.
//
// Forward
//   k_ig_summary (kTile molecules per block, thread j = feature j): m_b = readout of the atom rows of molecule b
//     ("add": a sum in atom order, "mean": that sum / max(n_b, 1) - readout_col of common.h, the function
//     k_segment_reduce_fwd calls, so the head's readout has the backbone's bits) or the caller's m_b (external readout);
//     s_b = sigmoid(m_b); h_b = s_b W with a
//     fp32 fma chain over k in index order (W read once per block for its kTile molecules).
//   k_ig_scores (one block per molecule, one wave per atom): pos_i = <x_i, h_b>, neg_i = <x_i, h_{(b+1) mod B}> (fp32
//     lane partials, then a fixed xor tree); per molecule the fp64 sums of softplus(-pos_i) and softplus(neg_i) and the
//     integer counts #(pos_i > 0), #(neg_i < 0) in atom order per wave, waves added in order.
//   k_ig_loss (one block): the per-molecule sums added in a fixed order (block_sum of head_common.h); loss = S_pos / N + S_neg / N (two means over N
//     atoms, fp64, stored as fp32; N = 0: NaN, the mean of an empty tensor), counts = the two totals.
// Backward, with c = gout[0] / N (fp32): g_pos_i = -c / (1 + exp(pos_i)) (= (sigmoid(pos_i) - 1) c),
//   g_neg_i = c / (1 + exp(-neg_i)) (= sigmoid(neg_i) c).  k_ig_bwd (kTile molecules per block, thread j = feature j):
//     dh_b = sum_{i in b} g_pos_i x_i + sum_{i in (b-1) mod B} g_neg_i x_i   (per molecule, atom order, no atomics);
//     ds_b = dh_b W^T; dm_b = ds_b s_b (1 - s_b);
//     dx_i = g_pos_i h_b + g_neg_i h_{(b+1) mod B} + dm_b (/ max(n_b, 1) for "mean") - the discriminator's and the
//       readout's paths in one store; with an external readout dm [B, F] is written instead and dx has no readout term.
//   dW = s^T dh is the caller's (ops.linear_wgrad: the split-operand weight-gradient GEMM).
// Every sum has a fixed order and there are no atomics: the same inputs give the same bits.
// Capacity launches (`_dyn`): N is a capacity (the row stride of `scores`); the real atom count is read from dyn_N.
// The molecule offsets mol_ptr [B + 1] are the real ones (B is exact), so rows past the real count are neither read nor
// written.
#include "geossl_hip.h"
#include "head_common.h"

using namespace geossl;

namespace {

constexpr int kTile = 4;             // molecules per block of k_ig_summary / k_ig_bwd
constexpr int kScoreBlock = 256;     // k_ig_scores: 4 waves, one atom per wave at a time
constexpr int kScoreWaves = kScoreBlock / 64;

template <int F>
__global__ __launch_bounds__(F) void k_ig_summary(const float* __restrict__ x, const int32_t* __restrict__ mol_ptr,
                                                  int B, int readout, const float* __restrict__ m_in,
                                                  const float* __restrict__ W, float* __restrict__ s_out,
                                                  float* __restrict__ h_out) {
  __shared__ float ss[kTile][F];
  const int j = threadIdx.x;
  const int b0 = blockIdx.x * kTile;
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    const int b = b0 + t;
    float v = 0.0f;
    if (b < B) {
      if (readout == kExternal) {
        v = m_in[(size_t)b * F + j];
      } else {
        v = readout_col(x, F, j, mol_ptr[b], mol_ptr[b + 1], readout == kMean);
      }
      v = sigmoidf_(v);
      s_out[(size_t)b * F + j] = v;
    }
    ss[t][j] = v;
  }
  __syncthreads();
  float acc[kTile];
#pragma unroll
  for (int t = 0; t < kTile; ++t) acc[t] = 0.0f;
#pragma unroll 4
  for (int k = 0; k < F; ++k) {
    const float w = W[(size_t)k * F + j];
#pragma unroll
    for (int t = 0; t < kTile; ++t) acc[t] = fmaf(ss[t][k], w, acc[t]);
  }
#pragma unroll
  for (int t = 0; t < kTile; ++t)
    if (b0 + t < B) h_out[(size_t)(b0 + t) * F + j] = acc[t];
}

template <int V>
__global__ __launch_bounds__(kScoreBlock) void k_ig_scores(const float* __restrict__ x, int N_cap,
                                                           const int32_t* __restrict__ mol_ptr, int B,
                                                           const float* __restrict__ h, float* __restrict__ scores,
                                                           double* __restrict__ part, int32_t* __restrict__ hits) {
  constexpr int F = 64 * V;
  __shared__ double wsum[2][kScoreWaves];
  __shared__ int wcnt[2][kScoreWaves];
  const int b = blockIdx.x;
  const int bn = b + 1 == B ? 0 : b + 1;
  const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float hp[V], hn[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    hp[v] = h[(size_t)b * F + l * V + v];
    hn[v] = h[(size_t)bn * F + l * V + v];
  }
  const int a0 = mol_ptr[b], a1 = mol_ptr[b + 1];
  double tp = 0.0, tn = 0.0;   // (lane 0: this wave's terms in atom order)
  int cp = 0, cn = 0;
  for (int a = a0 + wave; a < a1; a += kScoreWaves) {
    const float* row = x + (size_t)a * F + l * V;
    float sp = 0.0f, sn = 0.0f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float xv = row[v];
      sp = fmaf(xv, hp[v], sp);
      sn = fmaf(xv, hn[v], sn);
    }
    sp = wave_sum(sp);
    sn = wave_sum(sn);
    if (l == 0) {
      scores[a] = sp;
      scores[(size_t)N_cap + a] = sn;
      tp += softplus_d(-(double)sp);   // BCE(pos, 1) = -log sigmoid(pos)
      tn += softplus_d((double)sn);    // BCE(neg, 0) = -log(1 - sigmoid(neg))
      cp += sp > 0.0f;
      cn += sn < 0.0f;
    }
  }
  if (l == 0) {
    wsum[0][wave] = tp;
    wsum[1][wave] = tn;
    wcnt[0][wave] = cp;
    wcnt[1][wave] = cn;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int q = threadIdx.x;
    double s = 0.0;
    int c = 0;
#pragma unroll
    for (int w = 0; w < kScoreWaves; ++w) {
      s += wsum[q][w];
      c += wcnt[q][w];
    }
    part[2 * (size_t)b + q] = s;
    hits[2 * (size_t)b + q] = c;
  }
}

// The four totals of the loss step, reduced by one tree.
struct IgSums {
  double pos, neg;   // sums of softplus(-pos_i), softplus(neg_i)
  int hit_pos, hit_neg;
  __device__ IgSums& operator+=(const IgSums& o) {
    pos += o.pos;
    neg += o.neg;
    hit_pos += o.hit_pos;
    hit_neg += o.hit_neg;
    return *this;
  }
};

// One block: thread t adds the molecules t, t + 256, ... in order, then a tree over the threads.
__global__ __launch_bounds__(kLossBlock) void k_ig_loss(const double* __restrict__ part, const int32_t* __restrict__ hits,
                                                        int B, int N_cap, const int32_t* __restrict__ dyn_N,
                                                        float* __restrict__ loss, int32_t* __restrict__ counts) {
  __shared__ IgSums red[kLossBlock];
  IgSums acc = {0.0, 0.0, 0, 0};
  for (int b = threadIdx.x; b < B; b += kLossBlock)
    acc += IgSums{part[2 * (size_t)b], part[2 * (size_t)b + 1], hits[2 * (size_t)b], hits[2 * (size_t)b + 1]};
  const IgSums s = block_sum<kLossBlock>(acc, red);
  if (threadIdx.x == 0) {
    const double n = (double)dyn_count(N_cap, dyn_N);
    loss[0] = (float)(s.pos / n + s.neg / n);
    counts[0] = s.hit_pos;
    counts[1] = s.hit_neg;
  }
}

template <int F>
__global__ __launch_bounds__(F) void k_ig_bwd(const float* __restrict__ x, int N_cap, const int32_t* __restrict__ dyn_N,
                                              const float* __restrict__ W, const int32_t* __restrict__ mol_ptr, int B,
                                              int readout, const float* __restrict__ s, const float* __restrict__ h,
                                              const float* __restrict__ scores, const float* __restrict__ gout,
                                              float* __restrict__ dx, float* __restrict__ dm_out,
                                              float* __restrict__ dh_out) {
  __shared__ float sdh[kTile][F];
  const int j = threadIdx.x;
  const int b0 = blockIdx.x * kTile;
  const float c = gout[0] / (float)dyn_count(N_cap, dyn_N);
  const float* pos = scores;
  const float* neg = scores + N_cap;
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    const int b = b0 + t;
    float acc = 0.0f;
    if (b < B) {
      const int bp = b == 0 ? B - 1 : b - 1;
      for (int a = mol_ptr[b], a1 = mol_ptr[b + 1]; a < a1; ++a)
        acc = fmaf(-c / (1.0f + expf(pos[a])), x[(size_t)a * F + j], acc);
      for (int a = mol_ptr[bp], a1 = mol_ptr[bp + 1]; a < a1; ++a)
        acc = fmaf(c / (1.0f + expf(-neg[a])), x[(size_t)a * F + j], acc);
      dh_out[(size_t)b * F + j] = acc;
    }
    sdh[t][j] = acc;
  }
  __syncthreads();
  // ds_b[j] = sum_k dh_b[k] W[j][k]: thread j walks row j of W (16-byte pieces), shared by the kTile molecules
  float ds[kTile];
#pragma unroll
  for (int t = 0; t < kTile; ++t) ds[t] = 0.0f;
  const float4* wrow = reinterpret_cast<const float4*>(W + (size_t)j * F);
#pragma unroll 2
  for (int k4 = 0; k4 < F / 4; ++k4) {
    const float4 w = wrow[k4];
#pragma unroll
    for (int t = 0; t < kTile; ++t) {
      ds[t] = fmaf(sdh[t][4 * k4 + 0], w.x, ds[t]);
      ds[t] = fmaf(sdh[t][4 * k4 + 1], w.y, ds[t]);
      ds[t] = fmaf(sdh[t][4 * k4 + 2], w.z, ds[t]);
      ds[t] = fmaf(sdh[t][4 * k4 + 3], w.w, ds[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    const int b = b0 + t;
    if (b >= B) break;
    const int bn = b + 1 == B ? 0 : b + 1;
    const float sv = s[(size_t)b * F + j];
    const float dm = ds[t] * (sv * (1.0f - sv));
    const int a0 = mol_ptr[b], a1 = mol_ptr[b + 1];
    float dr = 0.0f;   // the readout's backward for every atom of b
    if (readout == kExternal)
      dm_out[(size_t)b * F + j] = dm;
    else
      dr = readout_grad(dm, a0, a1, readout == kMean);
    const float hb = h[(size_t)b * F + j], hbn = h[(size_t)bn * F + j];
    for (int a = a0; a < a1; ++a) {
      const float gp = -c / (1.0f + expf(pos[a]));
      const float gn = c / (1.0f + expf(-neg[a]));
      dx[(size_t)a * F + j] = fmaf(gp, hb, gn * hbn) + dr;
    }
  }
}

inline bool width_ok(int F) { return F == 64 || F == 128 || F == 256; }

inline bool args_ok(int64_t N, int F, int64_t B, int readout, const float* m_in) {
  return N >= 0 && N < (1 << 30) && B >= 1 && B < (1 << 24) && width_ok(F) && readout >= kAdd &&
         readout <= kExternal && (readout == kExternal) == (m_in != nullptr);
}

}  // namespace

extern "C" int geossl_infograph_width_ok(int F) { return width_ok(F) ? 1 : 0; }

extern "C" int64_t geossl_infograph_fwd_workspace_floats(int64_t B) { return 6 * (B > 0 ? B : 1); }

extern "C" int geossl_infograph_fwd_dyn(const float* x, int64_t N, int F, const float* W, const int32_t* mol_ptr,
                                        int64_t B, int readout, const float* m_in, float* s, float* h, float* scores,
                                        float* workspace, float* loss, int32_t* counts, const int32_t* dyn_N,
                                        hipStream_t stream) {
  if (!args_ok(N, F, B, readout, m_in)) return (int)hipErrorInvalidValue;
  double* part = reinterpret_cast<double*>(workspace);
  int32_t* hits = reinterpret_cast<int32_t*>(workspace + 4 * B);
  const dim3 tiles((unsigned)((B + kTile - 1) / kTile));
  dispatch_int<64, 128, 256>(F, [&](auto f) {
    hipLaunchKernelGGL(k_ig_summary<decltype(f)::value>, tiles, dim3(F), 0, stream, x, mol_ptr, (int)B, readout, m_in, W,
                       s, h);
  });
  GEOSSL_CHECK_LAUNCH();
  const dim3 mols((unsigned)B), block(kScoreBlock);
  dispatch_int<1, 2, 4>(F / 64, [&](auto v) {
    hipLaunchKernelGGL(k_ig_scores<decltype(v)::value>, mols, block, 0, stream, x, (int)N, mol_ptr, (int)B, h, scores,
                       part, hits);
  });
  GEOSSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_ig_loss, dim3(1), dim3(kLossBlock), 0, stream, part, hits, (int)B, (int)N, dyn_N, loss, counts);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_infograph_fwd(const float* x, int64_t N, int F, const float* W, const int32_t* mol_ptr,
                                    int64_t B, int readout, const float* m_in, float* s, float* h, float* scores,
                                    float* workspace, float* loss, int32_t* counts, hipStream_t stream) {
  return geossl_infograph_fwd_dyn(x, N, F, W, mol_ptr, B, readout, m_in, s, h, scores, workspace, loss, counts,
                                  nullptr, stream);
}

extern "C" int geossl_infograph_bwd_dyn(const float* x, int64_t N, int F, const float* W, const int32_t* mol_ptr,
                                        int64_t B, int readout, const float* s, const float* h, const float* scores,
                                        const float* gout, float* dx, float* dm, float* dh, const int32_t* dyn_N,
                                        hipStream_t stream) {
  if (!args_ok(N, F, B, readout, dm)) return (int)hipErrorInvalidValue;
  const dim3 tiles((unsigned)((B + kTile - 1) / kTile));
  dispatch_int<64, 128, 256>(F, [&](auto f) {
    hipLaunchKernelGGL(k_ig_bwd<decltype(f)::value>, tiles, dim3(F), 0, stream, x, (int)N, dyn_N, W, mol_ptr, (int)B,
                       readout, s, h, scores, gout, dx, dm, dh);
  });
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_infograph_bwd(const float* x, int64_t N, int F, const float* W, const int32_t* mol_ptr,
                                    int64_t B, int readout, const float* s, const float* h, const float* scores,
                                    const float* gout, float* dx, float* dm, float* dh, hipStream_t stream) {
  return geossl_infograph_bwd_dyn(x, N, F, W, mol_ptr, B, readout, s, h, scores, gout, dx, dm, dh, nullptr, stream);
}
