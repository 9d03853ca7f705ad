// The three kernels around the backbone in MD17 evaluation (examples/finetune_md17.py:70-123) and its loader:
//
// geossl_energy_head_fwd, k_energy_fwd (kTile molecules per block, thread j = feature j): the energy head of :94-97 and
//   the seed of :99's position gradient in ONE launch, so that a forward that also returns forces needs no autograd
//   node for readout and head.
//   Heads: 0 = Linear(F, 1) (w [F], b [1]); 1 = PaiNN's create_output_layers() at its defaults, Dense(F, F/2, silu) then
//   Dense(F/2, 1) (W1 [F/2][F], b1 [F/2], w2 [F/2], b2 [1]) - property_head.hip's two heads, with its arithmetic:
//     m_b = readout_col of the atom rows of molecule b (common.h: the backbone's bits);
//     head 1: z_bk = b1_k + sum_j W1_kj m_bj (fp32 fma chain in j order), a_bk = silu(z_bk);
//     energy_b = bias + <w, m_b> (head 0) or b2 + <w2, a_b> (head 1): lane products, a fixed xor tree per wave, the waves
//       added in order;
//     seed = d(sum_b energy_b) / dh: dm_b = w (head 0), or dz_bk = w2_k silu'(z_bk) and dm_bj = sum_k dz_bk W1_kj (head
//       1) - k_prop_bwd's lines at dpred = 1; every atom row of molecule b receives dm_b (/ max(n_b, 1) for "mean").
//   Every row of seed that belongs to a molecule is written; no row at or past N is read or written.
//
// geossl_force_metrics_accumulate, k_force_metrics (one block): the two sums of absolute errors of :116-117 and their
//   element counts, added onto a persistent accumulator [sum |dE| (f64), sum |dF| (f64), count E (i64), count F (i64)]
//   that the caller zeroes before an epoch and reads once behind it.  The differences are formed in fp32 (the reference's
//   tensors are), pred_force = -dE_dpos; thread t adds the elements t, t + 256, ... in order into fp64, then the block
//   tree of head_common.h.  An element whose dE_dpos is NaN is skipped on both sides and not counted (:104-107); the
//   energies are never skipped.  The accumulator's address is the only state: a captured graph may hold the launch.
//
// geossl_gather_atom_rows, k_gather_rows (one block per molecule): dst rows [mol_ptr[b], mol_ptr[b + 1]) = src rows
//   from src_off[b] on, C floats per row - per-atom targets of a DeviceDataset (forces) into batch order, from the
//   offsets the position gather uploaded.
// Every sum has a fixed order and there are no atomics: the same inputs give the same bits.  All stores are plain vector
// stores.
#include "geossl_hip.h"
#include "head_common.h"

using namespace geossl;

namespace {

constexpr int kTile = 4;   // molecules per block of k_energy_fwd

enum Head { kLinear = 0, kMlp = 1 };

template <int F, bool MLP>
__global__ __launch_bounds__(F) void k_energy_fwd(const float* __restrict__ h, int N, const int32_t* __restrict__ mol_ptr,
                                                  int B, int readout, const float* __restrict__ W1,
                                                  const float* __restrict__ b1, const float* __restrict__ W2,
                                                  const float* __restrict__ b2, float* __restrict__ energy,
                                                  float* __restrict__ seed) {
  constexpr int K = MLP ? F / 2 : F;   // inputs of the last layer
  constexpr int W = F / 64;            // waves per block
  __shared__ float sm[kTile][F];
  __shared__ float sdz[kTile][MLP ? F / 2 : 1];
  __shared__ float red[kTile][W];
  const int j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const int b0 = blockIdx.x * kTile;
  int a0[kTile], a1[kTile];
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    const int b = b0 + t;
    a0[t] = a1[t] = 0;
    float v = 0.0f;
    if (b < B) {
      a0[t] = max(min(mol_ptr[b], N), 0);
      a1[t] = max(min(mol_ptr[b + 1], N), a0[t]);
      v = readout_col(h, F, j, a0[t], a1[t], readout == kMean);
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
        const float zk = acc[t], s = sigmoidf_(zk);
        prod[t] = mul_rn(w2, siluf_(zk));
        sdz[t][j] = mul_rn(w2, s * (1.0f + zk * (1.0f - s)));
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
  __syncthreads();   // (red and sdz)
  if (j < kTile) {
    const int b = b0 + j;
    if (b < B) {
      float s = 0.0f;
#pragma unroll
      for (int w = 0; w < W; ++w) s += red[j][w];
      energy[b] = s + (MLP ? b2[0] : b1[0]);
    }
  }
  float dm[kTile];
  if constexpr (MLP) {
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
    for (int t = 0; t < kTile; ++t) dm[t] = wj;
  }
#pragma unroll
  for (int t = 0; t < kTile; ++t) {
    if (b0 + t >= B) break;
    scatter_readout_col(seed, F, j, a0[t], a1[t], dm[t], readout == kMean);
  }
}

struct Metrics {
  double se, sf;
  long long ne, nf;
  __device__ __forceinline__ Metrics& operator+=(const Metrics& o) {
    se += o.se;
    sf += o.sf;
    ne += o.ne;
    nf += o.nf;
    return *this;
  }
};

__global__ __launch_bounds__(kLossBlock) void k_force_metrics(const float* __restrict__ pred_energy,
                                                              const float* __restrict__ y, int B,
                                                              const float* __restrict__ dE_dpos,
                                                              const float* __restrict__ force, int64_t n3,
                                                              double* __restrict__ sums, long long* __restrict__ counts) {
  __shared__ Metrics red[kLossBlock];
  Metrics m{0.0, 0.0, 0, 0};
  for (int k = threadIdx.x; k < B; k += kLossBlock) {
    m.se += (double)fabsf(sub_rn(pred_energy[k], y[k]));
    m.ne += 1;
  }
  for (int64_t k = threadIdx.x; k < n3; k += kLossBlock) {
    const float g = dE_dpos[k];
    if (g == g) {   // (a NaN of the predicted force drops the element on both sides, finetune_md17.py:104-107)
      m.sf += (double)fabsf(sub_rn(-g, force[k]));
      m.nf += 1;
    }
  }
  const Metrics tot = block_sum<kLossBlock>(m, red);
  if (threadIdx.x == 0) {
    sums[0] += tot.se;
    sums[1] += tot.sf;
    counts[0] += tot.ne;
    counts[1] += tot.nf;
  }
}

__global__ __launch_bounds__(256) void k_gather_rows(const float* __restrict__ src, int64_t n_src, int C,
                                                     const int32_t* __restrict__ src_off,
                                                     const int32_t* __restrict__ mol_ptr, int64_t n_dst,
                                                     float* __restrict__ dst) {
  const int b = blockIdx.x;
  const int64_t d0 = mol_ptr[b], d1 = mol_ptr[b + 1], s0 = src_off[b];
  if (d0 < 0 || d1 > n_dst || d1 < d0 || s0 < 0 || s0 + (d1 - d0) > n_src) return;   // (offsets outside the arrays)
  const int64_t count = (d1 - d0) * C;
  const float* s = src + s0 * C;
  float* d = dst + d0 * C;
  for (int64_t e = threadIdx.x; e < count; e += 256) d[e] = s[e];
}

inline bool width_ok(int F) { return F == 64 || F == 128 || F == 256; }

template <int F>
void launch_energy(int head, dim3 grid, hipStream_t stream, const float* h, int N, const int32_t* mol_ptr, int B,
                   int readout, const float* W1, const float* b1, const float* W2, const float* b2, float* energy,
                   float* seed) {
  if (head == kMlp)
    hipLaunchKernelGGL((k_energy_fwd<F, true>), grid, dim3(F), 0, stream, h, N, mol_ptr, B, readout, W1, b1, W2, b2,
                       energy, seed);
  else
    hipLaunchKernelGGL((k_energy_fwd<F, false>), grid, dim3(F), 0, stream, h, N, mol_ptr, B, readout, W1, b1, W2, b2,
                       energy, seed);
}

}  // namespace

extern "C" int geossl_energy_head_fwd(const float* h, int64_t N, int F, const int32_t* mol_ptr, int64_t B, int readout,
                                      int head, const float* W1, const float* b1, const float* W2, const float* b2,
                                      float* energy, float* seed, hipStream_t stream) {
  if (N < 0 || N >= (1 << 30) || B < 1 || B >= (1 << 24) || !width_ok(F) || (readout != kAdd && readout != kMean) ||
      (head != kLinear && head != kMlp) || h == nullptr || mol_ptr == nullptr || W1 == nullptr || b1 == nullptr ||
      energy == nullptr || seed == nullptr || (head == kMlp && (W2 == nullptr || b2 == nullptr)))
    return (int)hipErrorInvalidValue;
  const dim3 tiles((unsigned)((B + kTile - 1) / kTile));
  dispatch_int<64, 128, 256>(F, [&](auto f) {
    launch_energy<decltype(f)::value>(head, tiles, stream, h, (int)N, mol_ptr, (int)B, readout, W1, b1, W2, b2, energy,
                                      seed);
  });
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_force_metrics_accumulate(const float* pred_energy, const float* y, int64_t B,
                                               const float* dE_dpos, const float* force_target, int64_t N, void* acc,
                                               hipStream_t stream) {
  if (B < 0 || B >= (1 << 24) || N < 0 || N >= (1 << 30) || acc == nullptr ||
      (B > 0 && (pred_energy == nullptr || y == nullptr)) || (N > 0 && (dE_dpos == nullptr || force_target == nullptr)))
    return (int)hipErrorInvalidValue;
  double* sums = reinterpret_cast<double*>(acc);
  long long* counts = reinterpret_cast<long long*>(sums + 2);
  hipLaunchKernelGGL(k_force_metrics, dim3(1), dim3(kLossBlock), 0, stream, pred_energy, y, (int)B, dE_dpos,
                     force_target, (int64_t)3 * N, sums, counts);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_gather_atom_rows(const float* src, int64_t n_src, int C, const int32_t* src_off,
                                       const int32_t* mol_ptr, int64_t B, int64_t N, float* dst, hipStream_t stream) {
  if (src == nullptr || src_off == nullptr || mol_ptr == nullptr || dst == nullptr || n_src < 0 || C < 1 || C > 4096 ||
      B < 0 || B >= (1 << 24) || N < 0)
    return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)B), dim3(256), 0, stream, src, n_src, C, src_off, mol_ptr, N, dst);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
