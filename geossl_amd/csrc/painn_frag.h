// Filter operands of PaiNN's matrix-pipe interaction kernels (painn_mma.hip, painn_tile.hip; F = 128): the fragments of
// Wf' = [Wf | b | 0 ...] a wave keeps in registers, the magnitude its power-of-two scale comes from, and the exchange of
// the two halves of a wave.
#pragma once
#include "common.h"
#include "split.h"

namespace geossl {

constexpr int PM_F = 128;

// Wf' B fragments of this wave's 32 features, channel c, k-step ks: lane (col, kh) holds Wf'[c F + 32 m + col][16 ks + 8 kh + e]
template <int R>
__device__ __forceinline__ void load_filter_fragments(const float* __restrict__ Wf, const float* __restrict__ bf, int m,
                                                      int lane, float sW, u32x4 (&wh)[3][2], u32x4 (&wl)[3][2]) {
  const int col = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int rowi = c * PM_F + 32 * m + col;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = 16 * ks + 8 * kh + e;
        v[e] = (k < R ? Wf[(size_t)rowi * R + min(k, R - 1)] : (k == R ? bf[rowi] : 0.0f)) * sW;
      }
      const Frag2 f = split8h(v);
      wh[c][ks] = f.h;
      wl[c][ks] = f.l;
    }
  }
}

// largest magnitude of Wf' (all 3F rows), block-wide
template <int R>
__device__ __forceinline__ float filter_max(const float* __restrict__ Wf, const float* __restrict__ bf, float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float mx = 0.0f;
  for (int i = tid; i < 3 * PM_F * R; i += 256) mx = fmaxf(mx, fabsf(Wf[i]));
  for (int i = tid; i < 3 * PM_F; i += 256) mx = fmaxf(mx, fabsf(bf[i]));
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return mx;
}

// the value of lane l ^ 32 (v_permlane32_swap: one vector instruction, no LDS crossbar round trip)
__device__ __forceinline__ float swap_halves(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);  // r[0]: upper half <- lower half of u; r[1]: lower <- upper
  return __builtin_bit_cast(float, (threadIdx.x & 32) ? r[0] : r[1]);
}

}  // namespace geossl
