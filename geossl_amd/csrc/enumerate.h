// What the batch-assembly kernels share: unranking the extractor's tuple enumerations and the counter-based generator
// of the device-side draws (atom masking, sampled tuples).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace geossl {

// slot p of the lexicographic i<j enumeration of n atoms -> (a, b);  row(a) = a n - a (a + 1) / 2 - a - 1, slot = row(a) + b
__device__ __forceinline__ void pair_of_slot(int p, int n, int& a, int& b) {
  const float t = (float)(2 * n - 1);
  int g = (int)((t - sqrtf(fmaxf(t * t - 8.0f * (float)p, 0.0f))) * 0.5f);
  g = g < 0 ? 0 : (g > n - 2 ? n - 2 : g);
  // first slot of row a: a n - a (a + 1) / 2 (the float estimate is off by at most one)
  while (g > 0 && g * n - g * (g + 1) / 2 > p) --g;
  while (g < n - 2 && (g + 1) * n - (g + 1) * (g + 2) / 2 <= p) ++g;
  a = g;
  b = p - (g * n - g * (g + 1) / 2) + g + 1;
}

// slot q of itertools.permutations(range(n), 2): (a, b), b != a, at column a (n - 1) + (b < a ? b : b - 1)
__device__ __forceinline__ void perm_of_slot(int q, int n, int& a, int& b) {
  a = q / (n - 1);
  const int r = q - a * (n - 1);
  b = r < a ? r : r + 1;
}

// Philox-4x32-10 (Salmon et al., SC'11): words 0 and 1 of the block for counter (c0, c1, 0, 0) under the key's two words
__device__ __forceinline__ void philox_w01(uint32_t c0, uint32_t c1, uint64_t seed, uint32_t& w0, uint32_t& w1) {
  uint32_t c2 = 0, c3 = 0, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w0 = c0;
  w1 = c1;
}

// ... word 0 alone
__device__ __forceinline__ uint32_t philox_w0(uint32_t c0, uint32_t c1, uint64_t seed) {
  uint32_t w0, w1;
  philox_w01(c0, c1, seed, w0, w1);
  return w0;
}

__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = __lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

}  // namespace geossl
