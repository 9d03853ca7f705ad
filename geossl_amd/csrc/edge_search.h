// The edge range of a structure in a collated edge list (edges grouped by structure in batch order): a 256-ary search
// over the list's first row by one 256-thread block.  Shared by the layout kernels of painn_layout.hip and painn_inc.hip.
#pragma once
#include "common.h"

namespace geossl {

// first e in [0, E) with src[e] >= key (src non-decreasing by molecule), for TWO keys at once, by all 256 threads of the
// block (the two searches share their rounds: the probes of a round are in flight together)
__device__ __forceinline__ void block_lower_bound2(const int64_t* __restrict__ src, int E, int64_t key0, int64_t key1,
                                                   int& out0, int& out1) {
  int lo[2] = {0, 0}, hi[2] = {E, E};
  bool done[2] = {E == 0, E == 0};
  const int64_t key[2] = {key0, key1};
  while (!(done[0] && done[1])) {
    int step[2], p[2];
    bool below[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int len = hi[q] - lo[q];
      step[q] = (len + 255) / 256;
      p[q] = lo[q] + (int)threadIdx.x * step[q];
      below[q] = !done[q] && p[q] < hi[q] && src[p[q]] < key[q];
    }
    const int c0 = __syncthreads_count(below[0] ? 1 : 0);
    const int c1 = __syncthreads_count(below[1] ? 1 : 0);
    const int c[2] = {c0, c1};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (done[q]) continue;
      if (c[q] == 0) {
        hi[q] = lo[q];
        done[q] = true;
      } else if (step[q] == 1) {
        lo[q] = hi[q] = lo[q] + c[q];
        done[q] = true;
      } else {
        const int nlo = lo[q] + (c[q] - 1) * step[q] + 1, nhi = min(hi[q], lo[q] + c[q] * step[q]);
        lo[q] = nlo;
        hi[q] = nhi;
        if (lo[q] >= hi[q]) done[q] = true;
      }
    }
  }
  out0 = lo[0];
  out1 = lo[1];
}

}  // namespace geossl
