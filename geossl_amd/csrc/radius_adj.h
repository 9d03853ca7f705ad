// Which edges the radius graph has: the adjacency pass of torch_cluster.radius_graph's semantics, shared by every
// kernel that needs the edges (graph.hip: k_radius, sparse_pairs.hip), so that the rule is stated once.
#pragma once
#include "common.h"

namespace geossl {

__device__ __forceinline__ float dist2_nofma(const float* pi, const float* pj) {
  // fl32(fl32(fl32(dx*dx)+fl32(dy*dy))+fl32(dz*dz)), d = x_j - x_i, nothing contracted (common.h)
  return norm2_rn(pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2]);
}

// CFConv envelope, schnet.py:186: 0.5 * (cos(d * PI / cutoff) + 1.0), fp32 op by op
__device__ __forceinline__ float pair_envelope(float d, float cutoff) {
  return 0.5f * (cosf(mul_rn(d, GEOSSL_PI_F) / cutoff) + 1.0f);
}

// One WAVE scans the sources of target atom i of an n-atom molecule whose positions are staged at `sp` ([n][3]): sources
// in ascending order 64 at a time, a hit when the squared distance is below r2, the first `cap` hits kept (the self hit
// counts), the self hit dropped afterwards.  Per chunk c of 64 sources it calls
//     chunk(c, jn, d2, keep, kept, d_in)
// with jn = 64 c + lane this lane's source, d2 its squared distance (0 past the molecule), keep = this lane's edge
// jn -> i exists, kept = the wave's ballot of keep, d_in = edges of the earlier chunks.  Returns the in-degree of i.
// All 64 lanes of the wave must call it together (ballots); `lane` is the lane index inside the wave.
template <class Chunk>
__device__ __forceinline__ int radius_scan_target(const float* sp, int n, int i, int lane, float r2, int cap,
                                                  Chunk&& chunk) {
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  int found = 0, d_in = 0;
  for (int c = 0; c * 64 < n; ++c) {
    const int jn = c * 64 + lane;
    float d2 = 0.0f;
    bool hit = false;
    if (jn < n) {
      d2 = dist2_nofma(sp + 3 * i, sp + 3 * jn);
      hit = d2 < r2;
    }
    const unsigned long long mask = __ballot(hit);
    const int rank = found + __popcll(mask & lt);
    bool keep = hit && rank < cap;
    found += __popcll(mask);
    if (jn == i) keep = false;  // self edge dropped after the cap was applied
    const unsigned long long kept = __ballot(keep);
    chunk(c, jn, d2, keep, kept, d_in);
    d_in += __popcll(kept);
  }
  return d_in;
}

// dynamic LDS of k_radius: the bit matrix [max_n][ceil(max_n / 64)] and the positions
inline size_t radius_lds(int max_n) {
  const size_t words = (max_n + 63) / 64;
  return (size_t)max_n * words * 8 + (size_t)max_n * 12;
}

#define GEOSSL_RADIUS_MAX_N 1024  // largest molecule of the one-block-per-molecule graph kernels (bit matrix 128 KB)

}  // namespace geossl
