// The Gaussian-smearing fragments of one 32-row tile of pair rows, as the filter backward (filter_bwd.hip, two fp16
// pieces) multiplies them: B operand of dW1 = dU^T rbf with the pair row on K,
//     B[k = row = 16 ks + kperm(e, kh)][n = g = 32 gb + (lane & 31)],   kh = lane >> 5,
// split into two fp16 pieces at the fixed scale 2^14 (a Gaussian is <= 1).  A tile is 2 x 2 x 64 ITEMS
// (it = (gb * 2 + ks) * 64 + lane), an item two 16-byte words (piece h, piece l), the tile
//     [gb 2][ks 2][piece 2][64 lanes] of u32x4 = 8 KB,
// in LDS (BwdLdsH::rbf) and in the per-step image in HBM (k_rbf_fragments) alike.  The words depend on the row's distance,
// the model's centres / coeff and G only - not on the layer, the weights or any running operand scale - so the image is
// built once per step and every layer's launch copies it; ONE function forms an item for both, so they cannot drift.
#pragma once
#include "split.h"

namespace geossl {

constexpr int RBF_TILE_ROWS = 32;
constexpr int RBF_TILE_ITEMS = 2 * 2 * 64;
constexpr int RBF_TILE_WORDS = 2 * RBF_TILE_ITEMS;  // u32x4 per tile

// first word (piece h) of item `it` inside its tile; piece l is 64 words on
__device__ __forceinline__ int rbf_item_word(int it) { return (it >> 6) * 128 + (it & 63); }

// Item `it` of a tile.  d_of_row(r): distance of the tile's row r in [0, 32) - whatever the caller substitutes for rows
// past the real count included (their dO is exactly zero; the words only have to be finite).  Gaussians at and past G
// are zero, except column 63 when G < 64: a column of ONES, so that dW1[:, 63] = sum over the rows of dU = db1 comes
// out of the matrix pipe with the rest of dW1.
template <class DFn>
__device__ __forceinline__ Frag2 rbf_fragment_item(int it, DFn d_of_row, const float* __restrict__ offset, float coeff,
                                                   int G) {
  const int ln = it & 63, ks = (it >> 6) & 1, gb = it >> 7;
  const int gg = 32 * gb + (ln & 31);
  const float off = gg < G ? offset[gg] : 0.0f;
  const float pad = (gg == 63 && G < 64) ? 1.0f : 0.0f;
  float u8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float diff = d_of_row(16 * ks + kperm(e, ln >> 5)) - off;
    u8[e] = gg < G ? exp_neg(coeff * (diff * diff)) : pad;
  }
  return split8h_scaled(u8, 16384.0f);
}

}  // namespace geossl
