// PaiNN interaction on atom tiles: the filter on the matrix pipe without a molecule in LDS (PaiNNInteraction.forward,
// Geom3D/models/painn.py:54-64 with the filter of :241-245; F = 128, R in {8, 16, 20}).
//
// painn_mma.hip stages a whole molecule in LDS (at most 44 atoms) and lays the edge list out in groups.  A structure of
// hundreds of atoms (a protein pocket) fits neither, and at pocket density with a 32-neighbour cap almost every atom has
// exactly 32 edges: ONE ATOM IS ONE 32-ROW MFMA TILE.  So these kernels walk an atom's incidence list in tiles of 32
// rows, need no group layout, and read the rows of the atoms at the other end of the edges from L2 (lane = feature:
// 128 contiguous bytes per half-wave, channel and edge).
//
// Work split: a 256-thread block is a team of four waves, persistent over the atom list; wave m owns features
// 32 m .. 32 m + 31 of the three channels and keeps its Wf' = [Wf | b | 0] fragments in registers as two fp16 pieces
// under a power-of-two scale (painn_frag.h).  Per tile W = phi' Wf'^T with phi'_e = [phi_e, 1, 0 ..] (three products per
// k-step); the C layout puts the feature on the lane and 16 edge rows in the registers, so the sum over an atom's edges
// is a sum over registers, carried in the same registers from tile to tile for an atom with more than 32 edges, and the
// two halves of a wave are added once per atom (v_permlane32_swap).  Every order is fixed by the tile layout: results are
// bit-reproducible and do not depend on which block an atom lands in.
//
// Backward (over source atoms j): the first GEMM recomputes W; the lanes form dx, dmu_j and the filter cotangents
// t_c(e, f) IN THE ACCUMULATOR LAYOUT (column = feature on the lane, rows = edges in the registers), which is exactly the
// operand layout of a following 32x32x16 MFMA that contracts over those rows (split.h: kperm): the filter gradient
//     dWf'[c F + f][k] += sum_e t_c(e, f) phi'_e[k]
// takes t as its A operand with no lane movement; phi'^T comes from a wave-private LDS image of the tile's 32 rows, read
// with the same (k-step, half, element) -> edge map.  The 3 x 16 gradient accumulators of a wave live for the whole
// block and are stored once as the block's partial (summed by k_reduce_multi in block order).
// Precision of t: THREE bf16 PIECES for both operands of the second GEMM (six products per k-step, split.h).  bf16 has
// the exponent range of fp32, so no scale is involved: upstream gradients of any size (the tests go down to 2^-20)
// accumulate across tiles in one set of registers, which two fp16 pieces under per-tile scales could not do, and no
// max pass over the launch is needed.
//
// Built WITHOUT packed fp32 arithmetic (build.py: -fno-slp-vectorize), like painn_mma.hip.
#include "common.h"
#include "geossl_hip.h"
#include "painn_frag.h"
#include "split.h"
#include "tn.h"

using namespace geossl;

namespace {

constexpr int PT_FWD_BLOCKS = 512;  // blocks of a forward launch (two per CU), striding over the atom list
constexpr int PT_BWD_BLOCKS = 256;  // backward: one per CU (the general form's registers); one filter-gradient partial each
constexpr int PT_PSTR = 36;     // row stride of the phi' image in LDS (floats; 16-byte rows, off the bank period)

struct PainnTileArgs {
  const float* q;        // forward: q [N][F];            backward: dq_out [N][F]
  const float* mu;       // forward: mu [N][3][F] or NULL;  backward: dmu_out [N][3][F]
  const float* xc;       // context features [N][3F]
  const float* mu_src;   // backward: mu [N][3][F] or NULL
  const int64_t* idx_other;  // forward: idx_j, backward: idx_i
  const int64_t* inc_ptr;
  const int32_t* inc_idx;
  const float* phi;
  const float* fcut;
  const float* dir;
  const float* Wf;
  const float* bf;
  const int32_t* atom_list;
  const int32_t* dyn_nlist;
  int nlist;
  float* out0;   // forward: q_out;   backward: dxc [N][3F]
  float* out1;   // forward: mu_out;  backward: dmu_in [N][3][F] or NULL
  float* pw;     // backward: filter-gradient partials [blocks][3F][R]
  float* pb;     // backward: [blocks][3F]
};

// One row of a tile as it travels through the load pipeline: this lane's share of the edge's data.
template <int R>
struct TileRow {
  f32x4 p[3];   // radial basis: k = 8 kh .. 8 kh + 7 and (kh = 0) k = 16 .. 19
  float fc, d0, d1, d2;
  int other;
  __device__ __forceinline__ void request(const PainnTileArgs& A, int ec, int kh) {
    static_assert(R % 4 == 0 && R <= 20, "R: a multiple of 4, at most 20");
    const float* row = A.phi + (size_t)ec * R;
#pragma unroll
    for (int h = 0; h < 3; ++h) {
      const int kg = h < 2 ? 8 * kh + 4 * h : 16 + 8 * kh;  // first index of the group of four (kh is a run-time value)
      p[h] = *reinterpret_cast<const f32x4*>(row + min(kg, R - 4));
    }
    fc = A.fcut[ec];
    d0 = A.dir[3 * ec];
    d1 = A.dir[3 * ec + 1];
    d2 = A.dir[3 * ec + 2];
    other = (int)A.idx_other[ec];
  }
  // v[ks][e] = sc * phi'[16 ks + 8 kh + e],  phi' = [phi, 1, 0 ..]  (sc: a power of two, or 0 for a padding row)
  __device__ __forceinline__ void values(int kh, float sc, float (&v)[2][8]) const {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int kg = 16 * ks + 8 * kh + 4 * h;
        const f32x4 q = ks == 0 ? p[h] : p[2];
        const bool in = kg < R && (ks == 0 || h == 0), isb = kg == R;
        v[ks][4 * h + 0] = in ? q[0] * sc : (isb ? sc : 0.0f);
        v[ks][4 * h + 1] = in ? q[1] * sc : 0.0f;
        v[ks][4 * h + 2] = in ? q[2] * sc : 0.0f;
        v[ks][4 * h + 3] = in ? q[3] * sc : 0.0f;
      }
  }
};

struct TilePos {  // a team's position in its sequence of tiles (wave-uniform)
  int k, atom, pc, p0, p1, valid;
};

// Which list entries a block takes: k = first, first + stride, ... below end.  Blocks are dealt to the eight XCDs in turn,
// and each XCD has an L2 of its own: block b works inside the (b mod 8)-th of eight contiguous shares of the list, so that
// the rows its edges gather - atoms of the same structure, neighbours in the list - stay in ONE L2 instead of passing
// through all eight.  A function of the counts alone; an atom's results do not depend on it.
struct ListShare {
  int first, stride, end;
};
__device__ __forceinline__ ListShare list_share(int cnt) {
  const int nb = (int)gridDim.x, b = (int)blockIdx.x;
  if (nb % 8 != 0) return ListShare{b, nb, cnt};
  const int share = (cnt + 7) / 8, x = b & 7;
  return ListShare{x * share + (b >> 3), nb >> 3, min(cnt, (x + 1) * share)};
}

// W (scaled) of the tile's 32 rows, this wave's 32 features: NC channels, three products per k-step
template <int NC>
__device__ __forceinline__ void filter_tile(const Frag2 (&a)[2], const u32x4 (&wh)[3][2], const u32x4 (&wl)[3][2],
                                            f32x16 (&acc)[3]) {
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.0f;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {  // (independent accumulator chains, interleaved)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = mfma_f16(a[ks].l, wh[c][ks], acc[c]);
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = mfma_f16(a[ks].h, wl[c][ks], acc[c]);
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = mfma_f16(a[ks].h, wh[c][ks], acc[c]);
  }
}

// ------------------------------------------------------------------------------------------------- forward
// q_out[i] = q[i] + sum_e dq_e, mu_out[i] = mu[i] + sum_e (dmuR_e dir_e + dmumu_e mu[j_e]) over the edges e of target i,
// [dq, dmuR, dmumu]_e = W_e * x[j_e]   (painn.py:54-64).  MZ: mu is identically zero (A.mu is NULL): no mu rows are
// gathered and the dmumu * mu_j term drops out.
template <int R, bool MZ>
__global__ __launch_bounds__(256, 2) void k_painn_fwd_tile(PainnTileArgs A) {
  constexpr int F = PM_F;
  __shared__ __attribute__((aligned(16))) float tab_s[4][5 * 32];  // per wave: source atom, dir x, y, z, kk * fcut of the rows
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, m = tid >> 6, j = lane & 31, kh = lane >> 5;
  float* tab = tab_s[m];
  const int cnt = dyn_count(A.nlist, A.dyn_nlist);
  const float wmax = filter_max<R>(A.Wf, A.bf, red);
  int eW;
  const float sW = pow2_scale_to_2p14(wmax, eW);
  const float kk = __builtin_amdgcn_ldexpf(1.0f, eW - 28);  // undoes 2^(14 - eW) and the 2^14 of phi'
  u32x4 wh[3][2], wl[3][2];
  load_filter_fragments<R>(A.Wf, A.bf, m, lane, sW, wh, wl);
  const int f = 32 * m + j;  // this lane's feature
  const ListShare ls = list_share(cnt);
  const int stride = ls.stride;
  // half kh of a wave writes output components 2 kh, 2 kh + 1 of (q, mu x, mu y, mu z)
  auto write_atom = [&](int i, float t0, float t1) {
    const float* mi = A.mu + (size_t)i * 3 * F + f;
    float* mo = A.out1 + (size_t)i * 3 * F + f;
    if (kh == 0) {
      A.out0[(size_t)i * F + f] = A.q[(size_t)i * F + f] + t0;               // :63
      mo[0] = (MZ ? 0.0f : mi[0]) + t1;                                      // :64, x
    } else {
      mo[F] = (MZ ? 0.0f : mi[F]) + t0;                                      // y
      mo[2 * F] = (MZ ? 0.0f : mi[2 * F]) + t1;                              // z
    }
  };
  auto enter = [&](TilePos& t) {  // t.k set: the first tile of the next listed atom that has edges
    for (;;) {
      if (t.k >= ls.end) {
        t = TilePos{t.k, 0, 0, 0, 0, 0};
        return;
      }
      const int i = A.atom_list != nullptr ? A.atom_list[t.k] : t.k;
      const int p0 = (int)A.inc_ptr[i], p1 = (int)A.inc_ptr[i + 1];
      if (p1 > p0) {
        t = TilePos{t.k, i, p0, p0, p1, 1};
        return;
      }
      write_atom(i, 0.0f, 0.0f);  // an atom without edges keeps its features
      t.k += stride;
    }
  };
  auto advance = [&](TilePos& t) {
    if (!t.valid) return;
    t.pc += 32;
    if (t.pc >= t.p1) {
      t.k += stride;
      enter(t);
    }
  };
  auto edge_of = [&](const TilePos& t) {  // stage 1: the edge of this lane's row (clamped: always an edge of the atom)
    return t.valid ? A.inc_idx[min(t.pc + j, t.p1 - 1)] : 0;
  };
  TilePos T0{ls.first, 0, 0, 0, 0, 0};
  enter(T0);
  TilePos T1 = T0;
  advance(T1);
  TilePos T2 = T1;
  advance(T2);
  TileRow<R> r0, r1;
  int e0 = edge_of(T0), e1 = edge_of(T1), e2 = edge_of(T2);
  if (T0.valid) r0.request(A, e0, kh);
  float sq = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;  // this half's 16 rows of every tile of the current atom
  while (T0.valid) {
    // ---- requests one and two tiles ahead
    if (T1.valid) r1.request(A, e1, kh);
    TilePos T3 = T2;
    advance(T3);
    const int e3 = edge_of(T3);
    // ---- this tile: A fragments, row table
    const bool valid = T0.pc + j < T0.p1;
    float v[2][8];
    r0.values(kh, valid ? 16384.0f : 0.0f, v);
    Frag2 a[2];
    a[0] = split8h(v[0]);
    a[1] = split8h(v[1]);
    if (kh == 0) {
      reinterpret_cast<int*>(tab)[j] = r0.other;
      tab[32 + j] = r0.d0;
      tab[64 + j] = r0.d1;
      tab[96 + j] = r0.d2;
      tab[128 + j] = valid ? kk * r0.fc : 0.0f;
    }
    f32x16 acc[3];
    filter_tile<3>(a, wh, wl, acc);
    // ---- messages of the lane's 16 rows (register r = 4 q4 + e <-> row 8 q4 + 4 kh + e)
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int4 jo = *reinterpret_cast<const int4*>(tab + 8 * q4 + 4 * kh);
      const f32x4 d0 = *reinterpret_cast<const f32x4*>(tab + 32 + 8 * q4 + 4 * kh);
      const f32x4 d1 = *reinterpret_cast<const f32x4*>(tab + 64 + 8 * q4 + 4 * kh);
      const f32x4 d2 = *reinterpret_cast<const f32x4*>(tab + 96 + 8 * q4 + 4 * kh);
      const f32x4 kf = *reinterpret_cast<const f32x4*>(tab + 128 + 8 * q4 + 4 * kh);
      const int jov[4] = {jo.x, jo.y, jo.z, jo.w};
      float xv[4][3], mv[4][3];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          xv[e][c] = A.xc[(size_t)jov[e] * 3 * F + c * F + f];
          if constexpr (!MZ) mv[e][c] = A.mu[(size_t)jov[e] * 3 * F + c * F + f];
        }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * q4 + e;
        const float x0 = (acc[0][r] * kf[e]) * xv[e][0], x1 = (acc[1][r] * kf[e]) * xv[e][1];   // painn.py:241, :56
        sq += x0;                                                                            // :59
        if constexpr (MZ) {
          s0 += x1 * d0[e];
          s1 += x1 * d1[e];
          s2 += x1 * d2[e];
        } else {
          const float x2 = (acc[2][r] * kf[e]) * xv[e][2];
          s0 += x1 * d0[e] + x2 * mv[e][0];                                                  // :60-61
          s1 += x1 * d1[e] + x2 * mv[e][1];
          s2 += x1 * d2[e] + x2 * mv[e][2];
        }
      }
    }
    // ---- the atom's last tile: the halves exchange (half kh keeps components 2 kh, 2 kh + 1) and the atom is written
    if (T0.pc + 32 >= T0.p1) {  // uniform
      const float g0 = swap_halves(kh ? sq : s1), g1 = swap_halves(kh ? s0 : s2);
      const float t0 = kh ? g0 + s1 : sq + g0, t1 = kh ? g1 + s2 : s0 + g1;   // lower half's rows + upper half's rows
      write_atom(T0.atom, t0, t1);
      sq = s0 = s1 = s2 = 0.0f;
    }
    // ---- rotate the pipeline
    T0 = T1;
    T1 = T2;
    T2 = T3;
    e0 = e1;
    e1 = e2;
    e2 = e3;
    r0 = r1;
  }
}

// ------------------------------------------------------------------------------------------------ backward
// Over source atoms j (edges with idx_j[e] == j): dxc[j], dmu_in[j] and the block's filter-gradient partial - the
// arithmetic of k_painn_interaction_bwd (painn.hip).  MZ: mu is identically zero (A.mu_src is NULL): dmu_in is not
// written, and channel 2 of the filter (dmumu) has neither a dx nor a filter gradient.
template <int R, bool MZ>
__global__ __launch_bounds__(256) void k_painn_bwd_tile(PainnTileArgs A) {
  constexpr int F = PM_F, NC = MZ ? 2 : 3;
  __shared__ __attribute__((aligned(16))) float tab_s[4][6 * 32];         // per wave: target atom, dir x, y, z, kk * fcut, fcut
  __shared__ __attribute__((aligned(16))) float ptab_s[4][32 * PT_PSTR];  // per wave: phi' of the tile's rows
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, m = tid >> 6, j = lane & 31, kh = lane >> 5;
  float* tab = tab_s[m];
  float* ptab = ptab_s[m];
  const int cnt = dyn_count(A.nlist, A.dyn_nlist);
  const float wmax = filter_max<R>(A.Wf, A.bf, red);
  int eW;
  const float sW = pow2_scale_to_2p14(wmax, eW);
  const float kk = __builtin_amdgcn_ldexpf(1.0f, eW - 28);
  u32x4 wh[3][2], wl[3][2];
  load_filter_fragments<R>(A.Wf, A.bf, m, lane, sW, wh, wl);
  const int f = 32 * m + j;
  const ListShare ls = list_share(cnt);
  const int stride = ls.stride;
  // half 0 of a wave writes dxc[j], half 1 dmu_in[j] (residual mu_out = mu + dmu plus the edges that read mu[j])
  auto write_atom = [&](int a, float v0, float v1, float v2) {
    if (kh == 0) {
      float* o = A.out0 + (size_t)a * 3 * F + f;
      o[0] = v0;
      o[F] = v1;
      o[2 * F] = v2;
    } else if constexpr (!MZ) {
      float* o = A.out1 + (size_t)a * 3 * F + f;
      const float* g = A.mu + (size_t)a * 3 * F + f;
      o[0] = g[0] + v0;
      o[F] = g[F] + v1;
      o[2 * F] = g[2 * F] + v2;
    }
  };
  auto enter = [&](TilePos& t) {
    for (;;) {
      if (t.k >= ls.end) {
        t = TilePos{t.k, 0, 0, 0, 0, 0};
        return;
      }
      const int a = A.atom_list != nullptr ? A.atom_list[t.k] : t.k;
      const int p0 = (int)A.inc_ptr[a], p1 = (int)A.inc_ptr[a + 1];
      if (p1 > p0) {
        t = TilePos{t.k, a, p0, p0, p1, 1};
        return;
      }
      write_atom(a, 0.0f, 0.0f, 0.0f);  // an atom nobody reads: zero gradient of x, the residual alone for mu
      t.k += stride;
    }
  };
  auto advance = [&](TilePos& t) {
    if (!t.valid) return;
    t.pc += 32;
    if (t.pc >= t.p1) {
      t.k += stride;
      enter(t);
    }
  };
  auto edge_of = [&](const TilePos& t) { return t.valid ? A.inc_idx[min(t.pc + j, t.p1 - 1)] : 0; };
  float nx[3], nm[3];  // x[j], mu[j] of the atom the NEXT tile starts (requested a tile ahead)
  auto request_atom = [&](int a) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      nx[c] = A.xc[(size_t)a * 3 * F + c * F + f];
      nm[c] = MZ ? 0.0f : A.mu_src[(size_t)a * 3 * F + c * F + f];
    }
  };
  TilePos T0{ls.first, 0, 0, 0, 0, 0};
  enter(T0);
  TilePos T1 = T0;
  advance(T1);
  TilePos T2 = T1;
  advance(T2);
  TileRow<R> r0, r1;
  int e0 = edge_of(T0), e1 = edge_of(T1), e2 = edge_of(T2);
  nx[0] = nx[1] = nx[2] = nm[0] = nm[1] = nm[2] = 0.0f;
  if (T0.valid) {
    r0.request(A, e0, kh);
    request_atom(T0.atom);
  }
  f32x16 gw[3];  // dWf' of this wave's features: row = feature, column (lane) = k; channel c
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) gw[c][r] = 0.0f;
  float xj[3] = {0.0f, 0.0f, 0.0f}, mj[3] = {0.0f, 0.0f, 0.0f};
  float dx[3] = {0.0f, 0.0f, 0.0f}, dmj[3] = {0.0f, 0.0f, 0.0f};  // this half's 16 rows of every tile of the current atom
  while (T0.valid) {
    if (T0.pc == T0.p0) {  // (uniform) the first tile of an atom
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        xj[c] = nx[c];
        mj[c] = nm[c];
      }
    }
    // ---- requests one and two tiles ahead
    if (T1.valid) {
      r1.request(A, e1, kh);
      if (T1.pc == T1.p0) request_atom(T1.atom);
    }
    TilePos T3 = T2;
    advance(T3);
    const int e3 = edge_of(T3);
    // ---- this tile: phi' as the first GEMM's A fragments and as an LDS image for the second, row table
    const bool valid = T0.pc + j < T0.p1;
    float v[2][8];
    r0.values(kh, valid ? 1.0f : 0.0f, v);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 w = {v[ks][4 * h], v[ks][4 * h + 1], v[ks][4 * h + 2], v[ks][4 * h + 3]};
        *reinterpret_cast<f32x4*>(ptab + j * PT_PSTR + 16 * ks + 8 * kh + 4 * h) = w;
      }
    Frag2 a[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      float vs[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) vs[e] = v[ks][e] * 16384.0f;
      a[ks] = split8h(vs);
    }
    if (kh == 0) {
      reinterpret_cast<int*>(tab)[j] = r0.other;
      tab[32 + j] = r0.d0;
      tab[64 + j] = r0.d1;
      tab[96 + j] = r0.d2;
      tab[128 + j] = valid ? kk * r0.fc : 0.0f;
      tab[160 + j] = valid ? r0.fc : 0.0f;
    }
    f32x16 acc[3];
    filter_tile<NC>(a, wh, wl, acc);
    // ---- the lane's 16 rows: dx, dmu_j, and the filter cotangents t_c in place of W_c (register r <-> row 8 q4 + 4 kh + e)
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int4 io = *reinterpret_cast<const int4*>(tab + 8 * q4 + 4 * kh);
      const f32x4 d0 = *reinterpret_cast<const f32x4*>(tab + 32 + 8 * q4 + 4 * kh);
      const f32x4 d1 = *reinterpret_cast<const f32x4*>(tab + 64 + 8 * q4 + 4 * kh);
      const f32x4 d2 = *reinterpret_cast<const f32x4*>(tab + 96 + 8 * q4 + 4 * kh);
      const f32x4 kf = *reinterpret_cast<const f32x4*>(tab + 128 + 8 * q4 + 4 * kh);
      const f32x4 fc = *reinterpret_cast<const f32x4*>(tab + 160 + 8 * q4 + 4 * kh);
      const int iov[4] = {io.x, io.y, io.z, io.w};
      float gq[4], gm[4][3];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        gq[e] = A.q[(size_t)iov[e] * F + f];
#pragma unroll
        for (int c = 0; c < 3; ++c) gm[e][c] = A.mu[(size_t)iov[e] * 3 * F + c * F + f];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * q4 + e;
        const float W0 = acc[0][r] * kf[e], W1 = acc[1][r] * kf[e];
        const float s1 = gm[e][0] * d0[e] + gm[e][1] * d1[e] + gm[e][2] * d2[e];
        dx[0] = fmaf(gq[e], W0, dx[0]);
        dx[1] = fmaf(s1, W1, dx[1]);
        acc[0][r] = gq[e] * xj[0] * fc[e];
        acc[1][r] = s1 * xj[1] * fc[e];
        if constexpr (!MZ) {
          const float W2 = acc[2][r] * kf[e];
          const float s2 = gm[e][0] * mj[0] + gm[e][1] * mj[1] + gm[e][2] * mj[2];
          dx[2] = fmaf(s2, W2, dx[2]);
          const float x2 = W2 * xj[2];
          dmj[0] = fmaf(gm[e][0], x2, dmj[0]);
          dmj[1] = fmaf(gm[e][1], x2, dmj[1]);
          dmj[2] = fmaf(gm[e][2], x2, dmj[2]);
          acc[2][r] = s2 * xj[2] * fc[e];
        }
      }
    }
    // ---- filter gradient: gw[c] += t_c^T phi' over the tile's rows.  k-step s, half kh, element e <-> row
    // 16 s + kperm(e, kh): register 8 s + e of the accumulator layout
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float pv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) pv[e] = ptab[(16 * s + kperm(e, kh)) * PT_PSTR + j];
      const Frag3 pf = split8(pv);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        float tv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) tv[e] = acc[c][8 * s + e];
        const Frag3 tf = split8(tv);
        mma6(gw[c], tf, pf);
      }
    }
    // ---- the atom's last tile: the halves exchange and the atom is written
    if (T0.pc + 32 >= T0.p1) {  // uniform
      float o[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float got = swap_halves(kh ? dx[c] : dmj[c]);     // the other half's rows of what this half writes
        o[c] = kh ? got + dmj[c] : dx[c] + got;                 // lower half's rows + upper half's rows
        dx[c] = dmj[c] = 0.0f;
      }
      write_atom(T0.atom, o[0], o[1], o[2]);
    }
    T0 = T1;
    T1 = T2;
    T2 = T3;
    e0 = e1;
    e1 = e2;
    e2 = e3;
    r0 = r1;
  }
  // ---- the block's partial: gw[c][reg] = dWf'[c F + 32 m + c_row(reg, lane)][k = j]; column R is the bias
  float* pw = A.pw + (size_t)blockIdx.x * 3 * F * R;
  float* pb = A.pb + (size_t)blockIdx.x * 3 * F;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = c * F + 32 * m + c_row(r, lane);
      const float g = c < NC ? gw[c][r] : 0.0f;
      if (j < R) pw[(size_t)row * R + j] = g;
      if (j == R) pb[row] = g;
    }
}

inline bool tile_ok(int F, int R) { return F == PM_F && (R == 8 || R == 16 || R == 20); }
inline int tile_blocks(int64_t nlist, int cap) { return (int)(nlist < cap ? nlist : cap); }

}  // namespace

#define PAINN_TILE_LAUNCH(KERNEL, MZV, NB)                                                                        \
  do {                                                                                                            \
    if (R == 20) hipLaunchKernelGGL((KERNEL<20, MZV>), dim3((unsigned)(NB)), dim3(256), 0, stream, a);            \
    else if (R == 16) hipLaunchKernelGGL((KERNEL<16, MZV>), dim3((unsigned)(NB)), dim3(256), 0, stream, a);       \
    else hipLaunchKernelGGL((KERNEL<8, MZV>), dim3((unsigned)(NB)), dim3(256), 0, stream, a);                     \
  } while (0)

extern "C" int geossl_painn_tile_ok(int F, int R) { return tile_ok(F, R) ? 1 : 0; }

extern "C" int geossl_painn_interaction_fwd_tile(const float* q, const float* mu, const float* xc, const int64_t* idx_j,
                                                 const int64_t* inc_ptr, const int32_t* inc_idx, const float* phi,
                                                 const float* fcut, const float* dir, const float* Wf, const float* bf,
                                                 const int32_t* atom_list, int64_t nlist, const int32_t* dyn_nlist, int F,
                                                 int R, float* q_out, float* mu_out, hipStream_t stream) {
  if (!tile_ok(F, R) || nlist >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  if (nlist <= 0) return 0;
  PainnTileArgs a{};
  a.q = q; a.mu = mu; a.xc = xc; a.idx_other = idx_j; a.inc_ptr = inc_ptr; a.inc_idx = inc_idx; a.phi = phi; a.fcut = fcut;
  a.dir = dir; a.Wf = Wf; a.bf = bf; a.atom_list = atom_list; a.dyn_nlist = dyn_nlist; a.nlist = (int)nlist;
  a.out0 = q_out; a.out1 = mu_out;
  const int nb = tile_blocks(nlist, PT_FWD_BLOCKS);  // (a function of nlist alone: a captured launch serves any *dyn_nlist)
  if (mu == nullptr) PAINN_TILE_LAUNCH(k_painn_fwd_tile, true, nb);
  else PAINN_TILE_LAUNCH(k_painn_fwd_tile, false, nb);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t geossl_painn_interaction_bwd_tile_workspace_floats(int64_t nlist, int F, int R) {
  return (int64_t)tile_blocks(nlist > 0 ? nlist : 0, PT_BWD_BLOCKS) * (3 * (int64_t)F * R + 3 * F);
}

extern "C" int geossl_painn_interaction_bwd_tile(const float* dq_out, const float* dmu_out, const float* mu,
                                                 const float* xc, const int64_t* idx_i, const int64_t* inc_ptr,
                                                 const int32_t* inc_idx, const float* phi, const float* fcut,
                                                 const float* dir, const float* Wf, const float* bf,
                                                 const int32_t* atom_list, int64_t nlist, const int32_t* dyn_nlist, int F,
                                                 int R, float* dxc, float* dmu_in, float* dWf, float* dbf,
                                                 float* workspace, int accumulate, hipStream_t stream) {
  if (!tile_ok(F, R) || nlist >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
  if ((mu == nullptr) != (dmu_in == nullptr)) return (int)hipErrorInvalidValue;  // mu identically zero: no gradient of it
  if (nlist <= 0) return 0;
  const int nb = tile_blocks(nlist, PT_BWD_BLOCKS);
  PainnTileArgs a{};
  a.q = dq_out; a.mu = dmu_out; a.xc = xc; a.mu_src = mu; a.idx_other = idx_i; a.inc_ptr = inc_ptr; a.inc_idx = inc_idx;
  a.phi = phi; a.fcut = fcut; a.dir = dir; a.Wf = Wf; a.bf = bf; a.atom_list = atom_list; a.dyn_nlist = dyn_nlist;
  a.nlist = (int)nlist; a.out0 = dxc; a.out1 = dmu_in;
  a.pw = workspace;
  a.pb = workspace + (size_t)nb * 3 * F * R;
  if (mu == nullptr) PAINN_TILE_LAUNCH(k_painn_bwd_tile, true, nb);
  else PAINN_TILE_LAUNCH(k_painn_bwd_tile, false, nb);
  GEOSSL_CHECK_LAUNCH();
  ReduceMulti rm;  // both fixed-order sums over the block partials in one launch
  float* ow[1] = {dWf};
  float* ob[1] = {dbf};
  rm.add(a.pw, 3 * F * R, 3 * F * R, 3 * F * R, 1, ow, 1);
  rm.add(a.pb, 3 * F, 3 * F, 3 * F, 1, ob, 1);
  hipLaunchKernelGGL(geossl::k_reduce_multi, dim3(rm.blocks(), 1), dim3(256), 0, stream, rm, nb, accumulate);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
