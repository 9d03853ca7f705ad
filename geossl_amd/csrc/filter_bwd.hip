// Backward of the continuous-filter network (InteractionBlock.mlp inside CFConv, schnet.py:141-145,186-187) with
// respect to its weights, for all interaction blocks in ONE launch, on the bf16 matrix pipe (split.h).
//
// Upstream gradient per pair slot p = (i<j) of layer l (never stored per pair in HBM):
//     dO[p][c] = C(d_p) * ( flag0 * dagg_l[i][c] * x_l[j][c]  +  flag1 * dagg_l[j][c] * x_l[i][c] )
// and, with t the saved hidden activation and rbf the Gaussian smearing of d_p,
//     dt = dO W2 ;  dU = dt * ssp'(.) ;  dW1 += dU^T rbf ;  db1 += sum dU ;  dW2 += dO^T t ;  db2 += sum dO.
//
// A block works on tiles of pair slots: 32 rows in the three-piece kernel, 64 rows (two 32-row M blocks behind one
// build phase and one barrier pair) in the two-piece kernel.  A tile touches the atoms of at most a few molecules, so rows
// a_lo.. of x_l and dagg_l are staged in LDS with coalesced 16-byte loads (the staging arrays of tile t+1 are published
// during the MFMA phase of tile t, two barriers per tile); from them the block builds, pre-split
// into bf16 pieces and laid out as ready-made MFMA fragments (lane i at byte 16 i: conflict-free ds_read_b128),
//     dOr : dO as A operand with the pair row on M and the channel c on K      (for dt = dO W2; one lane per thread)
//     rbf : Gaussian smearing as B operand with the pair row on K              (for dW1 = dU^T rbf; role-B threads)
//     tf  : the saved activation t as B operand with the pair row on K         (for dW2 = dO^T t; role-A waves, from
//           the C-layout registers they hold anyway)
// The waves of a block are split by role:
//   role A (waves 0..NW-1), hidden units [32w, 32w+32):  dt for its slice (W2 slice as B fragments in registers), dU
//       in place; the C layout of dt (lane = h, register = pair row in `kperm` order) IS the A-fragment layout of
//       dW1's contraction over pair rows, so dU is split in registers and multiplied with the rbf fragments;
//   role B (waves NW..2NW-1), filter channels [32w, 32w+32):  dO with the channel on M is NOT evaluated a second
//       time - the dOr fragments of the wave's channel block go through the matrix pipe against a 16 x 32 selection
//       matrix (6 MFMAs), which lands them transposed in C layout = fragment order, exactly (a bf16 piece times
//       1.0); then dW2[channel block, all h] against the tf fragments, db2 from the same registers.
// T is read from HBM once, the dO tile is evaluated once.  Weight-gradient accumulators stay in registers across all
// tiles of a block; one partial per block, fixed-order reduction afterwards (no atomics).
#include "common.h"
#include "geossl_hip.h"
#include "rbf_frag.h"
#include "split.h"
#include "tn.h"

// atoms a staged window of a 64-row tile holds (tools/filter_bwd_window_share.py: fewer fresh windows per row than 40 atoms
// under a 32-row tile, no unstaged tile on the bench pools; 64 atoms = 64 staging registers per role-B lane: spilled)
#ifndef FB_CAP64
#define FB_CAP64 48
#endif

using namespace geossl;

namespace {

#ifdef FB_TIMING
__device__ long long fb_dbg[2 * 64 * 8];
__device__ long long fb_dbg2[2 * 64];
__device__ long long fb_dbg3[64 * 4];
#define FB_MARK(slot)                                                                                   \
  do {                                                                                                  \
    if (blockIdx.x == 3 && blockIdx.y == 0 && lane == 0 && (wave == 0 || wave == NW) && t - t_begin < 64) \
      fb_dbg[((wave == 0 ? 0 : 1) * 64 + (t - t_begin)) * 8 + (slot)] = clock64();                      \
  } while (0)
#define FB3(slot)                                                                                      \
  do {                                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                  \
    if (blockIdx.x == 3 && blockIdx.y == 0 && lane == 0 && wave == NW && tt - t_begin < 64 && tt > t_begin) \
      fb_dbg3[(tt - t_begin) * 4 + (slot)] = clock64();                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                  \
  } while (0)
#else
#define FB_MARK(slot) do {} while (0)
#define FB3(slot) do {} while (0)
#endif
constexpr int TR = 32;         // pair rows per tile
constexpr int ATOM_CAP = 40;   // atoms staged per tile (two 18..20-atom molecules, or more smaller ones)

template <int F>
struct BwdLds {
  static constexpr int AS = F + 4;  // staged atom row stride (16-byte aligned rows)
  static constexpr int KC = F / 16, CB = F / 32;
  u32x4* dOr;    // [KC][3][64]
  u32x4* tf;     // [CB][2][3][64]  t fragments: hidden-unit block x k-step x piece
  u32x4* rbf;    // [2][2][3][64]
  // staging arrays, double buffered (buffer t & 1 serves tile t): written during the MFMA phase of tile t-1, read
  // only by the build of tile t
  static constexpr int STAGE_FLOATS = 2 * ATOM_CAP * AS + TR + 4 * TR + 4;  // xs, ds, tdd, desc (int4), flags
  float* stage0;
  __device__ float* xs(int b) const { return stage0 + b * STAGE_FLOATS; }                       // [ATOM_CAP][AS]
  __device__ float* ds(int b) const { return xs(b) + ATOM_CAP * AS; }                            // [ATOM_CAP][AS]
  __device__ float* tdd(int b) const { return ds(b) + ATOM_CAP * AS; }                           // [TR] distances
  // [TR] {offset of atom i, of atom j (LDS floats if staged, else atom index), C*flag0, C*flag1}
  __device__ int4* desc(int b) const { return reinterpret_cast<int4*>(tdd(b) + TR); }
  __device__ int* flag(int b) const { return reinterpret_cast<int*>(desc(b) + TR); }             // [0] = window fits
  __device__ explicit BwdLds(uint8_t* smem) {
    dOr = reinterpret_cast<u32x4*>(smem);
    tf = dOr + KC * 3 * 64;
    rbf = tf + CB * 2 * 3 * 64;
    stage0 = reinterpret_cast<float*>(rbf + 2 * 2 * 3 * 64);
  }
  static size_t bytes() { return (size_t)(KC * 3 + CB * 6 + 12) * 1024 + (size_t)2 * STAGE_FLOATS * 4; }
};

template <int NW, bool ROLE_A>
__device__ __forceinline__ void filter_bwd_body(const float* __restrict__ pair_d, const float* __restrict__ pair_c,
                                                const uint8_t* __restrict__ pair_flag,
                                                const int32_t* __restrict__ pair_i,
                                                const int32_t* __restrict__ pair_j, int P, int N,
                                                const GeosslFilterWeights& w, const GeosslFilterGradIn& g, int G,
                                                const float* __restrict__ offset, float coeff,
                                                const float* __restrict__ T, float* __restrict__ partial_w1,
                                                float* __restrict__ partial_b1, float* __restrict__ partial_w2,
                                                float* __restrict__ partial_b2, int Pstride) {
  constexpr int F = 32 * NW, NT = 128 * NW, KC = F / 16, CB = F / 32, AS = BwdLds<F>::AS, Q = F / 4;
  static_assert(TR * (F / 8) == NT, "one dOr fragment lane per thread");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  const BwdLds<F> L(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, kh = lane >> 5;
  constexpr bool roleA = ROLE_A;
  const int hs = roleA ? wave : wave - NW;  // hidden-unit slice [32 hs, 32 hs + 32)
  const int l = blockIdx.y;
  const float* __restrict__ x = g.x[l];
  const float* __restrict__ dagg = g.dagg[l];
  const size_t lbase = (size_t)l * Pstride;  // (layer stride of T: the capacity the launch was built for; P: real rows)
  const float* __restrict__ Tl = T + lbase * F;   // uniform base: the per-lane part stays a 32-bit offset
  const uint32_t tcol = 32 * hs + j;               // this lane's hidden unit

  // ---- role A: W2 slice as B fragments of dt = dO W2:  B[k = c = 16ks + 8kh + e][n = h] = W2[c][h]
  Frag3 bw2[roleA ? KC : 1];
  f32x16 accw1[2];             // role A: dW1 rows [32hs, +32) x gaussians [0, 64): lane = g, register = h
  f32x16 accw2[roleA ? 1 : CB];  // role B: dW2 rows c of this wave's channel block (register) x all h (lane), per h block
  float bsum1 = 0.0f, bsum2 = 0.0f;
  if constexpr (roleA) {
    const float* w2 = w.w2[l] + 32 * hs + j;
#pragma unroll
    for (int ks = 0; ks < KC; ++ks) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = w2[(size_t)(16 * ks + 8 * kh + e) * F];
      bw2[ks] = split8(v);
    }
#pragma unroll
    for (int gb = 0; gb < 2; ++gb)
#pragma unroll
      for (int r = 0; r < 16; ++r) accw1[gb][r] = 0.0f;
  } else {
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) accw2[cb][r] = 0.0f;
  }
  // role B: selection matrices of the matrix-pipe transposition, as B fragments: step q (channels 16q..16q+15 of the
  // wave's block), lane (n = j, half kh), element e:  1.0 (bf16 0x3F80) iff 16q + 8kh + e == j
  u32x4 ident[2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int w2i = 0; w2i < 4; ++w2i) {
      const int e0 = 16 * q + 8 * kh + 2 * w2i;
      ident[q][w2i] = (e0 == j ? 0x3F80u : 0u) | (e0 + 1 == j ? 0x3F800000u : 0u);
    }
  // fragment-lane roles of this thread in the tile build
  const int r_row = tid & 31, r_kh = (tid >> 5) & 1, r_ks = tid >> 6;         // dOr: row, k half, k-step (c)
  const int ntiles = (P + TR - 1) / TR;
  const int per = (ntiles + gridDim.x - 1) / gridDim.x;  // contiguous tile range per block (atom reuse in L2)
  const int t_begin = blockIdx.x * per, t_end = min(ntiles, t_begin + per);
  // Global requests run one tile ahead of their use (they fly during the MFMA phase of the previous tile): the atom
  // window and the row descriptors are fetched and staged by the role-B waves (which have the registers to spare),
  // the saved activations by every wave for its own hidden unit.  `alo` = first atom of a tile's window
  // (= pair_i[r0]: pair slots are lexicographic inside a molecule) is fetched two tiles ahead.
  constexpr int NTB = 64 * NW;                              // staging threads (role B)
  constexpr int NPRE = (ATOM_CAP * Q + NTB - 1) / NTB;      // float4 per staging thread and array
  const int stid = tid - NTB;                               // role B: 0 .. NTB-1
  f32x4 px[roleA ? 1 : NPRE], pdg[roleA ? 1 : NPRE];
  int ai = 0, aj = 0;
  float cval = 0.0f, dd = 0.0f;
  unsigned fl_raw = 0u;
  float tc[16];
  auto request_atoms = [&](int tt, int alo_t) {  // role B: window of x / dagg rows + the row descriptors of tile tt
    if constexpr (!roleA) {
      const int rr0 = tt * TR;
      // clamped addresses, no predication (a predicated load compiles to a branch with a full wait per element);
      // slots past the window are never read back
      const int nwin = min(ATOM_CAP, N - alo_t);
      const f32x4* x4 = reinterpret_cast<const f32x4*>(x + (size_t)alo_t * F);
      const f32x4* d4 = reinterpret_cast<const f32x4*>(dagg + (size_t)alo_t * F);
#pragma unroll
      for (int u = 0; u < NPRE; ++u) {
        const int i = min(stid + NTB * u, nwin * Q - 1);
        px[u] = x4[i];
        pdg[u] = d4[i];
      }
      if (stid < TR) {  // one pair row per lane of the first role-B wave
        const int q = min(rr0 + stid, P - 1);  // raw values only: nothing here waits for the loads
        ai = pair_i[q];
        aj = pair_j[q];
        fl_raw = pair_flag[q];
        cval = pair_c[q];
        dd = pair_d[q];
      }
    }
  };
  // saved hidden activation of this lane's hidden unit: role A in C layout (register r <-> row c_row(r)), role B in
  // B-fragment layout (k-step s, element e <-> row 16s + 8kh + e); rows past P are clamped (their dO is 0)
  auto request_t = [&](int tt) {
    if constexpr (roleA) {
      const int rr0 = tt * TR;
#pragma unroll
      for (int r = 0; r < 16; ++r) tc[r] = Tl[(uint32_t)min(rr0 + c_row(r, lane), P - 1) * (uint32_t)F + tcol];
    }
  };
  // role B: publish the window + descriptors held in registers (requested earlier) as tile tt's staging buffer
  auto publish = [&](int tt, int alo_t) {
    if constexpr (!roleA) {
      const int bsel = tt & 1, rr0 = tt * TR;
      const int nwin = min(ATOM_CAP, N - alo_t);
      if (wave == NW) {
        const int amax = wave_max_i32(lane < TR ? aj + 1 : 0);
        const bool staged0 = amax - alo_t <= ATOM_CAP;
        if (lane < TR) {
          const unsigned fl = rr0 + lane < P ? fl_raw : 0u;  // rows past P contribute nothing
          const float m0 = (fl & 1u) ? cval : 0.0f, m1 = (fl & 2u) ? cval : 0.0f;
          L.tdd(bsel)[lane] = dd;
          L.desc(bsel)[lane] = staged0 ? make_int4((ai - alo_t) * AS, (aj - alo_t) * AS, __float_as_int(m0), __float_as_int(m1))
                                       : make_int4(ai, aj, __float_as_int(m0), __float_as_int(m1));
        }
        if (lane == 0) L.flag(bsel)[0] = staged0 ? 1 : 0;
      }
      float* xs = L.xs(bsel);
      float* ds = L.ds(bsel);
#pragma unroll
      for (int u = 0; u < NPRE; ++u) {
        const int i = stid + NTB * u;
        if (i < nwin * Q) {
          const int a = i / Q, q4 = i - a * Q;
          *reinterpret_cast<f32x4*>(xs + a * AS + 4 * q4) = px[u];
          *reinterpret_cast<f32x4*>(ds + a * AS + 4 * q4) = pdg[u];
        }
      }
    }
  };
  // prologue: tile t_begin published, atoms of tile t_begin + 1 in flight, activations of tile t_begin in flight.
  // alo_a = first atom of the window of the tile whose atoms are held in registers, alo_b = of the tile after it
  // (= pair_i[r0]: pair slots are lexicographic inside a molecule; fetched one step ahead of their use).
  int alo_a = 0, alo_b = 0;
  if (t_begin < t_end) {
    alo_a = pair_i[t_begin * TR];
    request_atoms(t_begin, alo_a);
    request_t(t_begin);
    publish(t_begin, alo_a);
    if (t_begin + 1 < t_end) {
      alo_a = pair_i[(t_begin + 1) * TR];
      request_atoms(t_begin + 1, alo_a);
      if (t_begin + 2 < t_end) alo_b = pair_i[(t_begin + 2) * TR];
    }
  }
  for (int t = t_begin; t < t_end; ++t) {
    const int r0 = t * TR;
    const int bsel = t & 1;
    FB_MARK(0);
    lds_barrier();  // previous tile fully consumed; this tile's staging buffer published (LDS only: the requests for the
                    // tiles ahead stay in flight; measured neutral against __syncthreads here)
    FB_MARK(1);
    const bool staged = L.flag(bsel)[0] != 0;
    // ---- tile build: every thread one dOr fragment lane; role A publishes its tf lanes, role B its rbf lanes
    auto build = [&](const float* xb, const float* db, int stride) {
      {  // dOr: A[m = row][k = c = 16 r_ks + 8 r_kh + e]
        const int4 q = L.desc(bsel)[r_row];
        const float qm0 = __int_as_float(q.z), qm1 = __int_as_float(q.w);
        const int c0 = 16 * r_ks + 8 * r_kh;
        const float* di = db + (size_t)q.x * stride + c0;
        const float* dj = db + (size_t)q.y * stride + c0;
        const float* xi = xb + (size_t)q.x * stride + c0;
        const float* xj = xb + (size_t)q.y * stride + c0;
        float v[8];
#pragma unroll
        for (int h4 = 0; h4 < 2; ++h4) {
          const float4 a = *reinterpret_cast<const float4*>(di + 4 * h4), b = *reinterpret_cast<const float4*>(xj + 4 * h4);
          const float4 c = *reinterpret_cast<const float4*>(dj + 4 * h4), d = *reinterpret_cast<const float4*>(xi + 4 * h4);
          v[4 * h4 + 0] = qm0 * (a.x * b.x) + qm1 * (c.x * d.x);
          v[4 * h4 + 1] = qm0 * (a.y * b.y) + qm1 * (c.y * d.y);
          v[4 * h4 + 2] = qm0 * (a.z * b.z) + qm1 * (c.z * d.z);
          v[4 * h4 + 3] = qm0 * (a.w * b.w) + qm1 * (c.w * d.w);
        }
        const Frag3 f = split8(v);
        u32x4* dst = L.dOr + (size_t)(r_ks * 3) * 64 + (r_row + 32 * r_kh);
        dst[0] = f.h;
        dst[64] = f.m;
        dst[128] = f.l;
      }
    };
    if (staged) build(L.xs(bsel), L.ds(bsel), 1);  // descriptors hold LDS float offsets
    else build(x, dagg, F);            // a run of tiny molecules: operands straight from global memory
    if constexpr (roleA) {
      // t slice of this wave's hidden units as B fragments of dW2's contraction over pair rows: the C layout held in
      // tc (lane = h, register r <-> row c_row(r)) is the fragment layout with k-step s <-> registers 8s..8s+7
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = tc[8 * s2 + e];
        const Frag3 f = split8(v);
        u32x4* dst = L.tf + (size_t)((hs * 2 + s2) * 3) * 64 + lane;
        dst[0] = f.h;
        dst[64] = f.m;
        dst[128] = f.l;
      }
    } else {
      for (int it = tid - NT / 2; it < 2 * 2 * 64; it += NT / 2) {  // rbf: B[k = row = 16ks + kperm(e, kh)][n = g]
        const int ln = it & 63, ks = (it >> 6) & 1, gb = it >> 7;
        const int gg = 32 * gb + (ln & 31);
        const float off = gg < G ? offset[gg] : 0.0f;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float diff = L.tdd(bsel)[16 * ks + kperm(e, ln >> 5)] - off;
          v[e] = gg < G ? exp_neg(coeff * (diff * diff)) : 0.0f;
        }
        const Frag3 f = split8(v);
        u32x4* dst = L.rbf + (size_t)((gb * 2 + ks) * 3) * 64 + ln;
        dst[0] = f.h;
        dst[64] = f.m;
        dst[128] = f.l;
      }
    }
    float tcur[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) tcur[r] = tc[r];
    FB_MARK(2);
    lds_barrier();
    FB_MARK(3);
    // While this tile is multiplied: publish the next tile's staging buffer (its atoms were requested one tile ago
    // and have arrived), request the atoms of the tile after it and the next tile's saved activations.
    if (t + 1 < t_end) {
#ifdef FB_TIMING
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (blockIdx.x == 3 && blockIdx.y == 0 && lane == 0 && (wave == 0 || wave == NW) && t - t_begin < 64)
        fb_dbg2[(wave == 0 ? 0 : 1) * 64 + (t - t_begin)] = clock64();
#endif
      publish(t + 1, alo_a);
      FB_MARK(7);
      if (t + 2 < t_end) {
        alo_a = alo_b;
        request_atoms(t + 2, alo_a);
        if (t + 3 < t_end) alo_b = pair_i[(t + 3) * TR];
      }
      request_t(t + 1);
    }
    FB_MARK(4);
    if constexpr (roleA) {
      // dt = dO W2 for this wave's hidden units (back-to-back MFMAs on one accumulator forward SrcC without a stall)
      f32x16 acc0, acc1;  // small-weight and large-weight piece products apart: better conditioned, and two
                          // independent MFMA chains
#pragma unroll
      for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
      {
        Frag3 a0, an;  // fragments of the next k-step are requested before this step's MFMAs issue
        {
          const u32x4* s0 = L.dOr + lane;
          a0.h = s0[0]; a0.m = s0[64]; a0.l = s0[128];
        }
#pragma unroll
        for (int ks = 0; ks < KC; ++ks) {
          if (ks + 1 < KC) {
            const u32x4* s0 = L.dOr + (size_t)((ks + 1) * 3) * 64 + lane;
            an.h = s0[0]; an.m = s0[64]; an.l = s0[128];
          }
          __builtin_amdgcn_sched_barrier(0);
          mma6x2(acc1, acc0, a0, bw2[ks]);
          __builtin_amdgcn_sched_barrier(0);
          if (ks + 1 < KC) a0 = an;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) acc0[r] += acc1[r];
      // dU = dt * ssp'(pre) (C layout: lane = hidden unit, register = pair row); registers 0..7 / 8..15 are the
      // elements of k-steps 0 / 1 of the contraction over pair rows
      Frag3 du[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = acc0[8 * s + e] * dssp_from_out(tcur[8 * s + e]);
          bsum1 += v[e];
        }
        du[s] = split8(v);
      }
      FB_MARK(6);
      // dW1[h][g] += sum_rows dU[row][h] * rbf(d_row)[g]
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        Frag3 b0, b1;
        const u32x4* s0 = L.rbf + (size_t)(s * 3) * 64 + lane;
        b0.h = s0[0]; b0.m = s0[64]; b0.l = s0[128];
        b1.h = s0[384]; b1.m = s0[448]; b1.l = s0[512];
        accw1[0] = mfma_bf16(du[s].l, b0.h, accw1[0]);
        accw1[1] = mfma_bf16(du[s].l, b1.h, accw1[1]);
        accw1[0] = mfma_bf16(du[s].h, b0.l, accw1[0]);
        accw1[1] = mfma_bf16(du[s].h, b1.l, accw1[1]);
        accw1[0] = mfma_bf16(du[s].m, b0.m, accw1[0]);
        accw1[1] = mfma_bf16(du[s].m, b1.m, accw1[1]);
        accw1[0] = mfma_bf16(du[s].m, b0.h, accw1[0]);
        accw1[1] = mfma_bf16(du[s].m, b1.h, accw1[1]);
        accw1[0] = mfma_bf16(du[s].h, b0.m, accw1[0]);
        accw1[1] = mfma_bf16(du[s].h, b1.m, accw1[1]);
        accw1[0] = mfma_bf16(du[s].h, b0.h, accw1[0]);
        accw1[1] = mfma_bf16(du[s].h, b1.h, accw1[1]);
      }
    } else {
      // Role B wave w owns filter output channels c in [32w, 32w+32).  Its dO^T fragments (lane = c, 8 pair rows) come
      // from the dOr fragments through the matrix pipe: D = dOr_piece * I (I = 16 x 32 selection of the channel block)
      // lands in C layout - lane = c, register = pair row in kperm order - i.e. in fragment order, and every value is
      // an exact bf16 number (one piece times 1), so packing is exact.  No second evaluation of dO in the other
      // orientation, no LDS traffic for it.
      f32x16 tp[3];
#pragma unroll
      for (int pc = 0; pc < 3; ++pc)
#pragma unroll
        for (int r = 0; r < 16; ++r) tp[pc][r] = 0.0f;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const u32x4* s0 = L.dOr + (size_t)((2 * hs + q) * 3) * 64 + lane;
        tp[0] = mfma_bf16(s0[0], ident[q], tp[0]);
        tp[1] = mfma_bf16(s0[64], ident[q], tp[1]);
        tp[2] = mfma_bf16(s0[128], ident[q], tp[2]);
      }
      FB_MARK(6);
      Frag3 da[2];  // A fragments of dW2 = dO^T t: k-step s <-> registers 8s..8s+7
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          da[s2].h[q] = pk_bf16(tp[0][8 * s2 + 2 * q], tp[0][8 * s2 + 2 * q + 1]);
          da[s2].m[q] = pk_bf16(tp[1][8 * s2 + 2 * q], tp[1][8 * s2 + 2 * q + 1]);
          da[s2].l[q] = pk_bf16(tp[2][8 * s2 + 2 * q], tp[2][8 * s2 + 2 * q + 1]);
        }
#pragma unroll
      for (int r = 0; r < 16; ++r) bsum2 += (tp[0][r] + tp[1][r]) + tp[2][r];  // db2: rows of this half-wave
      // dW2[c][h] += sum_rows dO[row][c] * t[row][h], all four 32-wide blocks of h (t fragments published by role A)
      constexpr int CP = CB >= 2 ? 2 : 1;
#pragma unroll
      for (int hb = 0; hb < CB; hb += CP) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          Frag3 tb[CP];
#pragma unroll
          for (int u = 0; u < CP; ++u) {
            const u32x4* s0 = L.tf + (size_t)(((hb + u) * 2 + s2) * 3) * 64 + lane;
            tb[u].h = s0[0]; tb[u].m = s0[64]; tb[u].l = s0[128];
          }
#pragma unroll
          for (int u = 0; u < CP; ++u) accw2[hb + u] = mfma_bf16(da[s2].l, tb[u].h, accw2[hb + u]);
#pragma unroll
          for (int u = 0; u < CP; ++u) accw2[hb + u] = mfma_bf16(da[s2].h, tb[u].l, accw2[hb + u]);
#pragma unroll
          for (int u = 0; u < CP; ++u) accw2[hb + u] = mfma_bf16(da[s2].m, tb[u].m, accw2[hb + u]);
#pragma unroll
          for (int u = 0; u < CP; ++u) accw2[hb + u] = mfma_bf16(da[s2].m, tb[u].h, accw2[hb + u]);
#pragma unroll
          for (int u = 0; u < CP; ++u) accw2[hb + u] = mfma_bf16(da[s2].h, tb[u].m, accw2[hb + u]);
#pragma unroll
          for (int u = 0; u < CP; ++u) accw2[hb + u] = mfma_bf16(da[s2].h, tb[u].h, accw2[hb + u]);
        }
      }
    }
    FB_MARK(5);
  }
  // ---- one partial per block
  const size_t pb = (size_t)l * gridDim.x + blockIdx.x;
  if constexpr (roleA) {
    float* Pw = partial_w1 + pb * F * G;
#pragma unroll
    for (int gb = 0; gb < 2; ++gb) {
      const int gg = 32 * gb + j;
      if (gg < G) {
#pragma unroll
        for (int r = 0; r < 16; ++r) Pw[(size_t)(32 * hs + c_row(r, lane)) * G + gg] = accw1[gb][r];
      }
    }
    const float s = bsum1 + __shfl_xor(bsum1, 32, 64);
    if (kh == 0) partial_b1[pb * F + 32 * hs + j] = s;
  } else {
    float* Pw = partial_w2 + pb * F * F;
#pragma unroll
    for (int hb = 0; hb < CB; ++hb)
#pragma unroll
      for (int r = 0; r < 16; ++r) Pw[(size_t)(32 * hs + c_row(r, lane)) * F + 32 * hb + j] = accw2[hb][r];
    // db2[c]: each half-wave summed the pair rows its registers hold
    const float sb2 = bsum2 + __shfl_xor(bsum2, 32, 64);
    if (kh == 0) partial_b2[pb * F + 32 * hs + j] = sb2;
  }
}

// The two roles run separate instantiations of the body (their register sets differ: W2 fragments + dW1
// accumulators against dW2 accumulators); the branch is wave-uniform and both sides execute the same barriers.
template <int NW>
__global__ __launch_bounds__(128 * NW) void k_filter_bwd(const float* __restrict__ pair_d,
                                                         const float* __restrict__ pair_c,
                                                         const uint8_t* __restrict__ pair_flag,
                                                         const int32_t* __restrict__ pair_i,
                                                         const int32_t* __restrict__ pair_j, int P, int N,
                                                         GeosslFilterWeights w, GeosslFilterGradIn g, int G,
                                                         const float* __restrict__ offset, float coeff,
                                                         const float* __restrict__ T,
                                                         float* __restrict__ partial_w1,
                                                         float* __restrict__ partial_b1,
                                                         float* __restrict__ partial_w2,
                                                         float* __restrict__ partial_b2,
                                                         const int32_t* __restrict__ dyn_P,
                                                         const int32_t* __restrict__ dyn_N) {
  const int Pstride = P;
  P = dyn_count(P, dyn_P);
  N = dyn_count(N, dyn_N);
  if ((int)(threadIdx.x >> 6) < NW)
    filter_bwd_body<NW, true>(pair_d, pair_c, pair_flag, pair_i, pair_j, P, N, w, g, G, offset, coeff, T, partial_w1,
                              partial_b1, partial_w2, partial_b2, Pstride);
  else
    filter_bwd_body<NW, false>(pair_d, pair_c, pair_flag, pair_i, pair_j, P, N, w, g, G, offset, coeff, T, partial_w1,
                               partial_b1, partial_w2, partial_b2, Pstride);
}

// =====================================================================================================================
// The same kernel on TWO fp16 pieces per operand (split.h: 3 MFMAs per product instead of 6, the selection-matrix
// transposition on two pieces instead of three), the default.  The three-bf16-piece form above stays selectable with
// GEOSSL_FILTER_BWD_BF16X3 for A/B runs.
#ifdef FB_TIMING
#define FBH_MARK(slot) FB_MARK(slot)
#else
#define FBH_MARK(slot) do {} while (0)
#endif
// TR: pair rows per tile, 32 or 64.  A 64-row tile is two 32-row M blocks (SUB = 2) with ONE build phase, ONE barrier pair
// and ONE set of per-tile bookkeeping (descriptors, window decision, operand exponents); every fragment array holds the
// 32-row layout once per M block.
template <int F, int TR>
struct BwdLdsH {
  static constexpr int AS = F + 4;  // staged atom row stride (16-byte aligned rows)
  static constexpr int KC = F / 16, CB = F / 32, SUB = TR / 32;
  static constexpr int CAP = TR == 64 ? FB_CAP64 : ATOM_CAP;  // atoms staged per window
  static constexpr int DOR_WORDS = KC * 2 * 64, TF_WORDS = CB * 2 * 2 * 64, RBF_WORDS = RBF_TILE_WORDS;  // per M block
  u32x4* dOr;    // [SUB][KC][2][64]
  u32x4* tf;     // [SUB][CB][2][2][64]  t fragments: hidden-unit block x k-step x piece
  u32x4* rbf;    // [SUB][2][2][2][64]
  int* et;       // [CB] running exponent of each role-A wave's t fragments; [CB] = scratch word of the unstaged path
  float* offs;   // [64] Gaussian centres, zero padded (the role-A waves rebuild the hidden row from them when T is not saved)
  // The atom window, ONE buffer: written (when a tile gets a fresh window) during the MFMA phase of tile t-1, i.e. after
  // the barrier that ends the build of tile t-1 - the last reader of the window it replaces - and read only by the build
  // of tile t, after the barrier that opens it.
  float* xs;     // [CAP][AS]
  float* ds;     // [CAP][AS]
  float* wmax;   // [CB][2] max |x|, max |dagg| of the window
  // the small per-tile arrays, double buffered (buffer t & 1 serves tile t)
  static constexpr int TILE_FLOATS = TR + 4 * TR + 4;  // tdd, desc (int4), flags
  float* tile0;
  __device__ float* tdd(int b) const { return tile0 + b * TILE_FLOATS; }                          // [TR] distances
  // [TR] {offset of atom i, of atom j (LDS floats if staged, else atom index), C*flag0, C*flag1}
  __device__ int4* desc(int b) const { return reinterpret_cast<int4*>(tdd(b) + TR); }
  __device__ int* flag(int b) const { return reinterpret_cast<int*>(desc(b) + TR); }             // [0] = window fits
  __device__ explicit BwdLdsH(uint8_t* smem) {
    dOr = reinterpret_cast<u32x4*>(smem);
    tf = dOr + SUB * DOR_WORDS;
    rbf = tf + SUB * TF_WORDS;
    et = reinterpret_cast<int*>(rbf + SUB * RBF_WORDS);
    offs = reinterpret_cast<float*>(et + 8);
    xs = offs + 64;
    ds = xs + CAP * AS;
    wmax = ds + CAP * AS;
    tile0 = wmax + 8;
  }
  static constexpr size_t bytes() {
    return (size_t)SUB * (DOR_WORDS + TF_WORDS + RBF_WORDS) * 16 + 32 + 256 + (size_t)(2 * CAP * AS + 8 + 2 * TILE_FLOATS) * 4;
  }
};

// RECOMP: T == nullptr - the hidden row t = ssp(W1 rbf(d) + b1) is not read back from HBM (the forward did not store it:
// 0.96 GB written and read again per step at the bench size) but rebuilt by the role-A waves from the row's distance:
// one K = 64 product per tile against the wave's W1 slice (held as B fragments), the Gaussians as A fragments in
// registers - the forward kernel's arithmetic with the operand roles swapped (rows on M, hidden units on N), which
// leaves t in the C layout the rest of the tile wants (lane = hidden unit, register = pair row).
//
// img != nullptr (a block-uniform branch of the form that reads the saved hidden rows; one kernel either way): the Gaussian
// fragments are not built here - the same words for every layer of the launch - but copied from the per-step image
// (rbf_frag.h, k_rbf_fragments): a role-B lane requests the two 16-byte words of its item of the NEXT tile at the start
// of a tile's MFMA phase and stores them to L.rbf where the build stores them otherwise.
template <int NW, bool ROLE_A, bool RECOMP, int TR>
__device__ __forceinline__ void filter_bwd_body_h(const float* __restrict__ pair_d, const float* __restrict__ pair_c,
                                                const uint8_t* __restrict__ pair_flag,
                                                const int32_t* __restrict__ pair_i,
                                                const int32_t* __restrict__ pair_j, int P, int N,
                                                const GeosslFilterWeights& w, const GeosslFilterGradIn& g, int G,
                                                const float* __restrict__ offset, float coeff,
                                                const float* __restrict__ T, float* __restrict__ partial_w1,
                                                float* __restrict__ partial_b1, float* __restrict__ partial_w2,
                                                float* __restrict__ partial_b2, int Pstride,
                                                const u32x4* __restrict__ img) {
  using Lds = BwdLdsH<32 * NW, TR>;
  constexpr int F = 32 * NW, NT = 128 * NW, KC = F / 16, CB = F / 32, AS = Lds::AS, Q = F / 4, SUB = Lds::SUB, CAP = Lds::CAP;
  static_assert(TR == 32 || TR == 64, "one or two 32-row M blocks per tile");
  static_assert(Lds::bytes() <= 160 * 1024, "fragments of all M blocks + one atom window in the LDS of a CU");
  static_assert(32 * (F / 8) == NT, "one dOr fragment lane per thread and M block");
  static_assert(RBF_TILE_ROWS == 32 && RBF_TILE_ITEMS % (64 * NW) == 0, "whole items per role-B lane, one image tile per M block");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  const Lds L(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, kh = lane >> 5;
  constexpr bool roleA = ROLE_A;
  const int hs = roleA ? wave : wave - NW;  // hidden-unit slice [32 hs, 32 hs + 32)
  const int l = blockIdx.y;
  const float* __restrict__ x = g.x[l];
  const float* __restrict__ dagg = g.dagg[l];
  const size_t lbase = (size_t)l * Pstride;  // (layer stride of T: the capacity the launch was built for; P: real rows)
  const float* __restrict__ Tl = T + lbase * F;   // uniform base: the per-lane part stays a 32-bit offset
  const uint32_t tcol = 32 * hs + j;               // this lane's hidden unit

  // ---- role A: W2 slice as B fragments of dt = dO W2:  B[k = c = 16ks + 8kh + e][n = h] = W2[c][h]
  Frag2 bw2[roleA ? KC : 1];
  // role A, RECOMP: W1 slice as B fragments of u = rbf W1^T:  B[k = g = 16ks + 8kh + e][n = h] = W1[h][g], scaled to 2^14
  Frag2 bw1[(roleA && RECOMP) ? 4 : 1];
  float inv1 = 0.0f, b1v = 0.0f;
  if constexpr (RECOMP) {
    for (int i = tid; i < 64; i += NT) L.offs[i] = i < G ? offset[i] : 0.0f;  // (visible after the first tile barrier)
    if constexpr (roleA) {
      const float* w1 = w.w1[l] + (size_t)(32 * hs + j) * G;
      float raw[4][8];
      float wm = 0.0f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int gg = 16 * ks + 8 * kh + e;
          raw[ks][e] = gg < G ? w1[min(gg, G - 1)] : 0.0f;
          wm = fmaxf(wm, fabsf(raw[ks][e]));
        }
      wm = wave_max(wm);
      int e1;
      const float s1 = pow2_scale_to_2p14(wm, e1);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        float v8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v8[e] = raw[ks][e] * s1;
        bw1[ks] = split8h(v8);
      }
      inv1 = 1.0f / (s1 * 16384.0f);  // a power of two: exact
      b1v = w.b1[l][32 * hs + j];
    }
  }
  int e2 = 0, eL = 0;          // role A: exponents of max |W2 slice| and of its largest column L1 norm (bounds dt)
  f32x16 accw1[2];             // role A: dW1 rows [32hs, +32) x gaussians [0, 64): lane = g, register = h
  f32x16 accw2[roleA ? 1 : CB];  // role B: dW2 rows c of this wave's channel block (register) x all h (lane), per h block
  float bsum1 = 0.0f, bsum2 = 0.0f;
  if constexpr (roleA) {
    const float* w2 = w.w2[l] + 32 * hs + j;
    float wm = 0.0f, l1 = 0.0f;
#pragma unroll
    for (int ks = 0; ks < KC; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float a = fabsf(w2[(size_t)(16 * ks + 8 * kh + e) * F]);
        wm = fmaxf(wm, a);
        l1 += a;
      }
    l1 += __shfl_xor(l1, 32, 64);  // the two halves of a lane pair hold the two halves of column h
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      wm = fmaxf(wm, __shfl_xor(wm, o, 64));
      l1 = fmaxf(l1, __shfl_xor(l1, o, 64));
    }
    const float s2 = pow2_scale_to_2p14(wm, e2);
    eL = max(__builtin_amdgcn_frexp_expf(l1), -12);  // (a floor: 2^(14 - EO - eL) must stay finite for EO >= -100)
#pragma unroll
    for (int ks = 0; ks < KC; ++ks) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = w2[(size_t)(16 * ks + 8 * kh + e) * F] * s2;
      bw2[ks] = split8h(v);
    }
#pragma unroll
    for (int gb = 0; gb < 2; ++gb)
#pragma unroll
      for (int r = 0; r < 16; ++r) accw1[gb][r] = 0.0f;
  } else {
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) accw2[cb][r] = 0.0f;
  }
  // role B: selection matrices of the matrix-pipe transposition, as B fragments: step q (channels 16q..16q+15 of the
  // wave's block), lane (n = j, half kh), element e:  1.0 (fp16 0x3C00) iff 16q + 8kh + e == j
  u32x4 ident[2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int w2i = 0; w2i < 4; ++w2i) {
      const int e0 = 16 * q + 8 * kh + 2 * w2i;
      ident[q][w2i] = (e0 == j ? 0x3C00u : 0u) | (e0 + 1 == j ? 0x3C000000u : 0u);
    }
  // fragment-lane roles of this thread in the tile build
  const int r_row = tid & 31, r_kh = (tid >> 5) & 1, r_ks = tid >> 6;         // dOr: row, k half, k-step (c)
  const int ntiles = (P + TR - 1) / TR;
  const int per = (ntiles + gridDim.x - 1) / gridDim.x;  // contiguous tile range per block (atom reuse in L2)
  const int t_begin = blockIdx.x * per, t_end = min(ntiles, t_begin + per);
  // Global requests run one tile ahead of their use (they fly during the MFMA phase of the previous tile): the atom
  // window and the row descriptors are fetched and staged by the role-B waves (which have the registers to spare),
  // the saved activations by every wave for its own hidden unit.  `alo` = first atom of a tile's window
  // (= pair_i[r0]: pair slots are lexicographic inside a molecule) is fetched two tiles ahead.
  constexpr int NTB = 64 * NW;                              // staging threads (role B)
  constexpr int NPRE = (CAP * Q + NTB - 1) / NTB;           // float4 per staging thread and array
  const int stid = tid - NTB;                               // role B: 0 .. NTB-1
  f32x4 px[roleA ? 1 : NPRE], pdg[roleA ? 1 : NPRE];
  int ai = 0, aj = 0;
  float cval = 0.0f, dd = 0.0f;
  unsigned fl_raw = 0u;
  float tc[SUB][16];
  // The staged window is STICKY: it stays as long as the next tile's atoms still fall inside it (pair slots are
  // lexicographic, so a window that starts at some atom of a molecule serves the rest of that molecule and the next one) -
  // about nine tiles in ten of 18-atom molecules neither fetch nor store a window.  Every wave takes the decision itself
  // from the same values: the second atoms of the tile's rows (ajn, fetched one tile before the decision; a lane per row of
  // a 64-row tile, a lane pair per row of a 32-row one) and the state walo = the window's first atom.  The decision of a
  // tile is taken when its requests are issued and kept (dec_*) until the tile is published one iteration later.
  int ajn = 0;
  int walo = 0;
  bool whave = false;
  bool dec_staged = false, dec_fresh = false;
  int dec_alo = 0;
  auto decide = [&](int alo_t) {
    const int amax = wave_max_i32(ajn + 1);
    const bool fits = whave && alo_t >= walo && amax - walo <= CAP;
    dec_fresh = !fits && amax - alo_t <= CAP;
    if (dec_fresh) {
      walo = alo_t;
      whave = true;
    }
    dec_staged = fits || dec_fresh;
    dec_alo = walo;
  };
  auto request_rows = [&](int tt) { ajn = pair_j[min(tt * TR + (lane & (TR - 1)), P - 1)]; };
  auto request_atoms = [&](int tt, int alo_t) {  // role B: window of x / dagg rows of tile tt (if it gets a new one); role A: its row descriptors
    if constexpr (!roleA) {
      if (!dec_fresh) return;
      // clamped addresses, no predication (a predicated load compiles to a branch with a full wait per element);
      // slots past the window are never read back
      const int nwin = min(CAP, N - alo_t);
      const f32x4* x4 = reinterpret_cast<const f32x4*>(x + (size_t)alo_t * F);
      const f32x4* d4 = reinterpret_cast<const f32x4*>(dagg + (size_t)alo_t * F);
#pragma unroll
      for (int u = 0; u < NPRE; ++u) {
        const int i = min(stid + NTB * u, nwin * Q - 1);
        px[u] = x4[i];
        pdg[u] = d4[i];
      }
    } else {
      if (tid < TR) {  // the row descriptors: one pair row per lane of the first role-A wave (role B is the longer path)
        const int q = min(tt * TR + tid, P - 1);  // raw values only: nothing here waits for the loads
        ai = pair_i[q];
        aj = pair_j[q];
        fl_raw = pair_flag[q];
        cval = pair_c[q];
        dd = pair_d[q];
      }
    }
  };
  // saved hidden activation of this lane's hidden unit: role A in C layout (register r <-> row c_row(r)), role B in
  // B-fragment layout (k-step s, element e <-> row 16s + 8kh + e); rows past P are clamped (their dO is 0)
  float dreq[SUB];  // RECOMP: distance of this lane's pair row of the tile whose hidden rows are rebuilt next, per M block
#pragma unroll
  for (int sb = 0; sb < SUB; ++sb) dreq[sb] = 0.0f;
  auto request_t = [&](int tt, int sb) {  // M block sb of tile tt
    if constexpr (roleA && !RECOMP) {
      const int rr0 = tt * TR + 32 * sb;
      if (rr0 + 32 <= P) {
        // a whole M block: row c_row(r) = (r & 3) + 8 (r >> 2) + 4 kh - register r is a constant number of rows behind the
        // lane's first row, so the sixteen requests share four bases and carry their offsets as immediates (as sixteen
        // clamped per-lane addresses they were ~50 vector instructions of a role-A wave's ~400 per tile)
        const float* tb = Tl + (size_t)(rr0 + 4 * kh) * F + tcol;
#pragma unroll
        for (int r = 0; r < 16; ++r) tc[sb][r] = tb[((r & 3) + 8 * (r >> 2)) * F];
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) tc[sb][r] = Tl[(uint32_t)min(rr0 + c_row(r, lane), P - 1) * (uint32_t)F + tcol];
      }
    }
    if constexpr (roleA && RECOMP) dreq[sb] = pair_d[min(tt * TR + 32 * sb + j, P - 1)];
  };
  // RECOMP: the hidden rows of a tile for this wave's units, u = rbf(d) W1^T + b1, t = ssp(u) (schnet.py:141-145,205-207),
  // into tc.  A operand = the Gaussians of row j (8 per k-step and half) built in registers - every role-A wave its own
  // copy, one per SIMD.  Runs at the END of the wave's MFMA phase for the NEXT tile: role A finishes that phase first
  // and would wait at the barrier (in-kernel marks: 2 k of a tile's 8.7 k cycles); inside the build phase, where the
  // hidden rows are consumed, it sat on the tile's critical path (0.85 -> 0.99 ms per launch).
  auto rebuild_t = [&](int sb) {
    if constexpr (roleA && RECOMP) {
      const float dj = dreq[sb];
      f32x16 au;
#pragma unroll
      for (int r = 0; r < 16; ++r) au[r] = 0.0f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const f32x4 o0 = *reinterpret_cast<const f32x4*>(L.offs + 16 * ks + 8 * kh);
        const f32x4 o1 = *reinterpret_cast<const f32x4*>(L.offs + 16 * ks + 8 * kh + 4);
        const float o[8] = {o0[0], o0[1], o0[2], o0[3], o1[0], o1[1], o1[2], o1[3]};
        float g8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float diff = dj - o[e];
          g8[e] = exp_neg(coeff * (diff * diff));  // (padded centres meet zero weights)
        }
        const Frag2 a = split8h_scaled(g8, 16384.0f);
        au = mfma_f16(a.l, bw1[ks].h, au);
        au = mfma_f16(a.h, bw1[ks].l, au);
        au = mfma_f16(a.h, bw1[ks].h, au);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) tc[sb][r] = ssp(fmaf(au[r], inv1, b1v));
    }
  };
  // IMG, role B: the words of this lane's items of tile tt's Gaussian fragments, from the image.  The image keeps its
  // 32-row tiles: M block sb of tile tt is image tile SUB tt + sb; the last image tile stands in for an M block that
  // lies past the capacity altogether (all its rows are past P: dO exactly zero, the words only have to be finite).
  constexpr bool IMG = !RECOMP;  // (the form that rebuilds the hidden rows keeps its own Gaussians)
  const bool use_img = IMG && img != nullptr;
  constexpr int NIT = (IMG && !ROLE_A) ? RBF_TILE_ITEMS / (64 * NW) : 1;
  const int nimg = (Pstride + RBF_TILE_ROWS - 1) / RBF_TILE_ROWS;
  u32x4 gfh[SUB][NIT], gfl[SUB][NIT];
#pragma unroll
  for (int sb = 0; sb < SUB; ++sb)
#pragma unroll
    for (int u = 0; u < NIT; ++u) gfh[sb][u] = gfl[sb][u] = u32x4{0u, 0u, 0u, 0u};
  auto request_rbf = [&](int tt) {
    if constexpr (IMG && !roleA) {
      if (!use_img) return;
#pragma unroll
      for (int sb = 0; sb < SUB; ++sb) {
        const u32x4* __restrict__ src = img + (size_t)min(SUB * tt + sb, nimg - 1) * RBF_TILE_WORDS;  // (uniform base, 32-bit lane offsets)
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
          const int w = rbf_item_word(64 * hs + lane + 64 * NW * u);
          gfh[sb][u] = src[w];
          gfl[sb][u] = src[w + 64];
        }
      }
    }
  };
  // publish what was requested earlier as tile tt's staging buffer: role B the atom window (and its largest magnitudes),
  // the first role-A wave the row descriptors (role B is the longer path of the phase)
  auto publish = [&](int tt) {
    const bool staged0 = dec_staged, fresh = dec_fresh;
    const int alo_t = dec_alo;  // descriptors are relative to the window in use
    if constexpr (roleA) {
      const int bsel = tt & 1, rr0 = tt * TR;
      if (wave == 0) {
        if (lane < TR) {
          const unsigned fl = rr0 + lane < P ? fl_raw : 0u;  // rows past P contribute nothing
          const float m0 = (fl & 1u) ? cval : 0.0f, m1 = (fl & 2u) ? cval : 0.0f;
          L.tdd(bsel)[lane] = dd;
          L.desc(bsel)[lane] = staged0 ? make_int4((ai - alo_t) * AS, (aj - alo_t) * AS, __float_as_int(m0), __float_as_int(m1))
                                       : make_int4(ai, aj, __float_as_int(m0), __float_as_int(m1));
        }
        if (lane == 0) {
          L.flag(bsel)[0] = staged0 ? 1 : 0;
          L.et[CB] = 0;
        }
      }
    } else if (fresh) {
      // (the one window buffer: this runs behind the barrier that ended the build of the previous tile, the last reader
      // of the window it overwrites, and in front of the barrier that opens the build of tile tt)
      const int nwin = min(CAP, N - alo_t);
      FB3(0);
      FB3(1);
      float* xs = L.xs;
      float* ds = L.ds;
      float mx = 0.0f, md = 0.0f;  // largest |x|, |dagg| of the window (clamped duplicates are window values too)
#pragma unroll
      for (int u = 0; u < NPRE; ++u) {
        const int i = stid + NTB * u;
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(px[u][0]), fabsf(px[u][1]))), fmaxf(fabsf(px[u][2]), fabsf(px[u][3])));
        md = fmaxf(fmaxf(md, fmaxf(fabsf(pdg[u][0]), fabsf(pdg[u][1]))), fmaxf(fabsf(pdg[u][2]), fabsf(pdg[u][3])));
        if (i < nwin * Q) {
          const int a = i / Q, q4 = i - a * Q;
          *reinterpret_cast<f32x4*>(xs + a * AS + 4 * q4) = px[u];
          *reinterpret_cast<f32x4*>(ds + a * AS + 4 * q4) = pdg[u];
        }
      }
      FB3(2);
      mx = wave_max(mx);
      md = wave_max(md);
      if (lane == 0) {
        L.wmax[2 * (wave - NW)] = mx;
        L.wmax[2 * (wave - NW) + 1] = md;
      }
      FB3(3);
    }
  };
  // prologue: tile t_begin published, atoms of tile t_begin + 1 in flight, activations of tile t_begin in flight.
  // alo_a = first atom of the window of the tile whose atoms are held in registers, alo_b = of the tile after it
  // (= pair_i[r0]: pair slots are lexicographic inside a molecule; fetched one step ahead of their use).
  int alo_a = 0, alo_b = 0;
  // Operand scales (powers of two, split.h).  EO: running exponent of the block's dO values - 2^EO exceeds every |dO| met
  // so far (bound: twice the product of the staged window's largest |x| and |dagg|); when a tile raises it, the weight
  // gradient accumulators (which hold sums scaled by it) are scaled down by the same power of two.  ET: the same for the
  // saved activations of one role-A wave's hidden units (published next to its fragments; the role-B waves follow it).
  int EO = -126, ET = -126;
  int ETs[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) ETs[cb] = -126;
  if (t_begin < t_end) {
    alo_a = pair_i[t_begin * TR];
    request_rows(t_begin);
    decide(alo_a);
    request_rbf(t_begin);
    request_atoms(t_begin, alo_a);
#pragma unroll
    for (int sb = 0; sb < SUB; ++sb) request_t(t_begin, sb);
    if constexpr (RECOMP) {
      lds_barrier();  // the Gaussian centres in LDS (block-uniform branch: every wave of the block takes it)
#pragma unroll
      for (int sb = 0; sb < SUB; ++sb) rebuild_t(sb);
    }
    publish(t_begin);
    if (t_begin + 1 < t_end) {
      alo_a = pair_i[(t_begin + 1) * TR];
      request_rows(t_begin + 1);
      decide(alo_a);
      request_atoms(t_begin + 1, alo_a);
      if (t_begin + 2 < t_end) {
        alo_b = pair_i[(t_begin + 2) * TR];
        request_rows(t_begin + 2);
      }
    }
  }
  for (int t = t_begin; t < t_end; ++t) {
    const int r0 = t * TR;
    const int bsel = t & 1;
    FBH_MARK(0);
#ifdef FBH_HALF_BARRIERS   // (timing experiment only, results are wrong: one barrier pair per TWO tiles - what a 64-row tile would save in barriers)
    if (!(t & 1))
#endif
    lds_barrier();  // previous tile fully consumed; this tile's staging buffer published (LDS only: the requests for the
                    // tiles ahead stay in flight; measured neutral against __syncthreads here)
    FBH_MARK(1);
    const bool staged = L.flag(bsel)[0] != 0;
    // ---- tile build: every thread one dOr fragment lane per M block; role A publishes its tf lanes, role B its rbf lanes
    float v[SUB][8];
    auto build = [&](const float* xb, const float* db, int stride) {
#pragma unroll
      for (int sb = 0; sb < SUB; ++sb) {  // dOr: A[m = row][k = c = 16 r_ks + 8 r_kh + e]
        const int4 q = L.desc(bsel)[32 * sb + r_row];
        const float qm0 = __int_as_float(q.z), qm1 = __int_as_float(q.w);
        const int c0 = 16 * r_ks + 8 * r_kh;
        const float* di = db + (size_t)q.x * stride + c0;
        const float* dj = db + (size_t)q.y * stride + c0;
        const float* xi = xb + (size_t)q.x * stride + c0;
        const float* xj = xb + (size_t)q.y * stride + c0;
#pragma unroll
        for (int h4 = 0; h4 < 2; ++h4) {
          const float4 a = *reinterpret_cast<const float4*>(di + 4 * h4), b = *reinterpret_cast<const float4*>(xj + 4 * h4);
          const float4 c = *reinterpret_cast<const float4*>(dj + 4 * h4), d = *reinterpret_cast<const float4*>(xi + 4 * h4);
          v[sb][4 * h4 + 0] = qm0 * (a.x * b.x) + qm1 * (c.x * d.x);
          v[sb][4 * h4 + 1] = qm0 * (a.y * b.y) + qm1 * (c.y * d.y);
          v[sb][4 * h4 + 2] = qm0 * (a.z * b.z) + qm1 * (c.z * d.z);
          v[sb][4 * h4 + 3] = qm0 * (a.w * b.w) + qm1 * (c.w * d.w);
        }
      }
    };
    float bound;
    if (staged) {
      build(L.xs, L.ds, 1);  // descriptors hold LDS float offsets
      float mx = 0.0f, md = 0.0f;
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        mx = fmaxf(mx, L.wmax[2 * i]);
        md = fmaxf(md, L.wmax[2 * i + 1]);
      }
      bound = 2.0f * mx * md;  // |dO| <= C (|dagg_i x_j| + |dagg_j x_i|), C <= 1
    } else {
      build(x, dagg, F);  // a run of tiny molecules: operands straight from global memory, exact largest magnitude
      float m = 0.0f;
#pragma unroll
      for (int sb = 0; sb < SUB; ++sb)
#pragma unroll
        for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf(v[sb][e]));
      m = wave_max(m);
      if (lane == 0) atomicMax(reinterpret_cast<unsigned*>(L.et + CB), __float_as_uint(m));  // zeroed by publish()
      lds_barrier();
      bound = __uint_as_float(*reinterpret_cast<volatile unsigned*>(L.et + CB));
    }
    {  // the block scale of dO: taken once per tile, for all its M blocks
      const int e_t = __builtin_amdgcn_readfirstlane(mag_exponent(bound));
      if (e_t > EO) {
        const float f = __builtin_amdgcn_ldexpf(1.0f, EO - e_t);
        if constexpr (roleA) {
#pragma unroll
          for (int gb = 0; gb < 2; ++gb)
#pragma unroll
            for (int r = 0; r < 16; ++r) accw1[gb][r] *= f;
        } else {
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) accw2[cb][r] *= f;
        }
        EO = e_t;
      }
      const float sO = __builtin_amdgcn_ldexpf(1.0f, 14 - EO);
#pragma unroll
      for (int sb = 0; sb < SUB; ++sb) {
        const Frag2 f = split8h_scaled(v[sb], sO);
        u32x4* dst = L.dOr + sb * Lds::DOR_WORDS + (size_t)(r_ks * 2) * 64 + (r_row + 32 * r_kh);
        dst[0] = f.h;
        dst[64] = f.l;
      }
    }
    if constexpr (roleA) {
      // t slice of this wave's hidden units as B fragments of dW2's contraction over pair rows: the C layout held in
      // tc (lane = h, register r <-> row c_row(r)) is the fragment layout with k-step s <-> registers 8s..8s+7
      float tm = 0.0f;
#pragma unroll
      for (int sb = 0; sb < SUB; ++sb)
#pragma unroll
        for (int r = 0; r < 16; ++r) tm = fmaxf(tm, fabsf(tc[sb][r]));
      tm = wave_max(tm);
      ET = max(ET, __builtin_amdgcn_readfirstlane(mag_exponent(tm)));
      const float sT = __builtin_amdgcn_ldexpf(1.0f, 14 - ET);
      if (lane == 0) L.et[hs] = ET;
#pragma unroll
      for (int sb = 0; sb < SUB; ++sb)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          float u8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) u8[e] = tc[sb][8 * s2 + e];
          const Frag2 f = split8h_scaled(u8, sT);
          u32x4* dst = L.tf + sb * Lds::TF_WORDS + (size_t)((hs * 2 + s2) * 2) * 64 + lane;
          dst[0] = f.h;
          dst[64] = f.l;
        }
    }
    // Gaussian fragments: by the role-B waves (role A also splits its saved activations in this phase; with the sticky
    // window role B has the shorter build)
    // (rbf_frag.h: B[k = row = 16ks + kperm(e, kh)][n = g], fixed scale 2^14, a column of ones at g = 63 when G < 64 -
    // db1 by the matrix pipe with the rest of dW1 instead of sixteen vector adds per role-A wave and tile)
    if (use_img) {
      if constexpr (IMG && !roleA) {  // this tile's words were requested one MFMA phase ago
#pragma unroll
        for (int sb = 0; sb < SUB; ++sb)
#pragma unroll
          for (int u = 0; u < NIT; ++u) {
            u32x4* dst = L.rbf + sb * Lds::RBF_WORDS + rbf_item_word(64 * hs + lane + 64 * NW * u);
            dst[0] = gfh[sb][u];
            dst[64] = gfl[sb][u];
          }
      }
    } else {
#ifndef FBH_RBF_BY_A
    if (!roleA) {
      for (int it = 64 * hs + lane; it < SUB * RBF_TILE_ITEMS; it += 64 * NW) {
#else
    if (NW == 1 ? roleA : (roleA ? hs < NW / 2 : hs >= NW / 2)) {
      for (int it = 64 * hs + lane; it < SUB * RBF_TILE_ITEMS; it += 64 * (NW == 1 ? 1 : NW)) {
#endif
        const int sb = it / RBF_TILE_ITEMS, ib = it % RBF_TILE_ITEMS;  // M block, item inside its 32-row tile
        const Frag2 f = rbf_fragment_item(ib, [&](int r) { return L.tdd(bsel)[32 * sb + r]; }, offset, coeff, G);
        u32x4* dst = L.rbf + sb * Lds::RBF_WORDS + rbf_item_word(ib);
        dst[0] = f.h;
        dst[64] = f.l;
      }
    }
    }
    // The activations of the NEXT tile are requested into tc while this tile's are still needed for ssp': a 32-row tile
    // keeps a copy and requests at the start of the MFMA phase; a 64-row tile has no registers for two copies - its role-A
    // wave requests M block sb of the next tile as soon as dU of M block sb is formed (LATE_T).
    constexpr bool LATE_T = SUB > 1;
    float tcur[LATE_T ? 1 : 16];
    if constexpr (!LATE_T) {
#pragma unroll
      for (int r = 0; r < 16; ++r) tcur[r] = tc[0][r];
    }
    FBH_MARK(2);
#ifdef FBH_HALF_BARRIERS
    if (!(t & 1))
#endif
    lds_barrier();
    FBH_MARK(3);
    // While this tile is multiplied: publish the next tile's staging buffer (its atoms were requested one tile ago
    // and have arrived), request the atoms of the tile after it and the next tile's saved activations.
    if (t + 1 < t_end) {
#ifdef FB_TIMING
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (blockIdx.x == 3 && blockIdx.y == 0 && lane == 0 && (wave == 0 || wave == NW) && t - t_begin < 64)
        fb_dbg2[(wave == 0 ? 0 : 1) * 64 + (t - t_begin)] = clock64();
#endif
      request_rbf(t + 1);  // first: nothing requested in this phase is waited for before these words are
      publish(t + 1);
      FBH_MARK(7);
      if (t + 2 < t_end) {
        alo_a = alo_b;
        decide(alo_a);  // tile t + 2: its rows' second atoms were fetched one iteration ago
        request_atoms(t + 2, alo_a);
        if (t + 3 < t_end) {
          alo_b = pair_i[(t + 3) * TR];
          request_rows(t + 3);
        }
      }
      if constexpr (!LATE_T || RECOMP) {  // (RECOMP: only the distances; the hidden rows are rebuilt at the end of the phase)
#pragma unroll
        for (int sb = 0; sb < SUB; ++sb) request_t(t + 1, sb);
      }
    }
    FBH_MARK(4);
    if constexpr (roleA) {
      // acc holds (2^(14-EO) dO)(2^(14-e2) W2); |dt| <= 2^EO * (largest column L1 norm of the W2 slice) < 2^(EO+eL)
      // dU = acc kdt ssp'(.) with kdt = 2^(EO + e2 - 28); the split wants dU 2^(14 - EO - eL): both powers of two, folded
      // into ONE scale 2^(e2 - eL - 14) of the split (exact), so the product with kdt is never formed
      const float kdt = __builtin_amdgcn_ldexpf(1.0f, EO + e2 - 28), sUk = __builtin_amdgcn_ldexpf(1.0f, e2 - eL - 14);
      // the M blocks of the tile one after the other: one set of dt accumulators and dU fragments at a time, the W2
      // fragments and the dW1 accumulators shared
#pragma unroll
      for (int sb = 0; sb < SUB; ++sb) {
        __builtin_amdgcn_sched_barrier(0);  // (nothing of the next M block hoisted into this one: registers)
        // dt = dO W2 for this wave's hidden units (back-to-back MFMAs on one accumulator forward SrcC without a stall)
        f32x16 acc0, acc1;  // small-weight and large-weight piece products apart: better conditioned, and two
                            // independent MFMA chains
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
        {
          const u32x4* dOs = L.dOr + sb * Lds::DOR_WORDS + lane;
          Frag2 a0, an;  // fragments of the next k-step are requested before this step's MFMAs issue
          a0.h = dOs[0]; a0.l = dOs[64];
#pragma unroll
          for (int ks = 0; ks < KC; ++ks) {
            if (ks + 1 < KC) {
              const u32x4* s0 = dOs + (size_t)((ks + 1) * 2) * 64;
              an.h = s0[0]; an.l = s0[64];
            }
            __builtin_amdgcn_sched_barrier(0);
            acc1 = mfma_f16(a0.l, bw2[ks].h, acc1);
            acc0 = mfma_f16(a0.h, bw2[ks].h, acc0);
            acc1 = mfma_f16(a0.h, bw2[ks].l, acc1);
            __builtin_amdgcn_sched_barrier(0);
            if (ks + 1 < KC) a0 = an;
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] += acc1[r];
        // dU = dt * ssp'(pre) (C layout: lane = hidden unit, register = pair row); registers 0..7 / 8..15 are the
        // elements of k-steps 0 / 1 of the contraction over pair rows
        Frag2 du[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          float u8[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            u8[e] = acc0[8 * s + e] * dssp_from_out(LATE_T ? tc[sb][8 * s + e] : tcur[8 * s + e]);
            if (G >= 64) bsum1 = fmaf(u8[e], kdt, bsum1);  // (no free column for the ones: the bias sum on the vector unit)
          }
          du[s] = split8h_scaled(u8, sUk);
        }
        if constexpr (LATE_T && !RECOMP) {
          if (t + 1 < t_end) request_t(t + 1, sb);
        }
        if (sb == SUB - 1) FBH_MARK(6);
        // dW1[h][g] += sum_rows dU[row][h] * rbf(d_row)[g]
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          Frag2 b0, b1;
          const u32x4* s0 = L.rbf + sb * Lds::RBF_WORDS + (size_t)(s * 2) * 64 + lane;
          b0.h = s0[0]; b0.l = s0[64];
          b1.h = s0[256]; b1.l = s0[320];
          accw1[0] = mfma_f16(du[s].l, b0.h, accw1[0]);
          accw1[1] = mfma_f16(du[s].l, b1.h, accw1[1]);
          accw1[0] = mfma_f16(du[s].h, b0.l, accw1[0]);
          accw1[1] = mfma_f16(du[s].h, b1.l, accw1[1]);
          accw1[0] = mfma_f16(du[s].h, b0.h, accw1[0]);
          accw1[1] = mfma_f16(du[s].h, b1.h, accw1[1]);
        }
      }
      if (t + 1 < t_end) {  // the next tile's hidden rows (its distances were requested above)
#pragma unroll
        for (int sb = 0; sb < SUB; ++sb) rebuild_t(sb);
      }
    } else {
      // follow the activation scales of the role-A waves (once per tile)
#pragma unroll
      for (int hb = 0; hb < CB; ++hb) {
        const int et = __builtin_amdgcn_readfirstlane(L.et[hb]);
        if (et != ETs[hb]) {
          const float f = __builtin_amdgcn_ldexpf(1.0f, ETs[hb] - et);
#pragma unroll
          for (int r = 0; r < 16; ++r) accw2[hb][r] *= f;
          ETs[hb] = et;
        }
      }
      // Role B wave w owns filter output channels c in [32w, 32w+32).  Its dO^T fragments (lane = c, 8 pair rows) come
      // from the dOr fragments through the matrix pipe: D = dOr_piece * I (I = 16 x 32 selection of the channel block)
      // lands in C layout - lane = c, register = pair row in kperm order - i.e. in fragment order, and every value is
      // an exact bf16 number (one piece times 1), so packing is exact.  No second evaluation of dO in the other
      // orientation, no LDS traffic for it.
#pragma unroll
      for (int sb = 0; sb < SUB; ++sb) {
        __builtin_amdgcn_sched_barrier(0);  // (nothing of the next M block hoisted into this one: registers)
        f32x16 tp[2];
#pragma unroll
        for (int pc = 0; pc < 2; ++pc)
#pragma unroll
          for (int r = 0; r < 16; ++r) tp[pc][r] = 0.0f;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const u32x4* s0 = L.dOr + sb * Lds::DOR_WORDS + (size_t)((2 * hs + q) * 2) * 64 + lane;
          tp[0] = mfma_f16(s0[0], ident[q], tp[0]);
          tp[1] = mfma_f16(s0[64], ident[q], tp[1]);
        }
        if (sb == SUB - 1) FBH_MARK(6);
        Frag2 da[2];  // A fragments of dW2 = dO^T t: k-step s <-> registers 8s..8s+7 (every value is an fp16 number)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f16x2 ph = {(_Float16)tp[0][8 * s2 + 2 * q], (_Float16)tp[0][8 * s2 + 2 * q + 1]};
            const f16x2 pl = {(_Float16)tp[1][8 * s2 + 2 * q], (_Float16)tp[1][8 * s2 + 2 * q + 1]};
            da[s2].h[q] = __builtin_bit_cast(uint32_t, ph);
            da[s2].l[q] = __builtin_bit_cast(uint32_t, pl);
          }
        {
          float rs = 0.0f;
#pragma unroll
          for (int r = 0; r < 16; ++r) rs += tp[0][r] + tp[1][r];
          bsum2 += rs * __builtin_amdgcn_ldexpf(1.0f, EO - 14);  // db2: rows of this half-wave
        }
        // dW2[c][h] += sum_rows dO[row][c] * t[row][h], all four 32-wide blocks of h (t fragments published by role A)
        constexpr int CP = CB >= 2 ? 2 : 1;
#pragma unroll
        for (int hb = 0; hb < CB; hb += CP) {
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            Frag2 tb[CP];
#pragma unroll
            for (int u = 0; u < CP; ++u) {
              const u32x4* s0 = L.tf + sb * Lds::TF_WORDS + (size_t)(((hb + u) * 2 + s2) * 2) * 64 + lane;
              tb[u].h = s0[0]; tb[u].l = s0[64];
            }
#pragma unroll
            for (int u = 0; u < CP; ++u) accw2[hb + u] = mfma_f16(da[s2].l, tb[u].h, accw2[hb + u]);
#pragma unroll
            for (int u = 0; u < CP; ++u) accw2[hb + u] = mfma_f16(da[s2].h, tb[u].l, accw2[hb + u]);
#pragma unroll
            for (int u = 0; u < CP; ++u) accw2[hb + u] = mfma_f16(da[s2].h, tb[u].h, accw2[hb + u]);
          }
        }
      }
    }
    FBH_MARK(5);
  }
  // ---- one partial per block
  const size_t pb = (size_t)l * gridDim.x + blockIdx.x;
  if constexpr (roleA) {
    float* Pw = partial_w1 + pb * F * G;
    const float kw1 = __builtin_amdgcn_ldexpf(1.0f, EO + eL - 28);  // dU carried 2^(14-EO-eL), the Gaussians 2^14
#pragma unroll
    for (int gb = 0; gb < 2; ++gb) {
      const int gg = 32 * gb + j;
      if (gg < G) {
#pragma unroll
        for (int r = 0; r < 16; ++r) Pw[(size_t)(32 * hs + c_row(r, lane)) * G + gg] = accw1[gb][r] * kw1;
      }
    }
    if (G < 64) {
      // db1 = column 63 of the dW1 accumulator (the ones column of the Gaussian fragments): lane j = 31 of block 1
      if (j == 31) {
#pragma unroll
        for (int r = 0; r < 16; ++r) partial_b1[pb * F + 32 * hs + c_row(r, lane)] = accw1[1][r] * kw1;
      }
    } else {
      const float s = bsum1 + __shfl_xor(bsum1, 32, 64);
      if (kh == 0) partial_b1[pb * F + 32 * hs + j] = s;
    }
  } else {
    float* Pw = partial_w2 + pb * F * F;
#pragma unroll
    for (int hb = 0; hb < CB; ++hb) {
      const float kw2 = __builtin_amdgcn_ldexpf(1.0f, EO + ETs[hb] - 28);
#pragma unroll
      for (int r = 0; r < 16; ++r) Pw[(size_t)(32 * hs + c_row(r, lane)) * F + 32 * hb + j] = accw2[hb][r] * kw2;
    }
    // db2[c]: each half-wave summed the pair rows its registers hold
    const float sb2 = bsum2 + __shfl_xor(bsum2, 32, 64);
    if (kh == 0) partial_b2[pb * F + 32 * hs + j] = sb2;
  }
}

// The two roles run separate instantiations of the body (their register sets differ: W2 fragments + dW1
// accumulators against dW2 accumulators); the branch is wave-uniform and both sides execute the same barriers.
// tile_rows (uniform over the launch): 64, or 32 for the 32-row form of the same kernel (GEOSSL_FILTER_BWD_TILE32); the
// form that rebuilds the hidden rows has the 32-row body only (see filter_bwd_launch).
template <int NW, bool RECOMP>
__global__ __launch_bounds__(128 * NW) __attribute__((amdgpu_waves_per_eu(2))) void k_filter_bwd_h(
    const float* __restrict__ pair_d, const float* __restrict__ pair_c, const uint8_t* __restrict__ pair_flag,
    const int32_t* __restrict__ pair_i, const int32_t* __restrict__ pair_j, int P, int N, GeosslFilterWeights w,
    GeosslFilterGradIn g, int G, const float* __restrict__ offset, float coeff, const float* __restrict__ T,
    float* __restrict__ partial_w1, float* __restrict__ partial_b1, float* __restrict__ partial_w2,
    float* __restrict__ partial_b2, const int32_t* __restrict__ dyn_P, const int32_t* __restrict__ dyn_N,
    const u32x4* __restrict__ img, int tile_rows) {
  const int Pstride = P;
  P = dyn_count(P, dyn_P);
  N = dyn_count(N, dyn_N);
  const bool roleA = (int)(threadIdx.x >> 6) < NW;
#define FB_BODY(ROLE_A, TRH)                                                                                           \
  filter_bwd_body_h<NW, ROLE_A, RECOMP, TRH>(pair_d, pair_c, pair_flag, pair_i, pair_j, P, N, w, g, G, offset, coeff, T, \
                                             partial_w1, partial_b1, partial_w2, partial_b2, Pstride, img)
  if (RECOMP || tile_rows == 32) {
    if (roleA) FB_BODY(true, 32); else FB_BODY(false, 32);
  } else if constexpr (!RECOMP) {
    if (roleA) FB_BODY(true, 64); else FB_BODY(false, 64);
  }
#undef FB_BODY
}

// The per-step image of the Gaussian fragments (rbf_frag.h): one block per 32-row tile of the CAPACITY P, one item per
// thread.  Distances as the tile build above reads them: row r of the list at r < n, the last real row's past it (tail
// tile and every tile past the real count n = dyn_count(P, dyn_P): finite words - their dO is exactly zero, which an
// unwritten word could still turn into NaN).  No real row at all: zeros.
__global__ __launch_bounds__(RBF_TILE_ITEMS) void k_rbf_fragments(const float* __restrict__ pair_d, int P, int G,
                                                                  const float* __restrict__ offset, float coeff,
                                                                  u32x4* __restrict__ image,
                                                                  const int32_t* __restrict__ dyn_P) {
  const int n = dyn_count(P, dyn_P);
  const int r0 = blockIdx.x * TR, it = threadIdx.x;
  u32x4* __restrict__ dst = image + (size_t)blockIdx.x * RBF_TILE_WORDS + rbf_item_word(it);
  if (n <= 0) {
    dst[0] = u32x4{0u, 0u, 0u, 0u};
    dst[64] = u32x4{0u, 0u, 0u, 0u};
    return;
  }
  const Frag2 f = rbf_fragment_item(it, [&](int r) { return pair_d[min(r0 + r, n - 1)]; }, offset, coeff, G);
  dst[0] = f.h;
  dst[64] = f.l;
}

inline int blocks_per_layer(int L, int ntiles) {
  int b = 256 / (L > 0 ? L : 1);  // one block per CU
  if (b < 1) b = 1;
  if (b > ntiles) b = ntiles;
  return b;
}

}  // namespace

#ifdef FB_TIMING
extern "C" int geossl_filter_bwd_debug_read(long long* host) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(fb_dbg), sizeof(long long) * 2 * 64 * 8);
}
extern "C" int geossl_filter_bwd_debug_read3(long long* host) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(fb_dbg3), sizeof(long long) * 64 * 4);
}
extern "C" int geossl_filter_bwd_debug_read2(long long* host) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(fb_dbg2), sizeof(long long) * 2 * 64);
}
#endif

extern "C" int64_t geossl_cfconv_filter_bwd_workspace_floats(int64_t P, int L, int F, int G) {
  const int ntiles = (int)((P + TR - 1) / TR);
  const int64_t nb = blocks_per_layer(L, ntiles);
  return (int64_t)L * nb * ((int64_t)F * G + F + (int64_t)F * F + F);
}

extern "C" int geossl_cfconv_filter_bwd(const float* pair_d, const float* pair_c, const uint8_t* pair_flag,
                                        const int32_t* pair_i, const int32_t* pair_j, int64_t P, int64_t N,
                                        const GeosslFilterWeights* w, const GeosslFilterGradIn* g, int L, int F, int G,
                                        const float* offset, float coeff, const float* T,
                                        const GeosslFilterGradOut* out, float* workspace, int accumulate,
                                        hipStream_t stream) {
  return geossl_cfconv_filter_bwd_dyn(pair_d, pair_c, pair_flag, pair_i, pair_j, P, N, w, g, L, F, G, offset, coeff, T, out,
                                      workspace, accumulate, nullptr, nullptr, stream);
}

namespace {

// every entry point of the weight-gradient launch; image: the Gaussian fragments of geossl_rbf_fragments, or nullptr
int filter_bwd_launch(const float* pair_d, const float* pair_c, const uint8_t* pair_flag, const int32_t* pair_i,
                      const int32_t* pair_j, int64_t P, int64_t N, const GeosslFilterWeights* w,
                      const GeosslFilterGradIn* g, int L, int F, int G, const float* offset, float coeff, const float* T,
                      const GeosslFilterGradOut* out, float* workspace, int accumulate, const int32_t* dyn_P,
                      const int32_t* dyn_N, const void* image, hipStream_t stream) {
  if (P <= 0 || L <= 0) return 0;
  // (G < 1: the kernels clamp the padded Gaussian index to G - 1, which would read in front of w1 and offset)
  if (L > GEOSSL_MAX_L || (F != 32 && F != 64 && F != 128) || G > 64 || G < 1) return (int)hipErrorInvalidValue;
  // (read per call: an A/B run times both forms in one process)
  const bool bf16x3 = getenv("GEOSSL_FILTER_BWD_BF16X3") != nullptr || getenv("GEOSSL_ARITH_24BIT") != nullptr;
  // the two-piece kernel works on 64-row tiles; GEOSSL_FILTER_BWD_TILE32 selects its 32-row form (the three-piece kernel
  // has that one only).  The workspace is sized for 32-row tiles, which never gives fewer blocks.
  // The form that rebuilds the hidden rows (T == NULL) keeps 32 rows as well: its role-A wave holds the W1 fragments next
  // to the W2 fragments, and a second set of hidden rows beside them does not fit 256 registers (63 spilled at F = 128).
  const bool tile32 = getenv("GEOSSL_FILTER_BWD_TILE32") != nullptr || T == nullptr;
  const int rows = (bf16x3 || tile32) ? TR : 64;
  const int ntiles = (int)((P + rows - 1) / rows);
  const int nb = blocks_per_layer(L, ntiles);
  dim3 grid(nb, L);
  float* pw1 = workspace;                          // [L][nb][F][G]
  float* pb1 = pw1 + (size_t)L * nb * F * G;       // [L][nb][F]
  float* pw2 = pb1 + (size_t)L * nb * F;           // [L][nb][F][F]
  float* pb2 = pw2 + (size_t)L * nb * F * F;       // [L][nb][F]
#define LAUNCH(NW)                                                                                                 \
  do {                                                                                                             \
    const size_t lds = BwdLds<32 * NW>::bytes();                                                                   \
    allow_big_lds(&k_filter_bwd<NW>);                                                                              \
    hipLaunchKernelGGL((k_filter_bwd<NW>), grid, dim3(128 * NW), lds, stream, pair_d, pair_c, pair_flag, pair_i,   \
                       pair_j, (int)P, (int)N, *w, *g, G, offset, coeff, T, pw1, pb1, pw2, pb2, dyn_P, dyn_N);     \
  } while (0)
#define LAUNCH_H(NW)                                                                                               \
  do {                                                                                                             \
    const size_t lds = tile32 ? BwdLdsH<32 * NW, 32>::bytes() : BwdLdsH<32 * NW, 64>::bytes();                     \
    if (T == nullptr) {                                                                                            \
      allow_big_lds(&k_filter_bwd_h<NW, true>);                                                                    \
      hipLaunchKernelGGL((k_filter_bwd_h<NW, true>), grid, dim3(128 * NW), lds, stream, pair_d, pair_c, pair_flag, \
                         pair_i, pair_j, (int)P, (int)N, *w, *g, G, offset, coeff, T, pw1, pb1, pw2, pb2, dyn_P,   \
                         dyn_N, nullptr, rows);                                                                    \
    } else {                                                                                                       \
      allow_big_lds(&k_filter_bwd_h<NW, false>);                                                                   \
      hipLaunchKernelGGL((k_filter_bwd_h<NW, false>), grid, dim3(128 * NW), lds, stream, pair_d, pair_c, pair_flag,\
                         pair_i, pair_j, (int)P, (int)N, *w, *g, G, offset, coeff, T, pw1, pb1, pw2, pb2, dyn_P,   \
                         dyn_N, img, rows);                                                                        \
    }                                                                                                              \
  } while (0)
  // (the three-piece form and the form that rebuilds the hidden rows keep the in-kernel Gaussians: an image is ignored)
  const u32x4* img = static_cast<const u32x4*>(image);
  if (bf16x3 && T == nullptr) return (int)hipErrorInvalidValue;  // (the three-piece form reads the saved hidden rows)
  if (!bf16x3) {
    if (F == 128) LAUNCH_H(4); else if (F == 64) LAUNCH_H(2); else LAUNCH_H(1);
  } else {
    if (F == 128) LAUNCH(4); else if (F == 64) LAUNCH(2); else LAUNCH(1);
  }
#undef LAUNCH_H
#undef LAUNCH
  GEOSSL_CHECK_LAUNCH();
  ReduceMulti rm;  // the four fixed-order partial sums in one launch
  rm.add(pw1, F * G, G, G, 1, out->dw1, L);
  rm.add(pb1, F, F, F, 1, out->db1, L);
  rm.add(pw2, F * F, F, F, 1, out->dw2, L);
  rm.add(pb2, F, F, F, 1, out->db2, L);
  hipLaunchKernelGGL(k_reduce_multi, dim3(rm.blocks(), L), dim3(256), 0, stream, rm, nb, accumulate);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int geossl_cfconv_filter_bwd_dyn(const float* pair_d, const float* pair_c, const uint8_t* pair_flag,
                                            const int32_t* pair_i, const int32_t* pair_j, int64_t P, int64_t N,
                                            const GeosslFilterWeights* w, const GeosslFilterGradIn* g, int L, int F,
                                            int G, const float* offset, float coeff, const float* T,
                                            const GeosslFilterGradOut* out, float* workspace, int accumulate,
                                            const int32_t* dyn_P, const int32_t* dyn_N, hipStream_t stream) {
  return filter_bwd_launch(pair_d, pair_c, pair_flag, pair_i, pair_j, P, N, w, g, L, F, G, offset, coeff, T, out, workspace,
                           accumulate, dyn_P, dyn_N, nullptr, stream);
}

extern "C" int geossl_cfconv_filter_bwd_frag(const float* pair_d, const float* pair_c, const uint8_t* pair_flag,
                                             const int32_t* pair_i, const int32_t* pair_j, int64_t P, int64_t N,
                                             const GeosslFilterWeights* w, const GeosslFilterGradIn* g, int L, int F,
                                             int G, const float* offset, float coeff, const float* T,
                                             const GeosslFilterGradOut* out, float* workspace, int accumulate,
                                             const void* image, hipStream_t stream) {
  return geossl_cfconv_filter_bwd_frag_dyn(pair_d, pair_c, pair_flag, pair_i, pair_j, P, N, w, g, L, F, G, offset, coeff, T,
                                           out, workspace, accumulate, nullptr, nullptr, image, stream);
}

extern "C" int geossl_cfconv_filter_bwd_frag_dyn(const float* pair_d, const float* pair_c, const uint8_t* pair_flag,
                                                 const int32_t* pair_i, const int32_t* pair_j, int64_t P, int64_t N,
                                                 const GeosslFilterWeights* w, const GeosslFilterGradIn* g, int L, int F,
                                                 int G, const float* offset, float coeff, const float* T,
                                                 const GeosslFilterGradOut* out, float* workspace, int accumulate,
                                                 const int32_t* dyn_P, const int32_t* dyn_N, const void* image,
                                                 hipStream_t stream) {
  if (image == nullptr) return (int)hipErrorInvalidValue;
  return filter_bwd_launch(pair_d, pair_c, pair_flag, pair_i, pair_j, P, N, w, g, L, F, G, offset, coeff, T, out, workspace,
                           accumulate, dyn_P, dyn_N, image, stream);
}

// (tests: the items of rbf_frag.h one after the other - [tile][item 256][piece 2] - with the distances of k_rbf_fragments)
namespace {
__global__ __launch_bounds__(RBF_TILE_ITEMS) void k_rbf_fragment_items(const float* __restrict__ pair_d, int P, int G,
                                                                       const float* __restrict__ offset, float coeff,
                                                                       u32x4* __restrict__ items,
                                                                       const int32_t* __restrict__ dyn_P) {
  const int n = dyn_count(P, dyn_P);
  const int r0 = blockIdx.x * TR, it = threadIdx.x;
  if (n <= 0) return;
  const Frag2 f = rbf_fragment_item(it, [&](int r) { return pair_d[min(r0 + r, n - 1)]; }, offset, coeff, G);
  u32x4* __restrict__ dst = items + ((size_t)blockIdx.x * RBF_TILE_ITEMS + it) * 2;
  dst[0] = f.h;
  dst[1] = f.l;
}
}  // namespace

extern "C" int geossl_rbf_fragment_items(const float* pair_d, int64_t P, int G, const float* offset, float coeff,
                                         void* items, const int32_t* dyn_P, hipStream_t stream) {
  if (P <= 0) return 0;
  if (G > 64 || G < 1 || P > INT32_MAX) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rbf_fragment_items, dim3((unsigned)((P + TR - 1) / TR)), dim3(RBF_TILE_ITEMS), 0, stream, pair_d,
                     (int)P, G, offset, coeff, static_cast<u32x4*>(items), dyn_P);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t geossl_rbf_fragments_bytes(int64_t P) {
  return P > 0 ? (P + TR - 1) / TR * (int64_t)RBF_TILE_WORDS * 16 : 0;
}

extern "C" int geossl_rbf_fragments(const float* pair_d, int64_t P, int G, const float* offset, float coeff, void* image,
                                    hipStream_t stream) {
  return geossl_rbf_fragments_dyn(pair_d, P, G, offset, coeff, image, nullptr, stream);
}

extern "C" int geossl_rbf_fragments_dyn(const float* pair_d, int64_t P, int G, const float* offset, float coeff,
                                        void* image, const int32_t* dyn_P, hipStream_t stream) {
  if (P <= 0) return 0;
  if (G > 64 || G < 1 || P > INT32_MAX) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rbf_fragments, dim3((unsigned)((P + TR - 1) / TR)), dim3(RBF_TILE_ITEMS), 0, stream, pair_d, (int)P,
                     G, offset, coeff, static_cast<u32x4*>(image), dyn_P);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
