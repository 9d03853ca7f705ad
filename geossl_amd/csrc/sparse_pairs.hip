// SchNet on structures above 255 atoms: the radius graph as a compacted list of the pairs that carry an edge, and the
// three operations that need to know where a pair's row is - the neighbour aggregation (forward and transposed) and the
// position gradient's scatter - on that list.  (The dense form gives every pair (a < b) of a molecule a slot in closed
// form, n (n - 1) / 2 of them; the neighbour cap of radius_graph leaves at most 33 edges per atom, so a 500-atom pocket
// has at most 16 500 pairs with an edge among 124 750 slots.)  The filter network (filter_fwd / filter_bwd /
// filter_dpos) takes rows with explicit pair_i / pair_j / pair_flag and runs on the list unchanged.
//
// The list: per molecule in batch order the pairs (a < b) with an edge in at least one direction, lexicographic, packed
// back to back; the number of rows is known on the device only (`n_pairs`, the dyn_P of the filter kernels), every
// array is sized by the host-side bound sum_m min(n_m (n_m - 1) / 2, 33 n_m) and the rows past the real ones are
// rewritten on every call (flag 0, pair_i = pair_j = 0, pair_c = 0, pair_d = cutoff).
//
// Incidence lists: atom t's pairs in ascending partner order (the pairs with pair_j == t first, then those with
// pair_i == t), entry k = (inc_pair[k] = row, inc_src[k] = partner | edge partner -> t << 30 | edge t -> partner << 31):
// a target's walk needs neither pair_i / pair_j nor the flags.
#include "common.h"
#include "radius_adj.h"
#include "geossl_hip.h"

using namespace geossl;

namespace {

constexpr int SP_THREADS = 256, SP_WAVES = SP_THREADS / 64;
constexpr unsigned SP_FWD = 1u << 30, SP_BWD = 1u << 31, SP_ATOM = SP_FWD - 1u;

// row stride of the bit matrix in 64-bit words: odd, so that the lanes of a wave that read one column (word a / 64 of
// 64 consecutive rows) fall into different LDS banks
__host__ __device__ inline int sp_stride(int max_n) { return ((max_n + 63) / 64) | 1; }

struct SpLds {
  unsigned long long* adj;  // [max_n][stride]: bit b of row a = edge b -> a (target a)
  float* sp;                // [max_n][3]
  int* up;                  // [max_n + 1] pairs (a, b > a) of atom a, then their exclusive scan
  int* inc;                 // [max_n + 1] incidence entries of atom a, then their exclusive scan
  int* s_a;                 // [SP_THREADS] block reductions and scans
  int* s_b;                 // [SP_THREADS]
  int* s_wcnt;              // [2][4][SP_WAVES] pairs per wave of a row atom's step, two buffers
};
// (all of it dynamic: the kernels are opted into the full 160 KB, which leaves no room for static LDS beside it)
inline size_t sp_lds_bytes(int max_n) {
  return (size_t)max_n * sp_stride(max_n) * 8 + (size_t)max_n * 12 + 2 * (size_t)(max_n + 1) * 4 +
         (2 * SP_THREADS + 2 * 4 * SP_WAVES) * 4;
}
__device__ __forceinline__ SpLds sp_carve(unsigned char* raw, int max_n) {
  SpLds L;
  L.adj = reinterpret_cast<unsigned long long*>(raw);
  L.sp = reinterpret_cast<float*>(L.adj + (size_t)max_n * sp_stride(max_n));
  L.up = reinterpret_cast<int*>(L.sp + 3 * (size_t)max_n);
  L.inc = L.up + max_n + 1;
  L.s_a = L.inc + max_n + 1;
  L.s_b = L.s_a + SP_THREADS;
  L.s_wcnt = L.s_b + SP_THREADS;
  return L;
}

// LDS holds max_n atoms: a molecule above the bound (the host checks it: layout.max_n, Bucket.fits) is given no pairs
// instead of a walk past the arrays
__device__ __forceinline__ int sp_mol_atoms(int n, int max_n) { return n <= max_n ? n : 0; }

// positions and the bit matrix of molecule [a0, a0 + n) into LDS: a wave per target atom (radius_adj.h says which
// edges exist)
__device__ __forceinline__ void sp_adjacency(const float* __restrict__ pos, int a0, int n, int ws, float r2, int cap,
                                             const SpLds& L) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 3 * n; i += SP_THREADS) L.sp[i] = pos[(size_t)a0 * 3 + i];
  __syncthreads();
  for (int i = wave; i < n; i += SP_WAVES)
    radius_scan_target(L.sp, n, i, lane, r2, cap, [&](int c, int, float, bool, unsigned long long kept, int) {
      if (lane == 0) L.adj[(size_t)i * ws + c] = kept;
    });
  __syncthreads();
}

// ---- pass 1: pairs per molecule and per atom ------------------------------------------------------------------------
__global__ __launch_bounds__(SP_THREADS) void k_sparse_count(const float* __restrict__ pos,
                                                             const int32_t* __restrict__ mol_ptr, int B, int max_n,
                                                             float r2, int cap, int32_t* __restrict__ mol_cnt,
                                                             int32_t* __restrict__ up_cnt, int32_t* __restrict__ lo_cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int m = blockIdx.x;
  if (m >= B) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a0 = mol_ptr[m], n = sp_mol_atoms(mol_ptr[m + 1] - a0, max_n), ws = sp_stride(max_n);
  const SpLds L = sp_carve(smem_raw, max_n);
  int* s_tot = L.s_a;
  sp_adjacency(pos, a0, n, ws, r2, cap, L);
  int tot = 0;
  for (int a = wave; a < n; a += SP_WAVES) {
    const int wa = a >> 6, ba = a & 63;
    int up = 0, lo = 0;
    for (int c = 0; c * 64 < n; ++c) {
      const int b = c * 64 + lane;
      const unsigned long long row = L.adj[(size_t)a * ws + c];
      bool on = false;
      if (b < n && b != a) on = (((row >> lane) | (L.adj[(size_t)b * ws + wa] >> ba)) & 1ull) != 0ull;
      const unsigned long long mk = __ballot(on);
      if (c < wa) lo += __popcll(mk);
      else if (c > wa) up += __popcll(mk);
      else {
        lo += __popcll(mk & ((1ull << ba) - 1ull));
        up += __popcll((mk >> ba) >> 1);
      }
    }
    if (lane == 0) {
      up_cnt[a0 + a] = up;
      lo_cnt[a0 + a] = lo;
    }
    tot += up;
  }
  if (lane == 0) s_tot[wave] = tot;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    for (int w = 0; w < SP_WAVES; ++w) t += s_tot[w];
    mol_cnt[m] = t;
  }
}

// ---- pass 2: the rows and the incidence lists -----------------------------------------------------------------------
// The block walks the row atoms a in ascending order, its 256 threads over the partners b > a, 256 at a time: thread
// tid owns the columns tid, tid + 256, ... and counts in registers how many pairs each has had so far - the position of
// (a, b) in b's list of smaller partners, ascending in a because the walk is.  The position of b in a's list of larger
// partners is a prefix over the block (ballots + the wave totals through LDS: one barrier per row atom).
__global__ __launch_bounds__(SP_THREADS) void k_sparse_fill(
    const float* __restrict__ pos, const int32_t* __restrict__ mol_ptr, int B, int N, int max_n, float r2, int cap,
    float cutoff, const int32_t* __restrict__ mol_cnt, const int32_t* __restrict__ up_cnt,
    const int32_t* __restrict__ lo_cnt, int Pcap, int32_t* __restrict__ pair_i, int32_t* __restrict__ pair_j,
    float* __restrict__ pair_d, float* __restrict__ pair_c, uint8_t* __restrict__ pair_flag,
    int32_t* __restrict__ inc_ptr, int32_t* __restrict__ inc_pair, uint32_t* __restrict__ inc_src,
    int32_t* __restrict__ n_pairs, const int32_t* __restrict__ dyn_N) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int m = blockIdx.x;
  if (m >= B) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a0 = mol_ptr[m], n_all = mol_ptr[m + 1] - a0, n = sp_mol_atoms(n_all, max_n), ws = sp_stride(max_n);
  const SpLds L = sp_carve(smem_raw, max_n);
  int* s_a = L.s_a;
  int* s_b = L.s_b;
  int(*s_wcnt)[4][SP_WAVES] = reinterpret_cast<int(*)[4][SP_WAVES]>(L.s_wcnt);
  // first row of this molecule = pairs of the molecules before it; the batch's total
  {
    int before = 0, all = 0;
    for (int k = tid; k < B; k += SP_THREADS) {
      const int v = mol_cnt[k];
      all += v;
      if (k < m) before += v;
    }
    s_a[tid] = before;
    s_b[tid] = all;
    __syncthreads();
    for (int o = SP_THREADS / 2; o > 0; o >>= 1) {
      if (tid < o) {
        s_a[tid] += s_a[tid + o];
        s_b[tid] += s_b[tid + o];
      }
      __syncthreads();
    }
  }
  const int base = s_a[0], total = min(s_b[0], Pcap);
  __syncthreads();
  if (m == 0 && tid == 0) n_pairs[0] = total;
  if (m == B - 1 && tid == 0) inc_ptr[dyn_count(N, dyn_N)] = 2 * total;  // (N real atoms: mol_ptr[B])
  if (n != n_all)  // (a molecule above the LDS bound: empty incidence lists)
    for (int a = tid; a < n_all; a += SP_THREADS) inc_ptr[a0 + a] = 2 * base;
  // rows past the real ones: harmless to a kernel that only knows the capacity (never a zero distance)
  for (int p = total + m * SP_THREADS + tid; p < Pcap; p += B * SP_THREADS) {
    pair_i[p] = 0;
    pair_j[p] = 0;
    pair_d[p] = cutoff;
    pair_c[p] = 0.0f;
    pair_flag[p] = 0;
  }
  sp_adjacency(pos, a0, n, ws, r2, cap, L);
  // exclusive scans of the per-atom counts (four consecutive atoms per thread)
  {
    int va[4], vb[4], ta = 0, tb = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int a = 4 * tid + q;
      va[q] = a < n ? up_cnt[a0 + a] : 0;
      vb[q] = a < n ? va[q] + lo_cnt[a0 + a] : 0;
      ta += va[q];
      tb += vb[q];
    }
    s_a[tid] = ta;
    s_b[tid] = tb;
    __syncthreads();
    for (int o = 1; o < SP_THREADS; o <<= 1) {
      const int xa = tid >= o ? s_a[tid - o] : 0, xb = tid >= o ? s_b[tid - o] : 0;
      __syncthreads();
      s_a[tid] += xa;
      s_b[tid] += xb;
      __syncthreads();
    }
    int ea = s_a[tid] - ta, eb = s_b[tid] - tb;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int a = 4 * tid + q;
      if (a < n) {
        L.up[a] = ea;
        L.inc[a] = eb;
        inc_ptr[a0 + a] = 2 * base + eb;
      }
      ea += va[q];
      eb += vb[q];
    }
    if (tid == 0) {
      L.up[n] = s_a[SP_THREADS - 1];
      L.inc[n] = s_b[SP_THREADS - 1];
    }
    __syncthreads();
  }
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const int nS = (n + SP_THREADS - 1) / SP_THREADS;  // at most 4: max_n <= 1024
  int colcnt[4] = {0, 0, 0, 0};
  for (int a = 0; a + 1 < n; ++a) {
    const int par = a & 1, wa = a >> 6, ba = a & 63;
    unsigned fl[4];
    unsigned long long msk[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      fl[s] = 0u;
      msk[s] = 0ull;
      if (s < nS && SP_THREADS * s + SP_THREADS - 1 > a) {  // (uniform over the block)
        const int b = SP_THREADS * s + tid;
        if (b < n && b > a) {
          const unsigned f0 = (unsigned)((L.adj[(size_t)a * ws + (b >> 6)] >> lane) & 1ull);  // edge b -> a
          const unsigned f1 = (unsigned)((L.adj[(size_t)b * ws + wa] >> ba) & 1ull);          // edge a -> b
          fl[s] = f0 | (f1 << 1);
        }
        msk[s] = __ballot(fl[s] != 0u);
      }
      if (lane == 0) s_wcnt[par][s][wave] = __popcll(msk[s]);
    }
    __syncthreads();  // (one per row atom: the counts alternate between two buffers)
    const int up0 = L.up[a];
    const int lo_a = (L.inc[a + 1] - L.inc[a]) - (L.up[a + 1] - up0);
    const int inc_a = 2 * base + L.inc[a] + lo_a;
    int run = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      int mine = 0;
#pragma unroll
      for (int w = 0; w < SP_WAVES; ++w) {
        if (w == wave) mine = run;
        run += s_wcnt[par][s][w];
      }
      if (fl[s] != 0u) {
        const int b = SP_THREADS * s + tid;
        const int rank = mine + __popcll(msk[s] & lt);
        const int p = base + up0 + rank;
        if (p < Pcap) {  // (always, when the capacity is the documented bound)
          const unsigned f0 = fl[s] & 1u, f1 = fl[s] >> 1;
          const float d = sqrtf(dist2_nofma(L.sp + 3 * a, L.sp + 3 * b));
          pair_i[p] = a0 + a;
          pair_j[p] = a0 + b;
          pair_d[p] = d;
          pair_c[p] = pair_envelope(d, cutoff);
          pair_flag[p] = (uint8_t)fl[s];
          // (both below 2 (base + pairs of this molecule) <= 2 Pcap whenever p < Pcap holds for the molecule's last row)
          const int ku = min(inc_a + rank, 2 * Pcap - 1), kl = min(2 * base + L.inc[b] + colcnt[s], 2 * Pcap - 1);
          inc_pair[ku] = p;
          inc_src[ku] = (unsigned)(a0 + b) | (f0 ? SP_FWD : 0u) | (f1 ? SP_BWD : 0u);
          inc_pair[kl] = p;
          inc_src[kl] = (unsigned)(a0 + a) | (f1 ? SP_FWD : 0u) | (f0 ? SP_BWD : 0u);
        }
        colcnt[s] += 1;
      }
    }
  }
}

// ---- live-pair list of a DENSE layout --------------------------------------------------------------------------------
// The pair slots with pair_flag != 0, in slot order, packed back to back: the rows the filter network has work for (a
// slot without an edge gets no filter row and sends no gradient).  row_slot[r] = dense slot of row r; n_live[0] = the
// number of rows, which stays on the device (the dyn_P of the filter kernels).  mol_live[m] = live slots of molecule m
// (geossl_pair_geometry_live); a wave compacts one molecule, its first row = the live slots of the molecules before it
// (summed by the block, as in k_sparse_fill).  Rows past n_live are rewritten on every call in the convention of the
// sparse list (flag 0, pair_i = pair_j = 0, pair_c = 0, pair_d = cutoff; row_slot = 0).  No atomics: deterministic.
constexpr int LP_THREADS = 256, LP_WAVES = LP_THREADS / 64;
__global__ __launch_bounds__(LP_THREADS) void k_live_pairs(
    const float* __restrict__ pair_d, const float* __restrict__ pair_c, const uint8_t* __restrict__ pair_flag,
    const int32_t* __restrict__ pair_i, const int32_t* __restrict__ pair_j, const int32_t* __restrict__ mol_ptr,
    const int32_t* __restrict__ pair_ptr, const int32_t* __restrict__ mol_live, int B, int P, float cutoff,
    const int32_t* __restrict__ dyn_P, float* __restrict__ out_d, float* __restrict__ out_c,
    uint8_t* __restrict__ out_flag, int32_t* __restrict__ out_i, int32_t* __restrict__ out_j,
    int32_t* __restrict__ row_slot, int32_t* __restrict__ n_live) {
  __shared__ int s_before[LP_WAVES], s_all[LP_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * LP_WAVES;
  const int Preal = dyn_count(P, dyn_P);  // slots at and past it do not exist
  {
    int before = 0, all = 0;
    for (int k = tid; k < B; k += LP_THREADS) {
      const int v = mol_live[k];
      all += v;
      if (k < m0) before += v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      before += __shfl_xor(before, o, 64);
      all += __shfl_xor(all, o, 64);
    }
    if (lane == 0) {
      s_before[wave] = before;
      s_all[wave] = all;
    }
    __syncthreads();
  }
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < LP_WAVES; ++w) {
    base += s_before[w];
    total += s_all[w];
  }
  total = min(total, P);
  if (blockIdx.x == 0 && tid == 0) n_live[0] = total;
  for (int p = total + blockIdx.x * LP_THREADS + tid; p < P; p += gridDim.x * LP_THREADS) {
    out_i[p] = 0;
    out_j[p] = 0;
    out_d[p] = cutoff;
    out_c[p] = 0.0f;
    out_flag[p] = 0;
    row_slot[p] = 0;
  }
  const int m = m0 + wave;
  if (m >= B) return;
  for (int k = m0; k < m; ++k) base += mol_live[k];
  const int n = mol_ptr[m + 1] - mol_ptr[m], s0 = pair_ptr[m], np = n * (n - 1) / 2;
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (int q0 = 0; q0 < np; q0 += 64) {  // (uniform over the wave)
    const int slot = s0 + q0 + lane;
    const bool in = q0 + lane < np && slot < Preal;
    const unsigned fl = in ? pair_flag[slot] : 0u;
    const unsigned long long mk = __ballot(fl != 0u);
    const int r = base + __popcll(mk & lt);
    if (fl != 0u && r < P) {
      out_i[r] = pair_i[slot];
      out_j[r] = pair_j[slot];
      out_d[r] = pair_d[slot];
      out_c[r] = pair_c[slot];
      out_flag[r] = (uint8_t)fl;
      row_slot[r] = slot;
    }
    base += __popcll(mk);
  }
}

// dst[l][r] = src[l][row_slot[r]] for the rows r < n_live of every layer (F floats each, 16-byte pieces): the hidden rows
// T of a forward that stored them per dense slot (the path with position gradients: filter_dpos reads T and Wf by one
// index), regrouped for the weight-gradient kernel on the live-pair list - so that this path forms the filter weight
// gradients in the launch, and to the bits, of the path without position gradients.
__global__ __launch_bounds__(256) void k_gather_live_rows(const float* __restrict__ src,
                                                          const int32_t* __restrict__ row_slot,
                                                          const int32_t* __restrict__ n_live, int P, int F4,
                                                          float* __restrict__ dst) {
  const int n = min(P, n_live[0]);
  const size_t lbase = (size_t)blockIdx.y * P;
  const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
  float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
  const int64_t total = (int64_t)n * F4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / F4), c = (int)(i - (int64_t)r * F4);
    d4[(lbase + r) * F4 + c] = s4[(lbase + row_slot[r]) * F4 + c];
  }
}

// ---- neighbour aggregation over the list ----------------------------------------------------------------------------
// out[t] = sum over t's incident pairs with the edge partner -> t (swap: t -> partner) of x[partner] * Wf[row], ascending
// partner, separate multiply and add: the rounding sequence of k_aggregate.  One wave per target atom, a lane owns VW
// adjacent columns; the entries of a target are read 64 at a time (one per lane), the rows of the ones that count four at
// a time (four filter rows and four x rows in flight).  Workgroup b runs on XCD b mod 8: the targets are dealt so that
// an XCD gets a contiguous range of atoms and a molecule's x rows stay in one L2.  Every row of out is written
// (`_dyn`: every row below the real count *dyn_N; N is then the capacity the grid was sized by).
template <int VW>
__global__ __launch_bounds__(SP_THREADS) void k_aggregate_sparse(const float* __restrict__ x,
                                                                 const float* __restrict__ Wf,
                                                                 const int32_t* __restrict__ inc_ptr,
                                                                 const int32_t* __restrict__ inc_pair,
                                                                 const uint32_t* __restrict__ inc_src, int N, int F,
                                                                 int swap, float* __restrict__ out,
                                                                 const int32_t* __restrict__ dyn_N) {
#pragma clang fp contract(off)
  typedef float V __attribute__((ext_vector_type(VW)));
  const int per = gridDim.x / 8;
  const int blk = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  const int t = blk * SP_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= dyn_count(N, dyn_N)) return;  // (a capacity launch: rows at and past the real count are not touched)
  const bool col = VW * lane < F;
  const int f = col ? VW * lane : 0;
  const int k0 = inc_ptr[t], k1 = inc_ptr[t + 1];
  const unsigned dir = swap ? SP_BWD : SP_FWD;
  V acc = V(0.0f);
  for (int kb = k0; kb < k1; kb += 64) {
    const int k = min(kb + lane, k1 - 1);
    const unsigned src = inc_src[k];
    const int row = inc_pair[k];
    unsigned long long mk = __ballot(kb + lane < k1 && (src & dir) != 0u);
    while (mk != 0ull) {
      V xv[4], wv[4];
      bool live[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        live[q] = mk != 0ull;
        const int u = live[q] ? __builtin_ctzll(mk) : 0;
        mk &= mk - 1ull;
        const unsigned s_u = (unsigned)__builtin_amdgcn_readlane((int)src, u) & SP_ATOM;
        const int r_u = __builtin_amdgcn_readlane(row, u);
        xv[q] = *reinterpret_cast<const V*>(x + (size_t)s_u * F + f);
        wv[q] = *reinterpret_cast<const V*>(Wf + (size_t)r_u * F + f);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const V tq = xv[q] * wv[q];
        const V sq = acc + tq;
        acc = live[q] ? sq : acc;
      }
    }
  }
  if (col) *reinterpret_cast<V*>(out + (size_t)t * F + f) = acc;
}

// ---- position gradient over the list --------------------------------------------------------------------------------
// dpos[t] = sum over t's pairs, ascending partner, of (sum_l dd[l][row]) * (pos[t] - pos[partner]) / d: the arithmetic
// of k_pair_position_grad per pair, one thread per atom, no atomics.
__global__ __launch_bounds__(64) void k_pair_position_grad_sparse(const float* __restrict__ pos,
                                                                  const float* __restrict__ pair_d,
                                                                  const float* __restrict__ dd,
                                                                  const int32_t* __restrict__ inc_ptr,
                                                                  const int32_t* __restrict__ inc_pair,
                                                                  const uint32_t* __restrict__ inc_src, int N, int64_t P,
                                                                  int L, float* __restrict__ dpos) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= N) return;
  const float px = pos[3 * (size_t)t], py = pos[3 * (size_t)t + 1], pz = pos[3 * (size_t)t + 2];
  float gx = 0.0f, gy = 0.0f, gz = 0.0f;
  const int k1 = inc_ptr[t + 1];
  for (int k = inc_ptr[t]; k < k1; ++k) {
    const int row = inc_pair[k];
    const size_t b = inc_src[k] & SP_ATOM;
    float s = 0.0f;
    for (int l = 0; l < L; ++l) s += dd[(size_t)l * P + row];
    const float dist = pair_d[row];
    if (s != 0.0f && dist > 0.0f) {
      const float k_ = s / dist;
      gx += k_ * (px - pos[3 * b]);
      gy += k_ * (py - pos[3 * b + 1]);
      gz += k_ * (pz - pos[3 * b + 2]);
    }
  }
  dpos[3 * (size_t)t] = gx;
  dpos[3 * (size_t)t + 1] = gy;
  dpos[3 * (size_t)t + 2] = gz;
}

}  // namespace

static int sparse_pairs_build(const float* pos, const int32_t* mol_ptr, int64_t B, int64_t N, int max_n, float r2,
                              int cap, float cutoff, int64_t capacity, int32_t* mol_cnt, int32_t* up_cnt,
                              int32_t* lo_cnt, int32_t* pair_i, int32_t* pair_j, float* pair_d, float* pair_c,
                              uint8_t* pair_flag, int32_t* inc_ptr, int32_t* inc_pair, uint32_t* inc_src,
                              int32_t* n_pairs, const int32_t* dyn_N, hipStream_t stream) {
  if (max_n < 1 || max_n > GEOSSL_RADIUS_MAX_N || B <= 0 || N <= 0 || capacity < 0 || capacity > (1ll << 29))
    return (int)hipErrorInvalidValue;
  const size_t lds = sp_lds_bytes(max_n);
  allow_big_lds(&k_sparse_count);
  allow_big_lds(&k_sparse_fill);
  hipLaunchKernelGGL(k_sparse_count, dim3((unsigned)B), dim3(SP_THREADS), lds, stream, pos, mol_ptr, (int)B, max_n, r2, cap,
                     mol_cnt, up_cnt, lo_cnt);
  GEOSSL_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_sparse_fill, dim3((unsigned)B), dim3(SP_THREADS), lds, stream, pos, mol_ptr, (int)B, (int)N, max_n,
                     r2, cap, cutoff, mol_cnt, up_cnt, lo_cnt, (int)capacity, pair_i, pair_j, pair_d, pair_c, pair_flag,
                     inc_ptr, inc_pair, inc_src, n_pairs, dyn_N);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_sparse_pairs_build(const float* pos, const int32_t* mol_ptr, int64_t B, int64_t N, int max_n,
                                         float r2, int cap, float cutoff, int64_t capacity, int32_t* mol_cnt,
                                         int32_t* up_cnt, int32_t* lo_cnt, int32_t* pair_i, int32_t* pair_j,
                                         float* pair_d, float* pair_c, uint8_t* pair_flag, int32_t* inc_ptr,
                                         int32_t* inc_pair, uint32_t* inc_src, int32_t* n_pairs, hipStream_t stream) {
  return sparse_pairs_build(pos, mol_ptr, B, N, max_n, r2, cap, cutoff, capacity, mol_cnt, up_cnt, lo_cnt, pair_i, pair_j,
                            pair_d, pair_c, pair_flag, inc_ptr, inc_pair, inc_src, n_pairs, nullptr, stream);
}

extern "C" int geossl_sparse_pairs_build_dyn(const float* pos, const int32_t* mol_ptr, int64_t B, int64_t N, int max_n,
                                             float r2, int cap, float cutoff, int64_t capacity, int32_t* mol_cnt,
                                             int32_t* up_cnt, int32_t* lo_cnt, int32_t* pair_i, int32_t* pair_j,
                                             float* pair_d, float* pair_c, uint8_t* pair_flag, int32_t* inc_ptr,
                                             int32_t* inc_pair, uint32_t* inc_src, int32_t* n_pairs,
                                             const int32_t* dyn_N, hipStream_t stream) {
  if (dyn_N == nullptr) return (int)hipErrorInvalidValue;
  return sparse_pairs_build(pos, mol_ptr, B, N, max_n, r2, cap, cutoff, capacity, mol_cnt, up_cnt, lo_cnt, pair_i, pair_j,
                            pair_d, pair_c, pair_flag, inc_ptr, inc_pair, inc_src, n_pairs, dyn_N, stream);
}

extern "C" int geossl_live_pairs_build(const float* pair_d, const float* pair_c, const uint8_t* pair_flag,
                                       const int32_t* pair_i, const int32_t* pair_j, const int32_t* mol_ptr,
                                       const int32_t* pair_ptr, const int32_t* mol_live, int64_t B, int64_t P,
                                       float cutoff, const int32_t* dyn_P, float* live_d, float* live_c,
                                       uint8_t* live_flag, int32_t* live_i, int32_t* live_j, int32_t* row_slot,
                                       int32_t* n_live, hipStream_t stream) {
  if (B <= 0 || P < 0 || P > (1ll << 30) || mol_live == nullptr || n_live == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_live_pairs, dim3((unsigned)((B + LP_WAVES - 1) / LP_WAVES)), dim3(LP_THREADS), 0, stream, pair_d,
                     pair_c, pair_flag, pair_i, pair_j, mol_ptr, pair_ptr, mol_live, (int)B, (int)P, cutoff, dyn_P, live_d,
                     live_c, live_flag, live_i, live_j, row_slot, n_live);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_gather_live_rows(const float* src, const int32_t* row_slot, const int32_t* n_live, int64_t P, int L,
                                       int F, float* dst, hipStream_t stream) {
  if (P <= 0 || L <= 0) return 0;
  if (F <= 0 || (F & 3) || P > (1ll << 30) || L > 65535 || n_live == nullptr) return (int)hipErrorInvalidValue;
  const int64_t work = (P * (F / 4) + 255) / 256;
  hipLaunchKernelGGL(k_gather_live_rows, dim3((unsigned)(work < 2048 ? work : 2048), (unsigned)L), dim3(256), 0, stream,
                     src, row_slot, n_live, (int)P, F / 4, dst);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

static int aggregate_sparse(const float* x, const float* Wf, const int32_t* inc_ptr, const int32_t* inc_pair,
                            const uint32_t* inc_src, int64_t N, int F, int swap, float* out, const int32_t* dyn_N,
                            hipStream_t stream) {
  if (N <= 0) return 0;
  if ((F != 32 && F != 64 && F != 128) || N > (1ll << 30)) return (int)hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((N + SP_WAVES - 1) / SP_WAVES), grid = 8 * ((blocks + 7) / 8);
  if (F == 128)
    hipLaunchKernelGGL(k_aggregate_sparse<2>, dim3(grid), dim3(SP_THREADS), 0, stream, x, Wf, inc_ptr, inc_pair, inc_src,
                       (int)N, F, swap, out, dyn_N);
  else
    hipLaunchKernelGGL(k_aggregate_sparse<1>, dim3(grid), dim3(SP_THREADS), 0, stream, x, Wf, inc_ptr, inc_pair, inc_src,
                       (int)N, F, swap, out, dyn_N);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_cfconv_aggregate_sparse(const float* x, const float* Wf, const int32_t* inc_ptr,
                                              const int32_t* inc_pair, const uint32_t* inc_src, int64_t N, int F,
                                              int swap, float* out, hipStream_t stream) {
  return aggregate_sparse(x, Wf, inc_ptr, inc_pair, inc_src, N, F, swap, out, nullptr, stream);
}

extern "C" int geossl_cfconv_aggregate_sparse_dyn(const float* x, const float* Wf, const int32_t* inc_ptr,
                                                  const int32_t* inc_pair, const uint32_t* inc_src, int64_t N, int F,
                                                  int swap, float* out, const int32_t* dyn_N, hipStream_t stream) {
  if (dyn_N == nullptr) return (int)hipErrorInvalidValue;
  return aggregate_sparse(x, Wf, inc_ptr, inc_pair, inc_src, N, F, swap, out, dyn_N, stream);
}

extern "C" int geossl_pair_position_grad_sparse(const float* pos, const float* pair_d, const float* dd,
                                                const int32_t* inc_ptr, const int32_t* inc_pair,
                                                const uint32_t* inc_src, int64_t N, int64_t P, int L, float* dpos,
                                                hipStream_t stream) {
  if (N <= 0) return 0;
  hipLaunchKernelGGL(k_pair_position_grad_sparse, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, stream, pos, pair_d, dd,
                     inc_ptr, inc_pair, inc_src, (int)N, P, L, dpos);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
