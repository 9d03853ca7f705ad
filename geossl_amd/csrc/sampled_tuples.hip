// Sampled atom tuples of a batch on the device: the reference's AtomTupleExtractor(ratio < 1)
// (Geom3D/dataloaders/dataloaders_AtomTuple.py:25-29; read by the reference's pretrain_GeoSSL.py:295 and
// pretrain_DistancePrediction.py:111) behind the gather of a capacity bucket.  The per-molecule count
// k_m = int(M_m * ratio) is a function of the sizes and stays host work (se_ptr); WHICH k_m of the M_m tuples are kept
// is data.  One block per molecule either draws them (the k_m smallest 64-bit Philox keys of
// the enumeration's slots, written in ascending slot order) or checks the list that is there (a collated batch's, a
// host-drawn one), and then builds the atom -> incident tuple lists of the heads for whatever list the molecule has:
// what geossl_incidence_count + an exclusive scan + geossl_incidence_fill (sides = 3) give, in one launch, with integer
// LDS counters only - the same bits every launch.  The rule is in include/geossl_hip.h (geossl_sampled_tuples).
#include "common.h"
#include "enumerate.h"
#include "geossl_hip.h"

using namespace geossl;

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_MAX_N = 255;        // atoms of a molecule: one thread per atom, local indices in a byte
constexpr int ST_KEYS = 4096;        // slots whose keys are kept in LDS (every molecule of up to 64 atoms, either option)
constexpr int ST_CHUNK = 4 * ST_KEYS;   // tuples staged per pass of the incidence fill (two bytes each: the same 32 KB)

__device__ __forceinline__ uint64_t slot_key(uint32_t s, uint32_t mol, uint64_t seed) {
  uint32_t w0, w1;
  philox_w01(s, mol, seed, w0, w1);
  return ((uint64_t)w0 << 32) | w1;
}

// inclusive scan over the block's 256 threads; total: the block's sum.  (wsum [4] is free again behind the call's last
// barrier only for a caller that puts a barrier before its next use - every caller here does.)
__device__ __forceinline__ int block_incl_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  v = wave_incl_scan(v);
  __syncthreads();
  if (lane == 63) wsum[wid] = v;
  __syncthreads();
  int add = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < ST_THREADS / 64; ++w) {
    add += w < wid ? wsum[w] : 0;
    tot += wsum[w];
  }
  total = tot;
  return v + add;
}

__global__ __launch_bounds__(ST_THREADS) void k_sampled_tuples(
    const int32_t* __restrict__ mol_ptr, const int32_t* __restrict__ se_ptr, int B, int option,
    const int32_t* __restrict__ mol_id, int draw, uint64_t seed, int N_cap, int S_cap, int64_t* sei0, int64_t* sei1,
    int64_t* __restrict__ inc_ptr, int32_t* __restrict__ inc_idx, int32_t* __restrict__ status) {
  // draw: the slots' keys; incidence fill: the staged tuples (uint16 each, read 16 bytes at a time)
  __shared__ __attribute__((aligned(16))) uint64_t keys[ST_KEYS];
  __shared__ int hist[ST_THREADS];
  __shared__ int deg[ST_THREADS];
  __shared__ int wsum[ST_THREADS / 64];
  __shared__ int sh_digit, sh_want;
  const int tid = threadIdx.x;
  const int m = blockIdx.x;
  const int a0 = mol_ptr[m], n = mol_ptr[m + 1] - a0;
  const int s0 = se_ptr[m], k = se_ptr[m + 1] - s0;
  const int M = n < 2 ? 0 : (option == 0 ? n * (n - 1) / 2 : n * (n - 1));
  // (uniform over the block.  The host sizes the buffers from the same numbers: a guard, not a path)
  if (a0 < 0 || n < 0 || n > ST_MAX_N || a0 + n > N_cap || s0 < 0 || k < 0 || s0 + k > S_cap || (draw && k > M)) {
    if (tid == 0 && status != nullptr) *status = 1;
    return;
  }
  // ---- draw: the k slots with the smallest (key, slot), in ascending slot order
  if (draw && k > 0) {
    const uint32_t mol = (uint32_t)mol_id[m];
    const bool in_lds = M <= ST_KEYS;
    if (in_lds)
      for (int s = tid; s < M; s += ST_THREADS) keys[s] = slot_key((uint32_t)s, mol, seed);
    // the k-th smallest key by a most-significant-digit radix select: eight passes over the keys, 8 bits each
    uint64_t prefix = 0;
    int want = k;
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      hist[tid] = 0;
      __syncthreads();   // (also: the keys above are written)
      for (int s = tid; s < M; s += ST_THREADS) {
        const uint64_t key = in_lds ? keys[s] : slot_key((uint32_t)s, mol, seed);
        if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(int)((key >> shift) & 255u)], 1);
      }
      __syncthreads();
      int total;
      const int h = hist[tid], incl = block_incl_scan(h, wsum, total);
      if (incl - h < want && want <= incl) {   // (one thread: the digit whose bin holds the want-th of the candidates)
        sh_digit = tid;
        sh_want = want - (incl - h);
      }
      __syncthreads();
      prefix |= (uint64_t)sh_digit << shift;
      want = sh_want;
      __syncthreads();   // (sh_* and hist are rewritten by the next pass)
    }
    // kept: key < prefix, and the first `want` slots with key == prefix.  Thread t owns the run of slots [t L, (t + 1) L)
    const int L = (M + ST_THREADS - 1) / ST_THREADS;
    const int r0 = min(M, tid * L), r1 = min(M, r0 + L);
    int n_less = 0, n_eq = 0;
    for (int s = r0; s < r1; ++s) {
      const uint64_t key = in_lds ? keys[s] : slot_key((uint32_t)s, mol, seed);
      n_less += key < prefix;
      n_eq += key == prefix;
    }
    int tot_less, tot_eq;
    const int less_before = block_incl_scan(n_less, wsum, tot_less) - n_less;
    int eq_seen = block_incl_scan(n_eq, wsum, tot_eq) - n_eq;
    int pos = less_before + min(eq_seen, want);
    for (int s = r0; s < r1; ++s) {
      const uint64_t key = in_lds ? keys[s] : slot_key((uint32_t)s, mol, seed);
      bool keep = key < prefix;
      if (key == prefix) keep = eq_seen++ < want;
      if (keep && pos < k) {
        int a, b;
        if (option == 0) pair_of_slot(s, n, a, b); else perm_of_slot(s, n, a, b);
        sei0[s0 + pos] = a0 + a;
        sei1[s0 + pos] = a0 + b;
        ++pos;
      }
    }
    __threadfence_block();
  }
  __syncthreads();   // (the molecule's tuples are in sei; the keys are dead)
  // ---- the atoms' degrees over the molecule's k tuples (both ends count); a tuple that leaves the molecule is reported
  deg[tid] = 0;
  __syncthreads();
  bool bad = false;
  for (int t = tid; t < k; t += ST_THREADS) {
    const int64_t u = sei0[s0 + t] - a0, v = sei1[s0 + t] - a0;
    if (u >= 0 && u < n && v >= 0 && v < n && u != v) {
      atomicAdd(&deg[(int)u], 1);
      atomicAdd(&deg[(int)v], 1);
    } else {
      bad = true;
    }
  }
  if (bad && status != nullptr) *status = 1;
  __syncthreads();
  if (inc_ptr == nullptr) return;
  int total;
  const int d = deg[tid];
  const int64_t base = 2 * (int64_t)s0 + (block_incl_scan(d, wsum, total) - d);
  if (tid < n) inc_ptr[a0 + tid] = base;
  if (m == B - 1 && tid == 0) inc_ptr[a0 + n] = 2 * ((int64_t)s0 + k);
  if (inc_idx == nullptr) return;
  // (a refused list: the entries its dropped tuples would have had name the molecule's first tuple - nothing stale)
  for (int f = total + tid; f < 2 * k; f += ST_THREADS) inc_idx[2 * (int64_t)s0 + f] = s0;
  // ---- atom -> incident tuples in ascending tuple order: the tuples staged in LDS chunk by chunk, one thread per atom
  uint16_t* ends = reinterpret_cast<uint16_t*>(keys);
  int cur = 0;
  for (int c0 = 0; c0 < k; c0 += ST_CHUNK) {
    const int cn = min(ST_CHUNK, k - c0);
    __syncthreads();   // (the previous chunk has been walked)
    for (int t = tid; t < cn; t += ST_THREADS) {
      const int64_t u = sei0[s0 + c0 + t] - a0, v = sei1[s0 + c0 + t] - a0;
      const bool ok = u >= 0 && u < n && v >= 0 && v < n && u != v;
      ends[t] = ok ? (uint16_t)((int)u | ((int)v << 8)) : (uint16_t)0xFFFFu;   // (255 is no atom: n <= 255)
    }
    __syncthreads();
    if (tid < n) {   // (eight staged tuples per 16-byte LDS read: the walk is bound by the latency of its reads)
      const ulonglong2* ends8 = reinterpret_cast<const ulonglong2*>(keys);
      const int full = cn >> 3;
      for (int q = 0; q < full; ++q) {
        const ulonglong2 w = ends8[q];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int e = (int)(((j < 4 ? w.x : w.y) >> (16 * (j & 3))) & 0xFFFFull);
          if ((e & 255) == tid || (e >> 8) == tid) inc_idx[base + cur++] = s0 + c0 + 8 * q + j;
        }
      }
      for (int t = full << 3; t < cn; ++t) {
        const int e = ends[t];
        if ((e & 255) == tid || (e >> 8) == tid) inc_idx[base + cur++] = s0 + c0 + t;
      }
    }
  }
}

}  // namespace

extern "C" int geossl_sampled_tuples(const int32_t* mol_ptr, const int32_t* se_ptr, int64_t B, int option,
                                     const int32_t* mol_id, int draw, uint64_t seed, int64_t N_cap, int64_t S_cap,
                                     int64_t* sei0, int64_t* sei1, int64_t* inc_ptr, int32_t* inc_idx, int32_t* status,
                                     hipStream_t stream) {
  if (B < 0 || B > (1 << 24) || (option != 0 && option != 1) || N_cap < 0 || S_cap < 0 || N_cap >= ((int64_t)1 << 31) ||
      2 * S_cap >= ((int64_t)1 << 31))
    return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  if (mol_ptr == nullptr || se_ptr == nullptr || sei0 == nullptr || sei1 == nullptr || (draw && mol_id == nullptr) ||
      (inc_idx != nullptr && inc_ptr == nullptr))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sampled_tuples, dim3((unsigned)B), dim3(ST_THREADS), 0, stream, mol_ptr, se_ptr, (int)B, option,
                     mol_id, draw ? 1 : 0, seed, (int)N_cap, (int)S_cap, sei0, sei1, inc_ptr, inc_idx, status);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
