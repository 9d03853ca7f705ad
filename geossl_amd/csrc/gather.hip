// Batch assembly on the device from a device-resident dataset of molecules.
//
// The reference's loader (examples/pretrain_GeoSSL.py:295-301: DataLoaderAtomTuple(dataset, batch_size, shuffle=True))
// collates a random subset of molecules on the host every step: BatchAtomTuple.from_data_list concatenates x /
// positions, writes batch = full((n_i,), i) and adds the cumulative node offset to super_edge_index /
// radius_edge_index (Geom3D/dataloaders/dataloaders_AtomTuple.py:46-73), after AtomTupleExtractor enumerated the atom
// tuples per molecule (:15-37).  Here the molecules live in HBM (concatenated x / positions, for PaiNN the concatenated
// per-molecule radius_edge_index of datasets_3D_Radius.py:120) and ONE launch writes a permutation slice straight into
// the static inputs of a replayed step graph: one block per chosen molecule
//   * gathers its atom rows (x, positions) and writes the batch vector,
//   * enumerates its super-edges (itertools.combinations / permutations order, node offset added) - the tuples are a
//     function of the atom count, nothing is read,
//   * writes the pair-slot atoms of the two-view batch (what geossl_pair_index_fill produces) and the atom -> incident
//     super-edge lists of the heads (what geossl_incidence_fill finds by searching; here in closed form),
//   * copies its radius edges with the node offset changed from the dataset's to the batch's;
// the blocks behind the last molecule clear a float buffer (the owner's flat gradient buffer).  All offsets come from
// the host's size table (cumulative sums over B integers, uploaded with the step's other pointer arrays): no read-back.
// HBM-bound integer work: a few hundred KB per step, one wave-coalesced store stream per array.
#include "common.h"
#include "enumerate.h"
#include "geossl_hip.h"

using namespace geossl;

namespace {

constexpr int GATHER_THREADS = 256;

// the blocks behind the molecules clear the float buffer
__device__ __forceinline__ void clear_zero_block(const GeosslGather& g, int B) {
  const int tid = threadIdx.x;
  if (g.zero == nullptr) return;
  const int64_t nb = (int64_t)gridDim.x - B;
  const int64_t t0 = ((int64_t)blockIdx.x - B) * GATHER_THREADS + tid, nt = nb * GATHER_THREADS;
  const int64_t n4 = g.zero_count >> 2;
  f32x4* z4 = reinterpret_cast<f32x4*>(g.zero);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  if ((reinterpret_cast<uintptr_t>(g.zero) & 15) == 0) {
    for (int64_t i = t0; i < n4; i += nt) z4[i] = zero4;
    for (int64_t i = (n4 << 2) + t0; i < g.zero_count; i += nt) g.zero[i] = 0.f;
  } else {
    for (int64_t i = t0; i < g.zero_count; i += nt) g.zero[i] = 0.f;
  }
}

// The index structures of molecule m (n atoms from batch row a0 on) that are a function of n alone: pair slots of the
// two-view batch, super-edges, incidence lists.  Shared by the whole-molecule and the masked gather.
__device__ __forceinline__ void gather_structures(const GeosslGather& g, int B, int m, int a0, int n) {
  const int tid = threadIdx.x;
  const int P = n * (n - 1) / 2;
  // ---- pair slots of the two-view batch (geossl_pair_index_fill) and, for "combination", the super-edges
  const bool comb_sei = g.sei0 != nullptr && g.option == 0;
  if (g.pair_i != nullptr || comb_sei) {
    const int N1 = g.mol_ptr[B];
    const int pp0 = g.pair_i != nullptr ? g.pair_ptr2[m] : 0, pp1 = g.pair_i != nullptr ? g.pair_ptr2[B + m] : 0;
    const int64_t se0 = comb_sei ? (int64_t)g.se_ptr[m] : 0;
    for (int p = tid; p < P; p += GATHER_THREADS) {
      int a, b;
      pair_of_slot(p, n, a, b);
      if (g.pair_i != nullptr) {
        g.pair_i[pp0 + p] = a0 + a;
        g.pair_j[pp0 + p] = a0 + b;
        g.pair_i[pp1 + p] = N1 + a0 + a;
        g.pair_j[pp1 + p] = N1 + a0 + b;
      }
      if (comb_sei) {
        g.sei0[se0 + p] = a0 + a;
        g.sei1[se0 + p] = a0 + b;
      }
    }
  }
  if (g.sei0 != nullptr && g.option == 1) {  // itertools.permutations order: (a, b), b != a, column a (n - 1) + (b < a ? b : b - 1)
    const int64_t se0 = g.se_ptr[m];
    for (int q = tid; q < 2 * P; q += GATHER_THREADS) {
      const int a = q / (n - 1), r = q - a * (n - 1), b = r < a ? r : r + 1;
      g.sei0[se0 + q] = a0 + a;
      g.sei1[se0 + q] = a0 + b;
    }
  }
  // ---- atom -> incident super-edges, ordered by super-edge id (geossl_incidence_fill, sides = 3)
  if (g.inc_idx != nullptr && n > 1) {
    const int se0 = g.se_ptr[m];
    const int64_t base = g.inc_ptr[a0];
    if (g.option == 0) {
      const int cnt = n - 1;           // atom k lies on (e, k) for e < k, then on (k, e + 1) for e >= k
      for (int f = tid; f < n * cnt; f += GATHER_THREADS) {
        const int k = f / cnt, e = f - k * cnt;
        const int a = e < k ? e : k, b = e < k ? k : e + 1;
        g.inc_idx[base + f] = se0 + a * n - a * (a + 1) / 2 - a - 1 + b;
      }
    } else {
      const int cnt = 2 * (n - 1);     // (e, k) for e < k; the n - 1 tuples (k, .); (e', k) for e' > k
      for (int f = tid; f < n * cnt; f += GATHER_THREADS) {
        const int k = f / cnt, e = f - k * cnt;
        int id;
        if (e < k) id = e * (n - 1) + k - 1;
        else if (e < k + n - 1) id = k * (n - 1) + (e - k);
        else id = (e - (n - 1) + 1) * (n - 1) + k;
        g.inc_idx[base + f] = se0 + id;
      }
    }
  }
}

__global__ __launch_bounds__(GATHER_THREADS) void k_gather_molecules(GeosslGather g, int B) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= B) {
    clear_zero_block(g, B);
    return;
  }
  const int m = blockIdx.x;
  const int a0 = g.mol_ptr[m], n = g.mol_ptr[m + 1] - a0;
  const int64_t s0 = g.src_off[m];
  // ---- atom rows
  {
    const int C = g.x_cols;
    const int64_t* xs = g.x_src + s0 * C;
    int64_t* xd = g.x_dst + (int64_t)a0 * C;
    for (int i = tid; i < n * C; i += GATHER_THREADS) xd[i] = xs[i];
    const float* ps = g.pos_src + s0 * 3;
    float* pd = g.pos_dst + (int64_t)a0 * 3;
    for (int i = tid; i < n * 3; i += GATHER_THREADS) pd[i] = ps[i];
    if (g.batch_dst != nullptr)
      for (int i = tid; i < n; i += GATHER_THREADS) g.batch_dst[a0 + i] = m;
  }
  gather_structures(g, B, m, a0, n);
  // ---- radius edges of the molecule: the dataset's node offset replaced by the batch's
  if (g.e0_dst != nullptr) {
    const int d0 = g.e_ptr[m], cnt = g.e_ptr[m + 1] - d0;
    const int64_t es = g.e_src_off[m];
    const int64_t shift = (int64_t)a0 - s0;
    for (int i = tid; i < cnt; i += GATHER_THREADS) {
      g.e0_dst[d0 + i] = g.e0_src[es + i] + shift;
      g.e1_dst[d0 + i] = g.e1_src[es + i] + shift;
    }
  }
}

// ---- masked gather (BFS atom masking of datasets_3D.py:24-67 / datasets_3D_Radius.py:43-87)
constexpr int MASK_MAX_N = 2048;   // 64 lanes x one 32-bit word of the visited / frontier bitsets

// position of the r-th set bit (0-based) of w
__device__ __forceinline__ int select_bit(uint32_t w, int r) {
  int pos = 0;
#pragma unroll
  for (int s = 16; s > 0; s >>= 1) {
    const uint32_t lo = w & ((1u << s) - 1u);
    const int c = __popc(lo);
    if (r >= c) {
      r -= c;
      w >>= s;
      pos += s;
    } else {
      w = lo;
    }
  }
  return pos;
}

// the r-th member (ascending) of the set whose lane words are w, incl = inclusive scan of their popcounts; uniform
__device__ __forceinline__ int wave_pick(uint32_t w, int r, int incl) {
  const int excl = incl - __popc(w);
  const uint64_t hit = __ballot(r >= excl && r < incl);
  const int L = __builtin_ctzll(hit);
  return __shfl(__lane_id() * 32 + select_bit(w, r - excl), L);
}

// kept atoms (ascending local indices) of molecule m drawn by wave 0: lane l owns atoms 32 l .. 32 l + 31
__device__ void bfs_draw(const GeosslMask& mk, int m, int64_t s0, int n, int k, uint32_t* kbits) {
  const int lane = __lane_id();
  const int lo = lane * 32;
  const uint32_t valid = lo >= n ? 0u : (n - lo >= 32 ? ~0u : ((1u << (n - lo)) - 1u));
  const uint32_t c0 = (uint32_t)mk.mol_id[m];
  uint32_t vis = 0, fr = 0;
  int atom = (int)(((uint64_t)philox_w0(c0, 0u, mk.seed) * (uint32_t)n) >> 32);
  for (int t = 1;; ++t) {
    if ((atom >> 5) == lane) vis |= 1u << (atom & 31);
    const int e0 = mk.bond_ptr[s0 + atom], e1 = mk.bond_ptr[s0 + atom + 1];
    for (int j = e0; j < e1; j += 64) {
      const int v = j + lane < e1 ? mk.bond_dst[j + lane] : -1;
      const int cnt = min(64, e1 - j);
      for (int q = 0; q < cnt; ++q) {
        const int u = __builtin_amdgcn_readlane(v, q);
        if ((unsigned)u < (unsigned)n && (u >> 5) == lane) fr |= 1u << (u & 31);
      }
    }
    fr &= ~vis;
    if (t == k) break;
    const int fc = wave_incl_scan(__popc(fr));
    const int ftot = __shfl(fc, 63);
    const uint32_t w = philox_w0(c0, (uint32_t)t, mk.seed);
    if (ftot > 0) {
      atom = wave_pick(fr, (int)(((uint64_t)w * (uint32_t)ftot) >> 32), fc);
    } else {
      const uint32_t un = valid & ~vis;
      atom = wave_pick(un, (int)(((uint64_t)w * (uint32_t)(n - t)) >> 32), wave_incl_scan(__popc(un)));
    }
  }
  kbits[lane] = vis;
}

__global__ __launch_bounds__(GATHER_THREADS) void k_gather_masked(GeosslGather g, GeosslMask mk, int B) {
  __shared__ int keep[MASK_MAX_N];
  __shared__ uint32_t kbits[64];
  __shared__ int kpre[64];
  __shared__ int wsum[GATHER_THREADS / 64];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= B) {
    clear_zero_block(g, B);
    return;
  }
  const int m = blockIdx.x;
  const int a0 = g.mol_ptr[m], k = g.mol_ptr[m + 1] - a0;
  const int n = mk.src_n[m];
  const int64_t s0 = g.src_off[m];
  if (n > MASK_MAX_N || k < 1 || k > n) return;   // (uniform over the block)
  const bool count_only = mk.e_count != nullptr;
  // ---- the kept bitset
  if (mk.keep_in != nullptr) {
    if (tid < 64) kbits[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < k; i += GATHER_THREADS) {
      const int v = mk.keep_in[a0 + i];
      if ((unsigned)v < (unsigned)n) atomicOr(&kbits[v >> 5], 1u << (v & 31));
    }
    __syncthreads();
  } else {
    if (tid < 64) bfs_draw(mk, m, s0, n, k, kbits);
    __syncthreads();
  }
  // ---- rank prefix per word and the kept list
  if (tid < 64) {
    const uint32_t w = kbits[tid];
    int pos = wave_incl_scan(__popc(w)) - __popc(w);
    kpre[tid] = pos;
    if (mk.keep_in == nullptr)
      for (uint32_t r = w; r != 0u; r &= r - 1u) keep[pos++] = tid * 32 + __builtin_ctz(r);
  }
  if (mk.keep_in != nullptr)
    for (int i = tid; i < k; i += GATHER_THREADS) {
      const int v = mk.keep_in[a0 + i];
      keep[i] = (unsigned)v < (unsigned)n ? v : 0;
    }
  __syncthreads();
  if (mk.keep_out != nullptr)
    for (int i = tid; i < k; i += GATHER_THREADS) mk.keep_out[a0 + i] = keep[i];
  if (!count_only) {
    // ---- atom rows: destination row i <- source row s0 + keep[i]
    const int C = g.x_cols;
    const int64_t* xs = g.x_src + s0 * C;
    int64_t* xd = g.x_dst + (int64_t)a0 * C;
    for (int i = tid; i < k * C; i += GATHER_THREADS) {
      const int r = i / C;
      xd[i] = xs[(int64_t)keep[r] * C + (i - r * C)];
    }
    const float* ps = g.pos_src + s0 * 3;
    float* pd = g.pos_dst + (int64_t)a0 * 3;
    for (int i = tid; i < k * 3; i += GATHER_THREADS) {
      const int r = i / 3;
      pd[i] = ps[(int64_t)keep[r] * 3 + (i - r * 3)];
    }
    if (g.batch_dst != nullptr)
      for (int i = tid; i < k; i += GATHER_THREADS) g.batch_dst[a0 + i] = m;
    gather_structures(g, B, m, a0, k);
  }
  // ---- radius edges: both ends kept, in edge order, renumbered by rank (a block-wide ballot scan)
  if (count_only ? g.e0_src != nullptr : g.e0_dst != nullptr) {
    const int64_t es = g.e_src_off[m];
    const int cnt = mk.e_src_cnt[m];
    const int d0 = count_only ? 0 : g.e_ptr[m], dcap = count_only ? 0 : g.e_ptr[m + 1] - d0;
    const int lane = tid & 63, wid = tid >> 6;
    int base = 0;
    for (int i0 = 0; i0 < cnt; i0 += GATHER_THREADS) {
      const int i = i0 + tid;
      bool keep_e = false;
      int na = 0, nb = 0;
      if (i < cnt) {
        const int64_t u = g.e0_src[es + i] - s0, v = g.e1_src[es + i] - s0;
        if (u >= 0 && u < n && v >= 0 && v < n) {
          const uint32_t wu = kbits[u >> 5], wv = kbits[v >> 5];
          const uint32_t bu = 1u << (u & 31), bv = 1u << (v & 31);
          if ((wu & bu) && (wv & bv)) {
            keep_e = true;
            na = kpre[u >> 5] + __popc(wu & (bu - 1u));
            nb = kpre[v >> 5] + __popc(wv & (bv - 1u));
          }
        }
      }
      const uint64_t bal = __ballot(keep_e);
      if (lane == 0) wsum[wid] = __popcll(bal);
      __syncthreads();
      int off = base, tot = 0;
#pragma unroll
      for (int w = 0; w < GATHER_THREADS / 64; ++w) {
        off += w < wid ? wsum[w] : 0;
        tot += wsum[w];
      }
      off += __popcll(bal & ((1ull << lane) - 1ull));
      if (keep_e && !count_only && off < dcap) {
        g.e0_dst[d0 + off] = a0 + na;
        g.e1_dst[d0 + off] = a0 + nb;
      }
      base += tot;
      __syncthreads();   // (wsum is rewritten by the next chunk)
    }
    if (count_only && tid == 0) mk.e_count[m] = base;
  } else if (count_only && tid == 0) {
    mk.e_count[m] = 0;
  }
}

// ---- edge offsets of a masked batch on the device: the exclusive prefix of the count launch's survivors per molecule.
// One block; B is scanned in chunks of the block's threads with a carry.  Every offset is clamped to E_cap (the gather
// and the edge layout behind this launch never leave the capacity-sized buffers) and the status word reports a total
// above it - the caller sizes E_cap from a host-side upper bound, so that is a guard and not a path.
__global__ __launch_bounds__(GATHER_THREADS) void k_masked_edge_offsets(const int32_t* __restrict__ e_count, int B,
                                                                         int E_cap, int views, int32_t* __restrict__ e_ptr,
                                                                         int32_t* __restrict__ dyn_E2,
                                                                         int32_t* __restrict__ status) {
  __shared__ long long part[GATHER_THREADS];
  const int tid = threadIdx.x;
  long long carry = 0;
  bool bad = false;
  for (int i0 = 0; i0 < B; i0 += GATHER_THREADS) {
    const int i = i0 + tid;
    int c = i < B ? e_count[i] : 0;
    if (c < 0) {   // (a molecule the count launch skipped leaves what was there)
      c = 0;
      bad = true;
    }
    part[tid] = c;
    __syncthreads();
    for (int o = 1; o < GATHER_THREADS; o <<= 1) {   // inclusive Hillis-Steele scan
      const long long a = tid >= o ? part[tid - o] : 0;
      __syncthreads();
      part[tid] += a;
      __syncthreads();
    }
    const long long incl = carry + part[tid];
    if (i < B) e_ptr[i + 1] = (int32_t)(incl < (long long)E_cap ? incl : (long long)E_cap);
    carry += part[GATHER_THREADS - 1];
    __syncthreads();   // (part is rewritten by the next chunk)
  }
  if (tid == 0) {
    const long long E = carry < (long long)E_cap ? carry : (long long)E_cap;
    e_ptr[0] = 0;
    *dyn_E2 = (int32_t)(views * E);
    if (carry > (long long)E_cap) bad = true;
  }
  if (bad && status != nullptr) *status = 1;
}

}  // namespace

extern "C" int geossl_gather_molecules(const GeosslGather* g, int64_t B, hipStream_t stream) {
  if (g == nullptr || B < 0 || B > (1 << 24)) return (int)hipErrorInvalidValue;
  if (B > 0 && (g->x_src == nullptr || g->pos_src == nullptr || g->src_off == nullptr || g->mol_ptr == nullptr ||
                g->x_dst == nullptr || g->pos_dst == nullptr || g->x_cols < 1 || (g->option != 0 && g->option != 1)))
    return (int)hipErrorInvalidValue;
  if ((g->sei0 != nullptr) != (g->sei1 != nullptr) || (g->pair_i != nullptr) != (g->pair_j != nullptr) ||
      (g->e0_dst != nullptr) != (g->e1_dst != nullptr))
    return (int)hipErrorInvalidValue;
  if ((g->sei0 != nullptr || g->inc_idx != nullptr) && g->se_ptr == nullptr) return (int)hipErrorInvalidValue;
  if (g->pair_i != nullptr && g->pair_ptr2 == nullptr) return (int)hipErrorInvalidValue;
  if (g->inc_idx != nullptr && g->inc_ptr == nullptr) return (int)hipErrorInvalidValue;
  if (g->e0_dst != nullptr && (g->e0_src == nullptr || g->e1_src == nullptr || g->e_src_off == nullptr || g->e_ptr == nullptr))
    return (int)hipErrorInvalidValue;
  if (g->zero_count < 0 || (g->zero == nullptr && g->zero_count > 0) || (reinterpret_cast<uintptr_t>(g->zero) & 3))
    return (int)hipErrorInvalidValue;
  int zero_blocks = 0;
  if (g->zero != nullptr && g->zero_count > 0) {
    const int64_t want = (g->zero_count / 4 + GATHER_THREADS - 1) / GATHER_THREADS;   // one float4 per thread and trip
    zero_blocks = (int)(want < 1 ? 1 : (want > 256 ? 256 : want));
  }
  if (B + zero_blocks == 0) return 0;
  hipLaunchKernelGGL(k_gather_molecules, dim3((unsigned)(B + zero_blocks)), dim3(GATHER_THREADS), 0, stream, *g, (int)B);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}


extern "C" int geossl_gather_masked_molecules(const GeosslGather* g, const GeosslMask* mk, int64_t B, hipStream_t stream) {
  if (g == nullptr || mk == nullptr || B < 0 || B > (1 << 24)) return (int)hipErrorInvalidValue;
  if (B == 0) return geossl_gather_molecules(g, 0, stream);   // (nothing to mask: only the buffer to clear)
  if (mk->max_n < 1 || mk->max_n > MASK_MAX_N || mk->src_n == nullptr || g->src_off == nullptr || g->mol_ptr == nullptr)
    return (int)hipErrorInvalidValue;
  if (mk->keep_in == nullptr && (mk->bond_ptr == nullptr || mk->bond_dst == nullptr || mk->mol_id == nullptr))
    return (int)hipErrorInvalidValue;
  if (mk->e_count != nullptr) {   // the count launch: kept lists and surviving radius edges only
    if (mk->keep_out == nullptr) return (int)hipErrorInvalidValue;
    if (g->e0_src != nullptr && (g->e1_src == nullptr || g->e_src_off == nullptr || mk->e_src_cnt == nullptr))
      return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gather_masked, dim3((unsigned)B), dim3(GATHER_THREADS), 0, stream, *g, *mk, (int)B);
    GEOSSL_CHECK_LAUNCH();
    return 0;
  }
  if (g->x_src == nullptr || g->pos_src == nullptr || g->x_dst == nullptr || g->pos_dst == nullptr || g->x_cols < 1 ||
      (g->option != 0 && g->option != 1))
    return (int)hipErrorInvalidValue;
  if ((g->sei0 != nullptr) != (g->sei1 != nullptr) || (g->pair_i != nullptr) != (g->pair_j != nullptr) ||
      (g->e0_dst != nullptr) != (g->e1_dst != nullptr))
    return (int)hipErrorInvalidValue;
  if ((g->sei0 != nullptr || g->inc_idx != nullptr) && g->se_ptr == nullptr) return (int)hipErrorInvalidValue;
  if (g->pair_i != nullptr && g->pair_ptr2 == nullptr) return (int)hipErrorInvalidValue;
  if (g->inc_idx != nullptr && g->inc_ptr == nullptr) return (int)hipErrorInvalidValue;
  if (g->e0_dst != nullptr && (g->e0_src == nullptr || g->e1_src == nullptr || g->e_src_off == nullptr ||
                               g->e_ptr == nullptr || mk->e_src_cnt == nullptr))
    return (int)hipErrorInvalidValue;
  if (g->zero_count < 0 || (g->zero == nullptr && g->zero_count > 0) || (reinterpret_cast<uintptr_t>(g->zero) & 3))
    return (int)hipErrorInvalidValue;
  int zero_blocks = 0;
  if (g->zero != nullptr && g->zero_count > 0) {
    const int64_t want = (g->zero_count / 4 + GATHER_THREADS - 1) / GATHER_THREADS;
    zero_blocks = (int)(want < 1 ? 1 : (want > 256 ? 256 : want));
  }
  hipLaunchKernelGGL(k_gather_masked, dim3((unsigned)(B + zero_blocks)), dim3(GATHER_THREADS), 0, stream, *g, *mk, (int)B);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_masked_edge_offsets(const int32_t* e_count, int64_t B, int64_t E_cap, int views, int32_t* e_ptr,
                                          int32_t* dyn_E2, int32_t* status, hipStream_t stream) {
  if (B <= 0 || B > (1 << 24) || e_count == nullptr || e_ptr == nullptr || dyn_E2 == nullptr || E_cap < 0 ||
      2 * E_cap >= ((int64_t)1 << 30) || (views != 1 && views != 2))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_masked_edge_offsets, dim3(1), dim3(GATHER_THREADS), 0, stream, e_count, (int)B, (int)E_cap, views,
                     e_ptr, dyn_E2, status);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
