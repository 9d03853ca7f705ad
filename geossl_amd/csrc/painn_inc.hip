// Both incidence lists of a collated one-view radius_edge_index (what layout.EdgeLayout.inc holds: the edges grouped by
// idx_i = row 0, the forward's scatter target, and by idx_j = row 1, the backward's; an atom's edges in ascending edge
// order) for structures of up to 1024 atoms, in ONE launch whose grid depends on capacities alone - the per-step rewrite
// of a sparse PaiNN bucket's edge part (geossl_amd/bucket.py), where k_painn_edge_layout (one block per molecule, at most
// 256 atoms, plus a group layout the atom-tile kernels do not read) stops.
//
// A 256-thread block owns (structure, slice of PI_APB = 16 atoms), so a 500-atom pocket is 32 blocks and not one:
//   * the structure's edge range [e0, e1) by the 256-ary search over the first row (edge_search.h): a collated batch
//     needs no host-side edge counts;
//   * the per-atom edge counts of the WHOLE structure on both sides by integer LDS atomics (counts only: their order
//     reaches no output), 1024 atoms x 2 sides x 4 B of LDS, and their exclusive scan by the block.  Every block of a
//     structure repeats this (Em / 256 rounds per thread) rather than wait for a scan launch: a structure's lists start
//     at e0, so no block needs anything from another;
//   * placement as a stable counting sort over (wave, atom of the slice): every wave takes a contiguous quarter of the
//     range (the same quarter in the counting pass, which also counts the slice's atoms per quarter), so an atom's slots
//     of quarter w lie behind those of the quarters before it; a wave streams its quarter in ascending order, 64 edges
//     per round with the next round's loads in flight, and ranks the round's edges of one atom by a ballot - one round
//     of ballots per DISTINCT atom of the slice among the 64 edges (64 * 16 / n edges of a round hit the slice on the
//     by-source side: two at 500 atoms), not per key of the structure.
// Integer work only; bit-reproducible.  An edge with an end outside its structure is left out and sets *status; the slots
// such edges leave free at the end of their structure's span get the span's first edge id, so that a kernel queued
// before the status word is read stays inside the edge arrays.
#include "common.h"
#include "edge_search.h"
#include "geossl_hip.h"

#include <algorithm>
#include <climits>

using namespace geossl;

namespace {

constexpr int PI_MAXN = GEOSSL_PAINN_INC_MAX_N;  // atoms per structure
constexpr int PI_APB = 16;                       // atoms per block (its slice of the structure)

struct PainnIncArgs {
  const int64_t* src_i;    // [E] row 0 of radius_edge_index
  const int64_t* src_j;    // [E] row 1
  const int32_t* mol_ptr;  // [B + 1]
  int E, N, B, max_n, slices;   // E, N: the capacities of the `_dyn` entry
  int64_t* iptr_i;         // [N + 1]
  int32_t* ilist_i;        // [E]
  int64_t* iptr_j;
  int32_t* ilist_j;
  int32_t* status;
  const int32_t* dyn_E;
  const int32_t* dyn_N;
};

template <bool DYN>
__global__ __launch_bounds__(256) void k_painn_incidence_layout(PainnIncArgs A) {
  __shared__ int cnt[2][PI_MAXN];   // per atom of the structure: edges by idx_i / idx_j, then their exclusive prefixes
  __shared__ int part[2][256];
  __shared__ int qrun[2][4][PI_APB];   // per (side, wave, atom of the slice): edges in the wave's quarter; then its next slot
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = (int)blockIdx.x / A.slices, first = ((int)blockIdx.x % A.slices) * PI_APB;
  const bool lead = first == 0;    // the structure's first block: status checks, the free slots, the tail of iptr
  int E = A.E, N = A.N;
  if (DYN) {  // real counts from device memory, uniform over the grid, clamped into the capacities
    const int gotE = *A.dyn_E, gotN = *A.dyn_N;
    E = min(max(gotE, 0), A.E);
    N = min(max(gotN, 0), A.N);
    if ((E != gotE || N != gotN) && tid == 0) *A.status = 1;
  }
  const int a0 = A.mol_ptr[m];
  int n = A.mol_ptr[m + 1] - a0;
  const bool inside = a0 >= 0 && n >= 0 && (int64_t)a0 + n <= N;   // (no write outside iptr on a broken mol_ptr)
  if (!inside) n = 0;
  const bool too_big = n > A.max_n;
  const int nn = too_big ? 0 : n;  // (a structure above the limit gets empty lists; the status word reports it)
  if (!lead && first >= nn) return;
  int e0, e1;
  block_lower_bound2(A.src_i, E, (int64_t)a0, (int64_t)a0 + n, e0, e1);
  if (lead && tid == 0) {
    // The structures' ranges share their ends (the same key, the same search), so they tile [e0 of the first, e1 of the
    // last): a list that is not grouped by structure in batch order leaves edges outside that span or inside a wrong
    // structure's range (caught by the histogram).
    if (!inside || too_big || (m == 0 && e0 != 0) || (m == A.B - 1 && (e1 != E || a0 + n != N))) *A.status = 1;
  }
  if (lead && m == A.B - 1)  // the lists end here; atoms past the real count (a capacity) have none
    for (int a = N + tid; a <= A.N; a += 256) {
      A.iptr_i[a] = E;
      A.iptr_j[a] = E;
    }
  if (lead && too_big)
    for (int t = tid; t < n; t += 256) {
      A.iptr_i[a0 + t] = e0;
      A.iptr_j[a0 + t] = e0;
    }
  // ---- counts per atom of the whole structure, both sides; wave w counts quarter w of the range, and the slice's atoms
  // per quarter on the side
  for (int i = tid; i < 2 * PI_MAXN; i += 256) (&cnt[0][0])[i] = 0;
  if (tid < 2 * 4 * PI_APB) (&qrun[0][0][0])[tid] = 0;
  __syncthreads();
  const int Em = e1 - e0, Q = (Em + 3) >> 2;   // (e0 <= e1: the search is monotone in its key)
  const int q0 = e0 + min(Em, wave * Q), q1 = e0 + min(Em, (wave + 1) * Q);
  int bad = 0;
#pragma unroll 4
  for (int e = q0 + lane; e < q1; e += 64) {
    const int64_t li = A.src_i[e] - a0, lj = A.src_j[e] - a0;
    if (li < 0 || li >= nn || lj < 0 || lj >= nn) {
      bad = 1;
    } else {
      atomicAdd(&cnt[0][(int)li], 1);
      atomicAdd(&cnt[1][(int)lj], 1);
      const unsigned si = (unsigned)((int)li - first), sj = (unsigned)((int)lj - first);
      if (si < (unsigned)PI_APB) atomicAdd(&qrun[0][wave][si], 1);
      if (sj < (unsigned)PI_APB) atomicAdd(&qrun[1][wave][sj], 1);
    }
  }
  if (bad && lead) *A.status = 1;
  __syncthreads();
  // ---- exclusive scan over the atoms: four consecutive atoms per thread, Hillis-Steele over the threads' sums
  int c[2][4], s[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    s[q] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c[q][k] = cnt[q][4 * tid + k];
      s[q] += c[q][k];
    }
    part[q][tid] = s[q];
  }
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int ai = tid >= o ? part[0][tid - o] : 0, aj = tid >= o ? part[1][tid - o] : 0;
    __syncthreads();
    part[0][tid] += ai;
    part[1][tid] += aj;
    __syncthreads();
  }
  const int kept = part[0][255];   // edges with both ends inside (the same number on either side)
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    int x = part[q][tid] - s[q];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      cnt[q][4 * tid + k] = x;
      x += c[q][k];
    }
  }
  __syncthreads();
  if (lead)  // the slots that left-out edges leave free at the end of the span
    for (int t = e0 + kept + tid; t < e1; t += 256) {
      A.ilist_i[t] = e0;
      A.ilist_j[t] = e0;
    }
  // ---- the slice's atoms: first slot of the atom (iptr), then of every quarter's share of its list
  if (tid < 2 * PI_APB) {
    const int side = tid / PI_APB, k = tid % PI_APB, la = first + k;
    if (la < nn) {
      int slot = e0 + cnt[side][la];
      (side == 0 ? A.iptr_i : A.iptr_j)[a0 + la] = slot;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int t = qrun[side][w][k];
        qrun[side][w][k] = slot;
        slot += t;
      }
    }
  }
  __syncthreads();
  // ---- placement: the wave's quarter in ascending edge order, 64 edges per round.  An edge's slot = its atom's next free
  // slot for this wave + its rank among the round's edges of the same atom (a ballot of the lanes that hold the atom).
  volatile int* run_i = qrun[0][wave];
  volatile int* run_j = qrun[1][wave];
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  auto load = [&](int c0, int64_t& gi, int64_t& gj) {
    const int e = c0 + lane;
    gi = gj = -1;
    if (e < q1) {
      gi = A.src_i[e] - a0;
      gj = A.src_j[e] - a0;
    }
  };
  auto place = [&](int key, volatile int* run, int32_t* list, int e) {   // key: atom of the slice, -1: none
    unsigned long long rem = __ballot(key >= 0);
    while (rem) {
      const int k = __builtin_amdgcn_readlane(key, __builtin_ctzll(rem));
      const unsigned long long mk = __ballot(key == k);
      const int base = run[k];
      if (key == k) list[base + __popcll(mk & lt)] = e;
      if (lane == 0) run[k] = base + __popcll(mk);
      rem &= ~mk;
    }
  };
  int64_t ni, nj;
  load(q0, ni, nj);
  for (int c0 = q0; c0 < q1; c0 += 64) {
    const int64_t gi = ni, gj = nj;
    if (c0 + 64 < q1) load(c0 + 64, ni, nj);
    int ki = -1, kj = -1;
    if (gi >= 0 && gi < nn && gj >= 0 && gj < nn) {   // (an edge that leaves its structure is on neither list)
      const unsigned si = (unsigned)((int)gi - first), sj = (unsigned)((int)gj - first);
      if (si < (unsigned)PI_APB) ki = (int)si;
      if (sj < (unsigned)PI_APB) kj = (int)sj;
    }
    place(ki, run_i, A.ilist_i, c0 + lane);
    place(kj, run_j, A.ilist_j, c0 + lane);
  }
}

int launch_incidence_layout(const int64_t* src_i, const int64_t* src_j, int64_t E, const int32_t* dyn_E,
                            const int32_t* mol_ptr, int64_t N, const int32_t* dyn_N, int64_t B, int max_n,
                            int64_t* iptr_i, int32_t* ilist_i, int64_t* iptr_j, int32_t* ilist_j, int32_t* status,
                            hipStream_t stream) {
  if (E < 0 || E > INT_MAX || N < 0 || N > INT_MAX || max_n < 1 || max_n > PI_MAXN) return (int)hipErrorInvalidValue;
  if (B <= 0) return 0;
  const int64_t slices = (std::min<int64_t>(max_n, std::max<int64_t>(N, 1)) + PI_APB - 1) / PI_APB;
  if (B * slices > INT_MAX) return (int)hipErrorInvalidValue;
  PainnIncArgs A{};
  A.src_i = src_i; A.src_j = src_j; A.mol_ptr = mol_ptr; A.E = (int)E; A.N = (int)N; A.B = (int)B; A.max_n = max_n;
  A.slices = (int)slices; A.iptr_i = iptr_i; A.ilist_i = ilist_i; A.iptr_j = iptr_j; A.ilist_j = ilist_j;
  A.status = status; A.dyn_E = dyn_E; A.dyn_N = dyn_N;
  if (dyn_E != nullptr)
    hipLaunchKernelGGL(k_painn_incidence_layout<true>, dim3((unsigned)(B * slices)), dim3(256), 0, stream, A);
  else
    hipLaunchKernelGGL(k_painn_incidence_layout<false>, dim3((unsigned)(B * slices)), dim3(256), 0, stream, A);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int64_t geossl_painn_incidence_layout_workspace_bytes(int64_t E_cap, int64_t N_cap, int64_t B) {
  (void)E_cap; (void)N_cap; (void)B;
  return 0;   // every block finds what it needs itself: one launch, nothing handed from one to the next
}

extern "C" int geossl_painn_incidence_layout(const int64_t* src_i, const int64_t* src_j, int64_t E,
                                             const int32_t* mol_ptr, int64_t N, int64_t B, int max_n, int64_t* iptr_i,
                                             int32_t* ilist_i, int64_t* iptr_j, int32_t* ilist_j, int32_t* status,
                                             void* workspace, hipStream_t stream) {
  (void)workspace;
  return launch_incidence_layout(src_i, src_j, E, nullptr, mol_ptr, N, nullptr, B, max_n, iptr_i, ilist_i, iptr_j,
                                 ilist_j, status, stream);
}

extern "C" int geossl_painn_incidence_layout_dyn(const int64_t* src_i, const int64_t* src_j, int64_t E_cap,
                                                 const int32_t* dyn_E, const int32_t* mol_ptr, int64_t N_cap, int64_t B,
                                                 int max_n, int64_t* iptr_i, int32_t* ilist_i, int64_t* iptr_j,
                                                 int32_t* ilist_j, int32_t* status, const int32_t* dyn_N,
                                                 void* workspace, hipStream_t stream) {
  (void)workspace;
  if (dyn_E == nullptr || dyn_N == nullptr) return (int)hipErrorInvalidValue;
  return launch_incidence_layout(src_i, src_j, E_cap, dyn_E, mol_ptr, N_cap, dyn_N, B, max_n, iptr_i, ilist_i, iptr_j,
                                 ilist_j, status, stream);
}
