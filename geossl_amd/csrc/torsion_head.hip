// Angle-prediction head on atom triples, examples/pretrain_TorsionAnglePrediction.py:16-27,64-78:
// pred_t = Linear(3F, 1)(cat(h_u, h_v, h_w)), loss = MSELoss(pred, super_edge_angle) = mean_t (pred_t - angle_t)^2, forward
// and backward; the producer of the angles (geossl_triple_angles: this project's definition, the reference tree has none)
// and the gather of a device-resident dataset's triples into a batch (geossl_gather_triples).
//
// A linear layer on a concatenation splits into per-atom projections: with W = [w_u | w_v | w_w],
//   a_i = w_u . h_i,  b_i = w_v . h_i,  c_i = w_w . h_i,  pred_t = ((a_{u_t} + b_{v_t}) + c_{w_t}) + bias,
// so the [T][3F] features of the reference are never formed.  Forward: one wave per atom computes (a_i, b_i, c_i)
// (k_cat_project<V, 3> of head_common.h), one pass over the triples computes pred, res = pred - angle and per-block fp64
// sums of res^2 (k_tor_triples), and one block adds the block sums in order and divides by T (k_head_loss).
// Backward, with d pred_t = (2 gout / T) res_t (MSELoss's mean and square backward):
//   dA_i / dB_i / dC_i = the sums of d pred_t over the triples in which atom i is u / v / w, each in ascending triple order
//   (k_tor_atom_grads); dh_i = dA_i w_u + dB_i w_v + dC_i w_w (written) and per block of atoms the partials of
//   dW = [sum dA_i h_i | sum dB_i h_i | sum dC_i h_i] and db = sum dA_i (k_cat_dh<3>); one launch adds the block partials
//   in block order (k_cat_wgrad<3>).
// How an atom finds its triples: the MOLECULE SCAN, not a three-sided incidence list.  The triples of a collated batch are
// grouped by molecule in batch order, so molecule m's triples are one run [first t with u_t >= mol_ptr[m], first t with
// u_t >= mol_ptr[m + 1]) that two binary searches find.  One block per molecule stages that run in LDS, kChunk triples at a
// time in order, and thread i walks the staged chunk for atom i (LDS broadcast reads).  n T_m compares per molecule:
// nothing at the script's sampling ratios (T_m = 4 .. 60), and a 33-atom molecule at ratio 1 (32 736 triples) is 32
// chunks.  It needs no index structure beside mol_ptr, which every batch already has - an incidence list would be a sampled,
// per-step structure to rebuild on the device before every replayed step.
// Every sum has a fixed order and there are no atomics: two launches on the same inputs give the same bits.
// Capacity launches (`_dyn`): N and T are capacities that size the grids; the real counts are read from dyn_N / dyn_T.
// Atoms and triples at and past them are never read or written, and the mean divides by the real T.  A triple with an
// atom outside [0, N) reads nothing: its prediction is NaN (and so is the loss).
#include "geossl_hip.h"
#include "head_common.h"

#include <algorithm>
#include <cmath>

using namespace geossl;

namespace {

constexpr int kTriBlock = 256;
constexpr int kTriPerThread = 4;
constexpr int kTriPerBlock = kTriBlock * kTriPerThread;
constexpr int kMolBlock = 256;                // k_tor_atom_grads: one thread per atom of the molecule (255 at most in a bucket)
constexpr int kChunk = 1024;                  // ... triples staged in LDS at a time (16 KB)

// Block k owns triples [k kTriPerBlock, (k + 1) kTriPerBlock); partial[k] = the sum of their res^2 in fp64 (per thread in
// triple order, then a tree over the block).  Blocks at and past the real T write nothing.
__global__ __launch_bounds__(kTriBlock) void k_tor_triples(const float* __restrict__ proj, const float* __restrict__ bias,
                                                           const int64_t* __restrict__ tri0,
                                                           const int64_t* __restrict__ tri1,
                                                           const int64_t* __restrict__ tri2,
                                                           const float* __restrict__ angle, int N_cap, int T_cap,
                                                           const int32_t* __restrict__ dyn_N,
                                                           const int32_t* __restrict__ dyn_T, float* __restrict__ pred,
                                                           float* __restrict__ res, double* __restrict__ partial) {
  const int T = dyn_count(T_cap, dyn_T);
  const int t0 = blockIdx.x * kTriPerBlock;
  if (t0 >= T) return;
  const int N = dyn_count(N_cap, dyn_N);
  const float b0 = bias[0];
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < kTriPerThread; ++k) {
    const int t = t0 + k * kTriBlock + threadIdx.x;
    if (t < T) {
      const int64_t u = tri0[t], v = tri1[t], w = tri2[t];
      float p = NAN;
      if (u >= 0 && u < N && v >= 0 && v < N && w >= 0 && w < N)
        p = add_rn(add_rn(add_rn(proj[3 * u], proj[3 * v + 1]), proj[3 * w + 2]), b0);
      const float r = p - angle[t];
      pred[t] = p;
      res[t] = r;
      acc += (double)r * (double)r;
    }
  }
  const double sum = block_sum_f64<kTriBlock>(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// first t in [0, T) with tri0[t] >= a (T when there is none): tri0 is non-decreasing over the molecules
__device__ __forceinline__ int first_triple_at(const int64_t* __restrict__ tri0, int T, int64_t a) {
  int lo = 0, hi = T;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tri0[mid] >= a) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Block m = molecule m: dABC[i] = (dA_i, dB_i, dC_i) of its atoms, d pred_t = (2 gout / T) res_t, every sum in ascending
// triple order.  An atom on no triple gets zeros.
__global__ __launch_bounds__(kMolBlock) void k_tor_atom_grads(const int64_t* __restrict__ tri0,
                                                              const int64_t* __restrict__ tri1,
                                                              const int64_t* __restrict__ tri2,
                                                              const float* __restrict__ res,
                                                              const int32_t* __restrict__ mol_ptr, int N_cap, int T_cap,
                                                              const int32_t* __restrict__ dyn_N,
                                                              const int32_t* __restrict__ dyn_T,
                                                              const float* __restrict__ gout, float* __restrict__ dABC) {
  __shared__ int su[kChunk], sv[kChunk], sw[kChunk];
  __shared__ float sg[kChunk];
  __shared__ int range[2];
  const int N = dyn_count(N_cap, dyn_N);
  const int T = dyn_count(T_cap, dyn_T);
  const int tid = threadIdx.x;
  const int a0 = min(mol_ptr[blockIdx.x], N), a1 = min(mol_ptr[blockIdx.x + 1], N);
  const int n = a1 - a0;
  if (n <= 0) return;   // (uniform over the block)
  if (tid < 2) range[tid] = first_triple_at(tri0, T, tid == 0 ? a0 : a1);
  __syncthreads();
  const int t0 = range[0], t1 = range[1];
  const float c = mul_rn(2.0f, gout[0]) / (float)T;   // MseLossBackward: 2 (pred - target) grad / numel
  for (int i0 = 0; i0 < n; i0 += kMolBlock) {          // (one pass for the molecules of a bucket: n <= 255)
    const int i = i0 + tid;                            // local atom; a0 + i is the batch atom
    float dA = 0.f, dB = 0.f, dC = 0.f;
    for (int q0 = t0; q0 < t1; q0 += kChunk) {
      const int cnt = min(kChunk, t1 - q0);
      __syncthreads();   // the chunk before this one has been read by every thread
      for (int q = tid; q < cnt; q += kMolBlock) {
        su[q] = (int)(tri0[q0 + q] - a0);
        sv[q] = (int)(tri1[q0 + q] - a0);
        sw[q] = (int)(tri2[q0 + q] - a0);
        sg[q] = mul_rn(c, res[q0 + q]);
      }
      __syncthreads();
      if (i < n) {
        for (int q = 0; q < cnt; ++q) {
          const float g = sg[q];
          if (su[q] == i) dA += g;
          if (sv[q] == i) dB += g;
          if (sw[q] == i) dC += g;
        }
      }
    }
    if (i < n) {
      float* o = dABC + 3 * (int64_t)(a0 + i);
      o[0] = dA;
      o[1] = dB;
      o[2] = dC;
    }
  }
}

// angle_t at the middle atom v of (u, v, w): atan2(|a x b|, a . b), a = pos_u - pos_v, b = pos_w - pos_v; 0 for a zero arm.
__global__ __launch_bounds__(256) void k_triple_angles(const float* __restrict__ pos, int64_t N,
                                                       const int64_t* __restrict__ tri0, const int64_t* __restrict__ tri1,
                                                       const int64_t* __restrict__ tri2, int64_t T,
                                                       float* __restrict__ angle) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int64_t u = tri0[t], v = tri1[t], w = tri2[t];
  if (u < 0 || u >= N || v < 0 || v >= N || w < 0 || w >= N) {
    angle[t] = NAN;
    return;
  }
  const float ax = pos[3 * u] - pos[3 * v], ay = pos[3 * u + 1] - pos[3 * v + 1], az = pos[3 * u + 2] - pos[3 * v + 2];
  const float bx = pos[3 * w] - pos[3 * v], by = pos[3 * w + 1] - pos[3 * v + 1], bz = pos[3 * w + 2] - pos[3 * v + 2];
  const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const float y = sqrtf(cx * cx + cy * cy + cz * cz);
  const float x = ax * bx + ay * by + az * bz;
  angle[t] = (y == 0.f && x == 0.f) ? 0.f : atan2f(y, x);   // (atan2f(0, -0) would be pi)
}

// Block m = molecule m of the batch: its cnt = t_ptr[m + 1] - t_ptr[m] triples, local atom indices from column
// t_src_off[m] of the dataset's [3][stride] list on, + mol_ptr[m]; its angles beside them.
__global__ __launch_bounds__(256) void k_gather_triples(const int32_t* __restrict__ tri_src, int64_t stride,
                                                        const float* __restrict__ angle_src,
                                                        const int32_t* __restrict__ t_src_off,
                                                        const int32_t* __restrict__ t_ptr,
                                                        const int32_t* __restrict__ mol_ptr, int64_t* __restrict__ tri0,
                                                        int64_t* __restrict__ tri1, int64_t* __restrict__ tri2,
                                                        float* __restrict__ angle_dst) {
  const int m = blockIdx.x;
  const int d0 = t_ptr[m], cnt = t_ptr[m + 1] - d0;
  const int64_t s0 = t_src_off[m];
  const int64_t a0 = mol_ptr[m];
  for (int i = threadIdx.x; i < cnt; i += 256) {
    tri0[d0 + i] = a0 + tri_src[s0 + i];
    tri1[d0 + i] = a0 + tri_src[stride + s0 + i];
    tri2[d0 + i] = a0 + tri_src[2 * stride + s0 + i];
    angle_dst[d0 + i] = angle_src[s0 + i];
  }
}

inline int64_t tri_blocks(int64_t T) { return std::max<int64_t>(1, (T + kTriPerBlock - 1) / kTriPerBlock); }
inline bool width_ok(int F) { return wave_row_width_ok(F); }

}  // namespace

extern "C" int geossl_torsion_head_width_ok(int F) { return width_ok(F) ? 1 : 0; }

extern "C" int64_t geossl_torsion_head_fwd_workspace_floats(int64_t T) { return 2 * tri_blocks(T); }

extern "C" int64_t geossl_torsion_head_bwd_workspace_floats(int64_t N, int F) {
  return 3 * std::max<int64_t>(N, 1) + atom_blocks(N) * (3 * (int64_t)F + 1);
}

extern "C" int geossl_torsion_head_fwd_dyn(const float* h, int64_t N, int F, const float* W, const float* bias,
                                           const int64_t* tri0, const int64_t* tri1, const int64_t* tri2,
                                           const float* angle, int64_t T, float* proj, float* pred, float* res,
                                           float* workspace, float* loss, const int32_t* dyn_N, const int32_t* dyn_T,
                                           hipStream_t stream) {
  if (N < 0 || T < 0 || N >= (1 << 30) || T >= (1 << 30) || !width_ok(F)) return (int)hipErrorInvalidValue;
  if (N > 0) {
    const int e = launch_cat_project<3>(h, N, F, W, dyn_N, proj, stream);
    if (e != 0) return e;
  }
  double* partial = reinterpret_cast<double*>(workspace);
  if (T > 0) {
    hipLaunchKernelGGL(k_tor_triples, dim3((unsigned)tri_blocks(T)), dim3(kTriBlock), 0, stream, proj, bias, tri0, tri1,
                       tri2, angle, (int)N, (int)T, dyn_N, dyn_T, pred, res, partial);
    GEOSSL_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_head_loss<kTriPerBlock>, dim3(1), dim3(kLossBlock), 0, stream, partial, 0, (int)T, dyn_T, loss);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_torsion_head_fwd(const float* h, int64_t N, int F, const float* W, const float* bias,
                                       const int64_t* tri0, const int64_t* tri1, const int64_t* tri2, const float* angle,
                                       int64_t T, float* proj, float* pred, float* res, float* workspace, float* loss,
                                       hipStream_t stream) {
  return geossl_torsion_head_fwd_dyn(h, N, F, W, bias, tri0, tri1, tri2, angle, T, proj, pred, res, workspace, loss,
                                     nullptr, nullptr, stream);
}

extern "C" int geossl_torsion_head_bwd_dyn(const float* h, int64_t N, int F, const float* W, const int64_t* tri0,
                                           const int64_t* tri1, const int64_t* tri2, int64_t T, const float* res,
                                           const int32_t* mol_ptr, int64_t B, const float* gout, float* dh, float* dW,
                                           float* db, float* workspace, int accumulate, const int32_t* dyn_N,
                                           const int32_t* dyn_T, hipStream_t stream) {
  if (N < 0 || T < 0 || B < 0 || N >= (1 << 30) || T >= (1 << 30) || B > (1 << 24) || !width_ok(F))
    return (int)hipErrorInvalidValue;
  if (N > 0 && (B < 1 || mol_ptr == nullptr)) return (int)hipErrorInvalidValue;
  float* dABC = workspace;
  float* part = workspace + 3 * std::max<int64_t>(N, 1);
  if (N > 0) {
    hipLaunchKernelGGL(k_tor_atom_grads, dim3((unsigned)B), dim3(kMolBlock), 0, stream, tri0, tri1, tri2, res, mol_ptr,
                       (int)N, (int)T, dyn_N, dyn_T, gout, dABC);
    GEOSSL_CHECK_LAUNCH();
  }
  return launch_cat_bwd<3>(h, N, F, W, dABC, part, dyn_N, dh, dW, db, accumulate, stream);
}

extern "C" int geossl_torsion_head_bwd(const float* h, int64_t N, int F, const float* W, const int64_t* tri0,
                                       const int64_t* tri1, const int64_t* tri2, int64_t T, const float* res,
                                       const int32_t* mol_ptr, int64_t B, const float* gout, float* dh, float* dW,
                                       float* db, float* workspace, int accumulate, hipStream_t stream) {
  return geossl_torsion_head_bwd_dyn(h, N, F, W, tri0, tri1, tri2, T, res, mol_ptr, B, gout, dh, dW, db, workspace,
                                     accumulate, nullptr, nullptr, stream);
}

extern "C" int geossl_triple_angles(const float* pos, int64_t N, const int64_t* tri0, const int64_t* tri1,
                                    const int64_t* tri2, int64_t T, float* angle, hipStream_t stream) {
  if (N < 0 || T < 0 || T >= ((int64_t)1 << 38)) return (int)hipErrorInvalidValue;
  if (T == 0) return 0;
  hipLaunchKernelGGL(k_triple_angles, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, stream, pos, N, tri0, tri1, tri2,
                     T, angle);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_gather_triples(const int32_t* tri_src, int64_t stride, const float* angle_src,
                                     const int32_t* t_src_off, const int32_t* t_ptr, const int32_t* mol_ptr, int64_t B,
                                     int64_t* tri0, int64_t* tri1, int64_t* tri2, float* angle_dst, hipStream_t stream) {
  if (B < 0 || B > (1 << 24) || stride < 0) return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  if (tri_src == nullptr || angle_src == nullptr || t_src_off == nullptr || t_ptr == nullptr || mol_ptr == nullptr ||
      tri0 == nullptr || tri1 == nullptr || tri2 == nullptr || angle_dst == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gather_triples, dim3((unsigned)B), dim3(256), 0, stream, tri_src, stride, angle_src, t_src_off,
                     t_ptr, mol_ptr, tri0, tri1, tri2, angle_dst);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
