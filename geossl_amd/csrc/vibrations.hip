// Normal-mode analysis of B independent molecules on a force field (geossl_amd/vibrations.py): the Hessian by central
// differences of the replayed force pass, its fp64 finishing pass, and a batched symmetric eigensolver.  One round is
//   geossl_hessian_displace -> force pass on the image batch -> geossl_hessian_collect ;
// all of its state is device memory, so ONE captured graph of these launches is replayed R + 1 times without host work.
//
//   x0 [N][3] fp32            the reference geometry (N atoms of B molecules, mol_ptr [B + 1])
//   img [2 C][N][3] fp32      the image batch the force pass reads: image 2 c is (c, +), image 2 c + 1 is (c, -)
//   grad [2 C][N][3] fp32     dE/dpos of the image batch; energy_img [2 C][B] fp32
//   delta [1] fp32            the step, device data
//   state [4] int64           (round, round in flight, unused, unused)
//   hessian [B][M][M] fp64    M >= 3 n_max; row-major, the molecule's 3 n_b block in the leading corner
//
// k_displace (block (b, j): molecule b of image j = 2 c + s): r = state[0], k = r C + c.  Every coordinate of the molecule
//   is copied from x0; when k < 3 n_b, local coordinate k becomes fl32(x0_k + delta) (s = 0) or fl32(x0_k - delta) (s = 1):
//   one fp32 addition.  Block (0, 0) writes state[1] = r.
// k_collect (block (b, c)): r = state[1], k = r C + c.  r < R and k < 3 n_b: row k of H_b,
//   H[k][t] = ((double)g+[t] - (double)g-[t]) / ((double)x+_k - (double)x-_k)   for t < 3 n_b,
//   the denominator from the two fp32 coordinates the images hold.  Rows with k >= 3 n_b are not touched.  r == R, c == 0:
//   energy[b] = energy_img[0][b] and fmax[b] = sqrt(max_i |g_i|^2) of image 0, in fp64.  Block (0, 0) writes state[0] = r + 1.
//   No launch reads a word that one of its blocks writes.
// k_finish (one block per molecule, m = 3 n_b), fp64, in this order:
//   asymmetry = max_{i<j} |H_ij - H_ji| ;  H_ij = H_ji = (H_ij + H_ji) / 2 ;  D_ij = D_ji = H_ij / sqrt(m_i m_j) ;
//   H and D are zero outside the m x m block.  project >= 1: the translations T_a = sqrt(m_i) e_a; project == 2: also the
//   rotations R_a = sqrt(m_i) e_a x (x_i - com), com = sum m_i x_i / sum m_i.  Modified Gram-Schmidt in the order Tx Ty Tz Rx
//   Ry Rz: n0 = |v|, v -= (u . v) u for every kept u in order, n1 = |v|; v is dropped unless n1 > kDropTol n0 (so a zero
//   vector is dropped), else kept as v / n1.  n_projected = the number kept, p.  With V the kept vectors:
//   W_a = D v_a (row sums in column order), S_ab = v_a . W_b, and for i <= j
//   D'_ij = D'_ji = D_ij - sum_a (W_a[i] v_a[j] + v_a[i] W_a[j]) + sum_a v_a[i] sum_b S_ab v_b[j]   ( = (P D P)_ij, P = I - V V^T).
//   Sums over atoms and coordinates: per thread in index order, then the fixed tree of block_sum.
// k_jacobi (one block per matrix, dimension m = dims[b] <= M <= 99): cyclic Jacobi in round-robin order, A and V in LDS.
//   A is read from the upper triangle of the input, padded with one zero row and column when m is odd (n' = m or m + 1
//   players).  Round t = 0 .. n' - 2 of a sweep pairs slot 0: (n' - 1, t), slot k >= 1: ((t + k) mod (n' - 1),
//   (t - k) mod (n' - 1)); (p, q) = (min, max).
//   Rotation of a pair:  theta = (a_qq - a_pp) / (2 a_pq),  t = sgn(theta) / (|theta| + sqrt(theta^2 + 1))  (sgn(0) = 1),
//   c = 1 / sqrt(t^2 + 1),  s = t c.   Skip rule: |a_pq| <= 2^-52 |A|_F (a quarter of the stop threshold: rounding noise
//   inside a cluster of equal eigenvalues, which a rotation would only stir), or q is the padding index: c = 1, s = t = 0.
//   All rotations of a round are computed first, then applied as A <- J^T A J, V <- V J with J_pp = J_qq = c, J_pq = s,
//   J_qp = -s: the 2 x 2 block of two different pairs (p, q), (r, u) is computed once as R1^T (B R2) and written to both
//   triangles; the block of one pair is a_pp - t a_pq, a_qq + t a_pq, 0.  A stays exactly symmetric.
//   Stop rule, tested before every sweep and after the last: max_{i<j} |a_ij| <= 2^-50 |A|_F (|A|_F of the input, by
//   the tree).  At most max_sweeps sweeps are made: sweeps[b] = the number made, converged[b] = the last test's result.
//   Then the eigenvalues a_ii are ranked ascending (ties by index) and eigenvalues[b][rank] / column `rank` of modes[b]
//   receive them; eigenvalues past m are NaN, modes outside m x m zero.
// No atomics anywhere: the same bits every launch.  Every loop bound is a launch argument or a clamped device word.
#include "geossl_hip.h"
#include "head_common.h"

#include <cmath>

using namespace geossl;

namespace {

constexpr int kDisplaceBlock = 64;
constexpr int kBlock = 256;
constexpr int kJacobiMax = 99;
constexpr double kDropTol = 1e-5;
constexpr double kStopFactor = 8.8817841970012523e-16;   // 2^-50

enum State { kRound = 0, kInFlight = 1 };

__device__ __forceinline__ double block_max(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ double block_add(double v, double* red) {
  const double r = block_sum<kBlock>(v, red);
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kDisplaceBlock) void k_displace(const float* __restrict__ x0,
                                                             const int32_t* __restrict__ mol_ptr,
                                                             const float* __restrict__ delta, int64_t* state, int N,
                                                             int C, float* __restrict__ img) {
  const int b = blockIdx.x, j = blockIdx.y, c = j >> 1;
  const int64_t r = state[kRound];
  const int a0 = max(min(mol_ptr[b], N), 0), a1 = max(min(mol_ptr[b + 1], N), a0);
  const int m = 3 * (a1 - a0);
  const int64_t k = r >= 0 ? r * (int64_t)C + c : -1;
  const float d = (j & 1) ? -delta[0] : delta[0];
  const float* src = x0 + 3 * (int64_t)a0;
  float* dst = img + 3 * ((int64_t)j * N + a0);
  for (int t = threadIdx.x; t < m; t += kDisplaceBlock) dst[t] = (int64_t)t == k ? add_rn(src[t], d) : src[t];
  if (b == 0 && j == 0 && threadIdx.x == 0) state[kInFlight] = r;
}

__global__ __launch_bounds__(kBlock) void k_collect(const float* __restrict__ img, const float* __restrict__ grad,
                                                    const float* __restrict__ energy_img,
                                                    const int32_t* __restrict__ mol_ptr, int64_t* state, int B, int N, int C,
                                                    int64_t R, int M, double* __restrict__ hessian,
                                                    double* __restrict__ energy, double* __restrict__ fmax_out) {
  __shared__ double red[kBlock];
  const int b = blockIdx.x, c = blockIdx.y;
  const int64_t r = state[kInFlight];
  const int a0 = max(min(mol_ptr[b], N), 0), a1 = max(min(mol_ptr[b + 1], N), a0);
  const int m = min(3 * (a1 - a0), M);
  const int64_t k = r >= 0 ? r * (int64_t)C + c : -1;
  if (r >= 0 && r < R && k < m) {
    const int64_t plus = 3 * ((int64_t)(2 * c) * N + a0), minus = 3 * ((int64_t)(2 * c + 1) * N + a0);
    const double den = (double)img[plus + k] - (double)img[minus + k];
    double* row = hessian + ((int64_t)b * M + k) * M;
    for (int t = threadIdx.x; t < m; t += kBlock) row[t] = ((double)grad[plus + t] - (double)grad[minus + t]) / den;
  }
  if (r == R && c == 0) {   // (uniform over the block)
    double f2 = 0.0;
    for (int i = a0 + (int)threadIdx.x; i < a1; i += kBlock) {
      const double gx = grad[3 * (int64_t)i], gy = grad[3 * (int64_t)i + 1], gz = grad[3 * (int64_t)i + 2];
      f2 = fmax(f2, gx * gx + gy * gy + gz * gz);
    }
    f2 = block_max(f2, red);
    if (threadIdx.x == 0) {
      energy[b] = (double)energy_img[b];
      fmax_out[b] = sqrt(f2);
    }
  }
  if (b == 0 && c == 0 && threadIdx.x == 0) state[kRound] = r + 1;
}

// work: per molecule 12 M + 40 doubles: V [6][M], W [6][M], S [6][6]
__global__ __launch_bounds__(kBlock) void k_finish(double* __restrict__ hessian, const float* __restrict__ x0,
                                                   const double* __restrict__ masses,
                                                   const int32_t* __restrict__ mol_ptr, int N, int M, int project,
                                                   double* __restrict__ D, double* __restrict__ asymmetry,
                                                   int32_t* __restrict__ n_projected, double* __restrict__ work) {
  __shared__ double red[kBlock];
  __shared__ double com[3];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int a0 = max(min(mol_ptr[b], N), 0), a1 = max(min(mol_ptr[b + 1], N), a0);
  const int m = min(3 * (a1 - a0), M);
  double* H = hessian + (int64_t)b * M * M;
  double* Db = D + (int64_t)b * M * M;
  double* V = work + (int64_t)b * (12 * (int64_t)M + 40);
  double* W = V + 6 * (int64_t)M;
  double* S = W + 6 * (int64_t)M;
  const double* mass = masses + a0;

  // ---- asymmetry, (H + H^T) / 2, mass-weighting; zeros outside the block
  double asym = 0.0;
  for (int e = tid; e < M * M; e += kBlock) {
    const int i = e / M, j = e - i * M;
    if (i >= m || j >= m) {
      H[e] = 0.0;
      Db[e] = 0.0;
    } else if (i <= j) {
      const double hij = H[i * M + j], hji = H[j * M + i];
      asym = fmax(asym, fabs(hij - hji));
      const double h = 0.5 * (hij + hji);
      const double mm = mass[i / 3] * mass[j / 3];
      const double d = h / sqrt(mm);
      H[i * M + j] = h;
      H[j * M + i] = h;
      Db[i * M + j] = d;
      Db[j * M + i] = d;
    }
  }
  asym = block_max(asym, red);
  if (tid == 0) asymmetry[b] = asym;
  const int nvec = project == 1 ? 3 : (project == 2 ? 6 : 0);
  if (nvec == 0 || m == 0) {
    if (tid == 0) n_projected[b] = 0;
    return;
  }

  // ---- the centre of mass and the raw vectors
  double sm = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
  for (int i = tid; i < m / 3; i += kBlock) {
    const double w = mass[i];
    sm += w;
    sx += w * (double)x0[3 * (int64_t)(a0 + i)];
    sy += w * (double)x0[3 * (int64_t)(a0 + i) + 1];
    sz += w * (double)x0[3 * (int64_t)(a0 + i) + 2];
  }
  sm = block_add(sm, red);
  sx = block_add(sx, red);
  sy = block_add(sy, red);
  sz = block_add(sz, red);
  if (tid == 0) {
    com[0] = sx / sm;
    com[1] = sy / sm;
    com[2] = sz / sm;
  }
  __syncthreads();
  for (int i = tid; i < m / 3; i += kBlock) {
    const double w = sqrt(mass[i]);
    const double rx = (double)x0[3 * (int64_t)(a0 + i)] - com[0], ry = (double)x0[3 * (int64_t)(a0 + i) + 1] - com[1],
                 rz = (double)x0[3 * (int64_t)(a0 + i) + 2] - com[2];
    for (int a = 0; a < 3; ++a)
      for (int ax = 0; ax < 3; ++ax) V[a * M + 3 * i + ax] = a == ax ? w : 0.0;
    if (nvec == 6) {
      // e_x x r = (0, -rz, ry);  e_y x r = (rz, 0, -rx);  e_z x r = (-ry, rx, 0)
      V[3 * M + 3 * i] = 0.0;
      V[3 * M + 3 * i + 1] = -w * rz;
      V[3 * M + 3 * i + 2] = w * ry;
      V[4 * M + 3 * i] = w * rz;
      V[4 * M + 3 * i + 1] = 0.0;
      V[4 * M + 3 * i + 2] = -w * rx;
      V[5 * M + 3 * i] = -w * ry;
      V[5 * M + 3 * i + 1] = w * rx;
      V[5 * M + 3 * i + 2] = 0.0;
    }
  }
  __syncthreads();

  // ---- modified Gram-Schmidt; kept vectors move to the slots 0 .. p - 1
  int p = 0;
  for (int a = 0; a < nvec; ++a) {
    double* v = V + a * M;
    double q = 0.0;
    for (int i = tid; i < m; i += kBlock) q += v[i] * v[i];
    const double n0 = sqrt(block_add(q, red));
    for (int u = 0; u < p; ++u) {
      const double* uu = V + u * M;
      double d = 0.0;
      for (int i = tid; i < m; i += kBlock) d += uu[i] * v[i];
      d = block_add(d, red);
      for (int i = tid; i < m; i += kBlock) v[i] -= d * uu[i];
      __syncthreads();
    }
    q = 0.0;
    for (int i = tid; i < m; i += kBlock) q += v[i] * v[i];
    const double n1 = sqrt(block_add(q, red));
    if (n1 > kDropTol * n0) {   // (uniform over the block)
      double* dst = V + p * M;
      for (int i = tid; i < m; i += kBlock) dst[i] = v[i] / n1;
      ++p;
    }
    __syncthreads();
  }
  if (tid == 0) n_projected[b] = p;
  if (p == 0) return;

  // ---- W = D V, S = V^T W, D' = P D P
  for (int e = tid; e < p * m; e += kBlock) {
    const int a = e / m, i = e - a * m;
    const double* v = V + a * M;
    double acc = 0.0;
    for (int j = 0; j < m; ++j) acc += Db[i * M + j] * v[j];
    W[a * M + i] = acc;
  }
  __syncthreads();
  for (int e = tid; e < p * p; e += kBlock) {
    const int a = e / p, c = e - a * p;
    double acc = 0.0;
    for (int i = 0; i < m; ++i) acc += V[a * M + i] * W[c * M + i];
    S[a * 6 + c] = acc;
  }
  __syncthreads();
  for (int e = tid; e < m * m; e += kBlock) {
    const int i = e / m, j = e - i * m;
    if (i > j) continue;
    double t = 0.0, q = 0.0;
    for (int a = 0; a < p; ++a) {
      t += W[a * M + i] * V[a * M + j] + V[a * M + i] * W[a * M + j];
      double sv = 0.0;
      for (int c = 0; c < p; ++c) sv += S[a * 6 + c] * V[c * M + j];
      q += V[a * M + i] * sv;
    }
    const double d = Db[i * M + j] - t + q;
    Db[i * M + j] = d;
    Db[j * M + i] = d;
  }
}

__device__ __forceinline__ void round_pair(int t, int k, int np2, int& p, int& q) {
  // np2 = n' (even); slot 0: (n' - 1, t); slot k: ((t + k) mod (n' - 1), (t - k) mod (n' - 1))
  const int w = np2 - 1;
  int a, c;
  if (k == 0) {
    a = w;
    c = t;
  } else {
    a = (t + k) % w;
    c = (t - k + w) % w;
  }
  p = min(a, c);
  q = max(a, c);
}

__global__ __launch_bounds__(kBlock) void k_jacobi(const double* __restrict__ A, const int32_t* __restrict__ dims, int M,
                                                   int ld, int max_sweeps, double* __restrict__ eigenvalues,
                                                   double* __restrict__ modes, int32_t* __restrict__ sweeps,
                                                   int32_t* __restrict__ converged) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  double* sA = reinterpret_cast<double*>(smem_raw);   // [ld][ld]
  double* sV = sA + ld * ld;                          // [ld][ld]
  double* rot = sV + ld * ld;                         // [ld / 2][3]: c, s, t   (afterwards: the permutation, as ints)
  double* red = rot + 3 * (ld / 2);                   // [kBlock]               (afterwards: the eigenvalues)
  const int b = blockIdx.x, tid = threadIdx.x;
  const int m = max(min(dims[b], M), 0);
  const int np = (m + 1) / 2, n2 = 2 * np;            // pairs per round, players
  const double* Ab = A + (int64_t)b * M * M;

  double f2 = 0.0;
  for (int e = tid; e < n2 * n2; e += kBlock) {
    const int i = e / n2, j = e - i * n2;
    const double a = (i < m && j < m) ? Ab[min(i, j) * M + max(i, j)] : 0.0;
    sA[i * ld + j] = a;
    sV[i * ld + j] = i == j ? 1.0 : 0.0;
    f2 += a * a;
  }
  __syncthreads();
  const double thr = kStopFactor * sqrt(block_add(f2, red));

  int sw = 0, conv = 0;
  for (int it = 0; it <= max_sweeps; ++it) {
    double off = 0.0;
    for (int e = tid; e < m * m; e += kBlock) {
      const int i = e / m, j = e - i * m;
      if (i < j) off = fmax(off, fabs(sA[i * ld + j]));
    }
    off = block_max(off, red);
    if (off <= thr) {
      conv = 1;
      break;
    }
    if (it == max_sweeps) break;
    for (int t = 0; t < n2 - 1; ++t) {
      if (tid < np) {
        int p, q;
        round_pair(t, tid, n2, p, q);
        const double apq = sA[p * ld + q];
        double c = 1.0, s = 0.0, tt = 0.0;
        if (q < m && fabs(apq) > 0.25 * thr) {
          const double theta = (sA[q * ld + q] - sA[p * ld + p]) / (2.0 * apq);
          tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          c = 1.0 / sqrt(tt * tt + 1.0);
          s = tt * c;
        }
        rot[3 * tid] = c;
        rot[3 * tid + 1] = s;
        rot[3 * tid + 2] = tt;
      }
      __syncthreads();
      for (int e = tid; e < np * np; e += kBlock) {
        const int k1 = e / np, k2 = e - k1 * np;
        if (k1 > k2) continue;
        int p, q, r, u;
        round_pair(t, k1, n2, p, q);
        const double c1 = rot[3 * k1], s1 = rot[3 * k1 + 1];
        if (k1 == k2) {
          const double tt = rot[3 * k1 + 2], apq = sA[p * ld + q];
          if (s1 != 0.0) {
            sA[p * ld + p] -= tt * apq;
            sA[q * ld + q] += tt * apq;
            sA[p * ld + q] = 0.0;
            sA[q * ld + p] = 0.0;
          }
          continue;
        }
        round_pair(t, k2, n2, r, u);
        const double c2 = rot[3 * k2], s2 = rot[3 * k2 + 1];
        const double bpr = sA[p * ld + r], bpu = sA[p * ld + u], bqr = sA[q * ld + r], bqu = sA[q * ld + u];
        const double tpr = c2 * bpr - s2 * bpu, tpu = s2 * bpr + c2 * bpu;
        const double tqr = c2 * bqr - s2 * bqu, tqu = s2 * bqr + c2 * bqu;
        const double npr = c1 * tpr - s1 * tqr, nqr = s1 * tpr + c1 * tqr;
        const double npu = c1 * tpu - s1 * tqu, nqu = s1 * tpu + c1 * tqu;
        sA[p * ld + r] = npr;
        sA[r * ld + p] = npr;
        sA[p * ld + u] = npu;
        sA[u * ld + p] = npu;
        sA[q * ld + r] = nqr;
        sA[r * ld + q] = nqr;
        sA[q * ld + u] = nqu;
        sA[u * ld + q] = nqu;
      }
      for (int e = tid; e < m * np; e += kBlock) {
        const int i = e / np, k = e - i * np;
        int p, q;
        round_pair(t, k, n2, p, q);
        const double c = rot[3 * k], s = rot[3 * k + 1];
        const double vp = sV[i * ld + p], vq = sV[i * ld + q];
        sV[i * ld + p] = c * vp - s * vq;
        sV[i * ld + q] = s * vp + c * vq;
      }
      __syncthreads();
    }
    ++sw;
  }

  // ---- ascending rank sort (ties by index), columns permuted
  int* perm = reinterpret_cast<int*>(rot);
  __syncthreads();
  if (tid < m) {
    red[tid] = sA[tid * ld + tid];
    perm[tid] = tid;   // (NaN eigenvalues rank alike: every slot still names a column)
  }
  __syncthreads();
  if (tid < m) {
    const double x = red[tid];
    int rank = 0;
    for (int j = 0; j < m; ++j) {
      const double y = red[j];
      rank += (y < x || (y == x && j < tid)) ? 1 : 0;
    }
    rank = min(rank, m - 1);
    perm[rank] = tid;
  }
  __syncthreads();
  for (int e = tid; e < M; e += kBlock)
    eigenvalues[(int64_t)b * M + e] = e < m ? red[perm[e]] : __builtin_nan("");
  double* Vb = modes + (int64_t)b * M * M;
  for (int e = tid; e < M * M; e += kBlock) {
    const int i = e / M, j = e - i * M;
    Vb[e] = (i < m && j < m) ? sV[i * ld + perm[j]] : 0.0;
  }
  if (tid == 0) {
    sweeps[b] = sw;
    converged[b] = conv;
  }
}

}  // namespace

extern "C" int geossl_hessian_displace(const float* x0, const int32_t* mol_ptr, const float* delta, int64_t* state,
                                       int64_t B, int64_t N, int64_t C, float* img, hipStream_t stream) {
  if (N < 1 || N >= (1 << 24) || B < 1 || B >= (1 << 16) || C < 1 || 2 * C > 65535 || 2 * C * N >= (1ll << 28) ||
      x0 == nullptr || mol_ptr == nullptr || delta == nullptr || state == nullptr || img == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_displace, dim3((unsigned)B, (unsigned)(2 * C)), dim3(kDisplaceBlock), 0, stream, x0, mol_ptr, delta,
                     state, (int)N, (int)C, img);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_hessian_collect(const float* img, const float* grad, const float* energy_img,
                                      const int32_t* mol_ptr, int64_t* state, int64_t B, int64_t N, int64_t C, int64_t R,
                                      int64_t M, double* hessian, double* energy, double* fmax, hipStream_t stream) {
  if (N < 1 || N >= (1 << 24) || B < 1 || B >= (1 << 16) || C < 1 || C > 65535 || 2 * C * N >= (1ll << 28) || R < 0 ||
      M < 1 || M > 3 * 255 || img == nullptr || grad == nullptr || energy_img == nullptr || mol_ptr == nullptr ||
      state == nullptr || hessian == nullptr || energy == nullptr || fmax == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_collect, dim3((unsigned)B, (unsigned)C), dim3(kBlock), 0, stream, img, grad, energy_img, mol_ptr,
                     state, (int)B, (int)N, (int)C, R, (int)M, hessian, energy, fmax);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t geossl_hessian_finish_workspace(int64_t B, int64_t M) { return B * (12 * M + 40); }

extern "C" int geossl_hessian_finish(double* hessian, const float* x0, const double* masses, const int32_t* mol_ptr,
                                     int64_t B, int64_t N, int64_t M, int project, double* D, double* asymmetry,
                                     int32_t* n_projected, double* workspace, hipStream_t stream) {
  if (N < 1 || N >= (1 << 24) || B < 1 || B >= (1 << 16) || M < 1 || M > 3 * 255 || project < 0 || project > 2 ||
      hessian == nullptr || x0 == nullptr || masses == nullptr || mol_ptr == nullptr || D == nullptr ||
      asymmetry == nullptr || n_projected == nullptr || workspace == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_finish, dim3((unsigned)B), dim3(kBlock), 0, stream, hessian, x0, masses, mol_ptr, (int)N, (int)M,
                     project, D, asymmetry, n_projected, workspace);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_sym_eig_jacobi(const double* A, const int32_t* dims, int64_t B, int64_t M, int max_sweeps,
                                     double* eigenvalues, double* modes, int32_t* sweeps, int32_t* converged,
                                     hipStream_t stream) {
  if (B < 1 || B >= (1 << 24) || M < 1 || M > kJacobiMax || max_sweeps < 0 || max_sweeps > 4096 || A == nullptr ||
      dims == nullptr || eigenvalues == nullptr || modes == nullptr || sweeps == nullptr || converged == nullptr)
    return (int)hipErrorInvalidValue;
  const int ld = (int)M + ((int)M & 1);
  const size_t lds = sizeof(double) * ((size_t)2 * ld * ld + 3 * (ld / 2) + kBlock);
  allow_big_lds(&k_jacobi);
  hipLaunchKernelGGL(k_jacobi, dim3((unsigned)B), dim3(kBlock), lds, stream, A, dims, (int)M, ld, max_sweeps, eigenvalues,
                     modes, sweeps, converged);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
