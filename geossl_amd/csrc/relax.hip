// Structure relaxation of B independent replicas on a force field (geossl_amd/relax.py): FIRE in ASE's form, mass-weighted,
// in the Simulator's units, with per-molecule adaptive state and per-molecule convergence decided on the device.  A step is
//   force pass on pos -> geossl_fire_step ;
// all of its state is device memory, so a captured graph of these launches replays without host work, and
// geossl_fire_active, the last node of such a graph, leaves the ONE word the host reads per replay group:
//
//   pos, vel [N][3] fp32      positions (the force pass's input) and velocities
//   grad [N][3], energy [B]   dE/dpos and E at the positions the step FOUND (kept from the pass, like geossl_md_finish)
//   cinv_mass [N] fp32        ACCEL / m (A fs^-2 per kcal mol^-1 A^-1)
//   params [8] fp32           ftol, dt_max, dt_min, max_step, f_inc, f_dec, alpha_start, f_alpha
//   iparams [4] int64         n_min, record_every, the call counter of trajectory slot 0, unused
//   mol_dt, mol_alpha [B]     fp32: the molecule's time step and mixing coefficient
//   mol_state [B][4] int32    npos (downhill steps in a row), done (latched), nsteps (steps that moved it), calls (steps
//                             launched on it, frozen or not: the clock of the recording)
//
// k_fire_step (one wave per molecule b, lane l takes the atoms l, l + 64, ...), F = -grad_new:
//   pass 1, fp64 over the fp32 inputs, sums per lane in atom order and then a fixed tree over the 64 lanes in LDS, maxima
//   order-free:   fm2 = max_i |F_i|^2,  P = sum F.v,  vv = sum v.v,  ff = sum F.F ;  fmax = sqrt(fm2)
//   converged = done != 0 or fmax < ftol                                  (fp64 against the fp32 word)
//   if the call counter hits a slot - d = calls - first >= 0, d % record_every == 0, d / record_every < frames - the frame
//   AS THE STEP FOUND IT is written: pos, vel (incoming), energy_new, (float) fmax, dt, alpha, npos (incoming) and
//   `converged` (after the test at these positions).
//   converged: done = 1, calls += 1, nothing else of the molecule changes.  Otherwise, every product that is not part of an
//   fma rounded on its own:
//     downhill = P > 0 or vv == 0                                         (fp64)
//     downhill:  c = (float)(alpha sqrt(vv / ff))  (fp64, rounded once; 0 when ff == 0);  oma = 1 - alpha  (one rounding)
//                v1 = fma(c, F, oma v)  with  oma v  rounded
//                npos > n_min:  dt' = min(dt f_inc, dt_max) (product rounded),  alpha' = alpha f_alpha (rounded)
//                npos' = npos + 1
//     uphill:    v1 = 0,  alpha' = alpha_start,  dt' = max(dt f_dec, dt_min) (product rounded),  npos' = 0
//     a = F cinv_mass (rounded);  v2 = fma(dt', a, v1);  dr = dt' v2 (rounded)
//   pass 2:  dm2 = max_i |dr_i|^2 in fp64;  s = dm2 > max_step^2 ? (float)(max_step / sqrt(dm2)) : 1   (fp64, rounded once)
//   pass 3:  vel = v2,  pos = fma(s, dr, pos);  nsteps += 1, calls += 1
//   (passes 2 and 3 form v2 and dr from the same inputs by the same operations: vel and pos are written in pass 3 only.)
//   evaluate_only: pass 1 alone, the frame goes into slot 0 (frames >= 1), and nothing else is written: not grad, energy,
//   the molecule's words or its counters.
// Every block reads and writes the words of its own molecule only; params and iparams are read-only: no launch reads a
// word that one of its blocks writes.  No atomics: the same bits every launch.  All stores are plain vector stores.
// k_fire_active (one block): active[0] = the number of molecules with done == 0, counted per thread in molecule order and
// then by the same tree.
#include "geossl_hip.h"
#include "head_common.h"

using namespace geossl;

namespace {

constexpr int kWave = 64;
constexpr int kActiveBlock = 256;

enum Param { kFtol = 0, kDtMax = 1, kDtMin = 2, kMaxStep = 3, kFInc = 4, kFDec = 5, kAlphaStart = 6, kFAlpha = 7 };
enum IParam { kNMin = 0, kRecordEvery = 1, kFirst = 2 };
enum MolWord { kNpos = 0, kDone = 1, kNsteps = 2, kCalls = 3 };

__device__ __forceinline__ double wave_max(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kWave / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  return red[0];
}

struct Kick {
  float v2[3], dr[3];
};

// the per-atom fp32 chain of the header comment, for one atom
__device__ __forceinline__ Kick fire_kick(const float* __restrict__ vel, const float* grad_new, int64_t k0, float cinv,
                                          bool downhill, float c, float oma, float dtn) {
  Kick o;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const float F = -grad_new[k0 + ax];
    const float v1 = downhill ? fmaf(c, F, mul_rn(oma, vel[k0 + ax])) : 0.0f;
    o.v2[ax] = fmaf(dtn, mul_rn(F, cinv), v1);
    o.dr[ax] = mul_rn(dtn, o.v2[ax]);
  }
  return o;
}

// grad_new / energy_new may be grad / energy themselves (no __restrict__ on the four)
__global__ __launch_bounds__(kWave) void k_fire_step(float* __restrict__ pos, float* __restrict__ vel,
                                                     const float* grad_new, const float* energy_new, float* grad,
                                                     float* energy, const float* __restrict__ cinv_mass,
                                                     const int32_t* __restrict__ mol_ptr, int B, int N,
                                                     const float* __restrict__ params,
                                                     const int64_t* __restrict__ iparams, float* __restrict__ mol_dt,
                                                     float* __restrict__ mol_alpha, int32_t* __restrict__ mol_state,
                                                     int evaluate_only, int64_t frames, float* __restrict__ traj_pos,
                                                     float* __restrict__ traj_vel, float* __restrict__ traj_energy,
                                                     float* __restrict__ traj_fmax, float* __restrict__ traj_dt,
                                                     float* __restrict__ traj_alpha, int32_t* __restrict__ traj_npos,
                                                     int32_t* __restrict__ traj_done) {
  __shared__ double red[5][kWave];
  const int b = blockIdx.x;
  const float dt = mol_dt[b], alpha = mol_alpha[b];
  const int32_t npos = mol_state[4 * b + kNpos], done = mol_state[4 * b + kDone];
  const int32_t nsteps = mol_state[4 * b + kNsteps], calls = mol_state[4 * b + kCalls];
  const int64_t every = iparams[kRecordEvery], d = (int64_t)calls - iparams[kFirst];
  int64_t slot = -1;
  if (evaluate_only) slot = 0;
  else if (every >= 1 && d >= 0 && d % every == 0) slot = d / every;
  const bool record = traj_pos != nullptr && slot >= 0 && slot < frames;
  const int a0 = max(min(mol_ptr[b], N), 0), a1 = max(min(mol_ptr[b + 1], N), a0);

  // ---- pass 1: the reductions at the positions the step found, and their frame
  double fm2 = 0.0, P = 0.0, vv = 0.0, ff = 0.0;
  for (int i = a0 + (int)threadIdx.x; i < a1; i += kWave) {
    double f2 = 0.0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const int64_t k = 3 * (int64_t)i + ax;
      const float g = grad_new[k];
      const double F = -(double)g, v = (double)vel[k];
      f2 += F * F;
      P += F * v;
      vv += v * v;
      if (!evaluate_only && grad != grad_new) grad[k] = g;
      if (record) {
        const int64_t t = slot * 3 * (int64_t)N + k;
        traj_pos[t] = pos[k];
        traj_vel[t] = vel[k];
      }
    }
    ff += f2;
    fm2 = fmax(fm2, f2);
  }
  fm2 = wave_max(fm2, red[0]);
  P = block_sum<kWave>(P, red[1]);
  vv = block_sum<kWave>(vv, red[2]);
  ff = block_sum<kWave>(ff, red[3]);
  const double fmax_b = sqrt(fm2);
  const bool converged = done != 0 || fmax_b < (double)params[kFtol];
  if (threadIdx.x == 0) {
    const float e = energy_new[b];
    if (!evaluate_only && energy != energy_new) energy[b] = e;
    if (record) {
      const int64_t t = slot * B + b;
      traj_energy[t] = e;
      traj_fmax[t] = (float)fmax_b;
      traj_dt[t] = dt;
      traj_alpha[t] = alpha;
      traj_npos[t] = npos;
      traj_done[t] = converged ? 1 : 0;
    }
  }
  if (evaluate_only) return;
  if (converged) {   // frozen: the latch and the clock
    if (threadIdx.x == 0) {
      mol_state[4 * b + kDone] = 1;
      mol_state[4 * b + kCalls] = calls + 1;
    }
    return;
  }

  // ---- the decision and the molecule's scalars
  const bool downhill = P > 0.0 || vv == 0.0;
  float c = 0.0f, oma = 0.0f, dtn, alphan;
  int32_t nposn;
  if (downhill) {
    c = ff > 0.0 ? (float)((double)alpha * sqrt(vv / ff)) : 0.0f;
    oma = sub_rn(1.0f, alpha);
    const bool grow = (int64_t)npos > iparams[kNMin];
    dtn = grow ? fminf(mul_rn(dt, params[kFInc]), params[kDtMax]) : dt;
    alphan = grow ? mul_rn(alpha, params[kFAlpha]) : alpha;
    nposn = npos + 1;
  } else {
    dtn = fmaxf(mul_rn(dt, params[kFDec]), params[kDtMin]);
    alphan = params[kAlphaStart];
    nposn = 0;
  }

  // ---- pass 2: the longest displacement
  double dm2 = 0.0;
  for (int i = a0 + (int)threadIdx.x; i < a1; i += kWave) {
    const Kick q = fire_kick(vel, grad_new, 3 * (int64_t)i, cinv_mass[i], downhill, c, oma, dtn);
    double r2 = 0.0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) r2 += (double)q.dr[ax] * (double)q.dr[ax];
    dm2 = fmax(dm2, r2);
  }
  dm2 = wave_max(dm2, red[4]);
  const double ms = (double)params[kMaxStep];
  const float s = dm2 > ms * ms ? (float)(ms / sqrt(dm2)) : 1.0f;

  // ---- pass 3: the update
  for (int i = a0 + (int)threadIdx.x; i < a1; i += kWave) {
    const int64_t k0 = 3 * (int64_t)i;
    const Kick q = fire_kick(vel, grad_new, k0, cinv_mass[i], downhill, c, oma, dtn);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      vel[k0 + ax] = q.v2[ax];
      pos[k0 + ax] = fmaf(s, q.dr[ax], pos[k0 + ax]);
    }
  }
  if (threadIdx.x == 0) {
    mol_dt[b] = dtn;
    mol_alpha[b] = alphan;
    mol_state[4 * b + kNpos] = nposn;
    mol_state[4 * b + kNsteps] = nsteps + 1;
    mol_state[4 * b + kCalls] = calls + 1;
  }
}

__global__ __launch_bounds__(kActiveBlock) void k_fire_active(const int32_t* __restrict__ mol_state, int B,
                                                              int32_t* __restrict__ active) {
  __shared__ int red[kActiveBlock];
  int n = 0;
  for (int b = threadIdx.x; b < B; b += kActiveBlock) n += mol_state[4 * b + kDone] == 0 ? 1 : 0;
  const int total = block_sum<kActiveBlock>(n, red);
  if (threadIdx.x == 0) active[0] = total;
}

}  // namespace

extern "C" int geossl_fire_step(float* pos, float* vel, const float* grad_new, const float* energy_new, float* grad,
                                float* energy, const float* cinv_mass, const int32_t* mol_ptr, int64_t B, int64_t N,
                                const float* params, const int64_t* iparams, float* mol_dt, float* mol_alpha,
                                int32_t* mol_state, int evaluate_only, int64_t frames, float* traj_pos, float* traj_vel,
                                float* traj_energy, float* traj_fmax, float* traj_dt, float* traj_alpha,
                                int32_t* traj_npos, int32_t* traj_done, hipStream_t stream) {
  if (N < 1 || N >= (1 << 30) || B < 1 || B >= (1 << 24) || frames < 0 || pos == nullptr || vel == nullptr ||
      grad_new == nullptr || energy_new == nullptr || grad == nullptr || energy == nullptr || cinv_mass == nullptr ||
      mol_ptr == nullptr || params == nullptr || iparams == nullptr || mol_dt == nullptr || mol_alpha == nullptr ||
      mol_state == nullptr || (evaluate_only && frames < 1) ||
      (frames > 0 && (traj_pos == nullptr || traj_vel == nullptr || traj_energy == nullptr || traj_fmax == nullptr ||
                      traj_dt == nullptr || traj_alpha == nullptr || traj_npos == nullptr || traj_done == nullptr)))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fire_step, dim3((unsigned)B), dim3(kWave), 0, stream, pos, vel, grad_new, energy_new, grad, energy,
                     cinv_mass, mol_ptr, (int)B, (int)N, params, iparams, mol_dt, mol_alpha, mol_state, evaluate_only,
                     frames, traj_pos, traj_vel, traj_energy, traj_fmax, traj_dt, traj_alpha, traj_npos, traj_done);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_fire_active(const int32_t* mol_state, int64_t B, int32_t* active, hipStream_t stream) {
  if (B < 1 || B >= (1 << 24) || mol_state == nullptr || active == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fire_active, dim3(1), dim3(kActiveBlock), 0, stream, mol_state, (int)B, active);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
