// Molecular dynamics of B independent replicas on a force field (geossl_amd/md.py): the two halves of a velocity-Verlet
// (NVE) or BAOAB Langevin (NVT) step around the force pass, the thermostat's draws, the kinetic energies and the
// trajectory frames.  An MD step is  geossl_md_advance -> force pass on pos -> geossl_md_finish ; all of its state is
// device memory, so a captured graph of these launches replays without host work:
//
//   pos, vel [N][3] fp32      positions (the force pass's input) and velocities; between advance and finish vel holds
//                             the half-kicked (Langevin: thermostatted) velocity
//   grad [N][3], energy [B]   dE/dpos and E at pos, kept from the last finish (the next advance's acceleration)
//   cinv_mass [N] fp32        ACCEL / m (A fs^-2 per kcal mol^-1 A^-1), rsqrt_mass [N] fp32 = m^-1/2
//   ke_coef [N] fp64          m / (2 ACCEL): KE = sum ke_coef |v|^2 in kcal/mol
//   params [4] fp32           dt, c1 = exp(-gamma dt), sigma_T = sqrt(1 - c1^2) sqrt(KB T ACCEL), unused
//   state [8] int64           0: steps completed (advance reads it), 1: the step in flight + 1 (advance writes it, finish
//                             reads it and writes it back to word 0), 2: Philox seed, 3: record_every, 4: the step of
//                             trajectory slot 0, 5: thermostat (0 NVE, 1 Langevin), 6-7 unused
//
// k_md_advance (a thread per atom), with hdt = dt / 2 and every product that is not part of an fma rounded on its own:
//   a = (-grad) cinv_mass ; vh = fma(hdt, a, v)
//   NVE:       x = fma(dt, vh, x)                                                               vel = vh
//   Langevin:  x = fma(hdt, vh, x) ; vo = fma(c1, vh, (sigma_T rsqrt_mass) xi) ; x = fma(hdt, vo, x)   vel = vo
//   xi: the first three normals of Philox-4x32-10 at the counter (atom, step_lo, step_hi, 0) under the seed's two words,
//   Box-Muller as in philox.h; step = word 0.
// k_md_finish (one wave per molecule, lane l takes the atoms l, l + 64, ...):
//   a = (-grad_new) cinv_mass ; v = fma(hdt, a, vel) ; grad = grad_new, energy = energy_new
//   KE_b = sum over the molecule's atoms of ke_coef (vx^2 + vy^2 + vz^2) in fp64: per lane in atom order, then a fixed
//   tree over the 64 lanes in LDS - no atomics, the same bits every launch.
//   With s = word 1 and d = s - first: if d >= 0, d % record_every == 0 and d / record_every < frames, the frame (pos,
//   vel, energy_new, KE) goes into that slot of the trajectory buffers.  record_only: no kick, s = word 0, slot 0 is
//   written, no step word changes (the frame of a run's start).
// The step words: every block of advance reads word 0 and its first thread alone writes word 1; every block of finish
// reads word 1 and its first thread alone writes word 0 - no launch reads a word one of its own blocks writes.  All
// stores are plain vector stores.
#include "geossl_hip.h"
#include "head_common.h"
#include "philox.h"

using namespace geossl;

namespace {

constexpr int kAdvanceBlock = 256;
constexpr int kWave = 64;

enum StateWord { kStepDone = 0, kStepNext = 1, kSeed = 2, kRecordEvery = 3, kFirst = 4, kThermostat = 5 };

__device__ __forceinline__ void md_normals(uint64_t seed, uint64_t step, uint32_t atom, float (&xi)[3]) {
  const uint4 r = philox4x32_10(make_uint4(atom, (uint32_t)step, (uint32_t)(step >> 32), 0u),
                                make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  float z[4];
  normal4(r, z);
  xi[0] = z[0]; xi[1] = z[1]; xi[2] = z[2];
}

__global__ __launch_bounds__(kAdvanceBlock) void k_md_normals(uint64_t seed, uint64_t step, int N,
                                                              float* __restrict__ out) {
  const int i = blockIdx.x * kAdvanceBlock + threadIdx.x;
  if (i >= N) return;
  float xi[3];
  md_normals(seed, step, (uint32_t)i, xi);
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * (int64_t)i + c] = xi[c];
}

__global__ __launch_bounds__(kAdvanceBlock) void k_md_advance(float* __restrict__ pos, float* __restrict__ vel,
                                                              const float* __restrict__ grad,
                                                              const float* __restrict__ cinv_mass,
                                                              const float* __restrict__ rsqrt_mass,
                                                              const float* __restrict__ params,
                                                              int64_t* __restrict__ state, int N) {
  const int64_t step = state[kStepDone];
  const bool langevin = state[kThermostat] != 0;
  const uint64_t seed = (uint64_t)state[kSeed];
  if (blockIdx.x == 0 && threadIdx.x == 0) state[kStepNext] = step + 1;
  const int i = blockIdx.x * kAdvanceBlock + threadIdx.x;
  if (i >= N) return;
  const float dt = params[0], c1 = params[1], sigma = params[2];
  const float hdt = 0.5f * dt;
  const float cinv = cinv_mass[i];
  float xi[3] = {0.0f, 0.0f, 0.0f};
  float s = 0.0f;
  if (langevin) {
    md_normals(seed, (uint64_t)step, (uint32_t)i, xi);
    s = mul_rn(sigma, rsqrt_mass[i]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int64_t k = 3 * (int64_t)i + c;
    const float a = mul_rn(-grad[k], cinv);
    const float vh = fmaf(hdt, a, vel[k]);
    float x = pos[k];
    if (langevin) {
      x = fmaf(hdt, vh, x);
      const float vo = fmaf(c1, vh, mul_rn(s, xi[c]));
      x = fmaf(hdt, vo, x);
      vel[k] = vo;
    } else {
      x = fmaf(dt, vh, x);
      vel[k] = vh;
    }
    pos[k] = x;
  }
}

// grad_new / energy_new may be grad / energy themselves (no __restrict__ on the four)
__global__ __launch_bounds__(kWave) void k_md_finish(const float* __restrict__ pos, float* __restrict__ vel,
                                                     const float* grad_new, const float* energy_new, float* grad,
                                                     float* energy, const float* __restrict__ cinv_mass,
                                                     const double* __restrict__ ke_coef,
                                                     const int32_t* __restrict__ mol_ptr, int B, int N,
                                                     const float* __restrict__ params, int64_t* __restrict__ state,
                                                     int record_only, int64_t frames, float* __restrict__ traj_pos,
                                                     float* __restrict__ traj_vel, float* __restrict__ traj_pot,
                                                     double* __restrict__ traj_kin) {
  __shared__ double red[kWave];
  const int b = blockIdx.x;
  const int64_t s = state[record_only ? kStepDone : kStepNext];
  const int64_t every = state[kRecordEvery], d = s - state[kFirst];
  if (!record_only && b == 0 && threadIdx.x == 0) state[kStepDone] = s;
  int64_t slot = -1;
  if (record_only) slot = 0;
  else if (every >= 1 && d >= 0 && d % every == 0) slot = d / every;
  const bool record = traj_pos != nullptr && slot >= 0 && slot < frames;
  const float hdt = 0.5f * params[0];
  const int a0 = max(min(mol_ptr[b], N), 0), a1 = max(min(mol_ptr[b + 1], N), a0);
  double ke = 0.0;
  for (int i = a0 + (int)threadIdx.x; i < a1; i += kWave) {
    const float cinv = cinv_mass[i];
    double v2 = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t k = 3 * (int64_t)i + c;
      const float g = grad_new[k];
      float v = vel[k];
      if (!record_only) {
        v = fmaf(hdt, mul_rn(-g, cinv), v);
        vel[k] = v;
      }
      if (grad != grad_new) grad[k] = g;
      v2 += (double)v * (double)v;
      if (record) {
        const int64_t t = slot * 3 * (int64_t)N + k;
        traj_pos[t] = pos[k];
        traj_vel[t] = v;
      }
    }
    ke += ke_coef[i] * v2;
  }
  const double total = block_sum<kWave>(ke, red);
  if (threadIdx.x == 0) {
    const float e = energy_new[b];
    if (energy != energy_new) energy[b] = e;
    if (record) {
      traj_pot[slot * B + b] = e;
      traj_kin[slot * B + b] = total;
    }
  }
}

}  // namespace

extern "C" int geossl_md_normals(uint64_t seed, uint64_t step, int64_t N, float* out, hipStream_t stream) {
  if (N < 0 || N >= (1 << 30) || (N > 0 && out == nullptr)) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  hipLaunchKernelGGL(k_md_normals, dim3((unsigned)((N + kAdvanceBlock - 1) / kAdvanceBlock)), dim3(kAdvanceBlock), 0,
                     stream, seed, step, (int)N, out);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_md_advance(float* pos, float* vel, const float* grad, const float* cinv_mass,
                                 const float* rsqrt_mass, const float* params, int64_t* state, int64_t N,
                                 hipStream_t stream) {
  if (N < 1 || N >= (1 << 30) || pos == nullptr || vel == nullptr || grad == nullptr || cinv_mass == nullptr ||
      rsqrt_mass == nullptr || params == nullptr || state == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_md_advance, dim3((unsigned)((N + kAdvanceBlock - 1) / kAdvanceBlock)), dim3(kAdvanceBlock), 0,
                     stream, pos, vel, grad, cinv_mass, rsqrt_mass, params, state, (int)N);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}

extern "C" int geossl_md_finish(const float* pos, float* vel, const float* grad_new, const float* energy_new,
                                float* grad, float* energy, const float* cinv_mass, const double* ke_coef,
                                const int32_t* mol_ptr, int64_t B, int64_t N, const float* params, int64_t* state,
                                int record_only, int64_t frames, float* traj_pos, float* traj_vel, float* traj_pot,
                                double* traj_kin, hipStream_t stream) {
  if (N < 1 || N >= (1 << 30) || B < 1 || B >= (1 << 24) || frames < 0 || pos == nullptr || vel == nullptr ||
      grad_new == nullptr || energy_new == nullptr || grad == nullptr || energy == nullptr || cinv_mass == nullptr ||
      ke_coef == nullptr || mol_ptr == nullptr || params == nullptr || state == nullptr ||
      (frames > 0 && (traj_pos == nullptr || traj_vel == nullptr || traj_pot == nullptr || traj_kin == nullptr)))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_md_finish, dim3((unsigned)B), dim3(kWave), 0, stream, pos, vel, grad_new, energy_new, grad, energy,
                     cinv_mass, ke_coef, mol_ptr, (int)B, (int)N, params, state, record_only, frames, traj_pos, traj_vel,
                     traj_pot, traj_kin);
  GEOSSL_CHECK_LAUNCH();
  return 0;
}
