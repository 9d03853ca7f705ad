"""Molecular dynamics on a fine-tuned MD17 force field: NVE (velocity Verlet) and NVT (Langevin, BAOAB splitting) of B
independent replicas, the whole MD step captured once and replayed.

``Simulator(model, graph_pred_linear, batch, model_3d)`` takes the molecules of `batch` (a collated batch with host sizes
or a ``DeviceLoader`` handle; ragged sizes allowed) as B replicas.  On the fused route - what ``predict_MD17`` serves on
kernels alone (``finetune_md17._fused_predict_ok``) - positions, velocities, the gradient, parameters and step counter
live in device buffers, an MD step is  ``geossl_md_advance`` -> the force pass of ``finetune_md17._energy_and_gradient``
on the static positions -> ``geossl_md_finish``  (csrc/md_integrate.hip), and ``steps_per_replay`` such steps are ONE
captured graph: ``run`` replays it, finishes a remainder with eager launches of the same kernels, and reads nothing
back.  dt, the thermostat and ``record_every`` are device data: changing them needs no new capture, and the graph reads
the live parameter values of the modules (training between two runs needs none either while their addresses stay).

Units are MD17's: kcal/mol, A, amu, fs.  ``ACCEL`` converts kcal mol^-1 A^-1 amu^-1 into A fs^-2, ``KB`` is Boltzmann's
constant in kcal mol^-1 K^-1; the temperature of a molecule of n atoms is 2 KE / (KB dof) with dof = 3 n - 3 (n > 1:
``thermalize`` removes the centre-of-mass velocity and an invariant model keeps it zero) or 3 n (n = 1).

The step (hdt = dt / 2, a(x) = -ACCEL dE/dx / m):
  NVE       vh = v + hdt a(x);  x' = x + dt vh;                                           v' = vh + hdt a(x')
  Langevin  vh = v + hdt a(x);  xh = x + hdt vh;  vo = c1 vh + sigma_T m^-1/2 xi;  x' = xh + hdt vo;  v' = vo + hdt a(x')
with c1 = exp(-gamma dt), sigma_T = sqrt(1 - c1^2) sqrt(KB T ACCEL) and xi standard normals: on the fused route
Philox-4x32-10 at the counter (atom, step) under the seed (``ops.md_normals`` returns them), the same bits every run.

The fallback route - CPU tensors, a head or width the kernels do not serve, or an ``energy_and_gradient=callable(positions)
-> (E [B], dE/dpos [N, 3])`` hook - is the same algorithm in torch operations, in the dtype of the positions (fp64
allowed), on ``md17_energy_force_aten(..., create_graph=False)``.  Its Langevin draws come from ``torch.randn(generator=)``
seeded with `seed`: a DIFFERENT stream from the device's, so a fallback trajectory is not the fused one sample by sample.

Not built (refused with a sentence): structures above 255 atoms, and PaiNN off the interned complete pair list (one size
n <= 33) - its radius edges would have to be rebuilt every step."""
import math
from collections import namedtuple

import torch

from . import _lib, ops
from .replicas import ACCEL, GRAPH_DEFAULT_MAX_ATOMS, MAX_ATOMS, Replicas, default_masses

__all__ = ["Simulator", "Trajectory", "ACCEL", "KB", "default_masses", "STEPS_PER_REPLAY_DEFAULT", "USE_GRAPH_DEFAULT",
           "GRAPH_DEFAULT_MAX_ATOMS"]

KB = 8.31446261815324 / 4184          # kcal mol^-1 K^-1
# Measured defaults (tools/bench_md.py, profiles/md_bench.json).  steps_per_replay: the smallest value whose
# median lies within the spread of the best is 4 on seven of the twelve shapes and 16 on five; nothing separates them by
# more than 1.3 %.  use_graph None: replay up to GRAPH_DEFAULT_MAX_ATOMS (replicas.py), eager launches above.  The
# threshold is ONE data point: 64 replicas of 21 atoms is the largest measured batch on which the slowest replayed run beat
# the fastest run of the loop on predict_MD17 (with one exception below it, by 0.3 %); the next measured size, 1024
# replicas, has replay, eager and that loop within 2 % of one another; nothing in between was measured.
STEPS_PER_REPLAY_DEFAULT = 4
USE_GRAPH_DEFAULT = None

Trajectory = namedtuple("Trajectory", "positions velocities potential kinetic temperature steps")
Trajectory.__doc__ = """Recorded frames of ``Simulator.run``: positions, velocities [R, N, 3]; potential [R, B] (fp32: the
model's energies at the recorded positions); kinetic [R, B] fp64; temperature [R, B] fp64; steps [R] int64 (the step
counter of each frame).  Tensors on the simulator's device."""


class Simulator(Replicas):
    """See the module docstring.  masses: [N] in amu (None: ``default_masses(batch.x)``); dt in fs; thermostat None (NVE)
    or ("langevin", T in K, gamma in fs^-1); seed: of the thermostat's stream (None: drawn from torch's generator);
    use_graph: replay the captured step (None: for batches of at most GRAPH_DEFAULT_MAX_ATOMS atoms, where it was measured
    to win); steps_per_replay: MD steps in the captured graph; max_frames: frames the device-side trajectory buffer holds (a
    longer run is copied out in segments)."""

    def __init__(self, model, graph_pred_linear, batch, model_3d="schnet", masses=None, dt=0.5, thermostat=None,
                 seed=None, use_graph=USE_GRAPH_DEFAULT, steps_per_replay=STEPS_PER_REPLAY_DEFAULT, max_frames=1024,
                 energy_and_gradient=None):
        b = self._setup(model, graph_pred_linear, batch, model_3d, masses, use_graph, steps_per_replay, max_frames,
                        energy_and_gradient)
        self.dof = torch.tensor([3 * n - 3 if n > 1 else 3 * n for n in self.sizes], dtype=torch.float64)
        self.seed = int(torch.randint(0, 2 ** 62, (1,))) if seed is None else int(seed)
        if not 0 <= self.seed < 2 ** 63:
            raise ValueError("Simulator: seed is an integer in [0, 2^63) (a word of the int64 state buffer), got %d"
                             % self.seed)
        self._steps = 0
        self._dt, self._thermostat = float(dt), None
        self._route(b)
        self.set_dt(dt)
        if thermostat is None:
            self.set_thermostat()
        else:
            kind, T, gamma = thermostat
            if kind != "langevin":
                raise ValueError("Simulator: thermostat is None or (\"langevin\", T, gamma), got %r" % (kind,))
            self.set_thermostat(T=T, gamma=gamma)

    # ---- the two routes' own state (the common part: Replicas._init_fused / _init_fallback)
    def _alloc_fused(self, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        self._rsqrt = self.masses.rsqrt().to(**f32)
        self._ke_coef = (self.masses / (2.0 * ACCEL)).to(dev)
        self._params = torch.zeros(ops.MD_PARAM_WORDS, **f32)
        state = torch.zeros(ops.MD_STATE_WORDS, dtype=torch.int64)
        state[ops.MD_SEED], state[ops.MD_RECORD_EVERY] = self.seed, 1
        self._state = state.to(dev)
        R = self.max_frames
        self._frames = (torch.zeros(R, self.N, 3, **f32), torch.zeros(R, self.N, 3, **f32), torch.zeros(R, self.B, **f32),
                        torch.zeros(R, self.B, dtype=torch.float64, device=dev))

    def _alloc_fallback(self):
        dev, dt = self._pos.device, self._pos.dtype
        self._rsqrt = self.masses.rsqrt().to(device=dev, dtype=dt)[:, None]
        self._ke_coef = (self.masses / (2.0 * ACCEL)).to(dev)
        self._gen = torch.Generator().manual_seed(self.seed % (2 ** 63))

    # ---- state
    @property
    def step_count(self):
        return self._steps

    def set_velocities(self, v):
        v = torch.as_tensor(v)
        if tuple(v.shape) != (self.N, 3):
            raise ValueError("set_velocities: [%d, 3], got %s" % (self.N, tuple(v.shape)))
        self._vel.copy_(v.to(self._vel))

    def thermalize(self, T, generator=None):
        """Maxwell-Boltzmann velocities at T kelvin: per component N(0, KB T ACCEL / m), drawn on the host in fp64 from
        `generator` (None: torch's default); then every molecule of more than one atom loses its centre-of-mass velocity."""
        m = self.masses[:, None]
        v = torch.randn(self.N, 3, dtype=torch.float64, generator=generator) * torch.sqrt(KB * float(T) * ACCEL / m)
        mol = torch.repeat_interleave(torch.arange(self.B), torch.tensor(self.sizes))
        p = torch.zeros(self.B, 3, dtype=torch.float64).index_add_(0, mol, m * v)
        mt = torch.zeros(self.B, 1, dtype=torch.float64).index_add_(0, mol, m)
        many = torch.tensor(self.sizes)[:, None] > 1
        v = v - torch.where(many, p / mt, torch.zeros_like(p))[mol]
        self.set_velocities(v)
        return self

    def set_dt(self, dt):
        """The time step in fs of the following steps (device data: no new capture)."""
        self._dt = float(dt)
        self._write_params()

    def set_thermostat(self, T=None, gamma=None):
        """Langevin at T kelvin with friction gamma per fs for the following steps; both None: NVE.  Device data: no
        new capture."""
        if (T is None) != (gamma is None):
            raise ValueError("set_thermostat: T and gamma together, or neither (NVE)")
        self._thermostat = None if T is None else (float(T), float(gamma))
        self._write_params()

    def _coefficients(self):
        """(dt, c1, sigma_T) in fp64."""
        if self._thermostat is None:
            return self._dt, 1.0, 0.0
        T, gamma = self._thermostat
        c1 = math.exp(-gamma * self._dt)
        return self._dt, c1, math.sqrt(1.0 - c1 * c1) * math.sqrt(KB * T * ACCEL)

    def _write_params(self):
        if not self.fused:
            return
        dt, c1, sigma = self._coefficients()
        self._params.copy_(torch.tensor([dt, c1, sigma, 0.0], dtype=torch.float32))
        self._state[ops.MD_THERMOSTAT:ops.MD_THERMOSTAT + 1].fill_(0 if self._thermostat is None else 1)

    # ---- the fused route
    def _step(self):
        ops.md_advance(self._pos, self._vel, self._grad, self._cinv, self._rsqrt, self._params, self._state)
        energy, grad = self._force()
        ops.md_finish(self._pos, self._vel, grad, energy, self._grad, self._energy, self._cinv, self._ke_coef,
                      self._mol_ptr, self._params, self._state, self._frames)

    def _record_start(self):
        """The force pass at the current positions (live parameters) and frame 0 of a run."""
        energy, grad = self._force()
        ops.md_finish(self._pos, self._vel, grad, energy, self._grad, self._energy, self._cinv, self._ke_coef,
                      self._mol_ptr, self._params, self._state, self._frames, record_only=True)

    def _capture_steps(self, U):
        def dry_run():   # (the two integrator kernels on copies)
            pos, vel, state = self._pos.clone(), self._vel.clone(), self._state.clone()
            ops.md_advance(pos, vel, self._grad, self._cinv, self._rsqrt, self._params, state)
            ops.md_finish(pos, vel, self._grad, self._energy, self._grad, self._energy, self._cinv, self._ke_coef,
                          self._mol_ptr, self._params, state)

        def steps():
            for _ in range(U):
                self._step()
        return self._capture("the MD step", dry_run, steps)

    def _step_graph(self):
        U = self.steps_per_replay
        return self._graph(("md", U), lambda: self._capture_steps(U))

    def _advance_fused(self, n, graph):
        U = self.steps_per_replay
        q, r = divmod(n, U) if graph is not None else (0, n)
        for _ in range(q):
            graph.replay()
        for _ in range(r):
            self._step()

    def _run_fused(self, steps, every):
        R = steps // every + 1
        dev, first = self._pos.device, self._steps
        out = (torch.empty(R, self.N, 3, dtype=torch.float32, device=dev),
               torch.empty(R, self.N, 3, dtype=torch.float32, device=dev),
               torch.empty(R, self.B, dtype=torch.float32, device=dev),
               torch.empty(R, self.B, dtype=torch.float64, device=dev))
        graph = self._step_graph() if steps >= self.steps_per_replay else None
        word = lambda k, v: self._state[k:k + 1].fill_(int(v))
        word(ops.MD_RECORD_EVERY, every)
        word(ops.MD_FIRST, first)
        self._record_start()
        cap, f0, done = self.max_frames, 0, 0
        while f0 < R:
            nf = min(cap, R - f0)
            if f0 > 0:
                word(ops.MD_FIRST, first + f0 * every)
            target = (f0 + nf - 1) * every if f0 + nf < R else steps
            self._advance_fused(target - done, graph)
            done = target
            for o, fr in zip(out, self._frames):
                o[f0:f0 + nf].copy_(fr[:nf])
            f0 += nf
        self._steps += steps
        _lib.poll_status(self.model)
        return out

    # ---- the fallback route
    def _kinetic(self):
        v2 = self._vel.double().pow(2).sum(1)
        return torch.zeros(self.B, dtype=torch.float64, device=v2.device).index_add_(0, self._mol, self._ke_coef * v2)

    def _run_fallback(self, steps, every):
        pos, vel = self._pos, self._vel
        with torch.no_grad():
            energy, grad = self._force_fallback()
            frames = [(pos.clone(), vel.clone(), energy.float().clone(), self._kinetic())]
            for k in range(1, steps + 1):
                dt, c1, sigma = self._coefficients()
                hdt = 0.5 * dt
                vel.add_(-grad * self._cinv, alpha=hdt)
                if self._thermostat is None:
                    pos.add_(vel, alpha=dt)
                else:
                    pos.add_(vel, alpha=hdt)
                    xi = torch.randn(self.N, 3, dtype=torch.float64, generator=self._gen).to(vel)
                    vel.mul_(c1).add_(sigma * self._rsqrt * xi)
                    pos.add_(vel, alpha=hdt)
                energy, grad = self._force_fallback()
                vel.add_(-grad * self._cinv, alpha=hdt)
                if k % every == 0:
                    frames.append((pos.clone(), vel.clone(), energy.float().clone(), self._kinetic()))
        self._steps += steps
        return tuple(torch.stack([f[i] for f in frames]) for i in range(4))

    # ---- run
    def run(self, steps, record_every=1):
        """`steps` MD steps from the current state -> Trajectory of the frames at the steps step_count + k record_every,
        k = 0 (the state the run starts from) ... steps // record_every.  The fused route reads nothing back."""
        steps, every = int(steps), int(record_every)
        if steps < 0 or every < 1:
            raise ValueError("run: steps >= 0 and record_every >= 1")
        first = self._steps
        pos, vel, pot, kin = (self._run_fused if self.fused else self._run_fallback)(steps, every)
        temperature = 2.0 * kin / (KB * self.dof.to(kin.device))
        count = torch.arange(first, first + steps + 1, every, dtype=torch.int64, device=kin.device)
        return Trajectory(pos, vel, pot, kin, temperature, count)
