"""Structure relaxation on a fine-tuned MD17 force field: B independent replicas brought to a minimum of the model's own
energy surface by FIRE, the whole step captured once and replayed, convergence decided per replica on the device.

``Minimizer(model, graph_pred_linear, batch, model_3d)`` takes the same batches as ``md.Simulator`` (a collated batch with
host sizes or a ``DeviceLoader`` handle; ragged sizes allowed).  ``run(max_steps)`` returns a ``Relaxation``; the relaxed
``positions`` can be handed to a ``Simulator`` (``examples/relax_md17.py --then_md``).

The algorithm is this project's own definition: FIRE (Bitzek et al., PRL 97, 170201) in ASE's form, mass-weighted, in the
Simulator's units (kcal/mol, A, amu, fs; a = ACCEL F / m).  Per molecule b the state is dt_b, alpha_b, npos_b, done_b
(latched) and nsteps_b; the velocity v starts at 0.  One step at positions x, with F = -dE/dx and fmax_b = max_i |F_i|:

  if done_b or fmax_b < ftol:          done_b = 1; nothing of the molecule changes            (frozen)
  else:
    P = sum F.v, vv = sum v.v, ff = sum F.F                    (over the molecule's atoms, fp64, fixed order)
    if P > 0 or vv == 0:  v = (1 - alpha) v + alpha sqrt(vv / ff) F
                          if npos > n_min: dt = min(dt f_inc, dt_max); alpha = alpha f_alpha
                          npos += 1
    else:                 v = 0; alpha = alpha_start; dt = max(dt f_dec, dt_min); npos = 0
    v += dt a ;  dr = dt v ;  s = min(1, max_step / max_i |dr_i|) ;  x += s dr ;  nsteps_b += 1

On the fused route - exactly what ``Simulator.fused`` serves: SchNet up to 255 atoms, PaiNN on the interned complete pair
list, the heads the energy-head kernel takes - a step is the force pass of ``finetune_md17._energy_and_gradient`` on the
static positions -> ``geossl_fire_step`` (csrc/relax.hip, which states the fp32 rounding sequence), and
``steps_per_replay`` such steps plus ONE ``geossl_fire_active`` are one captured graph.  The host reads one word per
replay group - the number of molecules still moving - and nothing else; the run stops after the first group that leaves it
zero, or at ``max_steps``.  The tolerance and the limits are device data: changing them needs no new capture, and the graph
reads the live parameter values of the modules (it is rebuilt when their addresses move).

The fallback route - CPU tensors, a head or width the kernels do not serve, or an ``energy_and_gradient=callable(positions)
-> (E [B], dE/dpos [N, 3])`` hook - is the same algorithm in torch operations in the dtype of the positions (fp64 allowed).

Recording (``record_every`` >= 1): frame k is the state AS STEP k record_every FOUND IT - positions, the incoming velocity,
E, fmax, dt, alpha, npos, and `converged` after the test at these positions - so frame 0 is the start of the run, and the
state after the last step is a frame when the number of steps made is a multiple of ``record_every``.

Not built (refused with the Simulator's sentences): structures above 255 atoms, PaiNN off the interned complete pair list.
Neither are constraints (fixed atoms, cells) nor other optimisers (L-BFGS, conjugate gradients)."""
from collections import namedtuple

import torch

from . import _lib, ops
from .replicas import ACCEL, GRAPH_DEFAULT_MAX_ATOMS, Replicas, default_masses

__all__ = ["Minimizer", "Relaxation", "History", "ACCEL", "default_masses", "STEPS_PER_REPLAY_DEFAULT",
           "USE_GRAPH_DEFAULT", "GRAPH_DEFAULT_MAX_ATOMS"]

# Measured defaults (tools/bench_relax.py, profiles/relax_bench.json).  steps_per_replay: the smallest value whose
# median lies within the spread of the best is 4 on five of the six shapes and 16 on one (by 0.2 %); 4 also stops a converged
# batch at most 3 steps late.  use_graph None: the Simulator's rule - replay up to GRAPH_DEFAULT_MAX_ATOMS atoms, eager
# launches above: 64 replicas of 21 atoms is the largest measured batch on which the slowest replayed run beat the fastest
# eager run (by 1.1 - 2.8x up to there); at the next measured size, 1024 replicas, all routes lie within 2 %.
STEPS_PER_REPLAY_DEFAULT = 4
USE_GRAPH_DEFAULT = None

Relaxation = namedtuple("Relaxation", "positions energy fmax converged steps history")
Relaxation.__doc__ = """``Minimizer.run``'s result: positions [N, 3] (a copy of the final ones); energy [B] and fmax [B], the
model's at those FINAL positions; converged [B] bool (latched earlier, or fmax < tolerance now); steps [B] int64, the steps
that moved each molecule since the last reset; history None or a ``History``."""
History = namedtuple("History", "positions velocities energy fmax dt alpha npos converged steps")
History.__doc__ = """Recorded frames, leading dimension R: positions, velocities [R, N, 3]; energy, fmax, dt, alpha [R, B];
npos [R, B] int; converged [R, B] bool; steps [R] int64, the number of steps launched before each frame."""

_LIMITS = ("dt_max", "dt_min", "max_step", "f_inc", "f_dec", "alpha", "f_alpha")   # the fp32 block's words 1 .. 7


def _segment_max(values, mol, B):
    return torch.zeros(B, dtype=values.dtype, device=values.device).scatter_reduce_(0, mol, values, "amax")


def _segment_sum(values, mol, B):
    return torch.zeros(B, dtype=values.dtype, device=values.device).index_add_(0, mol, values)


class Minimizer(Replicas):
    """See the module docstring.  masses: [N] in amu (None: ``default_masses(batch.x)``); fmax: the tolerance on max_i
    |F_i| in kcal/mol/A; dt, dt_max, dt_min in fs; max_step in A; alpha: alpha_start; use_graph: replay the captured steps
    (None: for batches of at most GRAPH_DEFAULT_MAX_ATOMS atoms); steps_per_replay: steps per captured graph and per word
    read; max_frames: frames the device-side history buffer holds (a longer run is copied out in segments)."""

    def __init__(self, model, graph_pred_linear, batch, model_3d="schnet", masses=None, fmax=0.05, dt=0.5, dt_max=5.0,
                 dt_min=0.01, max_step=0.1, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99,
                 use_graph=USE_GRAPH_DEFAULT, steps_per_replay=STEPS_PER_REPLAY_DEFAULT, max_frames=1024,
                 energy_and_gradient=None):
        b = self._setup(model, graph_pred_linear, batch, model_3d, masses, use_graph, steps_per_replay, max_frames,
                        energy_and_gradient)
        self._dt0, self._ftol, self._n_min = float(dt), float(fmax), int(n_min)
        self._limits = dict(dt_max=float(dt_max), dt_min=float(dt_min), max_step=float(max_step), f_inc=float(f_inc),
                            f_dec=float(f_dec), alpha=float(alpha), f_alpha=float(f_alpha))
        self._check_settings()
        self._calls = 0
        self._route(b)
        self._write_params()
        self.reset()

    def _check_settings(self):
        L = self._limits
        if not (self._ftol >= 0 and self._dt0 > 0 and 0 < L["dt_min"] <= L["dt_max"] and L["max_step"] > 0
                and L["f_inc"] >= 1 and 0 < L["f_dec"] < 1 and 0 <= L["alpha"] <= 1 and 0 < L["f_alpha"] <= 1
                and self._n_min >= 0):
            raise ValueError("Minimizer: fmax >= 0, dt > 0, 0 < dt_min <= dt_max, max_step > 0, f_inc >= 1, 0 < f_dec < 1, "
                             "0 <= alpha <= 1, 0 < f_alpha <= 1 and n_min >= 0; got fmax %r, dt %r, n_min %r, %r"
                             % (self._ftol, self._dt0, self._n_min, L))

    # ---- the two routes' own state (the common part: Replicas._init_fused / _init_fallback)
    def _alloc_fused(self, dev):
        self._params = torch.zeros(ops.FIRE_PARAM_WORDS, dtype=torch.float32, device=dev)
        self._iparams = torch.zeros(ops.FIRE_IPARAM_WORDS, dtype=torch.int64, device=dev)
        self._mol_dt = torch.zeros(self.B, dtype=torch.float32, device=dev)
        self._mol_alpha = torch.zeros(self.B, dtype=torch.float32, device=dev)
        self._mol_state = torch.zeros(self.B, ops.FIRE_MOL_WORDS, dtype=torch.int32, device=dev)
        self._active = torch.zeros(1, dtype=torch.int32, device=dev)
        self._frames = ops.fire_frames(self.max_frames, self.N, self.B, dev)
        self._final = ops.fire_frames(1, self.N, self.B, dev)

    def _alloc_fallback(self):
        dev, dt = self._pos.device, self._pos.dtype
        self._mol_dt = torch.zeros(self.B, dtype=dt, device=dev)
        self._mol_alpha = torch.zeros(self.B, dtype=dt, device=dev)
        self._mol_state = torch.zeros(self.B, ops.FIRE_MOL_WORDS, dtype=torch.int64, device=dev)

    # ---- settings and state
    def _write_params(self):
        if not self.fused:
            return
        L = self._limits
        self._params.copy_(torch.tensor([self._ftol] + [L[k] for k in _LIMITS], dtype=torch.float32))
        self._iparams[ops.FIRE_N_MIN:ops.FIRE_N_MIN + 1].fill_(self._n_min)

    def set_tolerance(self, fmax):
        """The tolerance on max_i |F_i| of the following steps (device data: no new capture).  Latched molecules stay
        latched: ``reset`` releases them."""
        self._ftol = float(fmax)
        self._check_settings()
        self._write_params()

    def set_limits(self, dt_max=None, dt_min=None, max_step=None, n_min=None, f_inc=None, f_dec=None, alpha=None,
                   f_alpha=None):
        """Any of the step's limits for the following steps (device data: no new capture); None keeps a value."""
        given = dict(dt_max=dt_max, dt_min=dt_min, max_step=max_step, f_inc=f_inc, f_dec=f_dec, alpha=alpha,
                     f_alpha=f_alpha)
        old = dict(self._limits), self._n_min
        self._limits.update({k: float(v) for k, v in given.items() if v is not None})
        self._n_min = self._n_min if n_min is None else int(n_min)
        try:
            self._check_settings()
        except ValueError:
            self._limits, self._n_min = old
            raise
        self._write_params()

    def reset(self):
        """Velocities to 0, every molecule's dt, alpha and counters to their start, the latches released."""
        self._vel.zero_()
        self._mol_dt.fill_(self._dt0)
        self._mol_alpha.fill_(self._limits["alpha"])
        self._mol_state.zero_()
        self._calls = 0
        return self

    @property
    def steps(self):
        """[B] int64: the steps that moved each molecule since the last reset."""
        return self._mol_state[:, ops.FIRE_NSTEPS].long()

    # ---- the fused route
    def _step(self):
        energy, grad = self._force()
        ops.fire_step(self._pos, self._vel, grad, energy, self._grad, self._energy, self._cinv, self._mol_ptr,
                      self._params, self._iparams, self._mol_dt, self._mol_alpha, self._mol_state, self._frames)

    def _evaluate(self):
        """The force pass at the current positions (live parameters), the convergence test and its frame into `_final`."""
        energy, grad = self._force()
        ops.fire_step(self._pos, self._vel, grad, energy, self._grad, self._energy, self._cinv, self._mol_ptr,
                      self._params, self._iparams, self._mol_dt, self._mol_alpha, self._mol_state, self._final,
                      evaluate_only=True)

    def _group(self, n):
        for _ in range(n):
            self._step()
        ops.fire_active(self._mol_state, self._active)

    def _capture_group(self, U):
        def dry_run():   # (the two kernels on copies)
            pos, vel, st = self._pos.clone(), self._vel.clone(), self._mol_state.clone()
            ops.fire_step(pos, vel, self._grad, self._energy, self._grad, self._energy, self._cinv, self._mol_ptr,
                          self._params, self._iparams, self._mol_dt.clone(), self._mol_alpha.clone(), st)
            ops.fire_active(st, self._active.clone())
        return self._capture("the relaxation step", dry_run, lambda: self._group(U))

    def _run_fused(self, max_steps, every):
        U, cap, c0 = self.steps_per_replay, self.max_frames, self._calls
        graph = self._graph(("fire", U), lambda: self._capture_group(U)) if max_steps >= U else None
        word = lambda k, v: self._iparams[k:k + 1].fill_(int(v))
        word(ops.FIRE_RECORD_EVERY, every)
        word(ops.FIRE_FIRST, c0)
        out = [[] for _ in self._frames]
        done, f0, active = 0, 0, 1

        def flush():   # the frames recorded so far and not yet copied out; slot 0 moves behind them
            nonlocal f0
            have = -(-done // every) if every else 0
            if have > f0:
                for o, fr in zip(out, self._frames):
                    o.append(fr[:have - f0].clone())
                f0 = have
                word(ops.FIRE_FIRST, c0 + f0 * every)
        while active and done < max_steps:   # a group: U steps (the run's last: the rest), whatever the buffer holds
            target = min(done + U, max_steps)
            if graph is not None and target - done == U and (not every or target <= (f0 + cap) * every):
                graph.replay()
                done = target
            else:
                while done < target:
                    n = min(target, (f0 + cap) * every) - done if every else target - done
                    for _ in range(n):
                        self._step()
                    done += n
                    if every and done == (f0 + cap) * every:
                        flush()
                ops.fire_active(self._mol_state, self._active)
            if every and done == (f0 + cap) * every:
                flush()
            active = int(self._active.item())   # the one word read per group
        flush()
        self._calls += done
        self._evaluate()
        if every and done % every == 0:   # the state after the last step is a frame of its own
            for o, fr in zip(out, self._final):
                o.append(fr.clone())
        _lib.poll_status(self.model)
        final = [t[0] for t in self._final]
        return final[2].clone(), final[3].clone(), final[7] != 0, ([torch.cat(o) for o in out] if every else None), done

    # ---- the fallback route
    def _found(self):
        """The step's view of the current positions -> (F, energy, fmax, converged)."""
        energy, grad = self._force_fallback()
        F = -grad.to(self._pos.dtype)
        fmax = _segment_max((F * F).sum(1), self._mol, self.B).sqrt()
        return F, energy.to(self._pos.dtype), fmax, (self._mol_state[:, ops.FIRE_DONE] != 0) | (fmax < self._ftol)

    def _frame(self, energy, fmax, conv):
        st = self._mol_state
        return (self._pos.clone(), self._vel.clone(), energy.clone(), fmax.clone(), self._mol_dt.clone(),
                self._mol_alpha.clone(), st[:, ops.FIRE_NPOS].to(torch.int32), conv.to(torch.int32))

    def _step_fallback(self, F, conv):
        L, mol, st = self._limits, self._mol, self._mol_state
        v, dt, alpha, npos = self._vel, self._mol_dt, self._mol_alpha, st[:, ops.FIRE_NPOS]
        P, vv, ff = (_segment_sum((a * b).sum(1), mol, self.B) for a, b in ((F, v), (v, v), (F, F)))
        down = (P > 0) | (vv == 0)
        c = torch.where(ff > 0, alpha * torch.sqrt(vv / torch.where(ff > 0, ff, torch.ones_like(ff))), torch.zeros_like(ff))
        v1 = torch.where(down[mol, None], (1 - alpha)[mol, None] * v + c[mol, None] * F, torch.zeros_like(v))
        grow = down & (npos > self._n_min)
        dt_n = torch.where(down, torch.where(grow, (dt * L["f_inc"]).clamp(max=L["dt_max"]), dt),
                           (dt * L["f_dec"]).clamp(min=L["dt_min"]))
        alpha_n = torch.where(down, torch.where(grow, alpha * L["f_alpha"], alpha), torch.full_like(alpha, L["alpha"]))
        v2 = v1 + dt_n[mol, None] * (F * self._cinv)
        dr = dt_n[mol, None] * v2
        dm = _segment_max((dr * dr).sum(1), mol, self.B).sqrt()
        s = torch.where(dm > L["max_step"], L["max_step"] / torch.where(dm > 0, dm, torch.ones_like(dm)), torch.ones_like(dm))
        move = ~conv
        am = move[mol, None]
        self._vel.copy_(torch.where(am, v2, v))
        self._pos.copy_(torch.where(am, self._pos + s[mol, None] * dr, self._pos))
        self._mol_dt.copy_(torch.where(move, dt_n, dt))
        self._mol_alpha.copy_(torch.where(move, alpha_n, alpha))
        st[:, ops.FIRE_NPOS] = torch.where(move, torch.where(down, npos + 1, torch.zeros_like(npos)), npos)
        st[:, ops.FIRE_DONE] = conv.to(st.dtype)
        st[:, ops.FIRE_NSTEPS] += move.to(st.dtype)
        st[:, ops.FIRE_CALLS] += 1

    def _run_fallback(self, max_steps, every):
        U, frames, done, active = self.steps_per_replay, [], 0, 1
        with torch.no_grad():
            while active and done < max_steps:
                for _ in range(min(U, max_steps - done)):
                    F, energy, fmax, conv = self._found()
                    if every and done % every == 0:
                        frames.append(self._frame(energy, fmax, conv))
                    self._step_fallback(F, conv)
                    done += 1
                active = int((self._mol_state[:, ops.FIRE_DONE] == 0).sum())
            self._calls += done
            _, energy, fmax, conv = self._found()
            if every and done % every == 0:
                frames.append(self._frame(energy, fmax, conv))
        hist = [torch.stack([f[i] for f in frames]) for i in range(8)] if every else None
        return energy, fmax, conv, hist, done

    # ---- run
    def run(self, max_steps, record_every=0):
        """Up to `max_steps` steps from the current state (a second run continues where the first ended) -> Relaxation.
        The run stops after the first group of ``steps_per_replay`` steps that leaves no molecule moving.  record_every
        >= 1: ``history`` holds the frames of the module docstring; 0: None."""
        max_steps, every = int(max_steps), int(record_every)
        if max_steps < 0 or every < 0:
            raise ValueError("run: max_steps >= 0 and record_every >= 0")
        c0 = self._calls
        energy, fmax, conv, hist, done = (self._run_fused if self.fused else self._run_fallback)(max_steps, every)
        history = None
        if hist is not None:
            count = torch.arange(c0, c0 + done + 1, every, dtype=torch.int64, device=hist[0].device)[:hist[0].size(0)]
            history = History(*hist[:7], hist[7] != 0, count)
        return Relaxation(self._pos.clone(), energy, fmax, conv, self.steps, history)
