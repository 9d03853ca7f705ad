"""float64 restatement of the FIRE step of geossl_amd/relax.py, written from its definition, the fp32 restatement of the
state words, and the one-step check the relaxation tests share.

Units: kcal/mol, A, amu, fs; a = ACCEL F / m.  Per molecule (dt, alpha, npos, done, nsteps), v = 0 at the start:
  if done or fmax < ftol:          done = 1; nothing of the molecule changes
  else:  P = sum F.v, vv = sum v.v, ff = sum F.F
         P > 0 or vv == 0:  v = (1 - alpha) v + alpha sqrt(vv / ff) F;  if npos > n_min: dt = min(dt f_inc, dt_max),
                            alpha = alpha f_alpha;  npos += 1
         else:              v = 0; alpha = alpha_start; dt = max(dt f_dec, dt_min); npos = 0
         v += dt a;  dr = dt v;  s = min(1, max_step / max_i |dr_i|);  x += s dr;  nsteps += 1

`one_step` takes two consecutive RECORDED frames (frame k: x, v, dt, alpha, npos as step k found them and `done` after its
test; frame k + 1 likewise), whether the molecule was latched before frame k, and the twin's force F* at x with the
caller's bound eF on every component of the device's force error.  Per molecule:

  latched, or fmax* < ftol:  `done` is set and x', v', dt', alpha', npos' are BIT-identical to x, v, dt, alpha, npos.
  otherwise `done` is clear, the branch follows from P* = sum F*.v (downhill when P* > 0 or v = 0), the words dt', alpha',
  npos' equal the fp32 restatement `state_words` exactly, and with c* = alpha sqrt(vv / ff*), v1* = (1 - alpha) v + c* F*
  (uphill: 0), v* = v1* + dt' a F*, dr* = dt' v*, d* = max_i |dr*_i|, s* = min(1, max_step / d*), x* = x + s* dr*, per
  element (u = 2^-24, a = ACCEL / m, n the molecule's atoms, |F*|_2 the norm over the whole molecule):

    e_c   = c* sqrt(3 n) eF / (|F*|_2 - sqrt(3 n) eF)                the force error in sqrt(ff): | |F|_2 - |F*|_2 | <= sqrt(3 n) eF
    |v' - v*|   <= c* eF + e_c (|F*| + eF)                           ... through the mixing coefficient
                   + dt' a eF                                        ... through the kick
                   + 8 u (|v| + c* |F*| + dt' a |F*|)      =: b_v    the chain: 1 - alpha, (1 - alpha) v, c, the fma; F a, the fma; a
    |dr - dr*|  <= dt' b_v + 2 u |dr*|                     =: b_dr   one product
    e_d   = sqrt(3) max b_dr                                         |d - d*| <= the largest displacement error, as a vector
    e_s   = e_d / max(d* - e_d, max_step) + 2 u                      s(d) = min(1, max_step / d) has slope <= 1 / max(d, max_step):
                                                                     the clamp is continuous and needs no decision rule
    |x' - x*|   <= s* b_dr + e_s (|dr*| + b_dr) + 2 u (|x| + |dr*|)  the fma, and s rounded once

  A step is UNDECIDABLE and skipped when |fmax* - ftol| <= eF (unless latched), when |P*| <= eF sum |v| (v != 0), or when
  |F*|_2 <= 2 sqrt(3 n) eF (e_c has no bound).  At most 1 step in 10 may be skipped (`check_history`)."""
import numpy as np

ACCEL = 4.184e-4
U = 2.0 ** -24
DEFAULTS = dict(ftol=0.05, dt=0.5, dt_max=5.0, dt_min=0.01, max_step=0.1, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1,
                f_alpha=0.99)
DECISION_MARGIN = 1e-9   # `margins`: no decision of a kernel-alone test lies this close (relative) to its threshold


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def params32(p):
    """The parameters as the device holds them: the fp32 words, as Python floats (n_min stays an integer)."""
    return {k: (v if k == "n_min" else float(np.float32(v))) for k, v in p.items()}


def new_state(B, p):
    return dict(dt=np.full(B, p["dt"], np.float64), alpha=np.full(B, p["alpha_start"], np.float64),
                npos=np.zeros(B, np.int64), done=np.zeros(B, bool), nsteps=np.zeros(B, np.int64))


def fire_step(x, v, F, masses, mol, st, p, skip_clamp=False, keep_alpha=False):
    """One step in fp64 -> (x', v', st', info).  x, v, F [N, 3]; mol [N] the molecule of each atom; st from `new_state`.
    info: per molecule fmax, converged, downhill, grow, clamped, and `margins`, the relative distances of every decision
    taken from its threshold.  skip_clamp / keep_alpha: the teeth's two wrong steps."""
    x, v, F = (np.asarray(t, np.float64) for t in (x, v, F))
    m = np.asarray(masses, np.float64)
    B = len(st["dt"])
    xn, vn = x.copy(), v.copy()
    out = {k: a.copy() for k, a in st.items()}
    info = dict(fmax=np.zeros(B), converged=np.zeros(B, bool), downhill=np.zeros(B, bool), grow=np.zeros(B, bool),
                clamped=np.zeros(B, bool), margins=[])
    for b in range(B):
        i = np.flatnonzero(mol == b)
        Fb, vb = F[i], v[i]
        fmax = np.sqrt((Fb * Fb).sum(1).max()) if len(i) else 0.0
        info["fmax"][b] = fmax
        if not st["done"][b]:
            info["margins"].append(abs(fmax - p["ftol"]) / max(p["ftol"], 1e-300))
        if st["done"][b] or fmax < p["ftol"]:
            out["done"][b] = True
            info["converged"][b] = True
            continue
        P, vv, ff = (Fb * vb).sum(), (vb * vb).sum(), (Fb * Fb).sum()
        dt, alpha = st["dt"][b], st["alpha"][b]
        if vv > 0:
            info["margins"].append(abs(P) / np.sqrt(vv * ff))
        if P > 0 or vv == 0:
            info["downhill"][b] = True
            vb = (1 - alpha) * vb + alpha * np.sqrt(vv / ff) * Fb
            if st["npos"][b] > p["n_min"]:
                info["grow"][b] = True
                dt, alpha = min(dt * p["f_inc"], p["dt_max"]), alpha * p["f_alpha"]
            out["npos"][b] = st["npos"][b] + 1
        else:
            vb = np.zeros_like(vb)
            dt, out["npos"][b] = max(dt * p["f_dec"], p["dt_min"]), 0
            if not keep_alpha:
                alpha = p["alpha_start"]
        vb = vb + dt * ACCEL * Fb / m[i, None]
        dr = dt * vb
        d = np.sqrt((dr * dr).sum(1).max())
        info["margins"].append(abs(d - p["max_step"]) / p["max_step"])
        s = 1.0
        if d > p["max_step"] and not skip_clamp:
            info["clamped"][b] = True
            s = p["max_step"] / d
        xn[i], vn[i] = x[i] + s * dr, vb
        out["dt"][b], out["alpha"][b] = dt, alpha
        out["nsteps"][b] += 1
    return xn, vn, out, info


def state_words(dt, alpha, npos, downhill, p):
    """The fp32 sequence of one molecule's words on a moving step, np.float32 operations only -> (dt', alpha', npos')."""
    f = np.float32
    dt, alpha = f(dt), f(alpha)
    if downhill:
        if npos > p["n_min"]:
            dt, alpha = min(f(dt * f(p["f_inc"])), f(p["dt_max"])), f(alpha * f(p["f_alpha"]))
        return f(dt), f(alpha), int(npos) + 1
    return max(f(dt * f(p["f_dec"])), f(p["dt_min"])), f(p["alpha_start"]), 0


def minimize(x0, force, masses, mol, p, steps, B=None, st=None, v0=None, until_converged=False, **wrong):
    """`steps` steps in fp64 from x0 (v = 0) -> list of frames as each step FOUND the state, then the final one: dicts of
    x, v, F, energy (None unless force returns a pair), fmax, dt, alpha, npos, done (after the test at x), nsteps."""
    B = int(np.max(mol)) + 1 if B is None else B
    st = new_state(B, p) if st is None else st
    x = np.asarray(x0, np.float64).copy()
    v = np.zeros_like(x) if v0 is None else np.asarray(v0, np.float64).copy()
    frames = []

    def found(x, v, st):
        r = force(x)
        E, F = r if isinstance(r, tuple) else (None, r)
        F = np.asarray(F, np.float64)
        fm = np.array([np.sqrt((F[mol == b] ** 2).sum(1).max()) if (mol == b).any() else 0.0 for b in range(B)])
        return dict(x=x.copy(), v=v.copy(), F=F, energy=E, fmax=fm, dt=st["dt"].copy(), alpha=st["alpha"].copy(),
                    npos=st["npos"].copy(), done=st["done"] | (fm < p["ftol"]), nsteps=st["nsteps"].copy())
    for _ in range(steps):
        fr = found(x, v, st)
        frames.append(fr)
        if until_converged and fr["done"].all():
            return frames
        x, v, st, _ = fire_step(x, v, fr["F"], masses, mol, st, p, **wrong)
    frames.append(found(x, v, st))
    return frames


def one_step(fr, nx, F_twin, masses, mol, p, eF, latched=None, exact_words=True):
    """The check of the module docstring on one recorded step, fr -> nx (dicts with x, v, dt, alpha, npos, done; arrays as
    recorded, fp32 where the device's are).  p: the parameters as the device holds them (`params32`).  latched [B]: done
    before this frame (None: nobody).  exact_words False (frames of an fp64 run, whose words are not the fp32 sequence): the words to 1e-6
    relative.  -> (status [B] of "ok" / "skip" / a sentence saying what is wrong, worst ratio)."""
    f64 = lambda t: np.asarray(t, np.float64)
    x, v, xn, vn, Fs, m = f64(fr["x"]), f64(fr["v"]), f64(nx["x"]), f64(nx["v"]), f64(F_twin), f64(masses)
    B = len(fr["dt"])
    latched = np.zeros(B, bool) if latched is None else np.asarray(latched, bool)
    status, worst = [], 0.0
    for b in range(B):
        i = np.flatnonzero(mol == b)
        n = len(i)
        Fb, vb = Fs[i], v[i]
        fmax = np.sqrt((Fb * Fb).sum(1).max()) if n else 0.0
        if not latched[b] and abs(fmax - p["ftol"]) <= eF:
            status.append("skip")
            continue
        words = lambda f: (np.float32(f["dt"][b]), np.float32(f["alpha"][b]), int(f["npos"][b]))
        if latched[b] or fmax < p["ftol"]:
            frozen = (bool(fr["done"][b]) and np.array_equal(fr["x"][i], nx["x"][i])
                      and np.array_equal(fr["v"][i], nx["v"][i]) and words(fr) == words(nx) and bool(nx["done"][b]))
            status.append("ok" if frozen else "a converged molecule moved, changed its words or lost its latch")
            continue
        if fr["done"][b]:
            status.append("a molecule above the tolerance was reported converged")
            continue
        P, vv, ff = (Fb * vb).sum(), (vb * vb).sum(), (Fb * Fb).sum()
        if vv > 0 and abs(P) <= eF * np.abs(vb).sum():
            status.append("skip")
            continue
        eff = np.sqrt(3 * n) * eF
        if np.sqrt(ff) <= 2 * eff:
            status.append("skip")
            continue
        downhill = bool(P > 0 or vv == 0)
        dt, alpha, npos = words(fr)
        want = state_words(dt, alpha, npos, downhill, p)
        close = exact_words or (np.allclose([float(nx["dt"][b]), float(nx["alpha"][b])], [float(w) for w in want[:2]],
                                            rtol=1e-6, atol=0) and int(nx["npos"][b]) == want[2])
        if (words(nx) != want) if exact_words else not close:
            status.append("state words %r, the restatement gives %r" % (words(nx), want))
            continue
        dtn, alpha, a = float(want[0]), float(alpha), ACCEL / m[i, None]
        c = alpha * np.sqrt(vv / ff) if downhill else 0.0
        v1 = (1 - alpha) * vb + c * Fb if downhill else np.zeros_like(vb)
        vs = v1 + dtn * a * Fb
        drs = dtn * vs
        d = np.sqrt((drs * drs).sum(1).max())
        s = min(1.0, p["max_step"] / d) if d > 0 else 1.0
        xs = x[i] + s * drs
        e_c = c * eff / (np.sqrt(ff) - eff)
        b_v = c * eF + e_c * (np.abs(Fb) + eF) + dtn * a * eF + 8 * U * (np.abs(vb) + c * np.abs(Fb) + dtn * a * np.abs(Fb))
        b_dr = dtn * b_v + 2 * U * np.abs(drs)
        e_d = np.sqrt(3.0) * b_dr.max()
        e_s = e_d / max(d - e_d, p["max_step"]) + 2 * U
        b_x = s * b_dr + e_s * (np.abs(drs) + b_dr) + 2 * U * (np.abs(x[i]) + np.abs(drs))
        tiny = 1e-300
        rv, rx = float((np.abs(vn[i] - vs) / (b_v + tiny)).max()), float((np.abs(xn[i] - xs) / (b_x + tiny)).max())
        worst = max(worst, rv, rx)
        status.append("ok" if rv <= 1.0 and rx <= 1.0 else "v' off by %.3g, x' by %.3g of their bounds" % (rv, rx))
    return status, worst


def check_history(frames, forces, masses, mol, p, eps_force, usable=None, latched=None, exact_words=True):
    """one_step on every pair of consecutive frames of a record_every = 1 history.  frames: list of dicts (`one_step`);
    forces [R, N, 3]: the twin's at the recorded positions; eps_force: the relative force bound (eF = eps_force max |F| of
    the frame); usable [R]: frames the twin may be compared on; latched [B]: done before frame 0.
    -> (steps checked, steps skipped, [(step, molecule, what)] of the failures).  A step is skipped when an end is not
    usable or any molecule of it is undecidable; its decidable molecules are checked all the same."""
    R = len(frames)
    usable = np.ones(R, bool) if usable is None else np.asarray(usable, bool)
    B = len(frames[0]["dt"])
    latched = np.zeros(B, bool) if latched is None else np.asarray(latched, bool).copy()
    checked = skipped = 0
    bad = []
    for k in range(R - 1):
        if usable[k] and usable[k + 1]:
            eF = eps_force * np.abs(forces[k]).max()
            status, _ = one_step(frames[k], frames[k + 1], forces[k], masses, mol, p, eF, latched, exact_words)
            bad += [(k, b, s) for b, s in enumerate(status) if s not in ("ok", "skip")]
            if "skip" in status:
                skipped += 1
            else:
                checked += 1
        else:
            skipped += 1
        latched |= np.asarray(frames[k]["done"], bool)
    return checked, skipped, bad


def history_frames(h):
    """A ``relax.History`` (or any object with its fields as arrays / tensors) -> the list of frame dicts of `one_step`."""
    g = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    pos, vel, dt, alpha, npos, done = (g(getattr(h, k)) for k in ("positions", "velocities", "dt", "alpha", "npos",
                                                                   "converged"))
    return [dict(x=pos[k], v=vel[k], dt=dt[k], alpha=alpha[k], npos=npos[k], done=done[k]) for k in range(len(pos))]
