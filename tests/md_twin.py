"""float64 restatement of the integrators of geossl_amd/md.py, written from their definition, and the one-step check the
MD tests share.

Units: kcal/mol, A, amu, fs; a(x) = ACCEL F(x) / m.  With hdt = dt / 2:
  velocity Verlet  vh = v + hdt a(x);  x' = x + dt vh;                                        v' = vh + hdt a(x')
  BAOAB            vh = v + hdt a(x);  xh = x + hdt vh;  vo = c1 vh + s xi;  x' = xh + hdt vo;  v' = vo + hdt a(x')
(c1 = exp(-gamma dt), s = sqrt(1 - c1^2) sqrt(KB T ACCEL / m), xi standard normals).

`one_step` takes two consecutive RECORDED states and the twin's forces at the recorded positions, forms x*, v* from the
lines above and bounds |x' - x*|, |v' - v*| per element, u = 2^-24:
  |v' - v*| <= hdt (ACCEL / m) (eF(x) + eF(x')) + R_v,      R_v = 8 u (|v| + dt (|a(x)| + |a(x')|) + |s xi|)
  |x' - x*| <= (dt^2 / 2) (ACCEL / m) eF(x) + 4 u (|x| + dt |vh|) + dt R_v
eF(x): the caller's bound on the force error at x (a relative force bound times max |F(x)|).  The first terms carry the
force error through the kicks; the rest is the rounding of the fp32 chain (each fma rounds once, the acceleration and the
noise amplitude once each, the fp32 copies of dt, c1, ACCEL / m and s by u relative)."""
import numpy as np

ACCEL = 4.184e-4
KB = 8.31446261815324 / 4184
U = 2.0 ** -24


def verlet_step(x, v, force, masses, dt, stale_second_kick=False):
    m = np.asarray(masses, dtype=np.float64)[:, None]
    a = ACCEL * force(x) / m
    vh = v + 0.5 * dt * a
    xn = x + dt * vh
    an = a if stale_second_kick else ACCEL * force(xn) / m
    return xn, vh + 0.5 * dt * an


def baoab_step(x, v, force, masses, dt, c1, sigma_T, xi):
    m = np.asarray(masses, dtype=np.float64)[:, None]
    vh = v + 0.5 * dt * ACCEL * force(x) / m
    xh = x + 0.5 * dt * vh
    vo = c1 * vh + sigma_T / np.sqrt(m) * xi
    xn = xh + 0.5 * dt * vo
    return xn, vo + 0.5 * dt * ACCEL * force(xn) / m


def integrate(x0, v0, force, masses, dt, steps, langevin=None, xi=None, stale_second_kick=False):
    """`steps` steps in fp64 from (x0, v0) -> (positions [steps + 1, N, 3], velocities [steps + 1, N, 3]).  force(x) ->
    F [N, 3]; langevin = (c1, sigma_T) with xi(k) -> [N, 3] the draws of step k."""
    x, v = np.asarray(x0, dtype=np.float64).copy(), np.asarray(v0, dtype=np.float64).copy()
    xs, vs = [x], [v]
    for k in range(steps):
        if langevin is None:
            x, v = verlet_step(x, v, force, masses, dt, stale_second_kick)
        else:
            x, v = baoab_step(x, v, force, masses, dt, langevin[0], langevin[1], xi(k))
        xs.append(x)
        vs.append(v)
    return np.stack(xs), np.stack(vs)


def kinetic(v, masses, mol):
    """Per-molecule kinetic energy in kcal/mol of velocities v [N, 3]; mol [N] the molecule of each atom."""
    ke = 0.5 * np.asarray(masses, np.float64) * (np.asarray(v, np.float64) ** 2).sum(1) / ACCEL
    return np.bincount(mol, weights=ke)


def one_step(x_t, v_t, x_n, v_n, F_t, F_n, masses, dt, eF_t, eF_n, langevin=None, xi=None):
    """The check of the module docstring on one recorded step -> (worst |v' - v*| / bound, worst |x' - x*| / bound): at most
    1 when the step holds.  eF_t, eF_n: scalars or per-atom [N, 1] bounds on the force error."""
    f64 = lambda t: np.asarray(t, dtype=np.float64)
    x_t, v_t, x_n, v_n, F_t, F_n = map(f64, (x_t, v_t, x_n, v_n, F_t, F_n))
    m = f64(masses)[:, None]
    a_t, a_n = ACCEL * F_t / m, ACCEL * F_n / m
    vh = v_t + 0.5 * dt * a_t
    if langevin is None:
        noise = np.zeros_like(v_t)
        xs = x_t + dt * vh
        vs = vh + 0.5 * dt * a_n
    else:
        c1, sigma_T = langevin
        noise = sigma_T / np.sqrt(m) * f64(xi)
        vo = c1 * vh + noise
        xs = x_t + 0.5 * dt * vh + 0.5 * dt * vo
        vs = vo + 0.5 * dt * a_n
    R_v = 8 * U * (np.abs(v_t) + dt * (np.abs(a_t) + np.abs(a_n)) + np.abs(noise))
    bound_v = 0.5 * dt * (ACCEL / m) * (eF_t + eF_n) + R_v
    bound_x = 0.5 * dt * dt * (ACCEL / m) * eF_t + 4 * U * (np.abs(x_t) + dt * np.abs(vh)) + dt * R_v
    tiny = 1e-300
    return float((np.abs(v_n - vs) / (bound_v + tiny)).max()), float((np.abs(x_n - xs) / (bound_x + tiny)).max())


def check_trajectory(pos, vel, forces, masses, dt, eps_force, usable=None, langevin=None, xis=None):
    """one_step on every pair of consecutive frames of a record_every = 1 trajectory.  forces [R, N, 3]: the twin's at
    the recorded positions; eps_force: the relative force bound (eF = eps_force max |F| of the frame); usable [R]: frames
    the twin may be compared on (None: all) - a step with an unusable end is skipped.
    -> (steps checked, steps skipped, [(step, worst v ratio, worst x ratio)] of the steps that fail)."""
    R = len(pos)
    usable = np.ones(R, bool) if usable is None else np.asarray(usable, bool)
    checked = skipped = 0
    bad = []
    for k in range(R - 1):
        if not (usable[k] and usable[k + 1]):
            skipped += 1
            continue
        checked += 1
        eF = [eps_force * np.abs(forces[j]).max() for j in (k, k + 1)]
        rv, rx = one_step(pos[k], vel[k], pos[k + 1], vel[k + 1], forces[k], forces[k + 1], masses, dt, eF[0], eF[1],
                          langevin, None if xis is None else xis[k])
        if not (rv <= 1.0 and rx <= 1.0):
            bad.append((k, rv, rx))
    return checked, skipped, bad


# ---- numpy restatement of the device's thermostat stream (Philox-4x32-10, Box-Muller) -------------------------------
def philox4x32_10(counter, key):
    """counter uint32 [n, 4], key (k0, k1) -> uint32 [n, 4]."""
    c = [counter[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    M0, M1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(c, 1).astype(np.uint32)


def normals(seed, step, n):
    """The thermostat's draws of `step` under `seed` for atoms 0 .. n - 1 in fp64 -> [n, 3] (the device's are the fp32
    evaluation of the same expressions)."""
    ctr = np.zeros((n, 4), np.uint32)
    ctr[:, 0] = np.arange(n, dtype=np.uint32)
    ctr[:, 1], ctr[:, 2] = step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).astype(np.float64)
    r = np.floor(r / 256.0)
    u0, u1, u2, u3 = (r[:, 0] + 1) / 16777216.0, r[:, 1] / 16777216.0, (r[:, 2] + 1) / 16777216.0, r[:, 3] / 16777216.0
    ra, rb = np.sqrt(-2 * np.log(u0)), np.sqrt(-2 * np.log(u2))
    return np.stack([ra * np.cos(2 * np.pi * u1), ra * np.sin(2 * np.pi * u1), rb * np.cos(2 * np.pi * u3)], 1)


def stream_statistics(draws):
    """draws: list of [n, 3] arrays of consecutive steps -> per step (|mean|, |var - 1|) and the lag correlations of
    consecutive steps, each against its 5-standard-error limit: dict(mean, var, lag, n)."""
    n = draws[0].size
    out = dict(n=n, mean=[abs(d.mean()) for d in draws], var=[abs(d.var() - 1.0) for d in draws],
               lag=[abs((a * b).mean()) for a, b in zip(draws[:-1], draws[1:])])
    out["limits"] = dict(mean=5 / np.sqrt(n), var=5 * np.sqrt(2.0 / n), lag=5 / np.sqrt(n))
    return out


# ---- the twin's own trajectory of a test case: which starts the comparison can be made on -------------------------
def head_condition(kind, twin_cfg, params, buffers, head, z, pos, batch, edge_index):
    """Condition number of the energies as force_twin.max_err sees them: the energy head's last layer is a dot product
    E_b = bias + sum_k w_k a_bk; kappa = max_b (|bias| + sum_k |w_k a_bk|) / max_b |E_b|, in the twin's fp64.  ANY fp32
    evaluation of that sum - K rounded products, a tree of log2 K additions, the bias - may be off by (log2 K + 2) u
    sum |terms|, that is by (log2 K + 2) u kappa relative to max |E|, whatever else is exact."""
    import force_twin as tw
    import torch
    from oracle import nets
    dd = dict(dtype=torch.float64)
    P = {k: v.detach().to(**dd) for k, v in list(params.items()) + list(buffers.items()) if v.is_floating_point()}
    H = {k: v.detach().to(**dd) for k, v in head.items()}
    z, batch = torch.as_tensor(z), torch.as_tensor(batch)
    x = torch.as_tensor(pos, dtype=torch.float32).to(**dd)
    ei = torch.as_tensor(edge_index)
    with torch.no_grad():
        if kind == "schnet":
            rep = nets.schnet_forward(P, z, x, batch, twin_cfg["cutoff"], twin_cfg["num_interactions"],
                                      twin_cfg["readout"], edge_index=ei)
        else:
            rep = nets.painn_forward(P, z, x, ei, batch, twin_cfg["n_atom_basis"], twin_cfg["n_interactions"],
                                     twin_cfg["cutoff"], twin_cfg["readout"])
        if "weight" in H:
            a, w, b = rep, H["weight"], H["bias"]
        else:
            a = torch.nn.functional.silu(rep @ H["0.weight"].t() + H["0.bias"])
            w, b = H["1.weight"], H["1.bias"]
        terms = (a * w).abs().sum(1) + b.abs().sum()
        energy = tw.head_forward(rep, H)
    return float(terms.max() / energy.abs().max())


def head_condition_limit(kind, bound):
    """The largest kappa at which an fp32 head can meet `bound` on max|dE| / max|E| at all: bound / ((log2 K + 2) u), K
    the inputs of the head's last layer (SchNet's Linear(128, 1): 128; PaiNN's output layers: 64)."""
    K = 128 if kind == "schnet" else 64
    return bound / ((np.log2(K) + 2) * U)


def twin_trajectory_margin(kind, cfg, twin_cfg, params, buffers, head, raw, v0, masses, dt, steps, langevin=None,
                           seed=None, device="cpu"):
    """(the smallest cutoff margin (force_twin.cutoff_margin, A), the largest head_condition) over the frames of the
    twin's OWN fp64 trajectory from (raw positions, v0): forces from force_twin.predict on the frame's radius list,
    velocity Verlet or - langevin = (c1, sigma_T) with the device's draws of `seed` restated by `normals` - BAOAB."""
    import force_twin as tw
    import torch
    from oracle.graph import radius_graph_np
    z, bvec = raw["x"][:, 0].copy(), raw["batch"]

    def edges(x):
        p32 = x.astype(np.float32)
        return (tw.schnet_edges(p32, bvec, cfg["cutoff"]) if kind == "schnet"
                else torch.from_numpy(radius_graph_np(p32, cfg["cutoff"], bvec)))

    def force(x):
        return tw.predict(kind, twin_cfg, params, buffers, head, z, x, bvec, edges(x), device=device)[1].numpy()
    xs, _ = integrate(raw["positions"], v0, force, masses, dt, steps, langevin,
                      None if langevin is None else (lambda k: normals(seed, k, len(z))))
    return (min(tw.cutoff_margin(x.astype(np.float32), bvec, cfg["cutoff"]) for x in xs),
            max(head_condition(kind, twin_cfg, params, buffers, head, z, x, bvec, edges(x)) for x in xs))
