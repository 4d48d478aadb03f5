"""TEST INFRASTRUCTURE ONLY: the specification of the device-resident IRC follower, independent of the engine's sources.

The damped velocity Verlet path follower of Hratchian and Schlegel (J. Phys. Chem. A 106, 165, 2002) in fp64 numpy, written from
the equations: a classical trajectory with a = force_scale F / m whose speed is put back to v0 after every step.  Step i -> i+1 with
c_a = force_scale / (2 m_a), over the atoms that move (not fixed, finite mass):
    v_half = v_i + dt_i c_a F_i,   x_{i+1} = x_i + dt_i v_half,   v' = v_half + dt_i c_a F_{i+1}
    vv = sum |v'|^2,  P = sum F_{i+1}.v',  fmax2 = max |F_{i+1}|^2,  ds2 = sum m |x_{i+1} - x_i|^2
    D2 = sum |x_{i+1} - x'|^2,  x' = x_{i-1} + T v_{i-1} + T^2 c_a F_{i-1},  T = dt_{i-1} + dt_i      (from the second step on)
    c = v0 / sqrt(vv),   v_{i+1} = c v'
    dt_{i+1} = clamp(dt_i clamp(cbrt(error / sqrt(D2)), 1/2, 2), dt_min, dt_max)   (unchanged on the first step and when D2 = 0)
    s_{i+1} = s_i + sqrt(ds2)
    the path finishes when sqrt(fmax2) < fmax (reason 1), otherwise when P <= 0 (reason 2).
An energy that is not finite (cause 3), P or fmax2 not finite (cause 1), vv zero or not finite or D2 / ds2 not finite (cause 2) make
a path unusable, looked at in this order - unless no atom moves: then it is finished as it stands.  The control of the start images
is the same without a kick, an arc or a change of the time step.

The surface is tests/neb_oracle.py's double well with its two coordinates on atoms of different mass, X = x of atom 0 and Y = y of
atom 1, so that the path depends on the masses:
    E = (X^2 - 1)^2 + kappa (Y - A (1 - X^2))^2 + kappa / 2 sum (every other coordinate - its site)^2
The saddle is X = 0, Y = A (E = 1), the minima X = +-1, Y = 0; the Hessian at the saddle is diagonal, so the transition vector is e_X
whatever the masses.  The exact IRC is this module's own Euler integration of dq / ds = M^-1 F / |M^-1 F|."""
import functools
import math

import numpy as np

from tests import neb_oracle as NO

KAPPA, A = NO.KAPPA, NO.A
OK, BAD_FORCES, BAD_VELOCITY, BAD_ENERGY = 0, 1, 2, 3
MOVING, FINISHED, FROZEN, UNUSABLE = 0, 1, 2, 3
S_VV, S_P, S_FMAX2, S_D2, S_DS2, S_FREE = range(6)
cbrt = getattr(math, "cbrt", None) or (lambda x: float(np.cbrt(np.float64(x))))  # the C library's either way


def surface(x, sites, kappa=KAPPA, A_=A):
    """x [..., n, 3] -> e [...], f like x in fp64"""
    x = np.asarray(x, np.float64)
    X, Y = x[..., 0, 0], x[..., 1, 1]
    u = X * X - 1.0
    w = Y + A_ * u
    d = x - np.asarray(sites, np.float64)
    d[..., 0, 0] = 0.0
    d[..., 1, 1] = 0.0
    e = u * u + kappa * w * w + 0.5 * kappa * (d * d).sum((-1, -2))
    f = -kappa * d
    f[..., 0, 0] = -(4.0 * X * u + 2.0 * kappa * w * (2.0 * A_ * X))
    f[..., 1, 1] = -(2.0 * kappa * w)
    return e, f


def problem(n, m0, m1, seed=0):
    """-> x_ts [n,3] (fp32-representable: atom 0 at X = 0, atom 1 at Y = A, everything else on its site), u [n,3] = e_X, masses [n]
    (m0, m1, then seeded masses between 1 and 20), sites [n,3]"""
    rng = np.random.default_rng(seed)
    sites = rng.uniform(-2.0, 2.0, size=(n, 3)).astype(np.float32).astype(np.float64)
    x_ts = sites.copy()
    x_ts[0, 0], x_ts[1, 1] = 0.0, A
    u = np.zeros((n, 3))
    u[0, 0] = 1.0
    masses = np.concatenate([[m0, m1], rng.uniform(1.0, 20.0, size=n - 2)]).astype(np.float32).astype(np.float64)
    return x_ts.astype(np.float32), u, masses, sites


def moving(masses, fixed=None, force_scale=1.0):
    """the atoms that move: not fixed and c_a = fp32(force_scale / (2 m)) > 0"""
    ca = (force_scale / (2.0 * np.asarray(masses, np.float64))).astype(np.float32)
    free = ca > 0
    return free if fixed is None else free & (np.asarray(fixed) == 0)


def control(s, prm, sums, energy, start, step):
    """One path: s = dict(dt, arc, conv, reason, n_acc, n_rec) is updated in place -> ret, cause, (fp32(c), fp32(dt used)), slot"""
    one, zero = np.float32(1.0), np.float32(0.0)
    if s["conv"] >= 0:
        return FROZEN, OK, (one, zero), -1
    vv, P, fmax2, D2, ds2, nfree = (float(t) for t in sums)
    has2 = (not start) and s["n_acc"] >= 1
    c, dt, arc, reason = 1.0, s["dt"], s["arc"], 1
    if nfree > 0:
        if not math.isfinite(float(energy)):
            return UNUSABLE, BAD_ENERGY, (one, zero), -1
        if not (math.isfinite(P) and math.isfinite(fmax2)):
            return UNUSABLE, BAD_FORCES, (one, zero), -1
        if not (math.isfinite(vv) and vv > 0.0) or (has2 and not math.isfinite(D2)) or not math.isfinite(ds2):
            return UNUSABLE, BAD_VELOCITY, (one, zero), -1
        c = prm["v0"] / math.sqrt(vv)
        if has2 and D2 > 0.0:
            r = min(max(cbrt(prm["error"] / math.sqrt(D2)), 0.5), 2.0)
            dt = min(max(s["dt"] * r, prm["dt_min"]), prm["dt_max"])
        if not start:
            arc = s["arc"] + math.sqrt(ds2)
        reason = 1 if math.sqrt(fmax2) < prm["fmax"] else (2 if P <= 0.0 else 0)
    out = (np.float32(c), zero if start else np.float32(s["dt"]))
    s["dt"], s["arc"] = dt, arc
    s["n_acc"] = 0 if start else s["n_acc"] + 1
    if reason:
        s["conv"], s["reason"] = step, reason
    slot = -1
    if reason or s["n_acc"] % max(prm.get("every", 1), 1) == 0:
        if s["n_rec"] < prm.get("capacity", 512):
            slot = s["n_rec"]
        s["n_rec"] += 1
    return (FINISHED if reason else MOVING), OK, out, slot


def run(x_ts, u, sigma, masses, sites, prm, dt, initial_step, max_steps, fixed=None, force_scale=1.0):
    """One path in fp64 with nothing rounded -> dict(steps, reason, x, v, arc, dt, frames [steps+1,n,3], s [steps+1], power, cause)"""
    masses = np.asarray(masses, np.float64)
    mv = moving(masses, fixed, force_scale)[:, None]
    ca = np.where(mv[:, 0], force_scale / (2.0 * masses), 0.0)[:, None]
    m = np.where(mv[:, 0], masses, 0.0)[:, None]
    u = np.asarray(u, np.float64) * mv
    x = np.asarray(x_ts, np.float64) + sigma * initial_step * u
    v = sigma * prm["v0"] * u
    e, f = surface(x, sites)
    s = dict(dt=float(dt), arc=0.0, conv=-1, reason=0, n_acc=0, n_rec=0)
    frames, arcs, power = [], [], []
    gen1 = gen2 = None
    step, dt_i, x_prev = 0, 0.0, x
    while True:
        vp = v + dt_i * ca * f
        D2 = 0.0
        if gen2 is not None:
            T = gen2[3] + dt_i
            D2 = float((((x - (gen2[0] + T * gen2[1] + T * T * ca * gen2[2])) * mv) ** 2).sum())
        sums = [float(((vp * mv) ** 2).sum()), float((f * vp * mv).sum()), float(((f * mv) ** 2).sum(-1).max()), D2,
                float((m * (x - x_prev) ** 2).sum()), float(mv.sum())]
        ret, cause, (c, _), _ = control(s, prm, sums, e, step == 0, step)
        if ret == UNUSABLE:
            return dict(steps=step, cause=cause)
        v = float(prm["v0"] / math.sqrt(sums[0])) * vp * mv if sums[5] > 0 else vp * 0.0
        frames.append(x.copy())
        arcs.append(s["arc"])
        power.append(sums[1])
        if ret == FINISHED or step == max_steps:
            break
        gen2 = None if gen1 is None else gen1
        dt_i = s["dt"]
        gen1 = (x, v, f, dt_i)
        x_prev = x
        vh = v + dt_i * ca * f
        x = x + dt_i * vh
        v = vh
        e, f = surface(x, sites)
        step += 1
    return dict(steps=step, reason=s["reason"], conv=s["conv"], x=x, v=v, arc=s["arc"], dt=s["dt"], frames=np.array(frames), s=np.array(arcs),
                power=np.array(power), cause=0)


@functools.lru_cache(maxsize=None)
def exact_irc(m0, m1, h=1e-5, keep=10):
    """The IRC of the surface for masses (m0, m1) from the saddle towards X = +1, in the (X, Y) plane (every other coordinate stays
    on its site, where it feels no force): Euler steps of length h along M^-1 F / |M^-1 F| from (1e-4, A) until the energy no longer
    falls (the minimum lies within h) or 4 / h steps; every `keep`-th point -> [K,2]"""
    X, Y = 1e-4, A
    pts = [(0.0, A), (X, Y)]
    e_old = math.inf
    for i in range(int(4.0 / h)):
        uu = X * X - 1.0
        w = Y + A * uu
        e = uu * uu + KAPPA * w * w
        gx = -(4.0 * X * uu + 2.0 * KAPPA * w * (2.0 * A * X)) / m0
        gy = -(2.0 * KAPPA * w) / m1
        nrm = math.hypot(gx, gy)
        if not e < e_old or nrm == 0.0:
            break
        e_old = e
        X += h * gx / nrm
        Y += h * gy / nrm
        if i % keep == 0:
            pts.append((X, Y))
    pts.append((X, Y))
    return np.array(pts)


def distance_from(curve, X, Y):
    """the distance of every point (|X|, Y) from the polyline's points [K,2] (spacing 1e-4: half of it is the error of this distance)"""
    q = np.stack([np.abs(np.asarray(X, np.float64)), np.asarray(Y, np.float64)], -1)
    out = np.empty(len(q))
    for i in range(0, len(q), 64):
        d = q[i:i + 64, None, :] - curve[None]
        out[i:i + 64] = np.sqrt((d * d).sum(-1).min(1))
    return out


def curve_separation(c1, c2):
    """the largest distance of a point of c1 from c2 (subsampled)"""
    return float(distance_from(c2, c1[::20, 0], c1[::20, 1]).max())
