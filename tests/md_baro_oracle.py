"""TEST INFRASTRUCTURE ONLY: the specification of the barostat of the device-resident MD loop, independent of the engine's sources.

Isotropic stochastic cell rescaling (Bernetti and Bussi, J. Chem. Phys. 153, 114107, 2020), first order in eps = ln V, one barostat
per molecule:
    V = |det box|;  P = (2 K + tr W) / (3 V);  a = compressibility dt / tau;  d = -a (P0 - P) + sqrt(2 kT a / V) xi
    mu = exp(d / 3): box and positions;  nu = exp(-d / 3): velocities
in fp64 Python floats (math.exp and math.sqrt: the C library's), the factors rounded to fp32 once.  xi is the first normal of one
Philox4x32-10 call (tests/md_oracle.py, pure Python) with the counter (step lo, step hi, molecule, 1), through the loop's
uniform / Box-Muller map in fp32.  And the same scheme vectorised (numpy fp64, numpy's own generator) for ensemble statistics."""
import math

import numpy as np

from tests import md_oracle as O

MASK = 0xFFFFFFFF


def counter(step, mol):
    return (step & MASK, step >> 32, mol, 1)


def noise(seed, step, mol):
    """xi of the barostat of molecule `mol` after `step` completed steps.  The Box-Muller map one fp32 operation at a time, as the
    loop's contract has it (u from md_oracle.uniform is exact in fp32): -> Python float"""
    w = O.philox4x32_10(counter(step, mol), (seed & MASK, seed >> 32))
    f = np.float32
    u0, u1 = f(O.uniform(w[0])), f(O.uniform(w[1]))
    r0 = np.sqrt(f(-2.0) * np.log(u0))
    a0 = f(6.283185307179586) * u1
    return float(f(r0 * np.cos(a0)))


def noise_f64(seed, step, mol):
    """the same normal with the map in fp64 (agrees with `noise` to fp32 accuracy)"""
    return O.normals(O.philox4x32_10(counter(step, mol), (seed & MASK, seed >> 32)))[0]


def volume(box):
    b = [float(np.float32(t)) for t in np.asarray(box).reshape(9)]
    return abs((b[0] * (b[4] * b[8] - b[5] * b[7]) - b[1] * (b[3] * b[8] - b[5] * b[6])) + b[2] * (b[3] * b[7] - b[4] * b[6]))


def move(box, W, ekin, force_scale, P0, kT, a, xi=0.0):
    """One molecule: -> V, P, d (Python floats), mu32, nu32 (np.float32)"""
    w = [float(np.float32(t)) for t in np.asarray(W).reshape(9)]
    V = volume(box)
    K = float(np.float32(ekin)) / force_scale
    P = (2.0 * K + ((w[0] + w[4]) + w[8])) / (3.0 * V)
    d = -a * (P0 - P)
    if kT > 0.0:
        d = d + math.sqrt(2.0 * kT * a / V) * xi
    return V, P, d, np.float32(math.exp(d / 3.0)), np.float32(math.exp(-d / 3.0))


def moves(box, W, ekin, force_scale, P0, kT, a, seed=0, step=0):
    """every molecule of box, W [n,3,3], ekin [n] -> V, P (fp64 arrays), mu32, nu32 (fp32 arrays)"""
    out = [move(box[m], W[m], ekin[m], force_scale, P0, kT, a, noise(seed, step, m) if kT > 0.0 else 0.0) for m in range(len(ekin))]
    V, P, _, mu, nu = zip(*out)
    return np.array(V), np.array(P), np.array(mu, np.float32), np.array(nu, np.float32)


def ulp_distance(a, b):
    """|a - b| in units in the last place of fp32 (same-sign finite values)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def ideal_gas(R, n, steps, dt, friction, kT, P0, compressibility, tau, V0, seed=0, mass=1.0, force_scale=1.0):
    """The ideal gas (F = 0, W = 0) of R replicas of n atoms under Langevin + barostat, numpy fp64 with numpy's generator:
    per step O on the velocities, K, the move, V <- V exp(d), v <- v exp(-d / 3).  -> volumes [steps, R] (before each move).
    (Positions do not enter: P = 2 K / (3 V).)"""
    rng = np.random.default_rng(seed)
    c1 = math.exp(-friction * dt)
    c2 = math.sqrt(1.0 - c1 * c1)
    sigma = math.sqrt(kT * force_scale / mass)
    v = sigma * rng.normal(size=(R, n, 3))
    V = np.full(R, float(V0))
    a = compressibility * dt / tau
    out = np.empty((steps, R))
    for s in range(steps):
        v = c1 * v + c2 * sigma * rng.normal(size=v.shape)
        K = 0.5 * mass * (v * v).sum((1, 2)) / force_scale
        P = 2.0 * K / (3.0 * V)
        d = -a * (P0 - P) + np.sqrt(2.0 * kT * a / V) * rng.normal(size=R)
        out[s] = V
        V = V * np.exp(d)
        v = v * np.exp(-d / 3.0)[:, None, None]
    return out


# ---- the ensemble: an ideal gas under Langevin + barostat samples V ~ Gamma(N + 1, kT / P0) ----------------------------------------
# 256 replicas of N = 16 atoms, m = 1, force_scale = 1, kT = 0.025, P0 = 1e-3, compressibility = 1 / P0, tau = 20 dt, friction
# 0.1 / dt, V0 = N kT / P0, 3 000 steps of which the first 300 are dropped.  Bounds: the mean volume within 1 % of (N + 1) kT / P0
# (statistical standard error 0.18 %; N + 1 against N is 6 %), the relative standard deviation within 5 % of 1 / sqrt(N + 1)
# (covers the Euler bias of order dt / 2 tau; missing or doubled noise is far outside).
ENSEMBLE = dict(R=256, n=16, steps=3000, drop=300, dt=1.0, friction=0.1, kT=0.025, P0=1e-3, tau=20.0)


def ensemble_bounds(vol):
    """vol [steps, R] (all steps) -> (mean / expected mean, relative sd / expected), asserted by the caller"""
    e = ENSEMBLE
    v = np.asarray(vol, np.float64)[e["drop"]:]
    mean_ratio = v.mean() / ((e["n"] + 1) * e["kT"] / e["P0"])
    sd_ratio = (v.std() / v.mean()) * math.sqrt(e["n"] + 1)
    return mean_ratio, sd_ratio


def ensemble_state(seed=17):
    """-> box [R,3,3], x, v [R n,3], hk, mass, sigma [R n], c1, c2 for the ideal gas (fp32, as the loop takes them)"""
    e = ENSEMBLE
    R, n = e["R"], e["n"]
    rng = np.random.default_rng(seed)
    side = (n * e["kT"] / e["P0"]) ** (1.0 / 3.0)
    box = np.tile((np.eye(3) * side).astype(np.float32), (R, 1, 1))
    x = (rng.uniform(0, side, size=(R * n, 3))).astype(np.float32)
    v = (math.sqrt(e["kT"]) * rng.normal(size=(R * n, 3))).astype(np.float32)
    mass = np.ones(R * n, np.float32)
    hk = np.full(R * n, 0.5 * e["dt"], np.float32)
    sigma = np.full(R * n, math.sqrt(e["kT"]), np.float32)
    c1 = math.exp(-e["friction"] * e["dt"])
    return box, x, v, hk, mass, sigma, c1, math.sqrt(1 - c1 * c1)
