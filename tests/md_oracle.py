"""TEST INFRASTRUCTURE ONLY: the specification of the device-resident MD loop, independent of the engine's sources.

* the scheme in fp64 numpy:  v += hk F;  x += dt v;  [F = F(x)];  v += hk F;  [v = c1 v + c2 sigma xi];  E_kin = sum 0.5 m v^2
* the same scheme as an fp32 mirror, one rounded numpy operation per product and per sum, in the contract's order
* Philox4x32-10 in pure Python integers, written from the algorithm's definition (Salmon et al., SC'11, section 3.3 and table 2:
  a round maps (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key is bumped by the two
  Weyl constants between rounds), and the uniform / Box-Muller map of its four words in fp64."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 ints, key: 2 ints (32-bit each) -> tuple of 4 ints"""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(word):
    """u = ((r >> 8) + 0.5) 2^-24 with the sum rounded to fp32 (nearest even): the exact real number below one half, where the sum
    has 24 significant bits; in [2^-25, 1] overall"""
    return float(np.float32((int(word) >> 8) + 0.5)) * 2.0 ** -24


def normals(words):
    """four words -> (xi_x, xi_y, xi_z) in fp64: Box-Muller on (u0, u1) and the cosine branch on (u2, u3)"""
    u0, u1, u2, u3 = (uniform(w) for w in words)
    r0, r1 = math.sqrt(-2.0 * math.log(u0)), math.sqrt(-2.0 * math.log(u2))
    return r0 * math.cos(2.0 * math.pi * u1), r0 * math.sin(2.0 * math.pi * u1), r1 * math.cos(2.0 * math.pi * u3)


def noise(seed, step, atom):
    """xi of atom `atom` (caller's index) in the O step after `step` completed steps: key = seed, counter = (step, atom, 0)"""
    return normals(philox4x32_10((step & MASK, step >> 32, atom, 0), (seed & MASK, seed >> 32)))


def noise_array(seed, step, n):
    return np.array([noise(seed, step, i) for i in range(n)], dtype=np.float64)


# ---- the scheme, fp64 -------------------------------------------------------------------------------------------------------
def close_step(v, f, hk, mass, xi=None, c1=1.0, c2=0.0, sigma=None):
    """B [, O] and the per-atom kinetic energy, fp64.  v, f [n,3]; hk, mass, sigma [n]; xi [n,3] or None (no thermostat)."""
    v = np.asarray(v, np.float64) + np.asarray(hk, np.float64)[:, None] * np.asarray(f, np.float64)
    if xi is not None:
        v = c1 * v + (c2 * np.asarray(sigma, np.float64))[:, None] * np.asarray(xi, np.float64)
    m = np.asarray(mass, np.float64)
    ke = np.where(np.isinf(m), 0.0, 0.5 * np.where(np.isinf(m), 0.0, m) * (v * v).sum(1))
    return v, ke


def open_step(x, v, f, hk, dt):
    v = np.asarray(v, np.float64) + np.asarray(hk, np.float64)[:, None] * np.asarray(f, np.float64)
    return np.asarray(x, np.float64) + dt * v, v


# ---- the scheme, fp32 op by op (the rounding contract) ------------------------------------------------------------------------
def _f(a):
    return np.asarray(a, np.float32)


def close_step_f32(v, f, hk, mass, xi=None, c1=1.0, c2=0.0, sigma=None):
    v, f, hk, m = _f(v), _f(f), _f(hk)[:, None], _f(mass)
    v = v + hk * f  # numpy evaluates hk * f into an fp32 temporary, then adds: two rounded operations
    if xi is not None:
        c1, c2 = np.float32(c1), np.float32(c2)
        v = c1 * v + ((c2 * _f(sigma))[:, None] * _f(xi))
    s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    with np.errstate(invalid="ignore"):
        ke = np.where(np.isinf(m), np.float32(0), (np.float32(0.5) * m) * s)
    return v, ke.astype(np.float32)


def open_step_f32(x, v, f, hk, dt):
    v = _f(v) + _f(hk)[:, None] * _f(f)
    return _f(x) + np.float32(dt) * v, v
