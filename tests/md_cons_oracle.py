"""TEST INFRASTRUCTURE ONLY: the constraint stages of the device-resident MD loop in fp64 numpy, independent of the Gauss-Seidel
sweeps of csrc/tn_md_cons_math.h: the multipliers of SHAKE are the root of the full nonlinear system, found by Newton's method to
1e-13; the multipliers of RATTLE solve one linear system directly.  One cluster at a time: ``pairs`` [C,2] are indices into the
arrays given, ``w`` = 1 / m (0 for an atom of infinite mass)."""
import numpy as np


def _incidence(n, pairs):
    """[C, n]: +1 at a, -1 at b"""
    inc = np.zeros((len(pairs), n))
    for c, (a, b) in enumerate(pairs):
        inc[c, a], inc[c, b] = 1.0, -1.0
    return inc


def shake(x0, x_keep, w, pairs, d):
    """x0 [n,3] after the drift, x_keep [n,3] the step's start -> x with |x_a - x_b| = d_c, x = x0 + w_i sum_c lambda_c (+-) s_c"""
    x0, x_keep, w, d = (np.asarray(t, np.float64) for t in (x0, x_keep, w, d))
    inc = _incidence(len(x0), pairs)
    s = inc @ x_keep  # [C,3] reference directions
    lam = np.zeros(len(pairs))
    for _ in range(100):
        x = x0 + w[:, None] * (inc.T @ (lam[:, None] * s))
        r = inc @ x
        sigma = (r * r).sum(1) - d * d
        if np.abs(sigma).max() <= 1e-13 * (d * d).max():
            return x
        # d sigma_c / d lambda_c' = 2 r_c . (inc[c, i] w_i inc[c', i]) s_c'
        jac = 2.0 * ((inc * w[None, :]) @ inc.T) * (r @ s.T)
        lam = lam - np.linalg.solve(jac, sigma)
    raise RuntimeError("oracle: Newton did not converge")


def rattle(x, v0, w, pairs):
    """-> v with r_c . (v_a - v_b) = 0, v = v0 + w_i sum_c k_c (+-) r_c"""
    x, v0, w = (np.asarray(t, np.float64) for t in (x, v0, w))
    inc = _incidence(len(x), pairs)
    r = inc @ x
    mat = ((inc * w[None, :]) @ inc.T) * (r @ r.T)
    k = np.linalg.solve(mat, -(r * (inc @ v0)).sum(1))
    return v0 + w[:, None] * (inc.T @ (k[:, None] * r))


def open_step(x, v, f, hk, dt, w, pairs, d):
    """B, A, S in fp64 on the fp32 inputs -> (x, v)"""
    x, v, f, hk = (np.asarray(t, np.float64) for t in (x, v, f, hk))
    v1 = v + hk[:, None] * f
    x1 = x + float(dt) * v1
    x2 = shake(x1, x, w, pairs, d)
    return x2, v1 + (x2 - x1) / float(dt)


def close_step(x, v, f, hk, w, pairs):
    """B, R in fp64 (no thermostat) -> v"""
    x, v, f, hk = (np.asarray(t, np.float64) for t in (x, v, f, hk))
    return rattle(x, v + hk[:, None] * f, w, pairs)
