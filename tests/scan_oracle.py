"""TEST INFRASTRUCTURE ONLY: the relaxed coordinate scan of torchmd-net_amd/csrc/tn_scan_math.h restated in fp64 numpy, independently of
the header: the CVs and their gradients in the textbook form (acos-free angle, the torsion gradient of Bekker et al. as GROMACS writes
it), the multipliers by ``numpy.linalg.solve``, FIRE by ``tests.min_oracle.control64``.  ``run`` is the whole method on the analytic
surface of the tests; with ``store32=True`` the stored state (x, v) is rounded to fp32 after every step, as the device stores it."""
import math

import numpy as np

from tests import min_oracle

PI = math.pi


def cv_value_grad(cv, x):
    """one CV at x [n,3] fp64 -> (s, grad [n,3])"""
    kind, idx = cv[0], list(cv[1:])
    g = np.zeros_like(x)
    if kind == "distance":
        i, j = idx
        r = x[i] - x[j]
        s = np.linalg.norm(r)
        g[i], g[j] = r / s, -r / s
        return s, g
    if kind == "angle":
        i, j, k = idx
        a, b = x[i] - x[j], x[k] - x[j]
        la, lb = np.linalg.norm(a), np.linalg.norm(b)
        c = np.cross(a, b)
        lc = np.linalg.norm(c)
        s = math.atan2(lc, a @ b)
        cos, sin = (a @ b) / (la * lb), lc / (la * lb)
        ga = (cos * a / la - b / lb) / (la * sin)   # d theta / d a = -(b_hat - cos a_hat) / (|a| sin)
        gb = (cos * b / lb - a / la) / (lb * sin)
        g[i], g[k], g[j] = ga, gb, -(ga + gb)
        return s, g
    i, j, k, l = idx
    b1, b2, b3 = x[j] - x[i], x[k] - x[j], x[l] - x[k]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    lb2 = np.linalg.norm(b2)
    s = math.atan2(lb2 * (b1 @ n2), n1 @ n2)
    gi = -lb2 / (n1 @ n1) * n1
    gl = lb2 / (n2 @ n2) * n2
    p, q = (b1 @ b2) / (lb2 * lb2), (b3 @ b2) / (lb2 * lb2)
    g[i], g[l] = gi, gl
    g[j] = -gi - p * gi + q * gl
    g[k] = -gl + p * gi - q * gl
    return s, g


def diff(kind, a, b):
    d = a - b
    if kind != "torsion":
        return d
    return (d + PI) % (2 * PI) - PI if (d + PI) % (2 * PI) != 0 else PI  # into (-pi, pi]


def cv_all(cvs, x, fixed=None):
    """-> s [D], g [D,n,3] with the rows of fixed atoms zeroed"""
    s, g = zip(*(cv_value_grad(cv, x) for cv in cvs))
    g = np.array(g)
    if fixed is not None:
        g[:, np.asarray(fixed) != 0] = 0.0
    return np.array(s), g


def multipliers(cvs, x, F, v, fixed=None):
    """-> s [D], g [D,n,3], lambda [D], mu [D] (fp64)"""
    s, g = cv_all(cvs, x, fixed)
    gf = g.reshape(len(cvs), -1)
    M = gf @ gf.T
    return s, g, np.linalg.solve(M, gf @ F.reshape(-1)), np.linalg.solve(M, gf @ v.reshape(-1))


def drive(kind, t_fin, t_cur, step):
    d = diff(kind, t_fin, t_cur)
    if abs(d) <= step:
        return t_fin
    return diff(kind, t_cur + math.copysign(step, d), 0.0)


def constrain(cvs, x, t, tol, max_iter, fixed=None):
    """-> (x on the surface, corrections made) or (None, corrections) when it does not converge"""
    x = x.copy()
    for it in range(max_iter + 1):
        s, g = cv_all(cvs, x, fixed)
        sg = np.array([diff(cv[0], s[c], t[c]) for c, cv in enumerate(cvs)])
        if np.abs(sg).max() < tol:
            return x, it
        if it == max_iter:
            return None, it
        gf = g.reshape(len(cvs), -1)
        x = x - (np.linalg.solve(gf @ gf.T, sg) @ gf).reshape(x.shape)
    raise AssertionError


def surface(x, sites=None, kappa=0.0):
    """the analytic surface at x [n,3] fp64 -> (E, F [n,3])"""
    E, F = 0.0, np.zeros_like(x)
    for b in range(3):
        r, g = cv_value_grad(("distance", b, b + 1), x)
        E += 15.0 * (r - 1.5) ** 2
        F -= 30.0 * (r - 1.5) * g
    phi, gphi = cv_value_grad(("torsion", 0, 1, 2, 3), x)
    th = []
    for b in range(2):
        t, g = cv_value_grad(("angle", b, b + 1, b + 2), x)
        th.append(t)
        E += 4.0 * (t - 1.9) ** 2
        F -= (8.0 * (t - 1.9) + (1.5 * math.cos(phi) if b == 0 else 0.0)) * g
    E += 0.6 * (1 + math.cos(3 * phi)) + 0.3 * (1 - math.cos(phi)) + 1.5 * (th[0] - 1.9) * math.cos(phi)
    F -= (-1.8 * math.sin(3 * phi) + 0.3 * math.sin(phi) - 1.5 * (th[0] - 1.9) * math.sin(phi)) * gphi
    if len(x) > 4:
        d = x[4:] - np.asarray(sites)[4:]
        E += 0.5 * kappa * (d * d).sum()
        F[4:] -= kappa * d
    return E, F


def relaxed_energy(phi):
    """E*(phi) of the 4-atom chain with its torsion held at phi, and dE*/dphi"""
    c, s = np.cos(phi), np.sin(phi)
    E = 0.6 * (1 + np.cos(3 * phi)) + 0.3 * (1 - c) - 1.5 ** 2 * c * c / 16.0
    dE = -1.8 * np.sin(3 * phi) + 0.3 * s + 2.0 * 1.5 ** 2 * c * s / 16.0
    return E, dE


def chain(phi, n=4, sites=None, offset=0.0):
    """a start geometry [n,3]: the chain at r = 1.5, theta = 1.9 and torsion phi; further atoms at their sites + offset"""
    r, th = 1.5, 1.9
    x = np.zeros((n, 3))
    x[0] = [r * math.sin(th), 0.0, r * math.cos(th)]
    x[2] = [0.0, 0.0, r]
    x[3] = [r * math.sin(th) * math.cos(phi), r * math.sin(th) * math.sin(phi), r - r * math.cos(th)]
    if n > 4:
        x[4:] = np.asarray(sites)[4:] + offset
    return x


def run(cvs, x0, t_fin, drive_step, tol, max_iter, p, max_steps, sites=None, kappa=0.0, fixed=None, store32=False):
    """ONE point from x0 [n,3] to the targets t_fin [D] -> dict(steps, converged_at, x, E, cv, target, lam, fmax)"""
    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if store32 else (lambda a: a)
    free = np.ones(len(x0), bool) if fixed is None else (np.asarray(fixed) == 0)
    x, v = rnd(np.array(x0, np.float64)), np.zeros_like(x0, dtype=np.float64)
    st = dict(dt=p["dt"], alpha=p["alpha"], n_pos=0, converged_at=-1)
    t_cur = None
    for step in range(max_steps + 1):
        E, F = surface(x, sites, kappa)
        s, g, lam, mu = multipliers(cvs, x, F, v, fixed)
        if t_cur is None:
            t_cur = s.copy()
        Fp = F - np.tensordot(lam, g, 1)
        vp = v - np.tensordot(mu, g, 1)
        ff = (Fp * Fp).sum(1)[free]
        here = all(t_cur[c] == t_fin[c] for c in range(len(cvs)))
        q = dict(p, fmax=p["fmax"] if here else 0.0)
        ret, (c_v, c_f, d) = min_oracle.control64(st, q, (vp * Fp)[free].sum(), ff.sum(), (vp * vp)[free].sum(), ff.max(), step)
        out = dict(steps=step, converged_at=st["converged_at"], x=x, E=E, cv=s, target=t_cur.copy(), lam=lam, fmax=math.sqrt(ff.max()))
        if ret != min_oracle.MOVING or step == max_steps:
            return out
        v = np.where(free[:, None], c_v * vp + c_f * Fp, 0.0)
        x = x + d * v
        t_cur = np.array([drive(cv[0], t_fin[c], t_cur[c], drive_step[c]) for c, cv in enumerate(cvs)])
        x, _ = constrain(cvs, x, t_cur, tol, max_iter, fixed)
        x, v = rnd(x), rnd(v)
    raise AssertionError
