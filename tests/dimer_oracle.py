"""TEST INFRASTRUCTURE ONLY: the specification of the device-resident dimer saddle search, independent of the engine's sources.

Minimum-mode following (Henkelman and Jonsson, J. Chem. Phys. 111, 7010, 1999) with forward differences (Heyden, Bell and Keil, J.
Chem. Phys. 123, 224101, 2005) and the rotation from two curvature rows (Kaestner and Sherwood, J. Chem. Phys. 128, 014106, 2008),
the trial image at a right angle and evaluated with the others, driven by FIRE as ASE ships it with ONE controller per dimer
(tests/min_oracle.py).  A dimer is its midpoint R0, a unit axis N and a unit partner M at a right angle; with the forces F0, F1, F2
at R0, R0 + delta N, R0 + delta M, over the atoms that are not fixed:
    HN = -(F1 - F0) / delta,  HM = -(F2 - F0) / delta
    a = N.HN,  b = (N.HM + M.HN) / 2,  c = M.HM
    (co, si), co >= 0: the unit eigenvector of [[a, b], [b, c]] for the smaller eigenvalue.  b = 0: (1, 0) when a <= c (a tie keeps
    the axis), (0, 1) when a > c.  Otherwise theta = atan2(-2 b, c - a) / 2, (co, si) = (cos theta, sin theta): it minimises
    (a + c) / 2 + ((a - c) / 2) cos 2 theta + b sin 2 theta, and |theta| < pi / 2.
    nu = |co N + si M| from the vector,  N' = (co N + si M) / nu,  HN' = (co HN + si HM) / nu
    C = (co^2 a + 2 co si b + si^2 c) / nu^2 = N'.HN',   p = (co F0.N + si F0.M) / nu = F0.N'
    T = HN' - C N';   F_eff = F0 - 2 p N' when C < 0, else -p N'
    M' = T_perp / |T_perp| with T_perp = T - (T.N' / N'.N') N' - unless |T_perp|^2 is zero, not finite or at most FLOOR2 |HN'|^2:
    then the rotated partner R = -si N + co M takes T's place, and when that has no length either M' = 0.
A dimer converges at a step when sqrt(fmax2) < fmax AND C < 0.  An energy that is not finite (cause 3), a force or FIRE sum that is
not finite (cause 1) and a, b, c or nu^2 not finite or nu^2 = 0 (cause 2) make the dimer unusable - unless every atom is fixed: then
there is no mode and it converges as it stands.  Python floats are IEEE fp64; math.sqrt is correctly rounded and math.atan2 / cos /
sin are the C library's, so on the header's sums the coefficients below are the header's operations on the host."""
import math

import numpy as np

from tests import min_oracle as MO
from tests import neb_oracle as NO

OK, BAD_SUMS, BAD_MODE, BAD_ENERGY = 0, 1, 2, 3
KEEP, SWAP, ANGLE = 0, 1, 2          # the rotation's branches
RESIDUAL, ROTATED, NONE = 0, 1, 2    # where the next partner came from
FLOOR2 = 2.0 ** -40                  # the relative floor: |T_perp| <= 2^-20 |HN'| defines no direction
# the header's sums, in its order
S_A, S_B1, S_B2, S_C, S_PN, S_PM, S_FF, S_FREE = range(8)
P_TT, P_TN, P_NN, P_RR, P_RN, P_HH = range(6)
# the header's fp32 coefficients, in its order
C_CN, C_SN, C_CC, C_K0, C_E, C_CO, C_SI, C_MT, C_MR, C_MN = range(10)


def rotation(a, b, c):
    """-> co, si, branch"""
    if b == 0.0:
        return (1.0, 0.0, KEEP) if a <= c else (0.0, 1.0, SWAP)
    theta = 0.5 * math.atan2(-2.0 * b, c - a)
    return math.cos(theta), math.sin(theta), ANGLE


def mode_rotation(S, e, has_free=True):
    """the sums S [8], the three energies -> cause, (a, b, c), (co, si), branch"""
    S = [float(t) for t in S]
    if not has_free:
        return OK, (0.0, 0.0, 0.0), (1.0, 0.0), KEEP
    if not all(math.isfinite(float(t)) for t in e):
        return BAD_ENERGY, (0.0, 0.0, 0.0), (1.0, 0.0), KEEP
    if not all(math.isfinite(S[k]) for k in (S_FF, S_PN, S_PM)):
        return BAD_SUMS, (0.0, 0.0, 0.0), (1.0, 0.0), KEEP
    q = (S[S_A], 0.5 * (S[S_B1] + S[S_B2]), S[S_C])
    if not all(math.isfinite(t) for t in q):
        return BAD_MODE, q, (1.0, 0.0), KEEP
    co, si, branch = rotation(*q)
    return OK, q, (co, si), branch


def mode_coef(q, S, co, si, nu2, has_free=True):
    """-> cause, C, p, coef [7] np.float32 (cn, sn, cc, k0, e, fp32(co), fp32(si)), each rounded once"""
    z = np.zeros(7, np.float32)
    if not has_free:
        return OK, 0.0, 0.0, z
    nu2 = float(nu2)
    if not math.isfinite(nu2) or not nu2 > 0.0:
        return BAD_MODE, 0.0, 0.0, z
    nu = math.sqrt(nu2)
    C = (((co * co) * q[0] + ((2.0 * co) * si) * q[1]) + (si * si) * q[2]) / nu2
    p = (co * float(S[S_PN]) + si * float(S[S_PM])) / nu
    k0, e = (1.0, -2.0 * p) if C < 0.0 else (0.0, -p)
    return OK, C, p, np.array([co / nu, si / nu, C, k0, e, co, si], np.float32)


def partner_coef(P, has_free=True):
    """the partner sums P [6] -> branch, (mt, mr, mn) np.float32, |T|"""
    P = [float(t) for t in P]
    z = np.zeros(3, np.float32)
    if not has_free:
        return NONE, z, 0.0
    resid = math.sqrt(P[P_TT]) if P[P_TT] >= 0.0 else float("nan")
    if not math.isfinite(P[P_NN]) or not P[P_NN] > 0.0:
        return NONE, z, resid
    kt = P[P_TN] / P[P_NN]
    t2 = P[P_TT] - kt * P[P_TN]
    if math.isfinite(t2) and t2 > 0.0 and t2 > FLOOR2 * P[P_HH]:
        s = 1.0 / math.sqrt(t2)
        return RESIDUAL, np.array([s, 0.0, -(kt * s)], np.float32), resid
    kr = P[P_RN] / P[P_NN]
    r2 = P[P_RR] - kr * P[P_RN]
    if math.isfinite(r2) and r2 > 0.0:
        s = 1.0 / math.sqrt(r2)
        return ROTATED, np.array([0.0, s, -(kr * s)], np.float32), resid
    return NONE, z, resid


def fire64(state, p, sums, C, translate, has_free, step):
    """the dimer's controller on MO.control64 -> ret, (c_v, c_f, d) as Python floats"""
    if not has_free:
        return MO.control64(state, p, *sums, step)
    if not translate:
        if state["converged_at"] >= 0:
            return MO.FROZEN, (0.0, 0.0, 0.0)
        if not all(math.isfinite(float(t)) for t in sums):
            return MO.UNUSABLE, (0.0, 0.0, 0.0)
        return MO.MOVING, (0.0, 0.0, 0.0)
    return MO.control64(state, p if C < 0.0 else dict(p, fmax=0.0), *sums, step)


def fire(state, p, sums, C, translate, has_free, step):
    ret, c = fire64(state, p, sums, C, translate, has_free, step)
    return ret, tuple(np.float32(t) for t in c)


def sums64(N, M, f0, f1, f2, delta, fixed=None):
    """one dimer, [n,3] each -> S [8] in fp64 from fp64 terms"""
    N, M, f0, f1, f2 = (np.asarray(t, np.float64) for t in (N, M, f0, f1, f2))
    free = np.ones(len(N)) if fixed is None else (np.asarray(fixed) == 0).astype(np.float64)
    w = free[:, None]
    hn, hm = -(f1 - f0) / delta, -(f2 - f0) / delta
    return np.array([(N * hn * w).sum(), (N * hm * w).sum(), (M * hn * w).sum(), (M * hm * w).sum(), (f0 * N * w).sum(),
                     (f0 * M * w).sum(), ((f0 * f0 + f1 * f1 + f2 * f2) * w).sum(), free.sum()])


def step64(N, M, e, f0, f1, f2, delta, fixed=None):
    """One dimer's step in fp64, no coefficient rounded -> dict(cause, q, co, si, branch, nu2, C, p, Np, T, Feff, Mp, partner, resid)"""
    N, M, f0, f1, f2 = (np.asarray(t, np.float64) for t in (N, M, f0, f1, f2))
    still = np.zeros(len(N), bool) if fixed is None else np.asarray(fixed) != 0
    w = (~still)[:, None].astype(np.float64)
    has_free = bool((~still).any())
    S = sums64(N, M, f0, f1, f2, delta, fixed)
    cause, q, (co, si), branch = mode_rotation(S, e, has_free)
    out = dict(cause=cause, q=q, co=co, si=si, branch=branch, S=S)
    if cause or not has_free:
        out.update(C=0.0, p=0.0, Np=N * 0, T=N * 0, Feff=f0.copy(), Mp=M * 0, partner=NONE, resid=0.0, nu2=0.0)
        return out
    u = (co * N + si * M) * w
    nu2 = float((u * u).sum())
    out["nu2"] = nu2
    if not math.isfinite(nu2) or not nu2 > 0.0:
        out.update(cause=BAD_MODE, C=0.0, p=0.0)
        return out
    nu = math.sqrt(nu2)
    hn, hm = -(f1 - f0) / delta * w, -(f2 - f0) / delta * w
    Np, Hp = u / nu, (co * hn + si * hm) / nu
    C = (co * co * q[0] + 2.0 * co * si * q[1] + si * si * q[2]) / nu2
    p = (co * S[S_PN] + si * S[S_PM]) / nu
    T = Hp - C * Np
    R = (-si * N + co * M) * w
    Feff = np.where(still[:, None], f0, f0 - 2.0 * p * Np if C < 0.0 else -p * Np)
    P = [(T * T).sum(), (T * Np).sum(), (Np * Np).sum(), (R * R).sum(), (R * Np).sum(), (Hp * Hp).sum()]
    kt = P[P_TN] / P[P_NN]
    t2 = P[P_TT] - kt * P[P_TN]
    if math.isfinite(t2) and t2 > 0.0 and t2 > FLOOR2 * P[P_HH]:
        partner, Mp = RESIDUAL, (T - kt * Np) / math.sqrt(t2)
    else:
        kr = P[P_RN] / P[P_NN]
        r2 = P[P_RR] - kr * P[P_RN]
        partner, Mp = (ROTATED, (R - kr * Np) / math.sqrt(r2)) if math.isfinite(r2) and r2 > 0.0 else (NONE, N * 0)
    out.update(C=C, p=p, Np=Np, T=T, Feff=Feff, Mp=Mp, partner=partner, resid=math.sqrt(P[P_TT]), P=np.array(P))
    return out


def fire_sums(v, feff, fixed=None):
    """one dimer, [n,3] -> vf, ff, vv, fmax2 over the free atoms"""
    free = np.ones(len(v)) if fixed is None else (np.asarray(fixed) == 0).astype(np.float64)
    v, g = v * free[:, None], feff * free[:, None]
    ff = (g * g).sum(-1)
    return float((v * g).sum()), float(ff.sum()), float((v * v).sum()), float(ff.max()) if ff.size else 0.0


def orthonormal(mode, fixed=None, seed=0, n=None):
    """mode [n,3] (None: a seeded normal draw for n atoms) -> N, M [n,3] fp64: N = mode / |mode| over the free atoms, M a seeded normal draw made
    orthogonal to N and normalised; both zero on fixed atoms"""
    rng = np.random.default_rng(seed)
    n = len(mode) if mode is not None else n if n is not None else len(fixed)
    free = np.ones(n) if fixed is None else (np.asarray(fixed) == 0).astype(np.float64)
    draw = rng.normal(size=(2, n, 3))
    N = (draw[0] if mode is None else np.asarray(mode, np.float64)) * free[:, None]
    M = draw[1] * free[:, None]
    if not free.any():
        return N * 0, M * 0
    N = N / math.sqrt((N * N).sum())
    M = M - (M * N).sum() * N
    M = M / math.sqrt((M * M).sum())
    return N, M


def images(x0, N, M, delta):
    """-> [3,n,3] fp32: R0, R0 + fp32(delta) N, R0 + fp32(delta) M with fp32 operations"""
    x0, N, M = (np.asarray(t, np.float32) for t in (x0, N, M))
    d = np.float32(delta)
    return np.stack([x0, x0 + d * N, x0 + d * M])


def run(x0, N, M, sites, p, delta, translate, max_steps, fixed=None):
    """A whole search on the surface of tests/neb_oracle.py in fp64, one dimer: x0, N, M [n,3] -> dict(steps, conv, x, N, M, e, C
    (per step), resid, cause)"""
    x, N, M = (np.asarray(t, np.float64).copy() for t in (x0, N, M))
    still = np.zeros(len(x), bool) if fixed is None else np.asarray(fixed) != 0
    has_free = bool((~still).any())
    v, feff = np.zeros_like(x), np.zeros_like(x)
    state = MO.new_state(p, 1)[0]
    coef = (0.0, 0.0, 0.0)
    Cs, step = [], 0
    while True:
        if step > 0 and translate:
            v = np.where(still[:, None], 0.0, coef[0] * v + coef[1] * feff)
            x = np.where(still[:, None], x, x + coef[2] * v)
        e, f = NO.surface(np.stack([x, x + delta * N, x + delta * M]), sites)
        r = step64(N, M, e, f[0], f[1], f[2], delta, fixed)
        if r["cause"]:
            return dict(steps=step, conv=-1, x=x, N=N, M=M, e=e[0], C=Cs, cause=r["cause"])
        ret, coef = fire64(state, p, fire_sums(v, r["Feff"], fixed), r["C"], translate, has_free, step)
        assert ret != MO.UNUSABLE
        if has_free:
            N, M, feff = r["Np"], r["Mp"], r["Feff"]
        Cs.append(r["C"])
        if state["converged_at"] >= 0 or step == max_steps:
            return dict(steps=step, conv=state["converged_at"], x=x, N=N, M=M, e=float(e[0]), C=Cs, resid=r["resid"], cause=0)
        step += 1


def problem(n, start=(0.4, 0.3, 0.1), seed=0):
    """-> x0 [n,3] fp32-representable, sites [n,3] fp64: atom 0 at `start`, atoms j >= 1 at their seeded sites + N(0, 0.05)"""
    rng = np.random.default_rng(seed)
    sites = 2.0 * rng.normal(size=(n, 3))
    x = sites + 0.05 * rng.normal(size=(n, 3))
    x[0] = start
    return x.astype(np.float32), sites


def surface_hessian(x, sites, h=1e-5):
    """the Hessian of the surface at x [n,3] by fine central differences of its forces in fp64 -> [3n,3n], symmetrised"""
    x = np.asarray(x, np.float64)
    D = x.size
    H = np.zeros((D, D))
    for j in range(D):
        xp, xm = x.copy().reshape(-1), x.copy().reshape(-1)
        xp[j] += h
        xm[j] -= h
        H[:, j] = -(NO.surface(xp.reshape(x.shape), sites)[1] - NO.surface(xm.reshape(x.shape), sites)[1]).reshape(-1) / (2 * h)
    return 0.5 * (H + H.T)


def curvature_bound(n, fmax, delta):
    """|C + 4| at a converged dimer on the surface.  d^2 E / dx^2 of atom 0 at x = 0 is -4 + 4 kappa A (y - A): a midpoint within
    position_bound of the saddle changes it by at most 4 kappa A position_bound.  The forward difference adds (delta / 2) |d^3 E / dx^3|;
    the third derivative vanishes at x = 0 and grows with the fourth, 24 + 24 kappa A^2 = 36, times the same distance."""
    r = NO.position_bound(n, fmax)
    return 4.0 * NO.KAPPA * NO.A * r + 0.5 * delta * 36.0 * r
