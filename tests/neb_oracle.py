"""TEST INFRASTRUCTURE ONLY: the specification of the device-resident nudged elastic band, independent of the engine's sources.

NEB with the improved tangent (Henkelman and Jonsson, J. Chem. Phys. 113, 9978, 2000) and a climbing image, driven by FIRE as ASE
ships it with ONE controller per band (tests/min_oracle.py).  A band is M images of n atoms; images 0 and M - 1 never move.  For
every interior image i, with d+ = R_{i+1} - R_i and d- = R_i - R_{i-1} over the atoms that are not fixed:
    a = d+.d+,  b = d-.d-,  c = d+.d-,  p = F.d+,  q = F.d-
    E_{i+1} > E_i > E_{i-1}: (w+, w-) = (1, 0);  E_{i+1} < E_i < E_{i-1}: (0, 1);  otherwise hi / lo = the larger / smaller of
    |E_{i+1} - E_i| and |E_{i-1} - E_i| and (w+, w-) = (hi, lo) when E_{i+1} > E_{i-1}, else (lo, hi)
    |tau|^2 = w+^2 a + 2 w+ w- c + w-^2 b,   F.tau = w+ p + w- q
    g = (-(F.tau) / |tau| + k (sqrt a - sqrt b)) / |tau|;   the climber, when climbing is on: g = -2 (F.tau) / |tau|^2
    F_neb = F + (g w+) d+ + (g w-) d-
The climber is the lowest interior index with the largest energy.  An energy that is not finite (cause 3), |tau|^2 zero or not
finite (cause 2) and F.tau not finite (cause 1) make the band unusable - unless every atom is fixed: then no tangent is needed.
Python floats are IEEE fp64 and math.sqrt is correctly rounded, so the coefficients below are a sequence of single fp64 operations;
s+ and s- are rounded to fp32 once."""
import math

import numpy as np

from tests import min_oracle as MO

OK, BAD_SUMS, BAD_PATH, BAD_ENERGY = 0, 1, 2, 3

KAPPA, A = 2.0, 0.5  # the analytic surface of the tests: minima of atom 0 at (+-1, 0, 0), E = 0; saddle at (0, A, 0), E = 1
SADDLE = np.array([0.0, A, 0.0])


def weights(e_prev, e, e_next):
    if e_next > e > e_prev:
        return 1.0, 0.0
    if e_next < e < e_prev:
        return 0.0, 1.0
    up, dn = abs(e_next - e), abs(e_prev - e)
    hi, lo = max(up, dn), min(up, dn)
    return (hi, lo) if e_next > e_prev else (lo, hi)


def climber(e):
    """e [M] -> the lowest interior index with the largest energy"""
    best = 1
    for i in range(2, len(e) - 1):
        if e[i] > e[best]:
            best = i
    return best


def image_coef64(S, wp, wm, k, climbs):
    """-> (cause, (s+, s-) as Python floats)"""
    a, b, c, p, q = (float(t) for t in S)
    tau2 = ((wp * wp) * a + ((2.0 * wp) * wm) * c) + (wm * wm) * b
    if not math.isfinite(tau2) or not tau2 > 0.0:
        return BAD_PATH, (0.0, 0.0)
    ft = wp * p + wm * q
    if not math.isfinite(ft):
        return BAD_SUMS, (0.0, 0.0)
    if climbs:
        g = (-2.0 * ft) / tau2
    else:
        tau = math.sqrt(tau2)
        g = (-(ft / tau) + k * (math.sqrt(a) - math.sqrt(b))) / tau
    return OK, (g * wp, g * wm)


def image_control(e, i, S, k, climb, has_free=True):
    """e [M] (fp32 values or floats), interior image i, its sums S -> cause, (w+, w-), (s+, s-) rounded to np.float32 once.  When
    every atom is fixed (has_free false) the image has no degree of freedom: nothing is unusable, s = 0."""
    e = [float(t) for t in e]
    if not has_free:
        return OK, (0.0, 0.0), (np.float32(0), np.float32(0))
    if not all(math.isfinite(t) for t in e):
        return BAD_ENERGY, (0.0, 0.0), (np.float32(0), np.float32(0))
    wp, wm = weights(e[i - 1], e[i], e[i + 1])
    why, s = image_coef64(S, wp, wm, k, bool(climb) and climber(e) == i)
    return why, (wp, wm), (np.float32(s[0]), np.float32(s[1]))


def path_sums(pos, f, fixed=None):
    """pos, f [M,n,3] -> [M,5] fp64 sums of fp64 terms (endpoints zero)"""
    pos, f = np.asarray(pos, np.float64), np.asarray(f, np.float64)
    free = np.ones(pos.shape[1]) if fixed is None else (np.asarray(fixed) == 0).astype(np.float64)
    out = np.zeros((pos.shape[0], 5))
    for i in range(1, pos.shape[0] - 1):
        dp, dm = (pos[i + 1] - pos[i]) * free[:, None], (pos[i] - pos[i - 1]) * free[:, None]
        out[i] = [(dp * dp).sum(), (dm * dm).sum(), (dp * dm).sum(), (f[i] * dp).sum(), (f[i] * dm).sum()]
    return out


def band_force(pos, e, f, k, climb, fixed=None):
    """One band in fp64, the coefficients unrounded -> cause, F_neb [M,n,3] (zero on endpoints, F on fixed atoms)"""
    pos, f = np.asarray(pos, np.float64), np.asarray(f, np.float64)
    e = [float(t) for t in e]
    still = np.zeros(pos.shape[1], bool) if fixed is None else np.asarray(fixed) != 0
    if still.all():  # no degree of freedom: no tangent is needed
        out = f.copy()
        out[0] = out[-1] = 0.0
        return OK, out
    if not all(math.isfinite(t) for t in e):
        return BAD_ENERGY, None
    S = path_sums(pos, f, fixed)
    out = np.zeros_like(f)
    top = climber(e)
    for i in range(1, len(e) - 1):
        wp, wm = weights(e[i - 1], e[i], e[i + 1])
        why, (sp, sm) = image_coef64(S[i], wp, wm, k, bool(climb) and top == i)
        if why:
            return why, None
        out[i] = np.where(still[:, None], f[i], f[i] + sp * (pos[i + 1] - pos[i]) + sm * (pos[i] - pos[i - 1]))
    return OK, out


def surface(x, sites, kappa=KAPPA, A_=A):
    """x [..., n, 3] -> e [...], f like x in fp64: atom 0 feels (x^2 - 1)^2 + kappa (y - A (1 - x^2))^2 + kappa z^2, atoms j >= 1 feel
    kappa |r_j - s_j|^2 / 2"""
    x = np.asarray(x, np.float64)
    X, Y, Z = x[..., 0, 0], x[..., 0, 1], x[..., 0, 2]
    u = X * X - 1.0
    w = Y + A_ * u
    dr = x[..., 1:, :] - np.asarray(sites, np.float64)[1:]
    e = u * u + kappa * w * w + kappa * Z * Z + 0.5 * kappa * (dr * dr).sum((-1, -2))
    f = np.empty_like(x)
    f[..., 0, 0] = -(4.0 * X * u + 2.0 * kappa * w * (2.0 * A_ * X))
    f[..., 0, 1] = -(2.0 * kappa * w)
    f[..., 0, 2] = -(2.0 * kappa * Z)
    f[..., 1:, :] = -kappa * dr
    return e, f


def fire_sums(v, fneb, fixed=None):
    """one band, v and fneb [M,n,3] -> vf, ff, vv, fmax2 over the interior images"""
    free = np.ones(v.shape[1]) if fixed is None else (np.asarray(fixed) == 0).astype(np.float64)
    v, g = v[1:-1] * free[:, None], fneb[1:-1] * free[:, None]
    ff = (g * g).sum(-1)
    return float((v * g).sum()), float(ff.sum()), float((v * v).sum()), float(ff.max()) if ff.size else 0.0


def run(x, sites, p, spring, climb, max_steps, fixed=None):
    """A whole optimisation on the surface in fp64, x [G,M,n,3] -> steps taken, converged_at [G], final x, e [G,M], climber [G]"""
    x = np.asarray(x, np.float64).copy()
    G, M, n, _ = x.shape
    still = np.zeros(n, bool) if fixed is None else np.asarray(fixed) != 0
    still = np.broadcast_to(still[None, :, None], (M, n, 1)) | (np.arange(M) % (M - 1) == 0)[:, None, None]
    v = np.zeros_like(x)
    fneb = np.zeros_like(x)
    state = MO.new_state(p, G)
    coef = np.zeros((G, 3))
    step = 0
    while True:
        if step > 0:
            for b in range(G):
                frozen = still | (state[b]["converged_at"] >= 0)
                v[b] = np.where(frozen, 0.0, coef[b, 0] * v[b] + coef[b, 1] * fneb[b])
                x[b] = np.where(frozen, x[b], x[b] + coef[b, 2] * v[b])
        e, f = surface(x, sites)
        for b in range(G):
            if state[b]["converged_at"] >= 0:
                continue
            why, fneb[b] = band_force(x[b], e[b], f[b], spring, climb, fixed)
            assert why == OK, why
            ret, coef[b] = MO.control64(state[b], p, *fire_sums(v[b], fneb[b], fixed), step)
            assert ret != MO.UNUSABLE
        conv = np.array([s["converged_at"] for s in state])
        if (conv >= 0).all() or step == max_steps:
            return step, conv, x, e, np.array([climber(e[b]) for b in range(G)])
        step += 1


def interpolate(initial, final, n_images):
    t = np.linspace(0.0, 1.0, n_images)[:, None, None]
    return (1.0 - t) * np.asarray(initial, np.float64) + t * np.asarray(final, np.float64)


def problem(M, n, seed=0):
    """-> x [1,M,n,3] fp32-representable, sites [n,3] fp64: atom 0 from (-1, 0, 0) to (1, 0, 0), atoms j >= 1 at their seeded sites,
    interpolated linearly, the interior images perturbed by a seeded N(0, 0.05)"""
    rng = np.random.default_rng(seed)
    sites = 2.0 * rng.normal(size=(n, 3))
    a, b = sites.copy(), sites.copy()
    a[0], b[0] = (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0)
    x = interpolate(a, b, M)
    x[1:-1] += 0.05 * rng.normal(size=x[1:-1].shape)
    return x.astype(np.float32)[None], sites


def position_bound(n, fmax):
    """The climber's atom 0 from the saddle: at convergence |F| = |F_ci| <= sqrt(n) fmax (the climber's force is the true force with
    one component mirrored), the smallest curvature at the saddle is 4 in magnitude, and a factor 2 for anharmonicity."""
    return 2.0 * math.sqrt(n) * fmax / 4.0


def barrier_bound(n, fmax):
    """|E_climber - E_0 - 1|: a gradient g over a curvature lambda changes E by g^2 / (2 |lambda|); the curvatures are 4 (atom 0 at the
    saddle) and kappa = 2 (the wells), the squared gradients of all atoms sum to at most n fmax^2, so |dE| <= (sqrt(n) fmax)^2 / 4;
    plus the fp32 rounding of an energy of order 1, four half-ulps of 1 (2^-22) for the two energies and the evaluation's own rounding."""
    return (math.sqrt(n) * fmax) ** 2 / 4.0 + 2.0 ** -22
