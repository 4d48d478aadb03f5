"""TEST INFRASTRUCTURE ONLY: the specification of the device-resident minima hopping, independent of the engine's sources.

* the closed-form test surface: a 4-atom chain, bonds 1/2 20 (r - 1.5)^2, angles 1/2 8 (theta - 110 deg)^2, torsion
  0.15 (1 + cos 3 phi) + 0.05 (1 + cos phi); exactly three minima: trans (E = 0) and gauche+- (phi ~ +-62 deg, E ~ 0.0743)
* the whole algorithm for ONE walker in numpy (``Walker``): state per atom in ``dtype`` (fp64: the specification; fp32: the same
  statements on rounded storage, which measures how far rounding alone moves a trajectory), everything per walker in fp64, the
  distance between two geometries by an SVD Kabsch superposition, the noise from tests/md_oracle.py's Philox."""
import math

import numpy as np

from tests import md_oracle

QUENCH, COMPARE, LAUNCH, MD = range(4)
(NONE, START, SAME, KNOWN, ACCEPTED, REJECTED, UNCONVERGED, SINGULAR) = range(8)

CHAIN_START = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.0, 1.4, 0.0], [3.4, 1.6, 0.6]])
CHAIN_PARAMS = dict(dt=0.05, kT0=0.3, ediff0=0.1, mdmin=2, fmax=1e-3, rmsd_tol=0.1, energy_tol=1e-3)
K_BOND, R0, K_ANGLE, THETA0 = 20.0, 1.5, 8.0, math.radians(110.0)


def torsion_energy(phi):
    return 0.15 * (1.0 + math.cos(3.0 * phi)) + 0.05 * (1.0 + math.cos(phi))


def chain_torsion(x):
    x = np.asarray(x, dtype=np.float64)
    b1, b2, b3 = x[1] - x[0], x[2] - x[1], x[3] - x[2]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    return math.atan2(np.linalg.norm(b2) * np.dot(b1, n2), np.dot(n1, n2))


def chain_surface(x):
    """x [4,3] -> (E, F [4,3]) in fp64, analytic forces"""
    x = np.asarray(x, dtype=np.float64)
    E, F = 0.0, np.zeros((4, 3))
    for i in range(3):
        d = x[i] - x[i + 1]
        r = np.linalg.norm(d)
        E += 0.5 * K_BOND * (r - R0) ** 2
        g = K_BOND * (r - R0) * d / r
        F[i] -= g
        F[i + 1] += g
    for i in range(2):
        a, b = x[i] - x[i + 1], x[i + 2] - x[i + 1]
        la, lb = np.linalg.norm(a), np.linalg.norm(b)
        c = float(np.clip(np.dot(a, b) / (la * lb), -1.0, 1.0))
        theta, s = math.acos(c), math.sqrt(max(1.0 - c * c, 1e-300))
        E += 0.5 * K_ANGLE * (theta - THETA0) ** 2
        dEdt = K_ANGLE * (theta - THETA0)
        ga = -(b / lb - c * a / la) / (la * s)
        gb = -(a / la - c * b / lb) / (lb * s)
        F[i] -= dEdt * ga
        F[i + 2] -= dEdt * gb
        F[i + 1] += dEdt * (ga + gb)
    b1, b2, b3 = x[1] - x[0], x[2] - x[1], x[3] - x[2]
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    l2 = np.linalg.norm(b2)
    phi = math.atan2(l2 * np.dot(b1, n2), np.dot(n1, n2))
    E += torsion_energy(phi)
    dV = -0.45 * math.sin(3.0 * phi) - 0.05 * math.sin(phi)
    g0 = -l2 / np.dot(n1, n1) * n1
    g3 = l2 / np.dot(n2, n2) * n2
    p, q = np.dot(b1, b2) / (l2 * l2), np.dot(b3, b2) / (l2 * l2)
    g1 = q * g3 - (1.0 + p) * g0  # (Blondel, Karplus: J. Comput. Chem. 17, 1132, 1996)
    g2 = p * g0 - (1.0 + q) * g3
    for i, g in enumerate((g0, g1, g2, g3)):
        F[i] -= dV * g
    return E, F


def kabsch_rmsd(a, b, align="rotation"):
    """rmsd of a from b [n,3] in fp64: as they stand, centroids superposed, or after the best PROPER rotation (SVD, the sign of the
    determinant corrected)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = len(a)
    if align == "none":
        return math.sqrt(((a - b) ** 2).sum() / n)
    a, b = a - a.mean(0), b - b.mean(0)
    if align == "translation" or n < 3:
        return math.sqrt(((a - b) ** 2).sum() / n)
    U, s, Vt = np.linalg.svd(a.T @ b)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        s = s.copy()
        s[-1] = -s[-1]
    return math.sqrt(max(((a * a).sum() + (b * b).sum() - 2.0 * s.sum()) / n, 0.0))


FIRE = dict(dt=0.1, dt_max=1.0, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, max_step=0.2)
DEFAULTS = dict(beta1=1.1, beta2=1.1, beta3=1 / 1.1, alpha1=0.98, alpha2=1 / 0.98, mdmin=2, md_steps=400, opt_steps=2000, fmax=0.05,
                rmsd_tol=0.1, energy_tol=1e-3, capacity=32, seed=0)


class Walker:
    """One walker on ``surface(x) -> (E, F)``.  ``step()`` is one evaluation and what follows it; ``phases`` and ``outcomes`` log
    every step, ``ring`` holds dict(energy, pos, found_at, visits) by slot."""

    def __init__(self, surface, pos, masses, dtype=np.float64, align="rotation", force_scale=1.0, fire=None, **params):
        self.p = dict(DEFAULTS, **params)
        self.fire = dict(FIRE, **(fire or {}))
        self.surface, self.dtype, self.align, self.fs = surface, dtype, align, float(force_scale)
        self.x = np.array(pos, dtype=dtype)
        self.v = np.zeros_like(self.x)
        self.m = np.asarray(masses, dtype=np.float64).reshape(-1)
        self.kT, self.ediff = float(self.p["kT0"]), float(self.p["ediff0"])
        self.phase, self.cur, self.e_cur, self.ring, self.n_recorded = QUENCH, None, None, {}, 0
        self.best, self.e_best = None, None
        self.n = dict(hops=0, same=0, known=0, new=0, accepted=0, unconverged=0)
        self._fire_reset()
        self.quench_steps, self.steps = 0, 0
        self.phases, self.outcomes, self.epot, self.ekin, self.factors = [], [], [], [], []

    def _fire_reset(self):
        self.f_dt, self.f_alpha, self.f_npos = self.fire["dt"], self.fire["alpha"], 0

    def _fire_move(self, F, v):
        """FIRE as ASE ships it, from the sums of (v, F): returns the moved (x, v) or None when converged"""
        f = self.fire
        t = self.dtype
        F = F.astype(t)
        vf, ff, vv = float((v * F).sum()), float((F * F).sum()), float((v * v).sum())
        if math.sqrt(float((F.astype(np.float64) ** 2).sum(1).max())) < self.p["fmax"]:
            return None
        if vf > 0.0:
            c_v = 1.0 - self.f_alpha
            mix = self.f_alpha * math.sqrt(vv / ff) if ff > 0 and vv > 0 else 0.0
            if self.f_npos > f["n_min"]:
                self.f_dt = min(self.f_dt * f["f_inc"], f["dt_max"])
                self.f_alpha *= f["f_alpha"]
            self.f_npos += 1
        else:
            c_v, mix = 0.0, 0.0
            self.f_alpha = f["alpha"]
            self.f_dt *= f["f_dec"]
            self.f_npos = 0
        dt = self.f_dt
        c_f = mix + dt
        n2 = c_v * c_v * vv + 2.0 * c_v * c_f * vf + c_f * c_f * ff
        length = dt * math.sqrt(max(n2, 0.0))
        d = dt * (f["max_step"] / length) if length > f["max_step"] else dt
        v = (t(c_v) * v + t(c_f) * F).astype(t)
        return (self.x + t(d) * v).astype(t), v

    def _record(self, E):
        slot = self.n_recorded % self.p["capacity"]
        self.ring[slot] = dict(energy=E, pos=self.x.copy(), found_at=self.steps, visits=1)
        self.n_recorded += 1
        if self.e_best is None or E < self.e_best:
            self.best, self.e_best = self.x.copy(), E
        return slot

    def _draw(self):
        hop, seed, mask = self.n["hops"], self.p["seed"], md_oracle.MASK  # counter (hop lo, hop hi, atom, 2)
        xi = np.array([md_oracle.normals(md_oracle.philox4x32_10((hop & mask, hop >> 32, i, 2), (seed & mask, seed >> 32)))
                       for i in range(len(self.x))])
        t = self.dtype
        sig = np.sqrt(self.fs / self.m)
        self.v = (t(math.sqrt(self.kT)) * sig.astype(t)[:, None] * xi.astype(t)).astype(t)

    def _known(self, E):
        for slot in sorted(self.ring):
            r = self.ring[slot]
            if abs(E - r["energy"]) < self.p["energy_tol"] and kabsch_rmsd(self.x, r["pos"], self.align) < self.p["rmsd_tol"]:
                return slot
        return None

    def step(self):
        t = self.dtype
        E, F = self.surface(self.x)
        E = float(t(E))
        F = np.asarray(F).astype(t)
        self.steps += 1
        self.phases.append(self.phase)
        self.epot.append(E)
        out, ekin = NONE, 0.0
        hk = (0.5 * self.p["dt"] * self.fs / self.m).astype(t)[:, None]
        if self.phase == QUENCH:
            moved = self._fire_move(F, self.v)
            if moved is None:
                self.v[:] = 0
                self.phase = COMPARE
            elif self.cur is not None and self.quench_steps >= self.p["opt_steps"]:
                out = UNCONVERGED
                self.n["hops"] += 1
                self.n["unconverged"] += 1
                self.x = self.cur.copy()
                self._draw()
                self.phase = LAUNCH
            else:
                self.x, self.v = moved
                self.quench_steps += 1
        elif self.phase == COMPARE:
            accept = False
            if self.cur is None:
                out, accept = START, True
                hit = self._known(E)
                if hit is None:
                    self._record(E)
                else:
                    self.ring[hit]["visits"] += 1
            else:
                self.n["hops"] += 1
                if abs(E - self.e_cur) < self.p["energy_tol"] and kabsch_rmsd(self.x, self.cur, self.align) < self.p["rmsd_tol"]:
                    out = SAME
                    self.kT *= self.p["beta1"]
                    self.factors.append(("kT", self.p["beta1"]))
                    self.n["same"] += 1
                else:
                    hit = self._known(E)
                    if hit is not None:
                        out = KNOWN
                        self.kT *= self.p["beta2"]
                        self.factors.append(("kT", self.p["beta2"]))
                        self.ring[hit]["visits"] += 1
                        self.n["known"] += 1
                    else:
                        self.kT *= self.p["beta3"]
                        self.factors.append(("kT", self.p["beta3"]))
                        self.n["new"] += 1
                        self._record(E)
                        if E < self.e_cur + self.ediff:
                            out, accept = ACCEPTED, True
                            self.ediff *= self.p["alpha1"]
                            self.factors.append(("ediff", self.p["alpha1"]))
                            self.n["accepted"] += 1
                        else:
                            out = REJECTED
                            self.ediff *= self.p["alpha2"]
                            self.factors.append(("ediff", self.p["alpha2"]))
            if accept:
                self.cur, self.e_cur = self.x.copy(), E
            else:
                self.x = self.cur.copy()
            self._draw()
            self.phase = LAUNCH
        elif self.phase == LAUNCH:
            m = self.m[:, None]
            x64, v64 = self.x.astype(np.float64), self.v.astype(np.float64)
            M = m.sum()
            xc, vc = (m * x64).sum(0) / M, (m * v64).sum(0) / M
            d = x64 - xc
            w = np.zeros(3)
            if self.align == "rotation" and len(d) >= 3:
                L = (m * np.cross(d, v64 - vc)).sum(0)
                I = (m * ((d * d).sum(1)[:, None, None] * np.eye(3) - d[:, :, None] * d[:, None, :]).reshape(len(d), 9)).sum(0).reshape(3, 3)
                if np.linalg.eigvalsh(I)[0] > 1e-10 * np.trace(I):
                    w = np.linalg.solve(I, L)
                else:
                    out = SINGULAR
            self.v = (self.v - (vc + np.cross(w, d)).astype(t)).astype(t)
            self.v = (self.v + hk * F).astype(t)
            self.x = (self.x + t(self.p["dt"]) * self.v).astype(t)
            self.e_hist, self.md_k, self.md_count = [E], 0, 0
            self.phase = MD
        else:
            vclosed = (self.v + hk * F).astype(t)
            ekin = float((0.5 * self.m * (vclosed.astype(np.float64) ** 2).sum(1)).sum())
            self.e_hist.append(E)
            self.md_k += 1
            k = self.md_k
            if k >= 2 and self.e_hist[-2] < self.e_hist[-3] and self.e_hist[-2] <= self.e_hist[-1]:
                self.md_count += 1
            self.e_hist = self.e_hist[-3:]
            if self.md_count < self.p["mdmin"] and k < self.p["md_steps"]:
                self.v = (vclosed + hk * F).astype(t)
                self.x = (self.x + t(self.p["dt"]) * self.v).astype(t)
            else:
                self.v = np.zeros_like(self.x)
                self._fire_reset()
                moved = self._fire_move(F, self.v)
                if moved is None:
                    self.quench_steps, self.phase = 0, COMPARE
                else:
                    self.x, self.v = moved
                    self.quench_steps, self.phase = 1, QUENCH
        self.outcomes.append(out)
        self.ekin.append(ekin)
        return self

    def run(self, hops, max_steps=200000):
        while self.n["hops"] < hops and self.steps < max_steps:
            self.step()
        return self

    def minima(self):
        """the live ring entries, lowest energy first"""
        return sorted(self.ring.values(), key=lambda r: r["energy"])
