"""TEST INFRASTRUCTURE ONLY: the specification of the device-resident L-BFGS minimiser, independent of the engine's sources.

L-BFGS without line search as ASE ships it (ase.optimize.LBFGS, restated from its published form in float64): H0 = 1 / alpha, the
history of the last ``memory`` pairs, the step of every ATOM clamped to ``max_step``, ``damping``.  One instance per molecule.  After
every force evaluation (g = -F, over the free atoms):
    after a move: s = x - x_prev, y = F_prev - F; the pair enters the history only when s.y > 0 (ASE stores every pair: the one
    deviation); with ``memory`` pairs held the oldest leaves
    q = g;  newest ... oldest: a_i = rho_i s_i.q, q -= a_i y_i;  z = H0 q;  oldest ... newest: b = rho_i y_i.z, z += s_i (a_i - b);
    p = -z;  rho_i = 1 / (y_i.s_i)
    longest = max_i |p_i|;  c = damping (longest >= max_step ? max_step / longest : 1);  x <- x + c p
A molecule converges when max_i |F_i| < fmax and is then frozen; a fixed atom contributes to no sum and never moves.  The two loops run
on the vectors themselves, in the order written: this is the form the engine's coefficient-space recursion is compared with."""
import math

import numpy as np

#: ASE's defaults, under the key names of TorchMD_Net.capture_minimize(lbfgs=...), plus the convergence bound
LBFGS = dict(memory=100, alpha=70.0, max_step=0.2, damping=1.0, fmax=0.05)

MOVING, FROZEN, UNUSABLE = 0, 1, 2


class Molecule:
    """One optimiser: the history (lists, oldest first), the state before the last move, converged_at"""

    def __init__(self, p, free):
        self.p, self.free = p, np.asarray(free, bool)
        self.s, self.y, self.rho = [], [], []
        self.x_prev = self.f_prev = None
        self.converged_at = -1
        self.accepted, self.sy = 0, 0.0

    @property
    def h(self):
        return len(self.s)

    def update(self, s, y):
        """the candidate pair [n,3] (the rows of fixed atoms are ignored) -> accepted?"""
        s, y = np.where(self.free[:, None], s, 0.0).astype(np.float64), np.where(self.free[:, None], y, 0.0).astype(np.float64)
        self.sy = float(np.dot(s.ravel(), y.ravel()))
        self.accepted = int(self.sy > 0.0)
        if self.accepted:
            self.s.append(s)
            self.y.append(y)
            self.rho.append(1.0 / self.sy)
            if len(self.s) > self.p["memory"]:
                self.s.pop(0), self.y.pop(0), self.rho.pop(0)
        return self.accepted

    def direction(self, f):
        """the two loops on the vectors -> p [n,3] float64 (0 for a fixed atom)"""
        q = -np.where(self.free[:, None], f, 0.0).astype(np.float64).ravel()
        a = [0.0] * self.h
        for i in range(self.h - 1, -1, -1):
            a[i] = self.rho[i] * np.dot(self.s[i].ravel(), q)
            q = q - a[i] * self.y[i].ravel()
        z = q / self.p["alpha"]
        for i in range(self.h):
            b = self.rho[i] * np.dot(self.y[i].ravel(), z)
            z = z + self.s[i].ravel() * (a[i] - b)
        return -z.reshape(-1, 3)

    def control(self, x, f, step, pair=None):
        """One control after `step` steps from the positions and forces of this molecule's atoms [n,3].  -> (ret, p, c): p the
        direction and c the clamp factor of the next move (None, 0.0 unless MOVING).  ``pair``: the candidate (s, y) to take instead of
        x - x_prev and F_prev - F (an engine's own rounded candidate)"""
        self.accepted, self.sy = 0, 0.0
        if self.converged_at >= 0:
            return FROZEN, None, 0.0
        f = np.asarray(f, np.float64)
        ff = (np.where(self.free[:, None], f, 0.0) ** 2).sum(1)
        if not np.isfinite(ff).all() or not np.isfinite(np.asarray(x, np.float64)).all():
            return UNUSABLE, None, 0.0
        if math.sqrt(ff.max() if len(ff) else 0.0) < self.p["fmax"]:
            self.converged_at = step
            return FROZEN, None, 0.0
        if pair is not None:
            self.update(np.asarray(pair[0], np.float64), np.asarray(pair[1], np.float64))
        elif self.x_prev is not None:
            self.update(np.asarray(x, np.float64) - self.x_prev, self.f_prev - f)
        p = self.direction(f)
        return MOVING, p, clamp(p, self.p)

    def moved(self, x, f):
        """remember the state a move starts from"""
        self.x_prev, self.f_prev = np.array(x, np.float64), np.array(f, np.float64)


def clamp(p, par):
    """ASE's per-atom clamp -> c (a Python float)"""
    longest = math.sqrt(float((np.asarray(p, np.float64) ** 2).sum(1).max())) if len(p) else 0.0
    return par["damping"] * (par["max_step"] / longest) if longest >= par["max_step"] else par["damping"]


def two_loop(S, Y, g, alpha):
    """The two loops on given pairs (lists oldest first, flat float64 arrays) -> p"""
    q = np.array(g, np.float64)
    a = [0.0] * len(S)
    for i in range(len(S) - 1, -1, -1):
        a[i] = np.dot(S[i], q) / np.dot(Y[i], S[i])
        q = q - a[i] * Y[i]
    z = q / alpha
    for i in range(len(S)):
        b = np.dot(Y[i], z) / np.dot(Y[i], S[i])
        z = z + S[i] * (a[i] - b)
    return -z


def well_forces(kspring, x0, x, anharmonic=0.0):
    """Spring wells.  anharmonic = 0: F = -k d, d = x - x0.  Otherwise the quartic-softened spring E = k (u / 2 - 0.45 a u^2 +
    a^2 u^3 / 6), u = |d|^2: F = -k d (1 - 1.8 a u + a^2 u^2).  The bracket is positive everywhere (its discriminant is negative), so
    d = 0 is the only stationary point and the well confines; the radial curvature k (1 - 5.4 a u + 5 a^2 u^2) is NEGATIVE for
    0.237 < a u < 0.843, so the well is not convex and a step through that shell can violate s.y > 0."""
    d = np.asarray(x) - np.asarray(x0)
    k = np.asarray(kspring)[:, None]
    if anharmonic == 0.0:
        return -(k * d)
    u = (d * d).sum(1)[:, None]
    return -(k * d * (1.0 - 1.8 * anharmonic * u + (anharmonic * anharmonic) * (u * u)))


def wells(batch, n_mol, kspring, x0, x, p, max_steps, fixed=None, anharmonic=0.0):
    """The wells in fp64 -> steps taken, converged_at [n_mol], final x, per-step log: list of (h [n_mol], accepted [n_mol])"""
    batch = np.asarray(batch)
    k, x0, x = np.asarray(kspring, np.float64), np.asarray(x0, np.float64), np.asarray(x, np.float64).copy()
    free = np.ones(len(x), bool) if fixed is None else np.asarray(fixed) == 0
    idx = [np.nonzero(batch == m)[0] for m in range(n_mol)]
    mols = [Molecule(p, free[idx[m]]) for m in range(n_mol)]
    log = []
    step = 0
    while True:
        f = well_forces(k, x0, x, anharmonic)
        moves = []
        for m, mol in enumerate(mols):
            ret, d, c = mol.control(x[idx[m]], f[idx[m]], step)
            assert ret != UNUSABLE
            moves.append((ret, d, c))
        log.append((np.array([mol.h for mol in mols]), np.array([mol.accepted for mol in mols])))
        conv = np.array([mol.converged_at for mol in mols])
        if (conv >= 0).all() or step == max_steps:
            return step, conv, x, log
        for m, mol in enumerate(mols):
            ret, d, c = moves[m]
            mol.moved(x[idx[m]], f[idx[m]])
            if ret == MOVING:
                x[idx[m]] = x[idx[m]] + c * d
        step += 1
