"""TEST INFRASTRUCTURE ONLY: the specification of the anisotropic cell barostat of the device-resident MD loop, independent of the
engine's sources.

Anisotropic stochastic cell rescaling (Bernetti and Bussi, J. Chem. Phys. 153, 114107, 2020) written in the exponent, first order, one
barostat per molecule, row vectors (x -> x mu, box -> box mu), h = box:
    V = |det h|;  P = (2 Kt + W) / V;  a = compressibility dt / tau;  D_f = -(a / 3) (P0 I - P) + sqrt(2 kT a / (3 V)) Xi
    D = Pi(D_f);  mu = expm(D);  nu = expm(-D^T)
Pi: the identity ("anisotropic"), the diagonal ("diagonal"), or the diagonal with the two entries other than `axis` replaced by their
mean ("semi-isotropic").  In "anisotropic" mode h mu = L Q by Gram-Schmidt on its rows, top down, q2 = q0 x q1, and
Mx = mu Q^T, Mv = nu Q^T, Mf = Q^T, box' = L; in the two diagonal modes Q = I and box' = h mu.  numpy fp64 with scipy's (or torch's)
matrix exponential; the four results rounded to fp32 once.  Row r of Xi is the Box-Muller triple of one Philox4x32-10 call
(tests/md_oracle.py, pure Python) with the counter (step lo, step hi, molecule, 4 + r), through the loop's map in fp32.  And the same
scheme vectorised (torch fp64, numpy's generator) for ensemble statistics."""
import math

import numpy as np
import torch

from tests import md_oracle as O

MASK = 0xFFFFFFFF
TAG = 4
COUPLINGS = ("anisotropic", "diagonal", "semi-isotropic")

try:
    from scipy.linalg import expm as _expm
except ImportError:  # pragma: no cover
    def _expm(A):
        return torch.linalg.matrix_exp(torch.from_numpy(np.asarray(A, np.float64))).numpy()


def expm(A):
    return np.asarray(_expm(np.asarray(A, np.float64)))


def noise(seed, step, mol):
    """Xi [3,3] of molecule `mol` after `step` completed steps.  The Box-Muller map one fp32 operation at a time, as the loop's
    contract has it (u from md_oracle.uniform is exact in fp32)"""
    f = np.float32
    out = np.empty((3, 3))
    for r in range(3):
        w = O.philox4x32_10((step & MASK, step >> 32, mol, TAG + r), (seed & MASK, seed >> 32))
        u = [f(O.uniform(t)) for t in w]
        r0, r1 = np.sqrt(f(-2.0) * np.log(u[0])), np.sqrt(f(-2.0) * np.log(u[2]))
        a0, a1 = f(6.283185307179586) * u[1], f(6.283185307179586) * u[3]
        out[r] = [float(f(r0 * np.cos(a0))), float(f(r0 * np.sin(a0))), float(f(r1 * np.cos(a1)))]
    return out


def noise_f64(seed, step, mol):
    """the same normals with the map in fp64 (agrees with `noise` to fp32 accuracy)"""
    return np.array([O.normals(O.philox4x32_10((step & MASK, step >> 32, mol, TAG + r), (seed & MASK, seed >> 32))) for r in range(3)])


def ktensor(batch, mass, vel, n_mol):
    """-> Kt [n_mol,3,3] fp64 = sum over the atoms of 0.5 m v_a v_b (unit of m v^2); an atom of infinite mass contributes nothing"""
    m = np.asarray(mass, np.float32).astype(np.float64)
    v = np.asarray(vel, np.float32).astype(np.float64)
    t = np.where(np.isinf(m), 0.0, 0.5 * np.where(np.isinf(m), 0.0, m))[:, None, None] * v[:, :, None] * v[:, None, :]
    t[np.isinf(m)] = 0.0
    out = np.zeros((n_mol, 3, 3))
    np.add.at(out, np.asarray(batch), t)
    return out


def six(Kt):
    """[...,3,3] -> [...,6]: xx, xy, xz, yy, yz, zz"""
    Kt = np.asarray(Kt)
    return np.stack([Kt[..., 0, 0], Kt[..., 0, 1], Kt[..., 0, 2], Kt[..., 1, 1], Kt[..., 1, 2], Kt[..., 2, 2]], axis=-1)


def project(Df, coupling, axis=2):
    if coupling == "anisotropic":
        return np.array(Df, np.float64)
    d = np.diag(Df).astype(np.float64).copy()
    if coupling == "semi-isotropic":
        others = [i for i in range(3) if i != axis]
        d[others] = 0.5 * (d[others[0]] + d[others[1]])
    return np.diag(d)


def gram_schmidt(hp):
    """rows of hp, top down, q2 = q0 x q1: hp = L Q, L lower triangular -> L, Q"""
    q0 = hp[0] / np.linalg.norm(hp[0])
    u = hp[1] - (hp[1] @ q0) * q0
    q1 = u / np.linalg.norm(u)
    Q = np.stack([q0, q1, np.cross(q0, q1)])
    return np.tril(hp @ Q.T), Q


def move(box, W, Kt, force_scale, P0, kT, a, coupling, axis=2, Xi=None):
    """One molecule; Kt [3,3] in the unit of m v^2.  -> dict: V, P, D, mu, nu, L, Q (fp64) and Mx, Mv, Mf, box (fp32)"""
    h = np.asarray(box, np.float32).astype(np.float64).reshape(3, 3)
    w = np.asarray(W, np.float32).astype(np.float64).reshape(3, 3)
    V = abs(np.linalg.det(h))
    P = (2.0 * np.asarray(Kt, np.float64) / force_scale + w) / V
    Df = -(a / 3.0) * (P0 * np.eye(3) - P)
    if kT > 0.0:
        Df = Df + math.sqrt(2.0 * kT * a / (3.0 * V)) * np.asarray(Xi, np.float64)
    D = project(Df, coupling, axis)
    mu, nu = expm(D), expm(-D.T)
    hp = h @ mu
    if coupling == "anisotropic":
        L, Q = gram_schmidt(hp)
    else:
        L, Q = hp, np.eye(3)
    f = np.float32
    return dict(V=V, P=P, D=D, mu=mu, nu=nu, L=L, Q=Q, Mx=(mu @ Q.T).astype(f), Mv=(nu @ Q.T).astype(f), Mf=Q.T.astype(f), box=L.astype(f))


def moves(box, W, Kt, force_scale, P0, kT, a, coupling, axis=2, seed=0, step=0):
    """every molecule of box, W, Kt [n,3,3] -> dict of stacked arrays"""
    out = [move(box[m], W[m], Kt[m], force_scale, P0, kT, a, coupling, axis, noise(seed, step, m) if kT > 0.0 else None)
           for m in range(len(box))]
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


def ulp_distance(a, b):
    """|a - b| in units in the last place of fp32, counted across zero"""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    return np.abs(key(a) - key(b))


def close_to_oracle(got, ref64):
    """the issue's terms: every fp32 entry bit-equal to fp32(oracle), within one fp32 ulp of it, or within 1e-12 absolute -> bool array"""
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref64, np.float64)
    return (ulp_distance(got, ref.astype(np.float32)) <= 1) | (np.abs(got.astype(np.float64) - ref) <= 1e-12)


def _project_batch(Df, coupling, axis):
    if coupling == "anisotropic":
        return Df
    d = torch.diagonal(Df, dim1=1, dim2=2).clone()
    if coupling == "semi-isotropic":
        others = [i for i in range(3) if i != axis]
        mean = 0.5 * (d[:, others[0]] + d[:, others[1]])
        d[:, others[0]] = mean
        d[:, others[1]] = mean
    return torch.diag_embed(d)


def ideal_gas(R, n, steps, dt, friction, kT, P0, compressibility, tau, h0, coupling, axis=2, seed=0, mass=1.0, force_scale=1.0,
              kappa=0.0, eps0=0.0):
    """The ideal gas (F = 0) of R replicas of n atoms under Langevin + the cell barostat, torch fp64 with numpy's generator: per step O
    on the velocities, Kt, the move, h <- h mu, v <- v nu (no rotation: volumes and, in the diagonal modes, lengths do not need it).
    W = 0, or with kappa > 0 the synthetic W_aa = -kappa (ln h_aa - eps0).  -> volumes [steps,R], lengths [steps,R,3] before each move"""
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    c1 = math.exp(-friction * dt)
    c2 = math.sqrt(1.0 - c1 * c1)
    sigma = math.sqrt(kT * force_scale / mass)
    v = t(sigma * rng.normal(size=(R, n, 3)))
    h = t(h0).expand(R, 3, 3).clone()
    a = compressibility * dt / tau
    eye = torch.eye(3, dtype=torch.float64)
    vol, length = np.empty((steps, R)), np.empty((steps, R, 3))
    for s in range(steps):
        v = c1 * v + c2 * sigma * t(rng.normal(size=(R, n, 3)))
        V = torch.linalg.det(h).abs()
        Kt = 0.5 * mass * torch.einsum("rna,rnb->rab", v, v) / force_scale
        W = torch.zeros(R, 3, 3, dtype=torch.float64)
        if kappa > 0.0:
            W = torch.diag_embed(-kappa * (torch.log(torch.diagonal(h, dim1=1, dim2=2)) - eps0))
        P = (2.0 * Kt + W) / V[:, None, None]
        Df = -(a / 3.0) * (P0 * eye - P) + torch.sqrt(2.0 * kT * a / (3.0 * V))[:, None, None] * t(rng.normal(size=(R, 3, 3)))
        D = _project_batch(Df, coupling, axis)
        vol[s], length[s] = V.numpy(), torch.diagonal(h, dim1=1, dim2=2).numpy()
        h = h @ torch.linalg.matrix_exp(D)
        v = v @ torch.linalg.matrix_exp(-D.transpose(1, 2))
    return vol, length


# ---- the per-axis ensemble, exactly solvable ------------------------------------------------------------------------------------------
# An ideal gas of n = 16 atoms at kT = 0.025 (m = 1, force_scale = 1, Langevin friction 0.1, dt = 1) under P0 = 0 with the synthetic
# virial W_aa = -kappa (ln L_a - eps0), kappa = 10, eps0 = ln(400) / 3, compressibility 48, tau 20: the enthalpy is a sum over the
# axes of kappa / 2 (ln L_a - eps0)^2, the measure is V^n prod dL_a = prod L_a^(n+1) d ln L_a, so every e_a = ln L_a - eps0 is Gaussian
# with mean (n + 1) kT / kappa and variance kT / kappa ("diagonal"); in "semi-isotropic" mode the coupled pair shares one e with the
# same mean and variance kT / (2 kappa).  R = 256 replicas, 3 000 steps, the first 500 dropped.  Bounds: mean and variance within 5 %
# of theory - about 4 to 5 standard errors at roughly 12 800 independent samples; a noise amplitude off by sqrt(2) or a missing Ito
# cancellation (a shift of the mean by kT / kappa in n + 1 = 17: 6 %) is outside.
PER_AXIS = dict(R=256, n=16, steps=3000, drop=500, dt=1.0, friction=0.1, kT=0.025, P0=0.0, kappa=10.0, eps0=math.log(400.0) / 3.0,
                compressibility=48.0, tau=20.0)


def per_axis_state(seed=23):
    """-> box [R,3,3], x, v [R n,3], hk, mass, sigma [R n], c1, c2 for the per-axis ensemble (fp32, as the loop takes them)"""
    e = PER_AXIS
    R, n = e["R"], e["n"]
    rng = np.random.default_rng(seed)
    side = 400.0 ** (1.0 / 3.0)
    box = np.tile((np.eye(3) * side).astype(np.float32), (R, 1, 1))
    x = rng.uniform(0, side, size=(R * n, 3)).astype(np.float32)
    v = (math.sqrt(e["kT"]) * rng.normal(size=(R * n, 3))).astype(np.float32)
    c1 = math.exp(-e["friction"] * e["dt"])
    return (box, x, v, np.full(R * n, 0.5 * e["dt"], np.float32), np.ones(R * n, np.float32),
            np.full(R * n, math.sqrt(e["kT"]), np.float32), c1, math.sqrt(1 - c1 * c1))


def per_axis_ratios(lengths, coupling, axis=2):
    """lengths [steps,R,3] (all steps) -> list of (mean / theory, variance / theory) per independent strain, asserted by the caller:
    three for "diagonal"; for "semi-isotropic" the coupled pair (variance kT / 2 kappa) and then the free axis"""
    e = PER_AXIS
    eps = np.log(np.asarray(lengths, np.float64)[e["drop"]:]) - e["eps0"]
    mean, var = (e["n"] + 1) * e["kT"] / e["kappa"], e["kT"] / e["kappa"]
    if coupling == "diagonal":
        return [(eps[..., d].mean() / mean, eps[..., d].var() / var) for d in range(3)]
    others = [i for i in range(3) if i != axis]
    pair = 0.5 * (eps[..., others[0]] + eps[..., others[1]])
    return [(pair.mean() / mean, pair.var() / (0.5 * var)), (eps[..., axis].mean() / mean, eps[..., axis].var() / var)]
