"""TEST INFRASTRUCTURE ONLY: the specification of the cell relaxation of the device-resident FIRE minimiser, independent of the
engine's sources: ASE's UnitCellFilter scheme on top of tests/min_oracle.py's controller, one deformation gradient per molecule.

Row vectors.  Per molecule (fp64): the reference box H0, the deformation gradient D (I at the start), its velocity V_D, c =
cell_factor; the box is H = H0 D^T.  Per atom the integrated coordinate is xt = x D^-T, so x = xt D^T.  Generalised forces:
    atoms   Ft = F D
    cell    W_s = (W + W^T) / 2,  G = (W_s - p V I) D^-T,  V = |det H|;  hydrostatic: G <- (tr G / 3) I;  constant_volume:
            G <- G - (tr G / 3) I;  then the mask entry by entry;  the three rows of G / c are three more atoms at c D
Why: at fixed xt, dD strains the system by eps = D^-T dD^T, and W = -dE/d eps, so -dE/dD = W^T D^-T; V = V0 det D gives
-d(pV)/dD = -p V D^-T.  test_min_cell_host.py confirms the sign and the transpose by finite differences.
The cell rows' terms are added to the atoms' sums vf, ff, vv, fmax2; min_oracle.control64 then gives c_v, c_f, d, which are rounded
to fp32 once and used, widened, for the cell: V_D <- c_v V_D + c_f G / c, D <- D + (d V_D) / c.  Python floats: every statement is
one IEEE fp64 operation, in the order of the equations."""
import math

import numpy as np

from tests import min_oracle as O

OK, BAD_SUMS, BAD_VIRIAL, BAD_VOLUME = 0, 1, 2, 3

CELL = dict(mask=[[1.0] * 3] * 3, hydrostatic=False, constant_volume=False, pressure=0.0)


def det3(m):
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6])


def inv3(m, det):
    return [(m[4] * m[8] - m[5] * m[7]) / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
            (m[5] * m[6] - m[3] * m[8]) / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
            (m[3] * m[7] - m[4] * m[6]) / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det]


def _flat(a):
    return [float(t) for t in np.asarray(a, np.float64).reshape(-1)]


def cell_force(W, box, D, cp, c):
    """-> (why, G / c [9], V, stress [9]) of one molecule.  W and box are what the evaluation wrote and read (fp32 values)."""
    W, box, D, mask = _flat(W), _flat(box), _flat(D), _flat(cp["mask"])
    zero = [0.0] * 9
    if not all(math.isfinite(t) for t in W):
        return BAD_VIRIAL, zero, 0.0, zero
    V, det = abs(det3(box)), det3(D)
    if not (V > 0.0) or not math.isfinite(V) or not math.isfinite(det) or det == 0.0:
        return BAD_VOLUME, zero, 0.0, zero
    A = [0.5 * (W[3 * a + b] + W[3 * b + a]) for a in range(3) for b in range(3)]
    stress = [-t / V for t in A]
    pV = cp["pressure"] * V
    for k in (0, 4, 8):
        A[k] = A[k] - pV
    inv = inv3(D, det)
    G = [(A[3 * a] * inv[3 * b] + A[3 * a + 1] * inv[3 * b + 1]) + A[3 * a + 2] * inv[3 * b + 2] for a in range(3) for b in range(3)]
    if cp["hydrostatic"] or cp["constant_volume"]:
        t = ((G[0] + G[4]) + G[8]) / 3.0
        if cp["hydrostatic"]:
            G = [t if k in (0, 4, 8) else 0.0 for k in range(9)]
        else:
            for k in (0, 4, 8):
                G[k] = G[k] - t
    return OK, [(G[k] if mask[k] != 0.0 else 0.0) / c for k in range(9)], V, stress


def cell_sums(VD, Gc, sums):
    """the atoms' sums (vf, ff, vv, fmax2) with the three cell rows' terms added"""
    s = [float(t) for t in sums]
    for a in range(3):
        v, g = VD[3 * a:3 * a + 3], Gc[3 * a:3 * a + 3]
        t_ff = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
        s[0] = s[0] + ((g[0] * v[0] + g[1] * v[1]) + g[2] * v[2])
        s[1] = s[1] + t_ff
        s[2] = s[2] + ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        s[3] = t_ff if t_ff > s[3] else s[3]
    return s


def box_of(H0, D):
    """H0 D^T, nine fp64 entries"""
    return [(H0[3 * a] * D[3 * b] + H0[3 * a + 1] * D[3 * b + 1]) + H0[3 * a + 2] * D[3 * b + 2] for a in range(3) for b in range(3)]


def control(s, p, cp, c, sums, W, box, d32, H0, D, VD, step):
    """One molecule: the state dict s updated in place -> dict(ret, why, coef fp32 [3], sums [4], Gc, V, stress, D, VD, box fp32
    [9], d32 fp32 [9]); D, VD, box, d32 are the NEXT values (a frozen molecule: unchanged, VD = 0)."""
    box, d32, H0, D, VD = _flat(box), _flat(d32), _flat(H0), _flat(D), _flat(VD)
    out = dict(ret=O.FROZEN, why=OK, coef=np.zeros(3, np.float32), sums=[float(t) for t in sums], Gc=[0.0] * 9, V=0.0, stress=[0.0] * 9,
               D=list(D), VD=[0.0] * 9, box=np.array(box, np.float32), d32=np.array(d32, np.float32))
    if s["converged_at"] >= 0:
        return out
    why, Gc, V, stress = cell_force(W, box, D, cp, c)
    if why:
        return dict(out, ret=O.UNUSABLE, why=why)
    out.update(Gc=Gc, V=V, stress=stress, sums=cell_sums(VD, Gc, sums))
    before = dict(s)
    ret, coef = O.control(s, p, *out["sums"], step)
    out["ret"] = ret
    if ret == O.UNUSABLE:
        return dict(out, why=BAD_SUMS)
    if ret != O.MOVING:
        return out
    c_v, c_f, d = (float(t) for t in coef)
    VDn = [c_v * VD[k] + c_f * Gc[k] for k in range(9)]
    Dn = [D[k] + (d * VDn[k]) / c for k in range(9)]
    with np.errstate(over="ignore"):
        boxn, d32n = np.array(box_of(H0, Dn), np.float64).astype(np.float32), np.array(Dn, np.float64).astype(np.float32)
    Vn = abs(det3(_flat(boxn)))
    if not (np.isfinite(boxn).all() and np.isfinite(d32n).all() and Vn > 0.0 and math.isfinite(Vn)):
        s.update(before)
        return dict(out, ret=O.UNUSABLE, why=BAD_VOLUME)
    out.update(coef=np.array(coef, np.float32), D=Dn, VD=VDn, box=boxn, d32=d32n)
    return out


# ---- the test problem: a periodic crystal of nearest-neighbour springs -----------------------------------------------------------------
FCC = np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]])
R0, KSPRING = 1.0, 3.0  # the springs' rest length and constant


def crystal(reps=(1, 1, 1), shear=True):
    """fcc of lattice constant sqrt(2) R0 (nearest neighbours at R0), `reps` conventional cells, the box lower triangular and (with
    `shear`) triclinic -> x [N,3], H [3,3], bonds (i [M], j [M], n [M,3]): r = x_j - x_i + n H, every nearest-neighbour pair once"""
    a = math.sqrt(2.0) * R0
    reps = np.asarray(reps)
    frac = np.concatenate([(FCC + np.array([i, j, k])) / reps for i in range(reps[0]) for j in range(reps[1]) for k in range(reps[2])])
    H = np.diag(a * reps.astype(np.float64))
    if shear:
        H[1, 0], H[2, 0], H[2, 1] = 0.11 * a, -0.07 * a, 0.05 * a
    x = frac @ H
    N = len(x)
    bi, bj, bn = [], [], []
    for n in np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]):
        # the topology comes from the unsheared lattice: a shear of the box strains the bonds, it does not rewire them
        d = (frac[None, :, :] - frac[:, None, :] + n) * (a * reps)
        i, j = np.nonzero(np.abs(np.sqrt((d * d).sum(-1)) - R0) < 1e-6)
        # each bond once: (i, j, n) and (j, i, -n) are the same spring
        keep = (i < j) | ((i == j) & (tuple(n) > (0, 0, 0)))
        bi.append(i[keep]); bj.append(j[keep]); bn.append(np.repeat(n[None], keep.sum(), 0))
    bonds = (np.concatenate(bi), np.concatenate(bj), np.concatenate(bn).astype(np.float64))
    assert len(bonds[0]) == 6 * N  # twelve neighbours per atom
    return x, H, bonds


def crystal_efw(x, H, bonds):
    """fp64 -> energy, forces [N,3], virial W [3,3] = sum_bonds r (x) f (pair form; W = -dE/d eps under x -> x (I + eps), H likewise)"""
    x, H = np.asarray(x, np.float64), np.asarray(H, np.float64)
    i, j, n = bonds
    r = x[j] - x[i] + n @ H
    L = np.sqrt((r * r).sum(1))
    E = 0.5 * KSPRING * ((L - R0) ** 2).sum()
    f = -(KSPRING * (L - R0) / L)[:, None] * r  # on atom j; -f on atom i
    F = np.zeros_like(x)
    np.add.at(F, j, f)
    np.add.at(F, i, -f)
    return E, F, r.T @ f


def bond_lengths(x, H, bonds):
    i, j, n = bonds
    r = np.asarray(x, np.float64)[j] - np.asarray(x, np.float64)[i] + n @ np.asarray(H, np.float64)
    return np.sqrt((r * r).sum(1))


def generalised_forces(xt, H0, D, bonds, cp, c):
    """the scheme's forces at (xt, D) in fp64 -> Ft [N,3], G / c [3,3], enthalpy E + p V"""
    D = np.asarray(D, np.float64)
    H = np.asarray(H0, np.float64) @ D.T
    E, F, W = crystal_efw(np.asarray(xt, np.float64) @ D.T, H, bonds)
    why, Gc, V, _ = cell_force(W, H, D, cp, c)
    assert why == OK
    return F @ D, np.array(Gc).reshape(3, 3), E + cp["pressure"] * V


def project(G, cp):
    """what `hydrostatic` / `constant_volume` and the mask do to a full cell gradient (for the finite-difference check)"""
    G = np.array(G, np.float64)
    if cp["hydrostatic"]:
        G = np.eye(3) * (np.trace(G) / 3.0)
    elif cp["constant_volume"]:
        G = G - np.eye(3) * (np.trace(G) / 3.0)
    return G * np.asarray(cp["mask"], np.float64)


def relax(x, H0, bonds, p, cp, c, max_steps, fixed=None):
    """The whole scheme in fp64 with the coefficients unrounded for the atoms -> dict(steps, converged_at, x, H, D, fmax)"""
    x, H0 = np.asarray(x, np.float64), np.asarray(H0, np.float64)
    still = np.zeros(len(x), bool) if fixed is None else np.asarray(fixed) != 0
    xt, vt = x.copy(), np.zeros_like(x)
    D, VD = np.eye(3), np.zeros(9)
    s = O.new_state(p, 1)[0]
    step = 0
    while True:
        H = H0 @ D.T
        E, F, W = crystal_efw(xt @ D.T, H, bonds)
        Ft = np.where(still[:, None], 0.0, F @ D)
        ff = (Ft * Ft).sum(1)
        sums = [float((vt * Ft).sum()), float(ff.sum()), float((vt * vt).sum()), float(ff.max())]
        out = control(s, p, cp, c, sums, W, H, D, H0, D, VD, step)
        assert out["ret"] != O.UNUSABLE
        if s["converged_at"] >= 0 or step == max_steps:
            return dict(steps=step, converged_at=s["converged_at"], x=xt @ D.T, H=H, D=D, fmax=math.sqrt(out["sums"][3]), xt=xt)
        c_v, c_f, d = (float(t) for t in out["coef"])
        vt = np.where(still[:, None], 0.0, c_v * vt + c_f * Ft)
        xt = xt + d * vt
        D, VD = np.array(out["D"]).reshape(3, 3), np.array(out["VD"])
        step += 1


def length_bound(xt, D, H0, bonds, c, fmax):
    """The bound on max |L - R0| at a state that satisfies the convergence criterion at pressure 0.  With q the N + 3 rows of
    coordinates (xt, c D) and g the N + 3 rows of forces, every |g_r| < fmax, so |g|_2 < sqrt(N + 3) fmax.  Near the minimum the bond
    elongations are delta = R dq (R: the Jacobian of the bond lengths in q, here by central differences; dq orthogonal to the motions
    that change no length) and g = -k R^T delta, so |delta|_2 <= |g|_2 / (k sigma_min) with sigma_min the smallest non-zero singular
    value of R, and max |delta| <= |delta|_2.  The factor 1.01 covers the linearisation (|dq| ~ 1e-4 relative) and the rounding of the
    forces the run stopped on to fp32 (2^-24 relative)."""
    xt, D, H0 = np.asarray(xt, np.float64), np.asarray(D, np.float64), np.asarray(H0, np.float64)
    n = len(xt)

    def lengths(q):
        a, b = q[:3 * n].reshape(n, 3), q[3 * n:].reshape(3, 3) / c
        return bond_lengths(a @ b.T, H0 @ b.T, bonds)

    q = np.concatenate([xt.reshape(-1), c * D.reshape(-1)])
    R = np.stack([(lengths(q + 1e-6 * e) - lengths(q - 1e-6 * e)) / 2e-6 for e in np.eye(len(q))], 1)
    sv = np.linalg.svd(R, compute_uv=False)
    sigma = sv[sv > 1e-6 * sv[0]].min()
    return 1.01 * math.sqrt(n + 3) * fmax / (KSPRING * sigma)


def criterion_slack(x, box, bonds, c, fmax):
    """How far the largest row force of a converged fp32 run may exceed fmax when it is evaluated again in fp64 at (xt, D).  The run
    formed x = xt D32^T with three rounded products and two rounded sums per component and rounded D and the box to fp32, so each
    coordinate it evaluated is within e_x = 6 * 2^-24 max|x| of the fp64 value and each box entry within e_h = 2^-24 max|H|.  A bond
    vector r = x_j - x_i + n H then moves by at most e_r = sqrt(3) (2 e_x + 3 e_h) and its force by k e_r (1 + 2 |L - R0| / L) <=
    1.2 k e_r.  An atom has 12 bonds: its force moves by at most 14.4 k e_r, Ft by 1.1 times that (|D| <= 1.1).  A row of G / c moves
    by at most M (0.1 k e_r + 1.1 * 1.2 k e_r) 1.1 / c (M bonds; |r| <= 1.1, |f| <= 0.1 k, |D^-T| <= 1.1).  F and W were rounded to
    fp32 (2^-24 relative).  The slack is twice the sum."""
    eps = 2.0 ** -24
    e_x, e_h = 6 * eps * float(np.abs(x).max()), eps * float(np.abs(box).max())
    e_r = math.sqrt(3) * (2 * e_x + 3 * e_h)
    M = len(bonds[0])
    return 2 * (1.1 * 14.4 * KSPRING * e_r + M * (0.1 * KSPRING * e_r + 1.1 * 1.2 * KSPRING * e_r) * 1.1 / c + eps * fmax)
