"""TEST INFRASTRUCTURE ONLY: a float64 numpy statement of the ZBL and D2 pair priors (reference torchmdnet/priors/zbl.py:83-112,
priors/d2.py:163-201), written from the formulas and independent of csrc/tn_prior_math.h.  Energies per molecule, forces from the
analytic du/dr, the virial W_m[a][b] = -dE_m/d eps_ab, the per-atom energies e_i = 1/2 sum_j u_ij - and, behind every output element,
S: the sum of the ABSOLUTE pair terms it is made of, the scale of the tests' bounds (the terms cancel, so the result itself is not).

A prior is a dict: ZBL  dict(cutoff=, distance_scale=, energy_scale=, Z=[per species atomic number])
                   D2   dict(cutoff=, distance_scale=, energy_scale=, C6=[per species, J/mol nm^6], Rr=[per species, nm])"""
import numpy as np

BOHR, ZBL_E, AVOGADRO = 5.29177210903e-11, 2.30707755e-28, 6.02214076e23
ZBL_C = ((0.1818, 3.2), (0.5099, 0.9423), (0.2802, 0.4029), (0.02817, 0.2016))


def zbl_u(r, Zi, Zj, cutoff, distance_scale, energy_scale, deriv=0):
    """u(r) (deriv=0) or du/dr (deriv=1) of one ZBL pair, r < cutoff; any float type numpy carries (float64, longdouble)."""
    r = np.asarray(r)
    a = 0.8854 * BOHR / (Zi ** 0.23 + Zj ** 0.23)
    s = distance_scale / a
    phi = sum(c * np.exp(-k * r * s) for c, k in ZBL_C)
    cut = 0.5 * (np.cos(np.pi * r / cutoff) + 1.0)
    pre = ZBL_E / energy_scale / distance_scale * Zi * Zj
    if not deriv:
        return pre * phi * cut / r
    dphi = sum(-c * k * s * np.exp(-k * r * s) for c, k in ZBL_C)
    dcut = -0.5 * np.pi / cutoff * np.sin(np.pi * r / cutoff)
    return pre * ((dphi * cut + phi * dcut) / r - phi * cut / r ** 2)


def d2_u(r, C6i, C6j, Rri, Rrj, distance_scale, energy_scale, deriv=0, d=20.0, s6=1.0):
    """u(r) or du/dr of one D2 pair (hard cutoff: none here)."""
    r = np.asarray(r)
    snm = distance_scale * 1e9
    R = r * snm
    c6 = np.sqrt(C6i * C6j)
    rr = Rri + Rrj
    t = np.exp(-d * (R / rr - 1.0))
    f = 1.0 / (1.0 + t)
    pre = -s6 * c6 / (energy_scale * AVOGADRO)
    if not deriv:
        return pre * f / R ** 6
    df = d / rr * t * f * f
    return pre * (df / R ** 6 - 6.0 * f / R ** 7) * snm


def minimum_image(delta, box):
    """Triclinic minimum image, z -> y -> x, of delta [..., 3] (the neighbour search's convention)."""
    delta = delta.copy()
    for k in (2, 1, 0):
        s = np.round(delta[..., k] / box[k, k])
        delta -= s[..., None] * box[k]
    return delta


def pair_vectors(pos, box=None):
    """r_ij = pos_i - pos_j [n, n, 3]; with a box, the image is taken on pos[hi] - pos[lo] (hi > lo), so r_ji = -r_ij exactly."""
    d = pos[:, None, :] - pos[None, :, :]
    if box is not None:
        m = minimum_image(d, box)
        lower = np.tril(np.ones(d.shape[:2], bool), -1)[..., None]
        d = np.where(lower, m, -np.swapaxes(m, 0, 1))
    return d


def _terms(pos, z, box, zbl, d2):
    """[(pair vectors [n,n,3], r [n,n], u [n,n], du [n,n])] of the active priors of one molecule; zero outside the cutoff."""
    out = []
    n = len(pos)
    off = ~np.eye(n, dtype=bool)
    for kind, p in (("zbl", zbl), ("d2", d2)):
        if p is None:
            continue
        vec = pair_vectors(pos, box if kind == "zbl" else None)  # D2 never sees the box
        r = np.sqrt((vec ** 2).sum(-1))
        inside = off & (r > 0) & (r < p["cutoff"])
        rs = np.where(inside, r, 1.0)
        if kind == "zbl":
            Z = np.asarray(p["Z"], np.float64)[z]
            args = (Z[:, None], Z[None, :], p["cutoff"], p["distance_scale"], p["energy_scale"])
            u, du = zbl_u(rs, *args), zbl_u(rs, *args, deriv=1)
        else:
            C6, Rr = np.asarray(p["C6"], np.float64)[z], np.asarray(p["Rr"], np.float64)[z]
            args = (C6[:, None], C6[None, :], Rr[:, None], Rr[None, :], p["distance_scale"], p["energy_scale"])
            u, du = d2_u(rs, *args), d2_u(rs, *args, deriv=1)
        out.append((vec, rs, np.where(inside, u, 0.0), np.where(inside, du, 0.0), r, inside))
    return out


def evaluate(pos, z, batch, n_mol, box=None, zbl=None, d2=None):
    """-> dict(E [B], F [N,3], W [B,3,3], e [N]; S_E, S_F, S_W, S_e: the sums of absolute pair terms; margin: the smallest distance
    of a pair from a cutoff, in the caller's length unit).  ``box``: None, [3,3] or [B,3,3]."""
    pos, z, batch = np.asarray(pos, np.float64), np.asarray(z), np.asarray(batch)
    N = len(pos)
    E, W, e, F = np.zeros(n_mol), np.zeros((n_mol, 3, 3)), np.zeros(N), np.zeros((N, 3))
    S_E, S_W, S_e, S_F = np.zeros(n_mol), np.zeros((n_mol, 3, 3)), np.zeros(N), np.zeros((N, 3))
    margin = np.inf
    for m in range(n_mol):
        idx = np.nonzero(batch == m)[0]
        if len(idx) < 2:
            continue
        bm = None if box is None else np.asarray(box[m] if np.ndim(box) == 3 else box, np.float64)
        for (vec, r, u, du, r_raw, inside), p in zip(_terms(pos[idx], z[idx], bm, zbl, d2), [q for q in (zbl, d2) if q is not None]):
            off = ~np.eye(len(idx), dtype=bool)
            margin = min(margin, np.abs(r_raw[off] - p["cutoff"]).min())
            g = (du / r)[..., None] * vec  # d u_ij / d pos_i
            e[idx] += 0.5 * u.sum(1)
            S_e[idx] += 0.5 * np.abs(u).sum(1)
            F[idx] -= g.sum(1)
            S_F[idx] += np.abs(g).sum(1)
            w = -0.5 * g[..., :, None] * vec[..., None, :]
            W[m] += w.sum((0, 1))
            S_W[m] += np.abs(w).sum((0, 1))
        E[m], S_E[m] = e[idx].sum(), S_e[idx].sum()
    return dict(E=E, F=F, W=W, e=e, S_E=S_E, S_F=S_F, S_W=S_W, S_e=S_e, margin=margin)


def energy_only(pos, z, batch, n_mol, box=None, zbl=None, d2=None):
    return evaluate(pos, z, batch, n_mol, box, zbl, d2)["E"]
