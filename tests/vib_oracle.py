"""TEST INFRASTRUCTURE ONLY: the Hessian assembly and normal-mode preparation in plain numpy fp64, written from the equations
(include/tmdnet_amd.h, the tmdnet_vib_* block), not from the kernels: whole-array operations where the
kernels run entry by entry."""
import numpy as np

WAVENUMBER = 521.4709  # cm^-1 of sqrt(1 eV / (A^2 amu))


def plan(batch, fixed=None):
    """batch [N] non-decreasing, fixed [N] bool or None -> free_idx [n_free], fstart [B + 1], dims [B] = 3 nfree_b"""
    batch = np.asarray(batch, np.int64)
    B = int(batch.max()) + 1 if batch.size else 0
    free = np.ones(batch.shape, bool) if fixed is None else ~np.asarray(fixed, bool)
    free_idx = np.nonzero(free)[0].astype(np.int64)
    nfree = np.bincount(batch[free_idx], minlength=B).astype(np.int64)
    fstart = np.concatenate([[0], np.cumsum(nfree)]).astype(np.int64)
    return free_idx, fstart, 3 * nfree


def coordinate(free_idx, fstart, b, i):
    """(atom, component) of coordinate i of molecule b"""
    return int(free_idx[fstart[b] + i // 3]), i % 3


def central_entry(f_plus, f_minus, x_plus, x_minus):
    """-(F+ - F-) / (x+ - x-), the fp32 inputs widened, rounded to fp32 once"""
    num = np.asarray(f_plus, np.float32).astype(np.float64) - np.asarray(f_minus, np.float32).astype(np.float64)
    den = np.asarray(x_plus, np.float32).astype(np.float64) - np.asarray(x_minus, np.float32).astype(np.float64)
    return (-num / den).astype(np.float32)


def basis(x, m, mode):
    """x [n, 3], m [n] fp64 -> U [rank, 3 n]: translations (mode 1) or translations and rotations (mode 2), mass-weighted,
    orthonormalised in the order t_x t_y t_z r_x r_y r_z by modified Gram-Schmidt applied twice; kept when |w|^2 > 1e-12 |w0|^2"""
    n = x.shape[0]
    if mode == 0 or n == 0:
        return np.zeros((0, 3 * n))
    sm = np.sqrt(m)
    c = (m[:, None] * x).sum(0) / m.sum()
    cands = []
    for a in range(3):
        t = np.zeros((n, 3))
        t[:, a] = sm
        cands.append(t.reshape(-1))
    if mode == 2:
        for a in range(3):
            e = np.zeros(3)
            e[a] = 1.0
            cands.append((sm[:, None] * np.cross(e[None, :], x - c)).reshape(-1))
    kept = []
    for w0 in cands:
        w = w0.copy()
        for _ in range(2):
            for u in kept:
                w = w - (u @ w) * u
        if w @ w > 1e-12 * (w0 @ w0):
            kept.append(w / np.sqrt(w @ w))
    return np.array(kept).reshape(len(kept), 3 * n)


def finish(H, pos, mass, free_idx, fstart, project, mol_atoms=None):
    """H [B, D, D] (any float type; read as given), pos [N, 3], mass [N] -> (A [B, D, D] fp64, info [B, 8] fp64) as
    tmdnet_vib_finish writes them"""
    H = np.asarray(H).astype(np.float64)
    pos, mass = np.asarray(pos, np.float32).astype(np.float64), np.asarray(mass, np.float32).astype(np.float64)
    B, D = H.shape[0], H.shape[1]
    A, info = np.zeros((B, D, D)), np.zeros((B, 8))
    for b in range(B):
        idx = free_idx[fstart[b]:fstart[b + 1]]
        n = len(idx)
        Db = 3 * n
        h = H[b, :Db, :Db]
        mode = 0 if (mol_atoms is not None and n < mol_atoms[b]) else project
        info[b, 5], info[b, 4] = Db, mode
        if Db == 0:
            continue
        info[b, 0] = np.abs(h).max()
        info[b, 1] = np.abs(h - h.T).max()
        info[b, 2] = np.abs(h.reshape(Db, n, 3).sum(1)).max()
        m3 = np.repeat(mass[idx], 3)
        a = 0.5 * (h + h.T) / np.sqrt(np.outer(m3, m3))
        U = basis(pos[idx], mass[idx], mode)
        if len(U):
            P = np.eye(Db) - U.T @ U
            a = P @ a @ P
        info[b, 3] = len(U)
        A[b, :Db, :Db] = a
    return A, info


def spectrum(A, dims):
    """-> list of B ascending eigenvalue arrays of A[b, :D_b, :D_b]"""
    return [np.linalg.eigvalsh(0.5 * (A[b, :d, :d] + A[b, :d, :d].T)) if d else np.zeros(0) for b, d in enumerate(dims)]


def wavenumber_factor():
    """sqrt(eV / (A^2 amu)) / (2 pi c) in cm^-1 from CODATA 2018: e = 1.602176634e-19 C, amu = 1.66053906660e-27 kg, c = 299792458 m/s"""
    omega = np.sqrt(1.602176634e-19 / (1e-20 * 1.66053906660e-27))  # rad / s
    return omega / (2.0 * np.pi * 299792458.0 * 100.0)


def spring_hessian(x, bonds, k):
    """Hessian [3 n, 3 n] of E = sum_bonds k_ij (|x_i - x_j| - |x_i - x_j|_0)^2 / 2 AT the rest geometry x: per bond k e e^T blocks"""
    n = x.shape[0]
    H = np.zeros((3 * n, 3 * n))
    for (i, j), kk in zip(bonds, k):
        e = (x[i] - x[j]) / np.linalg.norm(x[i] - x[j])
        blk = kk * np.outer(e, e)
        H[3 * i:3 * i + 3, 3 * i:3 * i + 3] += blk
        H[3 * j:3 * j + 3, 3 * j:3 * j + 3] += blk
        H[3 * i:3 * i + 3, 3 * j:3 * j + 3] -= blk
        H[3 * j:3 * j + 3, 3 * i:3 * i + 3] -= blk
    return H


def spring_network(seed=4):
    """five molecules: a 7-atom cluster, three exactly collinear atoms, a diatomic, one atom, and a 7-atom cluster with one fixed atom;
    every pair of a molecule bonded by a spring.  -> batch, fixed, pos fp32, mass fp32, H [B, D, D] fp32 over the free coordinates"""
    rng = np.random.default_rng(seed)
    x = [rng.normal(size=(7, 3)) * 1.5,
         np.array([0.25, -1.0, 0.5]) + np.array([0.0, 1.0, 2.5])[:, None] * np.array([0.5, 1.0, -0.5]),  # exact in fp32
         np.array([[0.0, 0.0, 0.0], [0.75, -0.5, 1.25]]),
         np.array([[3.0, 1.0, -2.0]]),
         rng.normal(size=(7, 3)) * 1.5]
    sizes = [len(a) for a in x]
    batch = np.repeat(np.arange(len(x)), sizes).astype(np.int64)
    pos = np.concatenate(x).astype(np.float32)
    mass = rng.choice([1.008, 12.011, 15.999], size=len(batch)).astype(np.float32)
    fixed = np.zeros(len(batch), bool)
    fixed[sum(sizes[:4]) + 2] = True
    free_idx, fstart, dims = plan(batch, fixed)
    D = int(dims.max())
    H = np.zeros((len(x), D, D), np.float32)
    start = np.concatenate([[0], np.cumsum(sizes)])
    for b, xb in enumerate(x):
        n = len(xb)
        bonds = [(i, j) for i in range(n) for j in range(i + 1, n)]
        full = spring_hessian(pos[start[b]:start[b + 1]].astype(np.float64), bonds, 1.0 + rng.random(len(bonds)))
        keep = np.repeat(~fixed[start[b]:start[b + 1]], 3)
        h = full[np.ix_(keep, keep)].astype(np.float32)
        h = np.triu(h) + np.triu(h, 1).T  # exactly symmetric in fp32
        H[b, :dims[b], :dims[b]] = h
    return batch, fixed, pos, mass, H, np.bincount(batch)
