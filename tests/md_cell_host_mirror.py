"""TEST INFRASTRUCTURE ONLY: the anisotropic cell-rescaling arithmetic of the device-resident MD loop
(torchmd-net_amd/csrc/tn_md_cell_math.h) on the CPU, compiled host-only from tests/md_cell_host.hip into
oracle/_build/libmd_cell_host.so and called through ctypes on numpy arrays.  The statements are the header's own;
tests/test_md_cell_host.py compares them with tests/md_cell_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "md_cell_host.hip")
COUPLINGS = {"anisotropic": 0, "diagonal": 1, "semi-isotropic": 2}
_LIB = None


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libmd_cell_host.so")
        src = [SOURCE] + [os.path.join(ROOT, "torchmd-net_amd", "csrc", h) for h in ("tn_md_cell_math.h", "tn_md_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-O2", "-fPIC", "-shared", SOURCE, "-o", so])
        _LIB = C.CDLL(so)
        for name in ("cell_noise", "cell_expm", "cell_ktensor", "cell_move", "cell_scale"):
            getattr(_LIB, name).restype = None
        _LIB.cell_ideal_gas.restype = C.c_int64
    return _LIB


def _p(a):
    return C.c_void_p(0) if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def noise(seed, step, mols):
    """Xi [n,3,3] of the molecules `mols` after `step` completed steps, fp64 (widened fp32 normals)"""
    mols = _c(mols, np.uint32)
    out = np.full((len(mols), 3, 3), np.nan)
    lib().cell_noise(C.c_int64(len(mols)), C.c_uint64(seed), C.c_uint64(step), _p(mols), _p(out))
    return out


def expm(A):
    A, E = _c(A, np.float64), np.full((3, 3), np.nan)
    lib().cell_expm(_p(A), _p(E))
    return E


def ktensor(batch, mass, vel, n_mol):
    """-> kt [n_mol,6] fp64: xx, xy, xz, yy, yz, zz of sum 0.5 m v_a v_b"""
    batch, mass, vel = _c(batch, np.int64), _c(mass, np.float32), _c(vel, np.float32)
    kt = np.full((n_mol, 6), np.nan)
    lib().cell_ktensor(C.c_int64(len(mass)), C.c_int64(n_mol), _p(batch), _p(mass), _p(vel), _p(kt))
    return kt


def move(box, W, kt, force_scale, P0, kT, a, coupling, axis=2, seed=0, step=0):
    """box, W [n,3,3], kt [n,6] -> dict of V [n], P, D, mu, nu, L, Q [n,3,3] (fp64), Mx, Mv, Mf, box [n,3,3] (fp32), flag [n]"""
    box, W, kt = _c(box, np.float32), _c(W, np.float32), _c(kt, np.float64)
    n = len(kt)
    d = {k: np.full((n, 3, 3), np.nan) for k in ("P", "D", "mu", "nu", "L", "Q")}
    V, M, nb, flag = np.full(n, np.nan), np.full((n, 27), np.nan, np.float32), np.full((n, 3, 3), np.nan, np.float32), np.full(n, -1, np.int32)
    lib().cell_move(C.c_int64(n), _p(box), _p(W), _p(kt), C.c_double(force_scale), C.c_double(P0), C.c_double(kT), C.c_double(a),
                    C.c_uint64(seed), C.c_uint64(step), C.c_int32(COUPLINGS[coupling]), C.c_int32(axis), _p(V), _p(d["P"]), _p(d["D"]),
                    _p(d["mu"]), _p(d["nu"]), _p(d["L"]), _p(d["Q"]), _p(M), _p(nb), _p(flag))
    M = M.reshape(n, 3, 3, 3)
    d.update(V=V, Mx=M[:, 0].copy(), Mv=M[:, 1].copy(), Mf=M[:, 2].copy(), box=nb, flag=flag)
    return d


def scale(batch, Mx, Mv, Mf, diag, x, v, f):
    """-> (x, v, f) of every atom by the matrices of its molecule; diag: one product per component, f untouched"""
    batch = _c(batch, np.int64)
    M = _c(np.stack([Mx, Mv, Mf], axis=1), np.float32)
    x, v, f = _c(x, np.float32).copy(), _c(v, np.float32).copy(), _c(f, np.float32).copy()
    lib().cell_scale(C.c_int64(len(x)), _p(batch), _p(M), C.c_int32(int(diag)), _p(x), _p(v), _p(f))
    return x, v, f


def ideal_gas(box, x, v, hk, mass, sigma, dt, c1, c2, seed, force_scale, P0, kT, compressibility, tau, baro_seed, steps, coupling,
              axis=2, kappa=0.0, eps0=0.0):
    """R replicas of n atoms, F = 0, Langevin + the cell barostat for `steps` steps; W = 0, or with kappa > 0 the synthetic
    W_aa = -kappa (ln box_aa - eps0).  -> volumes [steps,R], lengths [steps,R,3] (before each move)"""
    box, x, v = _c(box, np.float32).copy(), _c(x, np.float32).copy(), _c(v, np.float32).copy()
    hk, mass, sigma = _c(hk, np.float32), _c(mass, np.float32), _c(sigma, np.float32)
    R = len(box)
    n = len(x) // R
    vol, length = np.full((steps, R), np.nan, np.float32), np.full((steps, R, 3), np.nan, np.float32)
    bad = lib().cell_ideal_gas(C.c_int64(R), C.c_int64(n), C.c_int64(steps), _p(box), _p(x), _p(v), _p(hk), _p(mass), _p(sigma),
                               C.c_float(dt), C.c_float(c1), C.c_float(c2), C.c_uint64(seed), C.c_double(force_scale), C.c_double(P0),
                               C.c_double(kT), C.c_double(compressibility), C.c_double(tau), C.c_uint64(baro_seed),
                               C.c_int32(COUPLINGS[coupling]), C.c_int32(axis), C.c_double(kappa), C.c_double(eps0), _p(vol), _p(length))
    assert bad == 0, bad
    return vol, length


def build_program(out, sanitize=True):
    """the stand-alone program of tests/md_cell_host.hip (its own main), a host build"""
    cmd = [hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DMD_CELL_HOST_MAIN"]
    if sanitize:
        cmd += ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd + [SOURCE, "-o", out])
    return out
