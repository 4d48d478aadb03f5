"""TEST INFRASTRUCTURE ONLY: the barostat arithmetic of the device-resident MD loop (torchmd-net_amd/csrc/tn_md_math.h) on the CPU,
compiled host-only from tests/md_baro_host.hip into oracle/_build/libmd_baro_host.so and called through ctypes on numpy arrays.
The statements are the header's own; tests/test_md_barostat_host.py compares them with tests/md_baro_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libmd_baro_host.so")
        src = [os.path.join(ROOT, "tests", "md_baro_host.hip"), os.path.join(ROOT, "torchmd-net_amd", "csrc", "tn_md_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", src[0], "-o", so])
        _LIB = C.CDLL(so)
        for name in ("baro_noise", "baro_move", "baro_scale"):
            getattr(_LIB, name).restype = None
        _LIB.baro_ideal_gas.restype = C.c_int64
    return _LIB


def _p(a):
    return C.c_void_p(0) if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def noise(seed, step, mols):
    """xi of the barostat of molecules `mols` after `step` completed steps, fp64 (the widened fp32 normal)"""
    mols = _c(mols, np.uint32)
    out = np.full(len(mols), np.nan, np.float64)
    lib().baro_noise(C.c_int64(len(mols)), C.c_uint64(seed), C.c_uint64(step), _p(mols), _p(out))
    return out


def move(box, W, ekin, force_scale, P0, kT, a, seed=0, step=0):
    """box, W [n,3,3], ekin [n] -> V, P (fp64), mu32, nu32 (fp32), flag (int32) per molecule"""
    box, W, ekin = _c(box, np.float32), _c(W, np.float32), _c(ekin, np.float32)
    n = len(ekin)
    V, P = np.full(n, np.nan), np.full(n, np.nan)
    mu, nu = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    flag = np.full(n, -1, np.int32)
    lib().baro_move(C.c_int64(n), _p(box), _p(W), _p(ekin), C.c_double(force_scale), C.c_double(P0), C.c_double(kT), C.c_double(a),
                    C.c_uint64(seed), C.c_uint64(step), _p(V), _p(P), _p(mu), _p(nu), _p(flag))
    return V, P, mu, nu, flag


def scale(batch, mu, nu, box, x, v):
    """-> (box, x, v) scaled: box and x by mu, v by nu of the atom's molecule"""
    batch, mu, nu = _c(batch, np.int64), _c(mu, np.float32), _c(nu, np.float32)
    box, x, v = _c(box, np.float32).copy(), _c(x, np.float32).copy(), _c(v, np.float32).copy()
    lib().baro_scale(C.c_int64(len(mu)), C.c_int64(len(x)), _p(batch), _p(mu), _p(nu), _p(box), _p(x), _p(v))
    return box, x, v


def ideal_gas(box, x, v, hk, mass, sigma, dt, c1, c2, seed, force_scale, P0, kT, compressibility, tau, baro_seed, steps):
    """R replicas of n atoms, F = 0 and W = 0, Langevin + barostat for `steps` steps -> volumes [steps, R] (before each move)"""
    box, x, v = _c(box, np.float32).copy(), _c(x, np.float32).copy(), _c(v, np.float32).copy()
    hk, mass, sigma = _c(hk, np.float32), _c(mass, np.float32), _c(sigma, np.float32)
    R = len(box)
    n = len(x) // R
    vol = np.full((steps, R), np.nan, np.float32)
    bad = lib().baro_ideal_gas(C.c_int64(R), C.c_int64(n), C.c_int64(steps), _p(box), _p(x), _p(v), _p(hk), _p(mass), _p(sigma),
                               C.c_float(dt), C.c_float(c1), C.c_float(c2), C.c_uint64(seed), C.c_double(force_scale), C.c_double(P0),
                               C.c_double(kT), C.c_double(compressibility), C.c_double(tau), C.c_uint64(baro_seed), _p(vol))
    assert bad == 0, bad
    return vol
