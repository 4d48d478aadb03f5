"""TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident FIRE minimiser (torchmd-net_amd/csrc/tn_min_math.h) on the CPU,
compiled host-only from tests/min_host.hip into oracle/_build/libmin_host.so and called through ctypes on numpy arrays.
The statements are the header's own; tests/test_min_host.py compares them with tests/min_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libmin_host.so")
        csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
        src = [os.path.join(ROOT, "tests", "min_host.hip"), os.path.join(csrc, "tn_min_math.h"), os.path.join(csrc, "tn_md_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", src[0], "-o", so])
        _LIB = C.CDLL(so)
        for name in ("min_terms", "min_control", "min_update"):
            getattr(_LIB, name).restype = None
        _LIB.min_wells.restype = C.c_int64
    return _LIB


def _p(a):
    return C.c_void_p(0) if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _fire_args(p):
    """the parameters of tests/min_oracle.py's dict in the order of the C entries (dt_max ... fmax)"""
    return (C.c_double(p["dt_max"]), C.c_int32(p["n_min"]), C.c_double(p["f_inc"]), C.c_double(p["f_dec"]), C.c_double(p["alpha"]),
            C.c_double(p["f_alpha"]), C.c_double(p["max_step"]), C.c_double(p["fmax"]))


def terms(v, f, fixed=None):
    """v, f [n,3] -> t [n,3] fp32: v.f, f.f, v.v per atom"""
    v, f = _c(v, np.float32), _c(f, np.float32)
    fixed = None if fixed is None else _c(fixed, np.uint8)
    t = np.full((len(v), 3), np.nan, np.float32)
    lib().min_terms(C.c_int64(len(v)), _p(v), _p(f), _p(fixed), _p(t))
    return t


def control(state, sums, p, step):
    """state = (dt, alpha, n_pos, converged_at) arrays [n], sums [n,4] -> new state, coef [n,3] fp32, ret [n]"""
    dt, alpha = _c(state[0], np.float64).copy(), _c(state[1], np.float64).copy()
    n_pos, conv = _c(state[2], np.int32).copy(), _c(state[3], np.int64).copy()
    sums = _c(sums, np.float64)
    n = len(dt)
    coef, ret = np.full((n, 3), np.nan, np.float32), np.full(n, -1, np.int32)
    lib().min_control(C.c_int64(n), _p(dt), _p(alpha), _p(n_pos), _p(conv), _p(sums), *_fire_args(p), C.c_int64(step), _p(coef), _p(ret))
    return (dt, alpha, n_pos, conv), coef, ret


def update(batch, conv, fixed, coef, x, v, f):
    """-> (x, v) after the per-atom update"""
    batch, conv, coef = _c(batch, np.int64), _c(conv, np.int64), _c(coef, np.float32)
    fixed = None if fixed is None else _c(fixed, np.uint8)
    x, v, f = _c(x, np.float32).copy(), _c(v, np.float32).copy(), _c(f, np.float32)
    lib().min_update(C.c_int64(len(x)), _p(batch), _p(conv), _p(fixed), _p(coef), _p(x), _p(v), _p(f))
    return x, v


def wells(batch, n_mol, kspring, x0, x, p, max_steps, fixed=None):
    """harmonic wells, fp32 -> steps taken, converged_at [n_mol], final x, final dt [n_mol]"""
    batch, kspring, x0 = _c(batch, np.int64), _c(kspring, np.float32), _c(x0, np.float32)
    fixed = None if fixed is None else _c(fixed, np.uint8)
    x = _c(x, np.float32).copy()
    n = len(x)
    v, f = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    dt, alpha = np.zeros(n_mol), np.zeros(n_mol)
    n_pos, conv = np.zeros(n_mol, np.int32), np.zeros(n_mol, np.int64)
    sums, coef = np.zeros((n_mol, 4)), np.zeros((n_mol, 3), np.float32)
    steps = lib().min_wells(C.c_int64(n_mol), C.c_int64(n), _p(batch), _p(kspring), _p(x0), _p(x), _p(v), _p(f), _p(fixed),
                            C.c_double(p["dt"]), *_fire_args(p), C.c_int64(max_steps), _p(dt), _p(alpha), _p(n_pos), _p(conv), _p(sums),
                            _p(coef))
    return int(steps), conv, x, dt
