"""TEST INFRASTRUCTURE ONLY: the per-atom arithmetic of the device-resident MD loop (torchmd-net_amd/csrc/tn_md_math.h) on the CPU,
compiled host-only from tests/md_host.hip into oracle/_build/libmd_host.so and called through ctypes on numpy arrays.  The
statements are the header's own; tests/test_md_host.py compares them with tests/md_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libmd_host.so")
        src = [os.path.join(ROOT, "tests", "md_host.hip"), os.path.join(ROOT, "torchmd-net_amd", "csrc", "tn_md_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", src[0], "-o", so])
        _LIB = C.CDLL(so)
        for name in ("md_philox", "md_uniform", "md_normals", "md_noise", "md_close", "md_open"):
            getattr(_LIB, name).restype = None
    return _LIB


def _p(a):
    return C.c_void_p(0) if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def philox(counters, keys):
    """counters [n,4], keys [n,2] uint32 -> [n,4] uint32"""
    counters, keys = _c(counters, np.uint32), _c(keys, np.uint32)
    out = np.zeros_like(counters)
    lib().md_philox(C.c_int64(len(counters)), _p(counters), _p(keys), _p(out))
    return out


def uniform(words):
    words = _c(words, np.uint32)
    out = np.full(words.shape, np.nan, np.float32)
    lib().md_uniform(C.c_int64(words.size), _p(words), _p(out))
    return out


def normals(words):
    """words [n,4] uint32 -> xi [n,3] fp32"""
    words = _c(words, np.uint32)
    out = np.full((len(words), 3), np.nan, np.float32)
    lib().md_normals(C.c_int64(len(words)), _p(words), _p(out))
    return out


def noise(seed, step, atoms):
    atoms = _c(atoms, np.uint32)
    out = np.full((len(atoms), 3), np.nan, np.float32)
    lib().md_noise(C.c_int64(len(atoms)), C.c_uint64(seed), C.c_uint64(step), _p(atoms), _p(out))
    return out


def close_step(v, f, hk, mass, sigma=None, c1=1.0, c2=0.0, seed=0, step=0):
    """-> (v after B [, O], ke per atom)"""
    v, f, hk, mass = _c(v, np.float32).copy(), _c(f, np.float32), _c(hk, np.float32), _c(mass, np.float32)
    sigma = None if sigma is None else _c(sigma, np.float32)
    ke = np.full(len(v), np.nan, np.float32)
    lib().md_close(C.c_int64(len(v)), _p(v), _p(f), _p(hk), _p(mass), _p(sigma), C.c_float(c1), C.c_float(c2), C.c_uint64(seed),
                   C.c_uint64(step), _p(ke))
    return v, ke


def open_step(x, v, f, hk, dt):
    """-> (x, v) after B, A"""
    x, v, f, hk = _c(x, np.float32).copy(), _c(v, np.float32).copy(), _c(f, np.float32), _c(hk, np.float32)
    lib().md_open(C.c_int64(len(x)), _p(x), _p(v), _p(f), _p(hk), C.c_float(dt))
    return x, v
