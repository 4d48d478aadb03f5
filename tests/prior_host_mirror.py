"""TEST INFRASTRUCTURE ONLY: the pair arithmetic of the ZBL / D2 priors (torchmd-net_amd/csrc/tn_prior_math.h) on the CPU, compiled
host-only from tests/prior_host.hip into oracle/_build/libprior_host.so and called through ctypes on numpy arrays.  The statements
are the header's own; tests/test_prior_host.py compares them with tests/prior_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torchmd-net_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "prior_host.hip"), os.path.join(CSRC, "tn_prior_math.h")]
_LIB = None


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libprior_host.so")
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SRC):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([_hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", SRC[0], "-o", so])
        _LIB = C.CDLL(so)
        _LIB.prior_zbl.restype = None
        _LIB.prior_d2.restype = None
        _LIB.prior_in_cutoff.restype = C.c_int32
        _LIB.prior_max_molecule_atoms.restype = C.c_int32
    return _LIB


def build_program(path, sanitize=True):
    """The stand-alone program of tests/prior_host.hip (its own main, nothing loaded into Python), with the host sanitizers."""
    cmd = [_hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DPRIOR_HOST_MAIN"]
    if sanitize:
        cmd += ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(cmd + [SRC[0], "-o", path])
    return path


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _pair(fn, r, a, b, c, d, cutoff, distance_scale, energy_scale):
    r = np.ascontiguousarray(r, dtype=np.float32)
    u, du = np.empty_like(r), np.empty_like(r)
    fn(C.c_int64(len(r)), _p(r), C.c_float(a), C.c_float(b), C.c_float(c), C.c_float(d), C.c_double(cutoff), C.c_double(distance_scale),
       C.c_double(energy_scale), _p(u), _p(du))
    return u, du


def zbl(r, Zi, Zj, cutoff, distance_scale, energy_scale):
    """-> (u, du/dr) fp32 at the fp32 distances r; the species values are tabulated in fp64 and rounded, as the model stages them"""
    f = lambda v: float(np.float32(v))
    return _pair(lib().prior_zbl, r, f(float(Zi) ** 0.23), f(float(Zj) ** 0.23), f(Zi), f(Zj), cutoff, distance_scale, energy_scale)


def d2(r, C6i, C6j, Rri, Rrj, cutoff, distance_scale, energy_scale):
    f = lambda v: float(np.float32(v))
    return _pair(lib().prior_d2, r, f(np.sqrt(C6i)), f(np.sqrt(C6j)), f(Rri), f(Rrj), cutoff, distance_scale, energy_scale)


def in_cutoff(d2_, cutoff):
    return bool(lib().prior_in_cutoff(C.c_float(d2_), C.c_float(cutoff)))


def max_molecule_atoms():
    return int(lib().prior_max_molecule_atoms())
