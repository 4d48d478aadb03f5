"""TEST INFRASTRUCTURE ONLY: the constraint arithmetic of the device-resident MD loop (torchmd-net_amd/csrc/tn_md_cons_math.h) on
the CPU, compiled host-only from tests/md_cons_host.hip into oracle/_build/libmd_cons_host.so and called through ctypes on numpy
arrays.  ``advance`` is one launch of k_md_clusters of csrc/tn_md_cons.hip, cluster by cluster; tests/test_md_constraints_host.py
compares it with tests/md_cons_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "md_cons_host.hip"), os.path.join(ROOT, "torchmd-net_amd", "csrc", "tn_md_cons_math.h"),
       os.path.join(ROOT, "torchmd-net_amd", "csrc", "tn_md_math.h")]
FAIL_SHAKE, FAIL_RATTLE = 1, 2
# Agreement of the header (Gauss-Seidel to tol = 1e-6, results rounded to fp32) with the Newton oracle of tests/md_cons_oracle.py:
# the largest difference over the six cases of tests/test_md_constraints_host.py as measured on the host is 7.8e-07 for the
# positions and 5.8e-07 for the velocities (positions and half-step velocities in units of max(1, max|x|), projected velocities
# absolute).  Asserted, there and on the GPU: ten times that; the margin covers compilers that contract the fp64 products
# differently on the host and on the device.
ORACLE_X, ORACLE_V = 7.8e-06, 5.8e-06
_LIB = None


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libmd_cons_host.so")
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SRC):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([_hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", SRC[0], "-o", so])
        _LIB = C.CDLL(so)
        _LIB.md_cons_advance.restype = C.c_uint32
    return _LIB


def build_program(path, sanitize=True):
    """The stand-alone program of tests/md_cons_host.hip (its own main, nothing loaded into Python), with the host sanitizers."""
    cmd = [_hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DMD_CONS_HOST_MAIN"]
    if sanitize:
        cmd += ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(cmd + [SRC[0], "-o", path])
    return path


def _p(a):
    return C.c_void_p(0) if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def advance(close, open_, tables, pos, vel, forces, hk, mass, dt, sigma=None, c1=1.0, c2=0.0, seed=0, step=0, tol=1e-6, max_iter=64,
            x_keep=None, v_keep=None):
    """One launch (close, open_) = (0,1) OPEN, (1,1) MIDDLE, (1,0) CLOSE, (0,0) the projection alone.  ``tables``: the dict of
    ``torchmdnet_amd.md.build_clusters`` plus ``constraint_d2``.  -> dict(pos, vel, x_keep, v_keep, part, fail), all copies."""
    n = len(pos)
    atoms, off = _c(tables["cluster_atoms"], np.int32), _c(tables["cluster_offsets"], np.int32)
    ends, d2 = _c(tables["constraint_ends"], np.int32), _c(tables["constraint_d2"], np.float64)
    pos, vel = _c(pos, np.float32).copy(), _c(vel, np.float32).copy()
    forces = _c(np.zeros((n, 3)) if forces is None else forces, np.float32)
    hk, mass = _c(np.zeros(n) if hk is None else hk, np.float32), _c(mass, np.float32)
    sigma = None if sigma is None else _c(sigma, np.float32)
    x_keep = np.zeros((n, 3), np.float32) if x_keep is None else _c(x_keep, np.float32).copy()
    v_keep = np.zeros((n, 3), np.float32) if v_keep is None else _c(v_keep, np.float32).copy()
    part = np.full(n, np.nan, np.float32)
    fail = lib().md_cons_advance(C.c_int(int(close)), C.c_int(int(open_)), C.c_int64(n), C.c_int64(len(atoms)), _p(atoms), _p(off), _p(ends),
                                 _p(d2), _p(pos), _p(vel), _p(forces), _p(hk), _p(mass), _p(sigma), C.c_float(dt), C.c_float(c1),
                                 C.c_float(c2), C.c_uint64(seed), C.c_uint64(step), C.c_double(tol), C.c_int(max_iter), _p(x_keep),
                                 _p(v_keep), _p(part))
    return dict(pos=pos, vel=vel, x_keep=x_keep, v_keep=v_keep, part=part, fail=int(fail))
