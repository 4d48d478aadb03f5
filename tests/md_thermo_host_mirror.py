"""TEST INFRASTRUCTURE ONLY: the global-thermostat arithmetic of the device-resident MD loop
(torchmd-net_amd/csrc/tn_md_thermo_math.h) on the CPU, compiled host-only from tests/md_thermo_host.hip into
oracle/_build/libmd_thermo_host.so and called through ctypes on numpy arrays.  The statements are the header's own;
tests/test_md_thermo_host.py compares them with tests/md_thermo_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torchmd-net_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "md_thermo_host.hip"), os.path.join(CSRC, "tn_md_thermo_math.h"), os.path.join(CSRC, "tn_md_math.h")]
CSVR, NHC, NONE = 0, 1, -1
_LIB = None


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libmd_thermo_host.so")
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SRC):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([_hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", SRC[0], "-o", so])
        _LIB = C.CDLL(so)
        _LIB.thermo_words.restype = None
        _LIB.thermo_scale.restype = None
        _LIB.thermo_moves.restype = C.c_int32
        _LIB.thermo_run.restype = C.c_int64
    return _LIB


def build_program(path, sanitize=True):
    """The stand-alone program of tests/md_thermo_host.hip (its own main, nothing loaded into Python), with the host sanitizers."""
    cmd = [_hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DMD_THERMO_HOST_MAIN"]
    if sanitize:
        cmd += ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(cmd + [SRC[0], "-o", path])
    return path


def _p(a):
    return C.c_void_p(0) if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def words(seed, step, mol, draw):
    out = np.zeros(4, np.uint32)
    lib().thermo_words(C.c_uint64(seed), C.c_uint64(step), C.c_uint32(mol), C.c_uint32(draw), _p(out))
    return tuple(int(w) for w in out)


def moves(kind, ekin, ndof, kT, tau, dt, seed=0, step=0, M=0, substeps=1, chain=None, reservoir=None, force_scale=1.0, mols=None):
    """One launch of the factor kernel on n molecules -> (flag of the block, alpha fp32 [n], chain [n,2,M], reservoir [n], flags [n]);
    alpha is NaN-filled and chain / reservoir are the inputs' copies, untouched, when the block's flag is set.  ``dt`` is rounded to
    fp32 first, as the C entry takes it."""
    ekin, ndof = _c(ekin, np.float32), _c(ndof, np.int32)
    n = len(ekin)
    mols = _c(np.arange(n) if mols is None else mols, np.uint32)
    chain = np.zeros((n, 2, M)) if chain is None else _c(chain, np.float64).copy()
    reservoir = np.zeros(n) if reservoir is None else _c(reservoir, np.float64).copy()
    assert chain.shape == (n, 2, M) and reservoir.shape == (n,) and ndof.shape == (n,) and mols.shape == (n,)
    alpha = np.full(n, np.nan, np.float32)
    flag = np.full(n, -1, np.int32)
    bad = lib().thermo_moves(C.c_int32(kind), C.c_int64(n), _p(mols), _p(ekin), _p(ndof), C.c_double(force_scale), C.c_double(kT),
                             C.c_double(tau), C.c_double(float(np.float32(dt))), C.c_int32(M), C.c_int32(substeps), C.c_uint64(seed),
                             C.c_uint64(step), _p(chain), _p(reservoir), _p(alpha), _p(flag))
    return int(bad), alpha, chain, reservoir, flag


def scale(batch, alpha, hk, v):
    """-> v scaled by alpha of the atom's molecule (atoms with hk = 0 keep their bits)"""
    batch, alpha, hk, v = _c(batch, np.int64), _c(alpha, np.float32), _c(hk, np.float32), _c(v, np.float32).copy()
    lib().thermo_scale(C.c_int64(len(v)), _p(batch), _p(alpha), _p(hk), _p(v))
    return v


def run(kind, x, v, hk, mass, ndof, dt, kappa, kT, tau, steps, seed=0, M=0, substeps=1, force_scale=1.0, step0=0, chain=None):
    """R molecules (len(ndof)) of n atoms each, harmonic atoms (kappa = 0: free), `steps` steps -> dict of x, v, chain, reservoir and
    the logs epot, ekin, scale, reservoir_log [steps, R]"""
    x, v = _c(x, np.float32).copy(), _c(v, np.float32).copy()
    hk, mass, ndof = _c(hk, np.float32), _c(mass, np.float32), _c(ndof, np.int32)
    R = len(ndof)
    n = len(x) // R
    assert R * n == len(x) == len(v) == len(hk) == len(mass)
    chain = np.zeros((R, 2, M)) if chain is None else _c(chain, np.float64).copy()
    res = np.zeros(R)
    epot, rlog = np.full((steps, R), np.nan), np.full((steps, R), np.nan)
    ekin, sc = np.full((steps, R), np.nan, np.float32), np.full((steps, R), np.nan, np.float32)
    bad = lib().thermo_run(C.c_int32(kind), C.c_int64(R), C.c_int64(n), C.c_int64(steps), C.c_uint64(step0), _p(x), _p(v), _p(hk), _p(mass),
                           _p(ndof), C.c_float(dt), C.c_float(kappa), C.c_double(force_scale), C.c_double(kT), C.c_double(tau), C.c_int32(M),
                           C.c_int32(substeps), C.c_uint64(seed), _p(chain), _p(res), _p(epot), _p(ekin), _p(sc), _p(rlog))
    assert bad == 0, bad
    return dict(x=x, v=v, chain=chain, reservoir=res, epot=epot, ekin=ekin, scale=sc, reservoir_log=rlog)
