"""TEST INFRASTRUCTURE ONLY: the arithmetic of the Hessian assembly and normal-mode preparation (torchmd-net_amd/csrc/tn_vib_math.h)
on the CPU, compiled host-only from tests/vib_host.hip into oracle/_build/libvib_host.so and called through ctypes on numpy arrays.
The statements are the header's own; tests/test_vib_host.py compares them with tests/vib_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.min_host_mirror import _c, _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "vib_host.hip")
SEED, PLUS, MINUS = 0, 1, 2
ANALYTIC, CENTRAL = 0, 1
_LIB = None


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libvib_host.so")
        csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
        src = [SOURCE] + [os.path.join(csrc, h) for h in ("tn_vib_math.h", "tn_md_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", SOURCE, "-o", so])
        _LIB = C.CDLL(so)
        for name in ("vib_seed", "vib_gather", "vib_finish"):
            getattr(_LIB, name).restype = None
    return _LIB


def _i64(a):
    return _c(a, np.int64)


def seed(mode, pos, batch, free_idx, fstart, R, col0, delta=0.0):
    """-> [R N, 3] fp32: the seed vector (SEED) or the displaced replicated positions (PLUS / MINUS)"""
    batch, free_idx, fstart = _i64(batch), _i64(free_idx), _i64(fstart)
    N, B = batch.shape[0], fstart.shape[0] - 1
    pos = None if pos is None else _c(pos, np.float32)
    out = np.full((R * N, 3), np.nan, np.float32)
    lib().vib_seed(C.c_int32(mode), C.c_int64(N), C.c_int64(B), C.c_int64(R), C.c_int64(col0), _p(pos), _p(batch), _p(free_idx), _p(fstart),
                   C.c_float(delta), _p(out))
    return out


def gather(mode, H, batch, free_idx, fstart, R, col0, a, f_minus=None, x_plus=None, x_minus=None, writes=None):
    """one pass into H [B, D, D] fp32 in place (and the write counts [B, D, D] int32 when given)"""
    batch, free_idx, fstart = _i64(batch), _i64(free_idx), _i64(fstart)
    assert H.dtype == np.float32 and H.flags.c_contiguous and (writes is None or (writes.dtype == np.int32 and writes.flags.c_contiguous))
    N, B, D = batch.shape[0], fstart.shape[0] - 1, H.shape[1]
    args = [None if t is None else _c(t, np.float32) for t in (a, f_minus, x_plus, x_minus)]
    lib().vib_gather(C.c_int32(mode), C.c_int64(N), C.c_int64(B), C.c_int64(free_idx.shape[0]), C.c_int64(D), C.c_int64(R), C.c_int64(col0),
                     _p(batch), _p(free_idx), _p(fstart), *[_p(t) for t in args], _p(H), _p(writes))
    return H


def finish(H, pos, mass, free_idx, fstart, project, mol_atoms=None):
    """H [B, D, D] fp32 -> A [B, D, D] fp64, info [B, 8] fp64"""
    H, pos, mass = _c(H, np.float32), _c(pos, np.float32), _c(mass, np.float32)
    free_idx, fstart = _i64(free_idx), _i64(fstart)
    mol_atoms = None if mol_atoms is None else _i64(mol_atoms)
    B, D = H.shape[0], H.shape[1]
    ws = np.full(B * (12 * D + 36), np.nan)
    A, info = np.full((B, D, D), np.nan), np.full((B, 8), np.nan)
    lib().vib_finish(C.c_int64(B), C.c_int64(D), C.c_int32(project), _p(H), _p(pos), _p(mass), _p(free_idx), _p(fstart), _p(mol_atoms), _p(ws),
                     _p(A), _p(info))
    return A, info
