"""TEST INFRASTRUCTURE ONLY: the committee reduction (torchmd-net_amd/csrc/tn_committee_math.h) on the CPU, compiled host-only from
tests/committee_host.hip into oracle/_build/libcommittee_host.so and called through ctypes on numpy arrays.  The statements are the
header's own; tests/test_committee_host.py compares them with tests/committee_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torchmd-net_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "committee_host.hip"), os.path.join(CSRC, "tn_committee_math.h")]
_LIB = None


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libcommittee_host.so")
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in SRC):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([_hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", SRC[0], "-o", so])
        _LIB = C.CDLL(so)
        for name in ("committee_reduce", "committee_gate_fires", "committee_max_members"):
            getattr(_LIB, name).restype = C.c_int32
    return _LIB


def build_program(path, sanitize=True):
    """The stand-alone program of tests/committee_host.hip (its own main, nothing loaded into Python), with the host sanitizers."""
    cmd = [_hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DCOMMITTEE_HOST_MAIN"]
    if sanitize:
        cmd += ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call(cmd + [SRC[0], "-o", path])
    return path


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def reduce(E, F, batch, B):
    """E [M,B], F [M,N,3] fp32, batch [N] int64 or None -> dict of the seven outputs (numpy); None when M is refused"""
    E = np.ascontiguousarray(E, dtype=np.float32).reshape(len(E), -1)
    F = np.ascontiguousarray(F, dtype=np.float32)
    M, N = F.shape[0], F.shape[1]
    batch = None if batch is None else np.ascontiguousarray(batch, dtype=np.int64)
    out = dict(energy=np.zeros(B, np.float32), forces=np.zeros((N, 3), np.float32), energy_std=np.zeros(B, np.float32),
               forces_std=np.zeros((N, 3), np.float32), deviation=np.zeros(N, np.float32), max_deviation=np.zeros(B, np.float32),
               max_atom=np.zeros(B, np.int64))
    rc = lib().committee_reduce(C.c_int32(M), _p(E), _p(F), C.c_int64(N), C.c_int64(B), _p(batch), *[_p(out[k]) for k in (
        "energy", "forces", "energy_std", "forces_std", "deviation", "max_deviation", "max_atom")])
    return None if rc else out


def gate_fires(D, threshold):
    return bool(lib().committee_gate_fires(C.c_float(D), C.c_float(threshold)))


def max_members():
    return int(lib().committee_max_members())
