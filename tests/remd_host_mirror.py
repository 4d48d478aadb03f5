"""TEST INFRASTRUCTURE ONLY: the replica-exchange arithmetic of the device-resident MD loop (torchmd-net_amd/csrc/tn_remd_math.h) on
the CPU, compiled host-only from tests/remd_host.hip into oracle/_build/libremd_host.so and called through ctypes on numpy arrays.
The statements are the header's own; tests/test_remd_host.py compares them with tests/remd_oracle.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libremd_host.so")
        csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
        src = [os.path.join(ROOT, "tests", "remd_host.hip"), os.path.join(csrc, "tn_remd_math.h"), os.path.join(csrc, "tn_md_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", src[0], "-o", so])
        _LIB = C.CDLL(so)
        for name in ("remd_uniform", "remd_decide", "remd_attempt", "remd_atoms", "remd_harmonic"):
            getattr(_LIB, name).restype = None
        _LIB.remd_pairs.restype = C.c_int32
    return _LIB


def _p(a):
    return C.c_void_p(0) if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def uniform(seed, step, index):
    index = _c(index, np.uint32)
    out = np.full(len(index), np.nan, np.float32)
    lib().remd_uniform(C.c_int64(len(index)), C.c_uint64(seed), C.c_uint64(step), _p(index), _p(out))
    return out


def decide(beta_lo, beta_hi, E_i, E_j, u):
    """elementwise decisions -> int32"""
    E_i = _c(E_i, np.float32)
    n = len(E_i)
    b = lambda a, t: _c(np.broadcast_to(np.asarray(a, t), (n,)), t)
    out = np.full(n, -1, np.int32)
    lib().remd_decide(C.c_int64(n), _p(b(beta_lo, np.float64)), _p(b(beta_hi, np.float64)), _p(E_i), _p(b(E_j, np.float32)),
                      _p(b(u, np.float32)), _p(out))
    return out


def pairs(a, R):
    out = np.full(max(R, 1), -1, np.int32)
    n = lib().remd_pairs(C.c_uint64(a), C.c_int32(R), _p(out))
    return out[:n].tolist()


def tables(kT, mass, force_scale=1.0):
    """what the caller stages for a ladder: beta [R] fp64, sigma_table [R,n], up, down [R-1] fp32 (fp64, rounded once)"""
    kT, m = np.asarray(kT, np.float64), np.asarray(mass, np.float64)
    table = np.sqrt(kT[:, None] * force_scale / m[None, :]).astype(np.float32)
    up = np.array([math.sqrt(kT[s + 1] / kT[s]) for s in range(len(kT) - 1)], np.float64).astype(np.float32)
    down = np.array([math.sqrt(kT[s] / kT[s + 1]) for s in range(len(kT) - 1)], np.float64).astype(np.float32)
    return 1.0 / kT, table, up, down


class Ladders:
    """The device state of G ladders of R slots and the decision launch on it."""

    def __init__(self, G, R, beta, every, seed):
        self.G, self.R, self.every, self.seed = G, R, every, seed
        self.beta = _c(beta, np.float64)
        self.slot = np.tile(np.arange(R, dtype=np.int32), G)
        self.holder = np.tile(np.arange(R, dtype=np.int32), (G, 1))
        self.accept = np.full((G, R - 1), 255, np.uint8)  # scratch: every entry is rewritten by every attempt
        self.counters = np.zeros((2, G, R - 1), np.int64)

    def attempt(self, step, epot):
        """after `step` completed steps, on the energies epot [G R] -> (slot_log [G R], accept_log [G,R-1])"""
        epot = _c(epot, np.float32)
        slot_log = np.full(self.G * self.R, -1, np.int32)
        accept_log = np.full((self.G, self.R - 1), 255, np.uint8)
        lib().remd_attempt(C.c_int32(self.G), C.c_int32(self.R), C.c_uint64(self.every), C.c_uint64(self.seed), C.c_uint64(step),
                           _p(self.beta), _p(epot), _p(self.slot), _p(self.holder), _p(self.accept), _p(slot_log), _p(accept_log),
                           _p(self.counters))
        return slot_log, accept_log

    def atoms(self, step, vel, sigma, table, up, down):
        """the per-atom launch that follows attempt(step, ...): -> (vel, sigma)"""
        vel, sigma = _c(vel, np.float32).copy(), _c(sigma, np.float32).copy()
        table = _c(table, np.float32)
        lib().remd_atoms(C.c_int32(self.G), C.c_int32(self.R), C.c_int32(table.shape[1]), C.c_uint64(self.every), C.c_uint64(step), _p(vel),
                         _p(sigma), _p(self.slot), _p(self.accept), _p(table), _p(_c(up, np.float32)), _p(_c(down, np.float32)))
        return vel, sigma


def harmonic(G, R, n, attempts, every, x, v, mass, kT, dt, friction, seed, k=1.0):
    """The protocol of remd_harmonic (tests/remd_host.hip), force_scale 1 -> dict of epot, ekin [attempts, G R], slot_log
    [attempts, G R], accept_log [attempts, G, R-1], counters [2, G, R-1]"""
    B = G * R
    x, v = _c(x, np.float32).copy(), _c(v, np.float32).copy()
    m1 = np.asarray(mass, np.float64)
    mass_all = np.tile(m1, B)
    beta, table, up, down = tables(kT, m1)
    lad = Ladders(G, R, beta, every, seed)
    sigma = _c(table[lad.slot].reshape(-1), np.float32)
    hk = (0.5 * dt / mass_all).astype(np.float32)
    c1 = math.exp(-friction * dt)
    c2 = math.sqrt(1.0 - c1 * c1)
    epot, ekin = np.full((attempts, B), np.nan, np.float32), np.full((attempts, B), np.nan, np.float32)
    slot_log = np.full((attempts, B), -1, np.int32)
    accept_log = np.full((attempts, G, R - 1), 255, np.uint8)
    lib().remd_harmonic(C.c_int32(G), C.c_int32(R), C.c_int32(n), C.c_int64(attempts), C.c_uint64(every), _p(x), _p(v), _p(hk),
                        _p(mass_all.astype(np.float32)), _p(sigma), C.c_float(dt), C.c_float(c1), C.c_float(c2), C.c_uint64(seed), C.c_float(k),
                        _p(beta), _p(table), _p(up), _p(down), _p(lad.slot), _p(lad.holder), _p(epot), _p(ekin), _p(slot_log), _p(accept_log),
                        _p(lad.counters), _p(lad.accept))
    return dict(epot=epot, ekin=ekin, slot_log=slot_log, accept_log=accept_log, counters=lad.counters, x=x, v=v, sigma=sigma,
                slot=lad.slot, holder=lad.holder)
