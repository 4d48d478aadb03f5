"""TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident minima hopping (torchmd-net_amd/csrc/tn_hop_math.h) on the CPU,
compiled host-only from tests/hop_host.hip into oracle/_build/libhop_host.so and called through ctypes on numpy arrays.  The
statements are the header's own and the sums are added in the device's order; tests/test_hop_host.py compares them with
tests/hop_oracle.py, tests/test_gpu_hop.py with the kernels.  ``HostHop`` has the buffers of ``torchmdnet_amd.hop.DeviceHop`` under
the same names, as numpy arrays, and is stepped with forces and energies the caller computes."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.min_host_mirror import _c, _p
from torchmdnet_amd import _C
from torchmdnet_amd.hop import COEF_LOG, COUNTERS, SUMS_LOG, fill_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "hop_host.hip")
_LIB = None


def sources():
    csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
    return [SOURCE, os.path.join(ROOT, "include", "tmdnet_amd.h")] + [os.path.join(csrc, h) for h in ("tn_hop_math.h", "tn_min_math.h",
                                                                                                      "tn_md_math.h")]


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libhop_host.so")
        src = sources()
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", SOURCE, "-o", so])
        _LIB = C.CDLL(so)
        for name in ("hop_host_destroy", "hop_host_reset", "hop_host_advance", "hop_host_status", "hop_host_pair_sums",
                     "hop_host_launch_solve", "hop_host_noise"):
            getattr(_LIB, name).restype = None
        _LIB.hop_host_create.restype = C.c_void_p
        _LIB.hop_host_rmsd2.restype = C.c_double
    return _LIB


def pair_sums(a, b):
    """the 18 sums of the pair (a, b), [n,3] fp32 each"""
    a, b = _c(a, np.float32), _c(b, np.float32)
    out = np.full(18, np.nan)
    lib().hop_host_pair_sums(C.c_int64(len(a)), _p(a), _p(b), _p(out))
    return out


def rmsd2(sums, align):
    return float(lib().hop_host_rmsd2(_p(_c(sums, np.float64)), C.c_int32(align)))


def rmsd(a, b, align=2):
    return float(np.sqrt(rmsd2(pair_sums(a, b), align)))


def launch_solve(sums, align=2):
    """the 16 sums of a launch -> u [3], omega [3] fp32, singular"""
    u, w, s = np.full(3, np.nan, np.float32), np.full(3, np.nan, np.float32), C.c_int32(-1)
    lib().hop_host_launch_solve(_p(_c(sums, np.float64)), C.c_int32(align), _p(u), _p(w), C.byref(s))
    return u, w, int(s.value)


def noise(seed, hop, n):
    xi = np.full((n, 3), np.nan, np.float32)
    lib().hop_host_noise(C.c_uint64(seed), C.c_uint64(hop), C.c_int64(n), _p(xi))
    return xi


class HostHop:
    """The loop on the CPU.  ``params``: ``torchmdnet_amd.hop.parse_hop``'s dict; ``pos`` [N,3], ``masses`` [N], ``batch`` [N] or None,
    ``fixed`` [N] or None.  ``step(energy [B], forces [N,3])`` is one ``tmdnet_hop_advance``; the logs hold the last step's row."""

    def __init__(self, params, pos, masses, batch=None, fixed=None, force_scale=1.0):
        self.params = params
        self.pos = _c(pos, np.float32).copy()
        N = len(self.pos)
        self.batch = np.zeros(N, np.int64) if batch is None else _c(batch, np.int64)
        B, cap = int(self.batch.max()) + 1, params["capacity"]
        self.n_atoms, self.n_mol = N, B
        m64 = np.array(masses, dtype=np.float64).reshape(-1).copy()
        still = np.isinf(m64)
        if fixed is not None:
            still = still | (np.asarray(fixed).reshape(-1) != 0)
        m64[still] = np.inf
        self.fixed = still.astype(np.uint8) if still.any() else None
        self.masses = m64.astype(np.float32)
        self.hk = (0.5 * params["dt"] * force_scale / m64).astype(np.float32)
        self.sig = np.sqrt(force_scale / m64).astype(np.float32)
        self.vel, self.forces = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
        self.minimum_pos, self.best_pos = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
        self.ring_pos = np.zeros((cap, N, 3), np.float32)
        self.ring_energy = np.zeros((B, cap))
        self.ring_found, self.ring_visits = np.zeros((B, cap), np.int64), np.zeros((B, cap), np.int64)
        self.kT, self.ediff, self.minimum_energy, self.best_energy = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
        self.phase = np.zeros(B, np.int32)
        self.counters = np.zeros((B, COUNTERS), np.int64)
        self.epot, self.fmax, self.ekin = np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)
        self.phase_log, self.outcome = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.sums, self.coef = np.zeros((B, SUMS_LOG)), np.zeros((B, COEF_LOG), np.float32)
        self._energy, self._forces = np.zeros(B, np.float32), np.zeros((N, 3), np.float32)
        self._h = C.c_void_p(lib().hop_host_create(C.c_int64(N), C.c_int64(B), C.c_int32(cap)))
        a = fill_args(_C.HopArgs(), params)
        for name, t in (("pos", self.pos), ("vel", self.vel), ("forces", self._forces), ("energy", self._energy), ("hk", self.hk),
                        ("mass", self.masses), ("sig", self.sig), ("fixed", self.fixed), ("batch", self.batch),
                        ("forces_keep", self.forces), ("cur_pos", self.minimum_pos), ("best_pos", self.best_pos),
                        ("ring_pos", self.ring_pos), ("ring_energy", self.ring_energy), ("ring_found", self.ring_found),
                        ("ring_visits", self.ring_visits), ("kT", self.kT), ("ediff", self.ediff), ("cur_energy", self.minimum_energy),
                        ("best_energy", self.best_energy), ("phase", self.phase), ("counters", self.counters), ("epot_row", self.epot),
                        ("fmax_row", self.fmax), ("ekin_row", self.ekin), ("phase_row", self.phase_log), ("outcome_row", self.outcome),
                        ("sums_row", self.sums), ("coef_row", self.coef)):
            setattr(a, name, None if t is None else t.ctypes.data)
        self._args = a
        self.reset()

    def __del__(self):
        if getattr(self, "_h", None) is not None and _LIB is not None:
            _LIB.hop_host_destroy(self._h)
            self._h = None

    @property
    def n_hops(self):
        return self.counters[:, 0]

    def reset(self, pos=None, kT=None, ediff=None, history="clear"):
        B = self.n_mol
        if pos is not None:
            self.pos[:] = pos
        self.vel[:] = 0
        if history == "clear":
            for t in (self.ring_pos, self.ring_energy, self.ring_found, self.ring_visits, self.best_pos, self.minimum_pos):
                t[...] = 0
        kT0 = np.broadcast_to(np.asarray(self.params["kT0"] if kT is None else kT, np.float64), (B,)).copy()
        e0 = np.broadcast_to(np.asarray(self.params["ediff0"] if ediff is None else ediff, np.float64), (B,)).copy()
        lib().hop_host_reset(self._h, C.byref(self._args), C.c_uint64(0), _p(kT0), _p(e0), C.c_int32(history == "keep"))
        return self

    def step(self, energy, forces, overflowed=False):
        self._energy[:] = energy
        self._forces[:] = forces
        lib().hop_host_advance(self._h, C.byref(self._args), C.c_int32(bool(overflowed)))
        return self

    def status(self):
        """-> (step, status)"""
        out = (C.c_uint64 * 2)()
        lib().hop_host_status(self._h, out)
        return int(out[0]), int(out[1])
