"""TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident L-BFGS minimiser (torchmd-net_amd/csrc/tn_lbfgs_math.h) on the CPU,
compiled host-only from tests/lbfgs_host.hip into oracle/_build/liblbfgs_host.so and called through ctypes on numpy arrays.
The statements are the header's own; tests/test_lbfgs_host.py compares them with tests/lbfgs_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "lbfgs_host.hip")
_LIB = None


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "liblbfgs_host.so")
        csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
        src = [SOURCE, os.path.join(csrc, "tn_lbfgs_math.h"), os.path.join(csrc, "tn_md_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", SOURCE, "-o", so])
        _LIB = C.CDLL(so)
        for name in ("lb_init", "lb_candidate", "lb_sums", "lb_control", "lb_direction", "lb_move"):
            getattr(_LIB, name).restype = None
        _LIB.lb_wells.restype = C.c_int64
    return _LIB


def _p(a):
    return C.c_void_p(0) if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _par(p):
    """the parameters of tests/lbfgs_oracle.py's dict in the order of the C entries (memory ... fmax)"""
    return C.c_int32(p["memory"]), C.c_double(p["alpha"]), C.c_double(p["max_step"]), C.c_double(p["damping"]), C.c_double(p["fmax"])


def candidate(x, x_prev, f, f_prev, fixed=None):
    """-> s, y [n,3] fp32"""
    x, x_prev, f, f_prev = (_c(a, np.float32) for a in (x, x_prev, f, f_prev))
    fixed = None if fixed is None else _c(fixed, np.uint8)
    s, y = np.full_like(x, np.nan), np.full_like(x, np.nan)
    lib().lb_candidate(C.c_int64(len(x)), _p(x), _p(x_prev), _p(f), _p(f_prev), _p(fixed), _p(s), _p(y))
    return s, y


class State:
    """The workspace of the device entries as numpy arrays, and its launches as methods"""

    def __init__(self, batch, n_mol, p, fixed=None):
        self.batch, self.n_mol, self.p = _c(batch, np.int64), int(n_mol), p
        self.n = len(self.batch)
        self.fixed = None if fixed is None else _c(fixed, np.uint8)
        B, M1 = self.n_mol, p["memory"] + 1
        self.M1, self.NP = M1, 6 * M1 + 4
        self.h, self.order, self.conv = np.zeros(B, np.int32), np.zeros((B, M1), np.int32), np.zeros(B, np.int64)
        self.SS, self.SY, self.YY = (np.zeros((B, M1, M1)) for _ in range(3))
        self.tot, self.delta = np.zeros((B, self.NP)), np.zeros((B, 2 * M1 + 1))
        self.S, self.Y = np.zeros((M1, self.n, 3), np.float32), np.zeros((M1, self.n, 3), np.float32)
        self.x_prev, self.f_prev = np.zeros((self.n, 3), np.float32), np.zeros((self.n, 3), np.float32)
        self.direction, self.longest2 = np.zeros((self.n, 3), np.float32), np.zeros(B)
        self.accepted, self.gp, self.ret = np.zeros(B, np.int32), np.zeros(B), np.zeros(B, np.int32)
        self.scale = np.zeros(B, np.float32)
        self.fresh = 1
        lib().lb_init(C.c_int64(B), C.c_int32(p["memory"]), _p(self.h), _p(self.order), _p(self.conv))

    def sums(self, x, f):
        """the candidate into the spare slot and every sum, from the positions and forces after a move -> tot"""
        x, f = _c(x, np.float32), _c(f, np.float32)
        lib().lb_sums(C.c_int64(self.n_mol), C.c_int64(self.n), _p(self.batch), C.c_int32(self.p["memory"]), C.c_int32(self.fresh),
                      _p(self.h), _p(self.order), _p(self.conv), _p(x), _p(self.x_prev), _p(f), _p(self.f_prev), _p(self.fixed),
                      _p(self.S), _p(self.Y), _p(self.tot))
        return self.tot

    def control(self, step, tot=None):
        """the controller of every molecule on self.tot (or `tot`) -> ret [n_mol]"""
        if tot is not None:
            self.tot = _c(tot, np.float64).reshape(self.n_mol, self.NP).copy()
        lib().lb_control(C.c_int64(self.n_mol), *_par(self.p), C.c_int32(self.fresh), C.c_int64(step), _p(self.h), _p(self.order),
                         _p(self.conv), _p(self.SS), _p(self.SY), _p(self.YY), _p(self.tot), _p(self.delta), _p(self.accepted),
                         _p(self.gp), _p(self.ret))
        if not (self.ret == 2).any():
            self.fresh = 0
        return self.ret

    def direct(self, f):
        """-> direction [n,3] fp32 of the move prepared, longest2 [n_mol]"""
        f = _c(f, np.float32)
        lib().lb_direction(C.c_int64(self.n_mol), C.c_int64(self.n), _p(self.batch), C.c_int32(self.p["memory"]), _p(self.h),
                           _p(self.order), _p(self.conv), _p(self.delta), _p(f), _p(self.fixed), _p(self.S), _p(self.Y), _p(self.direction),
                           _p(self.longest2))
        return self.direction, self.longest2

    def move(self, x, f):
        """-> the new x; x_prev, f_prev and scale are kept"""
        x, f = _c(x, np.float32).copy(), _c(f, np.float32)
        lib().lb_move(C.c_int64(self.n_mol), C.c_int64(self.n), _p(self.batch), _p(self.conv), _p(self.fixed), _p(self.longest2),
                      C.c_double(self.p["max_step"]), C.c_double(self.p["damping"]), _p(x), _p(self.direction), _p(f), _p(self.x_prev),
                      _p(self.f_prev), _p(self.scale))
        return x

    def pairs(self, m):
        """the pairs molecule m holds, oldest first, as flat float64 arrays over ITS atoms -> (S list, Y list)"""
        mine = self.batch == m
        slots = self.order[m, :self.h[m]]
        return [self.S[a][mine].astype(np.float64).ravel() for a in slots], [self.Y[a][mine].astype(np.float64).ravel() for a in slots]


def wells(batch, n_mol, kspring, x0, x, p, max_steps, fixed=None, anharmonic=0.0):
    """spring wells, fp32 -> steps taken, converged_at [n_mol], final x, h_log and acc_log [steps + 1, n_mol]"""
    batch, kspring, x0 = _c(batch, np.int64), _c(kspring, np.float32), _c(x0, np.float32)
    fixed = None if fixed is None else _c(fixed, np.uint8)
    x = _c(x, np.float32).copy()
    conv = np.zeros(n_mol, np.int64)
    h_log, acc_log = np.zeros((max_steps + 1, n_mol), np.int32), np.zeros((max_steps + 1, n_mol), np.int32)
    steps = lib().lb_wells(C.c_int64(n_mol), C.c_int64(len(x)), _p(batch), _p(kspring), _p(x0), _p(x), _p(fixed), C.c_float(anharmonic),
                           *_par(p), C.c_int64(max_steps), _p(conv), _p(h_log), _p(acc_log))
    steps = int(steps)
    return steps, conv, x, h_log[:max(steps, 0) + 1], acc_log[:max(steps, 0) + 1]
