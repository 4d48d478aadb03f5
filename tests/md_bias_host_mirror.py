"""TEST INFRASTRUCTURE ONLY: the collective-variable bias of the device-resident MD loop (torchmd-net_amd/csrc/tn_bias_math.h) on the
CPU, compiled host-only from tests/md_bias_host.hip into oracle/_build/libmd_bias_host.so and called through ctypes on numpy arrays.
The statements are the header's own; tests/test_md_bias_host.py compares them with tests/md_bias_oracle.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "md_bias_host.hip")
_LIB = None


def _sources():
    csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
    return [SRC, os.path.join(csrc, "tn_bias_math.h"), os.path.join(csrc, "tn_md_math.h")]


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libmd_bias_host.so")
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in _sources()):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-fPIC", "-shared", SRC, "-o", so])
        _LIB = C.CDLL(so)
        for name in ("bias_cv", "bias_diff", "bias_restraint", "bias_launch", "bias_sample"):
            getattr(_LIB, name).restype = None
        _LIB.bias_visible.restype = C.c_int64
        _LIB.bias_slot.restype = C.c_int64
        _LIB.bias_height.restype = C.c_double
    return _LIB


def build_program(out, sanitize=True):
    """the stand-alone program of tests/md_bias_host.hip (its own main), a host build; -> the command that built it"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DMD_BIAS_HOST_MAIN"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd += [SRC, "-o", out]
    subprocess.check_call(cmd)
    return cmd


def _p(a):
    return C.c_void_p(0) if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


KIND = {"distance": 0, "angle": 1, "torsion": 2}
RESTRAINT = {None: 0, "harmonic": 1, "upper": 2, "lower": 3}


def cv(kind, x):
    """kind [n] (names or ints), x [n,4,3] (unused slots ignored) -> s [n] fp64, g [n,4,3] fp64"""
    kind = _c([KIND.get(k, k) for k in kind], np.int32)
    x = _c(x, np.float32).reshape(len(kind), 4, 3)
    s, g = np.full(len(kind), np.nan), np.full((len(kind), 4, 3), np.nan)
    lib().bias_cv(C.c_int64(len(kind)), _p(kind), _p(x), _p(s), _p(g))
    return s, g


def diff(kind, a, b):
    a = _c(np.atleast_1d(a), np.float64)
    b = _c(np.broadcast_to(np.asarray(b, np.float64), a.shape), np.float64)
    out = np.full(a.shape, np.nan)
    lib().bias_diff(C.c_int64(a.size), C.c_int32(KIND.get(kind, kind)), _p(a), _p(b), _p(out))
    return out


def restraint(kind, kappa, delta):
    delta = _c(np.atleast_1d(delta), np.float64)
    n = delta.size
    kind = _c(np.broadcast_to(np.asarray([RESTRAINT.get(k, k) for k in np.atleast_1d(kind)], np.int32), (n,)), np.int32)
    kappa = _c(np.broadcast_to(np.asarray(kappa, np.float64), (n,)), np.float64)
    V, dV = np.full(n, np.nan), np.full(n, np.nan)
    lib().bias_restraint(C.c_int64(n), _p(kind), _p(kappa), _p(delta), _p(V), _p(dV))
    return V, dV


def visible(n, step0, pace, W, base, H):
    return int(lib().bias_visible(C.c_uint64(n), C.c_uint64(step0), C.c_uint64(pace), C.c_int32(W), C.c_uint64(base), C.c_int64(H)))


def slot(n, step0, pace, W, w, base, H):
    return int(lib().bias_slot(C.c_uint64(n), C.c_uint64(step0), C.c_uint64(pace), C.c_int32(W), C.c_int32(w), C.c_uint64(base), C.c_int64(H)))


def height(h0, V, kT, gamma):
    return float(lib().bias_height(C.c_double(h0), C.c_double(V), C.c_double(kT), C.c_double(gamma or 0.0)))


def tables(cvs):
    """cvs = [(kind, i, j, ...)] -> kinds [D], atoms [D,4], distinct [A], offsets [A+1], entries [32]: what the caller of
    tmdnet_md_bias stages (distinct atoms ascending, entries in CV order then slot order)"""
    kinds = [KIND[c[0]] for c in cvs]
    atoms = [list(c[1:]) + [-1] * (5 - len(c)) for c in cvs]
    distinct = sorted({i for row in atoms for i in row if i >= 0})
    offsets, entries = [0], []
    for a in distinct:
        entries += [(c << 2) | s for c, row in enumerate(atoms) for s, i in enumerate(row) if i == a]
        offsets.append(len(entries))
    return (_c(kinds, np.int32), _c(atoms, np.int32), _c(distinct, np.int32), _c(offsets, np.int32),
            _c(entries + [0] * (32 - len(entries)), np.int32))


class Walkers:
    """The state tmdnet_md_bias works on, for B walkers of n1 atoms each, and the launch on it."""

    def __init__(self, B, n1, cvs, restraints=(), kappa=None, center=None, metad=None, W=1, H=0, step0=0, base=0):
        self.B, self.n1, self.N, self.D = B, n1, B * n1, len(cvs)
        self.kinds, self.atoms, self.distinct, self.offsets, self.entries = tables(cvs)
        self.A = len(self.distinct)
        self.start = _c(np.arange(B) * n1, np.int32)
        self.res_kind = np.zeros(self.D, np.int32)
        for c, k in restraints:
            self.res_kind[c] = RESTRAINT[k]
        self.kappa = _c(np.zeros((B, self.D)) if kappa is None else kappa, np.float64)
        self.center = _c(np.zeros((B, self.D)) if center is None else center, np.float64)
        m = metad or {}
        self.mcv = list(m.get("cvs", []))
        self.dm = len(self.mcv)
        self.sigma = list(m.get("sigma", [])) + [0.0, 0.0]
        self.h0, self.kT, self.gamma, self.pace = m.get("height", 0.0), m.get("kT", 0.0), m.get("bias_factor") or 0.0, m.get("pace", 1)
        self.W, self.H = W, H
        self.head = _c([step0, base], np.uint64)
        self.hills = np.full((B // W, self.dm + 1, max(H, 1)), np.nan)  # unwritten slots are never read
        self.status = np.zeros(1, np.uint32)

    def launch(self, n, pos, forces, deposit=1, overflow=0, log_forces=True):
        """-> dict(forces, cv [B,D], restraint [B], bias [B], bias_forces [B,A,3]); rows keep NaN where nothing was written"""
        pos, f = _c(pos, np.float32), _c(forces, np.float32).copy()
        cvr, er, eb = np.full((self.B, self.D), np.nan), np.full(self.B, np.nan), np.full(self.B, np.nan)
        fl = np.full((self.B, self.A, 3), np.nan, np.float32)
        mc = self.mcv + [0, 0]
        lib().bias_launch(C.c_int32(self.N), C.c_int32(self.B), C.c_int32(self.D), C.c_int32(self.A), C.c_int32(self.W), C.c_int32(self.dm),
                          C.c_int32(mc[0]), C.c_int32(mc[1]), C.c_int32(deposit), _p(pos), _p(f), _p(self.kinds), _p(self.atoms),
                          _p(self.start), _p(self.distinct), _p(self.offsets), _p(self.entries), _p(self.res_kind), _p(self.kappa),
                          _p(self.center), C.c_double(self.sigma[0]), C.c_double(self.sigma[1]), C.c_double(self.h0), C.c_double(self.kT),
                          C.c_double(self.gamma), C.c_uint64(self.pace), C.c_int64(self.H), _p(self.head), C.c_uint64(n), _p(self.hills),
                          _p(self.status), C.c_int32(overflow), _p(cvr), _p(er), _p(eb), _p(fl if log_forces else None))
        return dict(forces=f, cv=cvr, restraint=er, bias=eb, bias_forces=fl)


def sample(B, W, steps, r0, dt, friction, seed, sigma, h0, kT, gamma, pace, H):
    """the protocol of bias_sample (tests/md_bias_host.hip) from r = r0 at rest -> (centres [G,n], heights [G,n], status, x)"""
    x = np.zeros((2 * B, 3), np.float32)
    x[1::2, 0] = r0
    v = np.zeros_like(x)
    c1 = math.exp(-friction * dt)
    c2 = math.sqrt(1.0 - c1 * c1)
    hills = np.zeros((B // W, 2, H))
    status = np.zeros(1, np.uint32)
    lib().bias_sample(C.c_int32(B), C.c_int32(W), C.c_int64(steps), _p(x), _p(v), C.c_float(dt), C.c_float(c1), C.c_float(c2),
                      C.c_uint64(seed), C.c_double(sigma), C.c_double(h0), C.c_double(kT), C.c_double(gamma), C.c_uint64(pace), C.c_int64(H),
                      _p(hills), _p(status))
    n = min(H, (steps // pace) * W)
    return hills[:, 0, :n].copy(), hills[:, 1, :n].copy(), int(status[0]), x
