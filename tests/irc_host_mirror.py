"""TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident IRC follower (torchmd-net_amd/csrc/tn_irc_math.h) on the CPU,
compiled host-only from tests/irc_host.hip into oracle/_build/libirc_host.so and called through ctypes on numpy arrays.  The
statements are the header's own and the sums are added in the device's order; tests/test_irc_host.py compares them with
tests/irc_oracle.py.  Shapes: pos, vel, forces and the generations [P,n,3]; ca, mass, fixed [n]; everything per path [P]."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.min_host_mirror import _c, _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "irc_host.hip")
N_SUMS = 6
S_VV, S_P, S_FMAX2, S_D2, S_DS2, S_FREE = range(6)
MOVING, FINISHED, FROZEN, UNUSABLE = 0, 1, 2, 3
_LIB = None


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libirc_host.so")
        csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
        src = [SOURCE] + [os.path.join(csrc, h) for h in ("tn_irc_math.h", "tn_md_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", SOURCE, "-o", so])
        _LIB = C.CDLL(so)
        for name in ("irc_start", "irc_terms", "irc_extrapolate", "irc_damp", "irc_sums", "irc_control_table", "irc_open", "irc_surface"):
            getattr(_LIB, name).restype = None
        _LIB.irc_close.restype = C.c_int32
        _LIB.irc_run.restype = C.c_int64
    return _LIB


def _fixed(fixed):
    return None if fixed is None else _c(fixed, np.uint8)


def half_inv_mass(masses, force_scale=1.0):
    """c_a = fp32(force_scale / (2 m_a)), formed in fp64 and rounded once; an infinite mass gives 0"""
    return (float(force_scale) / (2.0 * np.asarray(masses, np.float64))).astype(np.float32)


def start(x_ts, u, initial_step, v0, D=2, backward=False):
    """x_ts, u [G,n,3] -> pos, vel [G*D,n,3] fp32"""
    x_ts, u = _c(x_ts, np.float32), _c(u, np.float32)
    G, n, _ = x_ts.shape
    pos, vel = np.full((G * D, n, 3), np.nan, np.float32), np.full((G * D, n, 3), np.nan, np.float32)
    lib().irc_start(C.c_int64(G), C.c_int64(D), C.c_int64(n), C.c_int32(int(backward)), _p(x_ts), _p(u), C.c_double(initial_step),
                    C.c_double(v0), _p(pos), _p(vel))
    return pos, vel


def terms(pos, vel, f, ca, mass, dt, dt_prev, has2, x1, x2, v2, f2, fixed=None):
    """-> v' [P,n,3], t [P,n,5] fp32: |v'|^2, F.v', |F|^2, |x - x'|^2, m |x - x1|^2 per atom (zeros on atoms that never move)"""
    a = [_c(t, np.float32) for t in (pos, vel, f, ca, mass)]
    P, n, _ = a[0].shape
    g = [_c(t, np.float32) for t in (x1, x2, v2, f2)]
    dt, dt_prev, has2 = _c(dt, np.float32), _c(dt_prev, np.float32), _c(has2, np.int32)
    vp, t = np.full((P, n, 3), np.nan, np.float32), np.full((P, n, 5), np.nan, np.float32)
    lib().irc_terms(C.c_int64(P), C.c_int64(n), *(_p(t_) for t_ in a), _p(_fixed(fixed)), _p(dt), _p(dt_prev), _p(has2),
                    *(_p(t_) for t_ in g), _p(vp), _p(t))
    return vp, t


def extrapolate(x2, v2, f2, ca, T):
    x2, v2, f2, ca, T = (_c(t, np.float32) for t in (x2, v2, f2, ca, T))
    P, n, _ = x2.shape
    xp = np.full((P, n, 3), np.nan, np.float32)
    lib().irc_extrapolate(C.c_int64(P), C.c_int64(n), _p(x2), _p(v2), _p(f2), _p(ca), _p(T), _p(xp))
    return xp


def damp(vp, c):
    vp, c = _c(vp, np.float32), _c(c, np.float32)
    v = np.full(vp.shape, np.nan, np.float32)
    lib().irc_damp(C.c_int64(vp.shape[0]), C.c_int64(vp.shape[1]), _p(vp), _p(c), _p(v))
    return v


def control(sums, e, state, start_, step, prm):
    """sums [P,6], e [P], state = dict(dt, arc, conv, reason, n_acc, n_rec) of arrays [P] -> new state, out [P,2] fp32 (c, dt used),
    slot, cause, ret [P]"""
    sums, e = _c(sums, np.float64), _c(e, np.float32)
    P = len(sums)
    s = dict(dt=_c(state["dt"], np.float64).copy(), arc=_c(state["arc"], np.float64).copy(), conv=_c(state["conv"], np.int64).copy(),
             reason=_c(state["reason"], np.int32).copy(), n_acc=_c(state["n_acc"], np.int32).copy(), n_rec=_c(state["n_rec"], np.int32).copy())
    out = np.full((P, 2), np.nan, np.float32)
    slot, cause, ret = (np.full(P, -9, np.int32) for _ in range(3))
    lib().irc_control_table(C.c_int64(P), _p(sums), _p(e), C.c_int32(int(start_)), C.c_int64(step), *_prm(prm), _p(s["dt"]), _p(s["arc"]),
                            _p(s["conv"]), _p(s["reason"]), _p(s["n_acc"]), _p(s["n_rec"]), _p(out), _p(slot), _p(cause), _p(ret))
    return s, out, slot, cause, ret


def _prm(p):
    return (C.c_double(p["fmax"]), C.c_double(p["v0"]), C.c_double(p["error"]), C.c_double(p["dt_min"]), C.c_double(p["dt_max"]),
            C.c_int32(p.get("every", 1)), C.c_int32(p.get("capacity", 512)))


def surface(x, sites, kappa, A):
    """x [P,n,3] fp32 -> e [P] fp32, f like x: fp64 at the fp32 positions, rounded once"""
    x, sites = _c(x, np.float32), _c(sites, np.float64)
    P, n, _ = x.shape
    e, f = np.full(P, np.nan, np.float32), np.full(x.shape, np.nan, np.float32)
    lib().irc_surface(C.c_int64(P), C.c_int64(n), _p(x), _p(sites), C.c_double(kappa), C.c_double(A), _p(e), _p(f))
    return e, f


class Paths:
    """The state of P paths, stepped as the device steps it: ``close(e, f)`` is MIDDLE / CLOSE up to the move (-> 0 or the cause),
    ``open()`` the move.  The first ``close`` controls the start images."""

    def __init__(self, pos, vel, masses, prm, dt, fixed=None, force_scale=1.0, step0=0):
        self.pos, self.vel = _c(pos, np.float32).copy(), _c(vel, np.float32).copy()
        P, n, _ = self.pos.shape
        self.P, self.n, self.prm = P, n, dict(prm)
        self.cap = self.prm.get("capacity", 512)
        self.mass = _c(masses, np.float32)
        self.ca = half_inv_mass(masses, force_scale)
        self.fixed = _fixed(fixed)
        z = lambda: np.zeros((P, n, 3), np.float32)
        self.fkeep, self.x1, self.v1, self.f1, self.x2, self.v2, self.f2 = z(), z(), z(), z(), z(), z(), z()
        self.dt, self.arc = np.full(P, float(dt)), np.zeros(P)
        self.conv, self.reason = np.full(P, -1, np.int64), np.zeros(P, np.int32)
        self.n_acc, self.n_rec = np.zeros(P, np.int32), np.zeros(P, np.int32)
        self.dt_used, self.damp, self.rec = np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros((P, N_SUMS))
        self.frame_s, self.frame_e = np.zeros((P, self.cap)), np.zeros((P, self.cap), np.float32)
        self.frames = np.zeros((P, self.cap, n, 3), np.float32)
        self.step, self.fresh = int(step0), True

    def close(self, e, f):
        e, f = _c(e, np.float32), _c(f, np.float32)
        step = self.step + (0 if self.fresh else 1)
        p = self.prm
        bad = lib().irc_close(C.c_int64(self.P), C.c_int64(self.n), C.c_int32(int(self.fresh)), C.c_int64(step), _p(e), _p(f), _p(self.ca),
                              _p(self.mass), _p(self.fixed), *_prm(p), _p(self.pos), _p(self.vel), _p(self.fkeep), _p(self.x1), _p(self.v1),
                              _p(self.x2), _p(self.v2), _p(self.f2), _p(self.dt), _p(self.arc), _p(self.conv), _p(self.reason), _p(self.n_acc),
                              _p(self.n_rec), _p(self.dt_used), _p(self.damp), _p(self.rec), _p(self.frame_s), _p(self.frame_e),
                              _p(self.frames))
        if not bad:
            self.step, self.fresh = step, False
        return int(bad)

    def open(self):
        lib().irc_open(C.c_int64(self.P), C.c_int64(self.n), _p(self.ca), _p(self.fixed), _p(self.dt), _p(self.conv), _p(self.pos), _p(self.vel),
                       _p(self.fkeep), _p(self.x1), _p(self.v1), _p(self.f1), _p(self.x2), _p(self.v2), _p(self.f2))


def run(pos, vel, masses, sites, kappa, A, prm, dt, max_steps, fixed=None, force_scale=1.0):
    """whole paths on the surface in fp32 from the start images pos, vel [P,n,3] -> dict(steps (or -cause), conv, reason, arc, dt, n_rec
    [P], pos, vel, forces [P,n,3], frame_s, frame_e [P,C], frames [P,C,n,3], log [steps+1,P,4] = dt, c, arc, power)"""
    pos, vel = _c(pos, np.float32).copy(), _c(vel, np.float32).copy()
    P, n, _ = pos.shape
    cap = prm.get("capacity", 512)
    mass, ca, sites, fixed = _c(masses, np.float32), half_inv_mass(masses, force_scale), _c(sites, np.float64), _fixed(fixed)
    fkeep = np.zeros((P, n, 3), np.float32)
    conv, reason, arc, dt_, n_rec = np.zeros(P, np.int64), np.zeros(P, np.int32), np.zeros(P), np.zeros(P), np.zeros(P, np.int32)
    frame_s, frame_e, frames = np.zeros((P, cap)), np.zeros((P, cap), np.float32), np.zeros((P, cap, n, 3), np.float32)
    log = np.zeros((max_steps + 1, P, 4))
    steps = lib().irc_run(C.c_int64(P), C.c_int64(n), _p(sites), C.c_double(kappa), C.c_double(A), _p(ca), _p(mass), _p(fixed), C.c_double(dt),
                          *_prm(prm), C.c_int64(max_steps), _p(pos), _p(vel), _p(fkeep), _p(conv), _p(reason), _p(arc), _p(dt_), _p(n_rec),
                          _p(frame_s), _p(frame_e), _p(frames), _p(log))
    return dict(steps=int(steps), conv=conv, reason=reason, arc=arc, dt=dt_, n_rec=n_rec, pos=pos, vel=vel, forces=fkeep, frame_s=frame_s,
                frame_e=frame_e, frames=frames, log=log[:max(int(steps), 0) + 1])
