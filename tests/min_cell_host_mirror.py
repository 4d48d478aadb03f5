"""TEST INFRASTRUCTURE ONLY: the cell-relaxation arithmetic of the device-resident FIRE minimiser (torchmd-net_amd/csrc/tn_min_math.h)
on the CPU, compiled host-only from tests/min_cell_host.hip into oracle/_build/libmin_cell_host.so and called through ctypes on numpy
arrays.  The statements are the header's own; tests/test_min_cell_host.py compares them with tests/min_cell_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "min_cell_host.hip")
_LIB = None


def _sources():
    csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
    return [SOURCE, os.path.join(csrc, "tn_min_math.h"), os.path.join(csrc, "tn_md_math.h")]


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libmin_cell_host.so")
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in _sources()):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", SOURCE, "-o", so])
        _LIB = C.CDLL(so)
        for name in ("min_cell_positions", "min_cell_terms", "min_cell_reduce", "min_cell_control", "min_cell_update"):
            getattr(_LIB, name).restype = None
    return _LIB


def _p(a):
    return C.c_void_p(0) if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _fire_args(p):
    return (C.c_double(p["dt_max"]), C.c_int32(p["n_min"]), C.c_double(p["f_inc"]), C.c_double(p["f_dec"]), C.c_double(p["alpha"]),
            C.c_double(p["f_alpha"]), C.c_double(p["max_step"]), C.c_double(p["fmax"]))


def flags(cp):
    return int(bool(cp["hydrostatic"])) | (int(bool(cp["constant_volume"])) << 1)


def positions(batch, d32, xt):
    """x = xt D32^T, fp32 [n,3]"""
    batch, d32, xt = _c(batch, np.int64), _c(d32, np.float32), _c(xt, np.float32)
    x = np.full_like(xt, np.nan)
    lib().min_cell_positions(C.c_int64(len(xt)), _p(batch), _p(d32), _p(xt), _p(x))
    return x


def terms(batch, d32, vt, f, fixed=None):
    """-> Ft [n,3], t [n,3] fp32"""
    batch, d32, vt, f = _c(batch, np.int64), _c(d32, np.float32), _c(vt, np.float32), _c(f, np.float32)
    fixed = None if fixed is None else _c(fixed, np.uint8)
    ft, t = np.full_like(f, np.nan), np.full_like(f, np.nan)
    lib().min_cell_terms(C.c_int64(len(f)), _p(batch), _p(d32), _p(vt), _p(f), _p(fixed), _p(ft), _p(t))
    return ft, t


def reduce(n_mol, batch, d32, vt, f, fixed=None):
    """the atoms' sums [n_mol, 4], atoms in index order"""
    batch, d32, vt, f = _c(batch, np.int64), _c(d32, np.float32), _c(vt, np.float32), _c(f, np.float32)
    fixed = None if fixed is None else _c(fixed, np.uint8)
    sums = np.full((n_mol, 4), np.nan)
    lib().min_cell_reduce(C.c_int64(n_mol), C.c_int64(len(f)), _p(batch), _p(d32), _p(vt), _p(f), _p(fixed), _p(sums))
    return sums


def control(state, sums, W, box, d32, H0, D, VD, cell_factor, p, cp, step):
    """state = (dt, alpha, n_pos, converged_at) arrays [n]; sums [n,4] the atoms'; W, box, d32 [n,9] fp32; H0, D, VD [n,9] fp64 ->
    new state, dict(sums, coef, Gc, V, stress, D, VD, box, d32, ret, why)"""
    dt, alpha = _c(state[0], np.float64).copy(), _c(state[1], np.float64).copy()
    n_pos, conv = _c(state[2], np.int32).copy(), _c(state[3], np.int64).copy()
    n = len(dt)
    sums = _c(sums, np.float64).reshape(n, 4).copy()
    W, box, d32 = (_c(a, np.float32).reshape(n, 9) for a in (W, box, d32))
    H0, D, VD = (_c(a, np.float64).reshape(n, 9) for a in (H0, D, VD))
    cfac, mask = _c(cell_factor, np.float64).reshape(n), _c(cp["mask"], np.float64).reshape(9)
    o = dict(sums=sums, coef=np.full((n, 3), np.nan, np.float32), Gc=np.full((n, 9), np.nan), V=np.full(n, np.nan),
             stress=np.full((n, 9), np.nan), D=np.full((n, 9), np.nan), VD=np.full((n, 9), np.nan), box=np.full((n, 9), np.nan, np.float32),
             d32=np.full((n, 9), np.nan, np.float32), ret=np.full(n, -1, np.int32), why=np.full(n, -1, np.int32))
    lib().min_cell_control(C.c_int64(n), _p(dt), _p(alpha), _p(n_pos), _p(conv), _p(sums), _p(W), _p(box), _p(d32), _p(H0), _p(D), _p(VD),
                           _p(cfac), *_fire_args(p), _p(mask), C.c_int32(flags(cp)), C.c_double(cp["pressure"]), C.c_int64(step),
                           _p(o["coef"]), _p(o["Gc"]), _p(o["V"]), _p(o["stress"]), _p(o["D"]), _p(o["VD"]), _p(o["box"]), _p(o["d32"]),
                           _p(o["ret"]), _p(o["why"]))
    return (dt, alpha, n_pos, conv), o


def update(batch, conv, fixed, coef, d32_prev, d32, xt, vt, f, x):
    """-> (xt, vt, x) after the per-atom update"""
    batch, conv, coef = _c(batch, np.int64), _c(conv, np.int64), _c(coef, np.float32)
    fixed = None if fixed is None else _c(fixed, np.uint8)
    d32_prev, d32 = _c(d32_prev, np.float32), _c(d32, np.float32)
    xt, vt, x, f = _c(xt, np.float32).copy(), _c(vt, np.float32).copy(), _c(x, np.float32).copy(), _c(f, np.float32)
    lib().min_cell_update(C.c_int64(len(xt)), _p(batch), _p(conv), _p(fixed), _p(coef), _p(d32_prev), _p(d32), _p(xt), _p(vt), _p(f), _p(x))
    return xt, vt, x


def relax(x, H0, efw, p, cp, c, max_steps, batch=None, fixed=None):
    """The launch sequence on one molecule, written as a loop over the entries above: control of the start geometry, then per step
    update, forces, reduce, control.  efw(x fp32 [n,3], box fp32 [3,3]) -> (E, F, W); F and W are rounded to fp32 as an engine's
    would be.  -> dict(steps, converged_at, x, xt, box, D, d32, fmax, status)"""
    x = _c(x, np.float32).copy()
    n = len(x)
    batch = np.zeros(n, np.int64) if batch is None else batch
    H0 = _c(H0, np.float32).astype(np.float64).reshape(1, 9)
    box, d32 = H0.astype(np.float32), np.eye(3, dtype=np.float32).reshape(1, 9)
    D, VD = np.eye(3).reshape(1, 9), np.zeros((1, 9))
    xt, vt = x.copy(), np.zeros_like(x)
    state = (np.array([p["dt"]]), np.array([p["alpha"]]), np.zeros(1, np.int32), np.full(1, -1, np.int64))
    step = 0
    while True:
        _, F, W = efw(x, box.reshape(3, 3))
        F, W = _c(F, np.float32), _c(W, np.float32)
        state, o = control(state, reduce(1, batch, d32, vt, F, fixed), W, box, d32, H0, D, VD, [c], p, cp, step)
        if o["ret"][0] == 2:
            return dict(status=int(o["why"][0]), steps=step)
        if state[3][0] >= 0 or step == max_steps:
            return dict(steps=step, converged_at=int(state[3][0]), x=x, xt=xt, box=box.reshape(3, 3), D=D.reshape(3, 3), d32=d32.reshape(3, 3),
                        fmax=float(np.sqrt(o["sums"][0, 3])), status=0)
        d32_prev, d32, box, D, VD = d32, o["d32"], o["box"], o["D"], o["VD"]
        xt, vt, x = update(batch, state[3], fixed, o["coef"], d32_prev, d32, xt, vt, F, x)
        step += 1
