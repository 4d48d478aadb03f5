"""TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident nudged elastic band (torchmd-net_amd/csrc/tn_neb_math.h) on the
CPU, compiled host-only from tests/neb_host.hip into oracle/_build/libneb_host.so and called through ctypes on numpy arrays.
The statements are the header's own; tests/test_neb_host.py compares them with tests/neb_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.min_host_mirror import _c, _fire_args, _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "neb_host.hip")
_LIB = None


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libneb_host.so")
        csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
        src = [SOURCE] + [os.path.join(csrc, h) for h in ("tn_neb_math.h", "tn_min_math.h", "tn_md_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", SOURCE, "-o", so])
        _LIB = C.CDLL(so)
        for name in ("neb_path_terms", "neb_path_sums", "neb_image_control", "neb_project", "neb_fire_sums", "neb_move", "neb_surface"):
            getattr(_LIB, name).restype = None
        _LIB.neb_run.restype = C.c_int64
    return _LIB


def _shape(pos):
    """pos [G,M,n,3] -> G, M, n as c_int64"""
    G, M, n, _ = pos.shape
    return C.c_int64(G), C.c_int64(M), C.c_int64(n)


def _fixed(fixed):
    return None if fixed is None else _c(fixed, np.uint8)


def path_terms(pos, f, fixed=None):
    """pos, f [G,M,n,3] -> t [G,M,n,5] fp32: d+.d+, d-.d-, d+.d-, F.d+, F.d- per atom, zero on endpoints"""
    pos, f, fixed = _c(pos, np.float32), _c(f, np.float32), _fixed(fixed)
    t = np.full(pos.shape[:3] + (5,), np.nan, np.float32)
    lib().neb_path_terms(*_shape(pos), _p(pos), _p(f), _p(fixed), _p(t))
    return t


def path_sums(pos, f, fixed=None):
    """-> [G,M,5] fp64: the fp32 terms widened and added in atom order"""
    pos, f, fixed = _c(pos, np.float32), _c(f, np.float32), _fixed(fixed)
    s = np.full(pos.shape[:2] + (5,), np.nan)
    lib().neb_path_sums(*_shape(pos), _p(pos), _p(f), _p(fixed), _p(s))
    return s


def image_control(e, sums, k, climb, has_free=True):
    """e [G,M] fp32, sums [G,M,5] -> w [G,M,2] fp64, s [G,M,2] fp32, why [G,M] int32, climber [G] int32.  has_free: some atom is
    not fixed"""
    e, sums = _c(e, np.float32), _c(sums, np.float64)
    G, M = e.shape
    w, s = np.full((G, M, 2), np.nan), np.full((G, M, 2), np.nan, np.float32)
    why, climber = np.full((G, M), -1, np.int32), np.full(G, -1, np.int32)
    lib().neb_image_control(C.c_int64(G), C.c_int64(M), _p(e), _p(sums), C.c_double(k), C.c_int32(int(climb)), C.c_int32(int(has_free)),
                            _p(w), _p(s), _p(why), _p(climber))
    return w, s, why, climber


def project(pos, f, s, fixed=None):
    """-> F_neb [G,M,n,3] fp32"""
    pos, f, s, fixed = _c(pos, np.float32), _c(f, np.float32), _c(s, np.float32), _fixed(fixed)
    out = np.full(pos.shape, np.nan, np.float32)
    lib().neb_project(*_shape(pos), _p(pos), _p(f), _p(fixed), _p(s), _p(out))
    return out


def fire_sums(v, fneb, fixed=None):
    """-> [G,4] fp64: vf, ff, vv, fmax2 over the interior images"""
    v, fneb, fixed = _c(v, np.float32), _c(fneb, np.float32), _fixed(fixed)
    s = np.full((v.shape[0], 4), np.nan)
    lib().neb_fire_sums(*_shape(v), _p(v), _p(fneb), _p(fixed), _p(s))
    return s


def move(conv, coef, x, v, fneb, fixed=None):
    """-> (x, v) after the per-row update"""
    conv, coef, fixed = _c(conv, np.int64), _c(coef, np.float32), _fixed(fixed)
    x, v, fneb = _c(x, np.float32).copy(), _c(v, np.float32).copy(), _c(fneb, np.float32)
    lib().neb_move(*_shape(x), _p(conv), _p(fixed), _p(coef), _p(x), _p(v), _p(fneb))
    return x, v


def surface(x, sites, kappa, A):
    """x [..., n, 3] fp32 -> e [...] fp32, f like x: fp64 at the fp32 positions, rounded once"""
    x, sites = _c(x, np.float32), _c(sites, np.float64)
    n = x.shape[-2]
    n_img = x.size // (3 * n)
    e, f = np.full(x.shape[:-2], np.nan, np.float32), np.full(x.shape, np.nan, np.float32)
    lib().neb_surface(C.c_int64(n_img), C.c_int64(n), _p(x), _p(sites), C.c_double(kappa), C.c_double(A), _p(e), _p(f))
    return e, f


def run(x, sites, kappa, A, p, spring, climb, max_steps, fixed=None):
    """a whole optimisation on the surface in fp32 -> steps (or -cause), converged_at [G], final x, e [G,M], climber [G]"""
    x, sites, fixed = _c(x, np.float32).copy(), _c(sites, np.float64), _fixed(fixed)
    G, M = x.shape[:2]
    conv, e, climber = np.zeros(G, np.int64), np.zeros((G, M), np.float32), np.zeros(G, np.int32)
    steps = lib().neb_run(*_shape(x), _p(sites), C.c_double(kappa), C.c_double(A), _p(x), _p(fixed), C.c_double(p["dt"]), *_fire_args(p),
                          C.c_double(spring), C.c_int32(int(climb)), C.c_int64(max_steps), _p(conv), _p(e), _p(climber))
    return int(steps), conv, x, e, climber
