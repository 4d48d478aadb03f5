"""TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident relaxed coordinate scan (torchmd-net_amd/csrc/tn_scan_math.h) on the
CPU, compiled host-only from tests/scan_host.hip into oracle/_build/libscan_host.so and called through ctypes on numpy arrays.  The
statements are the header's own; tests/test_scan_host.py compares them with tests/scan_oracle.py.  Shapes: pos, vel, forces [G,n,3];
per point cv and target [G,4] (the first D used), mult [G,2,4] (lambda, mu), corr [G,16,2,3]."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.min_host_mirror import _c, _fire_args, _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "scan_host.hip")
KINDS = {"distance": 0, "angle": 1, "torsion": 2}
MAX_CV, MAX_ATOMS = 4, 16
_LIB = None


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def sources():
    csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
    return [SOURCE] + [os.path.join(csrc, h) for h in ("tn_scan_math.h", "tn_bias_math.h", "tn_min_math.h", "tn_md_math.h")]


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libscan_host.so")
        src = sources()
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", SOURCE, "-o", so])
        _LIB = C.CDLL(so)
        for name in ("scan_project", "scan_control", "scan_move", "scan_constrain", "scan_surface", "scan_tree_sums"):
            getattr(_LIB, name).restype = None
        _LIB.scan_tables.restype = C.c_int32
        _LIB.scan_drive.restype = C.c_double
        _LIB.scan_run.restype = C.c_int64
    return _LIB


def cv_arrays(cvs):
    """[("torsion", i, j, k, l), ...] -> kind [D] int32, atoms [D,4] int32 (-1 in unused slots)"""
    kind = np.array([KINDS[cv[0]] for cv in cvs], np.int32)
    atoms = np.full((len(cvs), 4), -1, np.int32)
    for c, cv in enumerate(cvs):
        atoms[c, :len(cv) - 1] = cv[1:]
    return kind, atoms


def tables(cvs, n):
    """-> (rc, the distinct atoms ascending)"""
    kind, atoms = cv_arrays(cvs)
    A, rel = C.c_int32(0), np.full(MAX_ATOMS, -1, np.int32)
    rc = lib().scan_tables(C.c_int32(len(cvs)), _p(kind), _p(atoms), C.c_int64(n), C.byref(A), _p(rel))
    return int(rc), rel[:A.value].copy()


def _fixed(fixed):
    return None if fixed is None else _c(fixed, np.uint8)


def project(cvs, pos, vel, forces, fixed=None):
    """-> dict(why [G], cv [G,4], mult [G,2,4], corr [G,16,2,3], fperp, vperp [G,n,3], sums [G,4], gdot [G,2,4])"""
    pos, vel, forces = _c(pos, np.float32), _c(vel, np.float32), _c(forces, np.float32)
    G, n, _ = pos.shape
    kind, atoms = cv_arrays(cvs)
    out = dict(why=np.full(G, -1, np.int32), cv=np.full((G, MAX_CV), np.nan), mult=np.full((G, 2, MAX_CV), np.nan, np.float32),
               corr=np.full((G, MAX_ATOMS, 2, 3), np.nan, np.float32), fperp=np.full(pos.shape, np.nan, np.float32),
               vperp=np.full(pos.shape, np.nan, np.float32), sums=np.full((G, 4), np.nan), gdot=np.full((G, 2, MAX_CV), np.nan))
    lib().scan_project(C.c_int64(G), C.c_int64(n), C.c_int32(len(cvs)), _p(kind), _p(atoms), _p(pos), _p(vel), _p(forces), _p(_fixed(fixed)),
                       _p(out["why"]), _p(out["cv"]), _p(out["mult"]), _p(out["corr"]), _p(out["fperp"]), _p(out["vperp"]), _p(out["sums"]),
                       _p(out["gdot"]))
    return out


def slices(n):
    """the slices a point of n atoms is reduced in (tn_loop.h's mol_slices for one molecule)"""
    return 1 if n <= 1024 else min((n + 1023) // 1024, 256)


def tree_sums(fperp, vperp, fixed=None):
    """FIRE's four sums of (v_perp, F_perp) [G,n,3] in the device's order of addition -> [G,4] fp64"""
    fperp, vperp = _c(fperp, np.float32), _c(vperp, np.float32)
    G, n, _ = fperp.shape
    out = np.full((G, 4), np.nan)
    lib().scan_tree_sums(C.c_int64(G), C.c_int64(n), C.c_int32(slices(n)), _p(fperp), _p(vperp), _p(_fixed(fixed)), _p(out))
    return out


def control(state, sums, t_cur, t_fin, step, p):
    """state = (dt, alpha, n_pos, converged_at) arrays [G]; t_cur [G,4], t_fin [G,D] -> new state, coef [G,3] fp32, ret [G]"""
    dt, alpha = _c(state[0], np.float64).copy(), _c(state[1], np.float64).copy()
    n_pos, conv = _c(state[2], np.int32).copy(), _c(state[3], np.int64).copy()
    sums, t_cur, t_fin = _c(sums, np.float64), _c(t_cur, np.float64), _c(t_fin, np.float64)
    G = len(dt)
    coef, ret = np.full((G, 3), np.nan, np.float32), np.full(G, -1, np.int32)
    lib().scan_control(C.c_int64(G), C.c_int32(t_fin.shape[1]), _p(dt), _p(alpha), _p(n_pos), _p(conv), _p(sums), _p(t_cur), _p(t_fin),
                       C.c_int64(step), *_fire_args(p), _p(coef), _p(ret))
    return (dt, alpha, n_pos, conv), coef, ret


def move(conv, coef, pos, vel, fperp, fixed=None):
    """-> pos, vel after tn_min::atom_move with each point's coefficients"""
    pos, vel = _c(pos, np.float32).copy(), _c(vel, np.float32).copy()
    G, n, _ = pos.shape
    lib().scan_move(C.c_int64(G), C.c_int64(n), _p(_c(conv, np.int64)), _p(_fixed(fixed)), _p(_c(coef, np.float32)), _p(pos), _p(vel),
                    _p(_c(fperp, np.float32)))
    return pos, vel


def constrain(cvs, pos, conv, t_cur, t_fin, drive, tol, max_iter, fixed=None):
    """the drive and the constraint step -> pos, t_cur [G,4], why2 [G], iters [G]"""
    pos, t_cur = _c(pos, np.float32).copy(), _c(t_cur, np.float64).copy()
    G, n, _ = pos.shape
    kind, atoms = cv_arrays(cvs)
    why2, iters = np.full(G, -1, np.int32), np.full(G, -1, np.int32)
    lib().scan_constrain(C.c_int64(G), C.c_int64(n), C.c_int32(len(cvs)), _p(kind), _p(atoms), _p(pos), _p(_fixed(fixed)),
                         _p(_c(conv, np.int64)), _p(t_cur), _p(_c(t_fin, np.float64)), _p(_c(drive, np.float64)), C.c_double(tol),
                         C.c_int32(max_iter), _p(why2), _p(iters))
    return pos, t_cur, why2, iters


def drive(kind, t_fin, t_cur, step):
    return float(lib().scan_drive(C.c_int32(KINDS[kind]), C.c_double(t_fin), C.c_double(t_cur), C.c_double(step)))


def surface(x, sites=None, kappa=0.0):
    """x [G,n,3] fp32 -> e [G] fp32, f [G,n,3] fp32: fp64 at the fp32 positions, rounded once"""
    x = _c(x, np.float32)
    G, n, _ = x.shape
    sites = np.zeros((n, 3)) if sites is None else _c(sites, np.float64)
    e, f = np.full(G, np.nan, np.float32), np.full(x.shape, np.nan, np.float32)
    lib().scan_surface(C.c_int64(G), C.c_int64(n), _p(x), _p(sites), C.c_double(kappa), _p(e), _p(f))
    return e, f


def run(cvs, pos, t_fin, drive_, tol, max_iter, p, max_steps, sites=None, kappa=0.0, fixed=None):
    """a whole scan on the surface in fp32 storage -> dict(steps (or -cause), conv [G], pos, e [G], cv, target [G,D], lam [G,D], fmax [G])"""
    pos, t_fin = _c(pos, np.float32).copy(), _c(t_fin, np.float64)
    G, n, _ = pos.shape
    D = len(cvs)
    kind, atoms = cv_arrays(cvs)
    sites = np.zeros((n, 3)) if sites is None else _c(sites, np.float64)
    conv, e = np.zeros(G, np.int64), np.zeros(G, np.float32)
    cv, tg, lam, fm = np.zeros((G, D)), np.zeros((G, D)), np.zeros((G, D), np.float32), np.zeros(G, np.float32)
    steps = lib().scan_run(C.c_int64(G), C.c_int64(n), C.c_int32(D), _p(kind), _p(atoms), _p(sites), C.c_double(kappa), _p(pos),
                           _p(_fixed(fixed)), _p(t_fin), _p(_c(drive_, np.float64)), C.c_double(tol), C.c_int32(max_iter),
                           C.c_double(p["dt"]), *_fire_args(p), C.c_int64(max_steps), _p(conv), _p(e), _p(cv), _p(tg), _p(lam), _p(fm))
    return dict(steps=int(steps), conv=conv, pos=pos, e=e, cv=cv, target=tg, lam=lam, fmax=fm)
