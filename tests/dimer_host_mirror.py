"""TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident dimer saddle search (torchmd-net_amd/csrc/tn_dimer_math.h) on the
CPU, compiled host-only from tests/dimer_host.hip into oracle/_build/libdimer_host.so and called through ctypes on numpy arrays.
The statements are the header's own; tests/test_dimer_host.py compares them with tests/dimer_oracle.py.  Shapes: mode, partner,
vel and the per-atom outputs are [G,n,3]; forces and positions of the three images [G,3,n,3]; energies [G,3]."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.min_host_mirror import _c, _fire_args, _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "dimer_host.hip")
N_SUMS, N_PART, N_COEF = 8, 6, 10
_LIB = None


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libdimer_host.so")
        csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
        src = [SOURCE] + [os.path.join(csrc, h) for h in ("tn_dimer_math.h", "tn_min_math.h", "tn_md_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            subprocess.check_call([hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-fPIC", "-shared", SOURCE, "-o", so])
        _LIB = C.CDLL(so)
        for name in ("dimer_sum_terms", "dimer_sums", "dimer_nu2", "dimer_rotation", "dimer_mode_coef", "dimer_project", "dimer_part_sums",
                     "dimer_partner", "dimer_fire_control", "dimer_atoms", "dimer_surface"):
            getattr(_LIB, name).restype = None
        _LIB.dimer_run.restype = C.c_int64
    return _LIB


def _gn(mode):
    G, n, _ = mode.shape
    return C.c_int64(G), C.c_int64(n)


def _fixed(fixed):
    return None if fixed is None else _c(fixed, np.uint8)


def _free(fixed):
    return C.c_int32(1 if fixed is None else int((np.asarray(fixed) == 0).any()))


def sum_terms(mode, partner, f, delta, fixed=None):
    """-> t [G,n,7] fp32: N.HN, N.HM, M.HN, M.HM, F0.N, F0.M, |F0|^2 + |F1|^2 + |F2|^2 per atom"""
    mode, partner, f, fixed = _c(mode, np.float32), _c(partner, np.float32), _c(f, np.float32), _fixed(fixed)
    t = np.full(mode.shape[:2] + (7,), np.nan, np.float32)
    lib().dimer_sum_terms(*_gn(mode), _p(mode), _p(partner), _p(f), _p(fixed), C.c_double(delta), _p(t))
    return t


def sums(mode, partner, f, delta, fixed=None):
    """-> S [G,8] fp64: the fp32 terms widened and added in atom order, then the number of free atoms"""
    mode, partner, f, fixed = _c(mode, np.float32), _c(partner, np.float32), _c(f, np.float32), _fixed(fixed)
    S = np.full((mode.shape[0], N_SUMS), np.nan)
    lib().dimer_sums(*_gn(mode), _p(mode), _p(partner), _p(f), _p(fixed), C.c_double(delta), _p(S))
    return S


def nu2(mode, partner, rot, fixed=None):
    """rot [G,2] = co, si -> nu^2 [G] from the vectors"""
    mode, partner, rot, fixed = _c(mode, np.float32), _c(partner, np.float32), _c(rot, np.float64), _fixed(fixed)
    out = np.full(mode.shape[0], np.nan)
    lib().dimer_nu2(*_gn(mode), _p(mode), _p(partner), _p(fixed), _p(rot), _p(out))
    return out


def rotation(S, e, has_free=True):
    """S [G,8], e [G,3] -> cause [G], q [G,3], rot [G,2], branch [G]"""
    S, e = _c(S, np.float64), _c(e, np.float32)
    G = len(S)
    cause, q, rot, branch = np.full(G, -1, np.int32), np.full((G, 3), np.nan), np.full((G, 2), np.nan), np.full(G, -1, np.int32)
    lib().dimer_rotation(C.c_int64(G), _p(S), _p(e), C.c_int32(int(has_free)), _p(cause), _p(q), _p(rot), _p(branch))
    return cause, q, rot, branch


def mode_coef(S, q, rot, nu2_, cause, has_free=True):
    """-> cause [G] (updated), Cp [G,2] = C, p, coef [G,10] fp32 with entries 0..6 written"""
    S, q, rot, nu2_ = _c(S, np.float64), _c(q, np.float64), _c(rot, np.float64), _c(nu2_, np.float64)
    G = len(S)
    cause = _c(cause, np.int32).copy()
    Cp, coef = np.full((G, 2), np.nan), np.zeros((G, N_COEF), np.float32)
    lib().dimer_mode_coef(C.c_int64(G), _p(S), _p(q), _p(rot), _p(nu2_), C.c_int32(int(has_free)), _p(cause), _p(Cp), _p(coef))
    return cause, Cp, coef


def project(mode, partner, f, delta, coef, fixed=None):
    """-> N', T, F_eff [G,n,3] fp32 and the partner terms [G,n,6]"""
    mode, partner, f, coef, fixed = _c(mode, np.float32), _c(partner, np.float32), _c(f, np.float32), _c(coef, np.float32), _fixed(fixed)
    np_, t, fe = (np.full(mode.shape, np.nan, np.float32) for _ in range(3))
    terms = np.full(mode.shape[:2] + (N_PART,), np.nan, np.float32)
    lib().dimer_project(*_gn(mode), _p(mode), _p(partner), _p(f), _p(fixed), C.c_double(delta), _p(coef), _p(np_), _p(t), _p(fe), _p(terms))
    return np_, t, fe, terms


def part_sums(vel, feff, terms, fixed=None):
    """-> fsums [G,4] (vf, ff, vv, fmax2 on F_eff), P [G,6]"""
    vel, feff, terms, fixed = _c(vel, np.float32), _c(feff, np.float32), _c(terms, np.float32), _fixed(fixed)
    G = vel.shape[0]
    fs, P = np.full((G, 4), np.nan), np.full((G, N_PART), np.nan)
    lib().dimer_part_sums(*_gn(vel), _p(vel), _p(feff), _p(terms), _p(fixed), _p(fs), _p(P))
    return fs, P


def partner(P, coef, has_free=True):
    """P [G,6], coef [G,10] -> coef with entries 7..9 written, |T| [G], branch [G]"""
    P, coef = _c(P, np.float64), _c(coef, np.float32).copy()
    G = len(P)
    resid, branch = np.full(G, np.nan), np.full(G, -1, np.int32)
    lib().dimer_partner(C.c_int64(G), _p(P), C.c_int32(int(has_free)), _p(coef), _p(resid), _p(branch))
    return coef, resid, branch


def fire_control(state, fsums, Cp, translate, has_free, step, p):
    """state = (dt, alpha, n_pos, converged_at) arrays [G] -> new state, fcoef [G,3] fp32, ret [G]"""
    dt, alpha = _c(state[0], np.float64).copy(), _c(state[1], np.float64).copy()
    n_pos, conv = _c(state[2], np.int32).copy(), _c(state[3], np.int64).copy()
    fsums, Cp = _c(fsums, np.float64), _c(Cp, np.float64)
    G = len(dt)
    fcoef, ret = np.full((G, 3), np.nan, np.float32), np.full(G, -1, np.int32)
    lib().dimer_fire_control(C.c_int64(G), _p(dt), _p(alpha), _p(n_pos), _p(conv), _p(fsums), _p(Cp), C.c_int32(int(translate)),
                             C.c_int32(int(has_free)), C.c_int64(step), *_fire_args(p), _p(fcoef), _p(ret))
    return (dt, alpha, n_pos, conv), fcoef, ret


def atoms(accept, move, frozen, translate, delta, coef, fcoef, np_, t, feff, pos, vel, mode, partner_, fixed=None):
    """the accept and / or the move of k_dimer_atoms -> pos [G,3,n,3], vel, mode, partner [G,n,3] after it"""
    pos, vel, mode, partner_ = (_c(a, np.float32).copy() for a in (pos, vel, mode, partner_))
    accept, frozen, fixed = _c(accept, np.uint8), _c(frozen, np.uint8), _fixed(fixed)
    coef, fcoef, np_, t, feff = (_c(a, np.float32) for a in (coef, fcoef, np_, t, feff))
    lib().dimer_atoms(*_gn(mode), _p(accept), C.c_int32(int(move)), _p(frozen), C.c_int32(int(translate)), _p(fixed), C.c_double(delta),
                      _p(coef), _p(fcoef), _p(np_), _p(t), _p(feff), _p(pos), _p(vel), _p(mode), _p(partner_))
    return pos, vel, mode, partner_


def surface(x, sites, kappa, A):
    """x [..., n, 3] fp32 -> e [...] fp32, f like x: fp64 at the fp32 positions, rounded once"""
    x, sites = _c(x, np.float32), _c(sites, np.float64)
    n = x.shape[-2]
    e, f = np.full(x.shape[:-2], np.nan, np.float32), np.full(x.shape, np.nan, np.float32)
    lib().dimer_surface(C.c_int64(x.size // (3 * n)), C.c_int64(n), _p(x), _p(sites), C.c_double(kappa), C.c_double(A), _p(e), _p(f))
    return e, f


def run(pos, mode, partner_, sites, kappa, A, p, delta, translate, max_steps, fixed=None):
    """a whole search on the surface in fp32: pos [G,3,n,3], mode, partner [G,n,3] -> dict(steps (or -cause), conv [G], pos, mode,
    partner, e [G,3], C [G], resid [G])"""
    pos, mode, partner_ = (_c(a, np.float32).copy() for a in (pos, mode, partner_))
    sites, fixed = _c(sites, np.float64), _fixed(fixed)
    G = mode.shape[0]
    conv, e, curv, resid = np.zeros(G, np.int64), np.zeros((G, 3), np.float32), np.zeros(G), np.zeros(G)
    steps = lib().dimer_run(*_gn(mode), _p(sites), C.c_double(kappa), C.c_double(A), _p(pos), _p(mode), _p(partner_), _p(fixed),
                            C.c_double(delta), C.c_int32(int(translate)), C.c_double(p["dt"]), *_fire_args(p), C.c_int64(max_steps),
                            _p(conv), _p(e), _p(curv), _p(resid))
    return dict(steps=int(steps), conv=conv, pos=pos, mode=mode, partner=partner_, e=e, C=curv, resid=resid)
