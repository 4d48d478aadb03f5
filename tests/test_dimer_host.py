"""No GPU: the arithmetic of the device-resident dimer saddle search (csrc/tn_dimer_math.h, compiled host-only by
tests/dimer_host_mirror.py) against tests/dimer_oracle.py - the scheme in fp64, written from the equations.  1. the rotation table,
2. the single-rounded per-atom operations, 3. whole searches on the analytic surface in both precisions, 4. the mode search,
5. fixed atoms, 6. the sanitizers on a stand-alone program, 7. the additive ABI and the signatures."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import dimer_host_mirror as H
from tests import dimer_oracle as O

NO, MO = O.NO, O.MO
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(MO.FIRE, fmax=1e-3)  # ASE's defaults, the bound of the surface runs
DELTA = 0.01
NAN, INF = float("nan"), float("inf")


def _bits32(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.asarray(a, np.float64).view(np.uint64)


# ---- 1. the rotation table -------------------------------------------------------------------------------------------------------------
# name, (a, b, c), nu^2, the energies, expected cause, expected branch, expected (co, si) where the table states them
ROT_TABLE = [
    ("b = 0, a < c: the axis stays", (-3.0, 0.0, 2.0), 1.0, (0, 0, 0), 0, O.KEEP, (1.0, 0.0)),
    ("b = 0, a > c: the partner is the axis", (2.0, 0.0, -3.0), 1.0, (0, 0, 0), 0, O.SWAP, (0.0, 1.0)),
    ("b = 0, a = c: a tie keeps the axis", (1.5, 0.0, 1.5), 1.0, (0, 0, 0), 0, O.KEEP, (1.0, 0.0)),
    ("b = -0, a > c", (2.0, -0.0, -3.0), 1.0, (0, 0, 0), 0, O.SWAP, (0.0, 1.0)),
    ("b > 0", (-1.0, 0.75, 2.0), 1.0, (0, 0, 0), 0, O.ANGLE, None),
    ("b < 0", (-1.0, -0.75, 2.0), 1.0, (0, 0, 0), 0, O.ANGLE, None),
    ("b > 0, a > c: co stays non-negative", (3.0, 0.5, -2.0), 1.0, (0, 0, 0), 0, O.ANGLE, None),
    ("b < 0, a > c: co stays non-negative", (3.0, -0.5, -2.0), 1.0, (0, 0, 0), 0, O.ANGLE, None),
    ("b != 0, a = c: 45 degrees", (1.0, 0.25, 1.0), 1.0, (0, 0, 0), 0, O.ANGLE, (math.sqrt(0.5), -math.sqrt(0.5))),
    ("nu^2 not 1", (-1.0, 0.75, 2.0), 0.9375, (0, 0, 0), 0, O.ANGLE, None),
    ("convex: C > 0", (1.0, 0.5, 2.0), 1.0, (0, 0, 0), 0, O.ANGLE, None),
    ("a NaN entry", (NAN, 0.5, 2.0), 1.0, (0, 0, 0), O.BAD_MODE, None, None),
    ("an infinite entry", (1.0, 0.5, INF), 1.0, (0, 0, 0), O.BAD_MODE, None, None),
    ("nu = 0", (-1.0, 0.75, 2.0), 0.0, (0, 0, 0), O.BAD_MODE, None, None),
    ("nu^2 NaN", (-1.0, 0.75, 2.0), NAN, (0, 0, 0), O.BAD_MODE, None, None),
    ("a NaN energy", (-1.0, 0.75, 2.0), 1.0, (0, NAN, 0), O.BAD_ENERGY, None, None),
    ("an infinite energy", (-1.0, 0.75, 2.0), 1.0, (0, 0, INF), O.BAD_ENERGY, None, None),
]


def _table_sums():
    S = np.zeros((len(ROT_TABLE), 8))
    for i, (_, (a, b, c), _, _, _, _, _) in enumerate(ROT_TABLE):
        S[i] = [a, 1.5 * b, 0.5 * b, c, 0.625, -1.25, 7.0, 4.0]  # b = (N.HM + M.HN) / 2 from two unequal halves
    e = np.array([t[3] for t in ROT_TABLE], np.float32)
    nu2 = np.array([t[2] for t in ROT_TABLE])
    return S, e, nu2


def test_rotation_table_equals_the_oracle_bit_for_bit_on_the_headers_sums():
    """Every branch of the rotation, both signs of b, co >= 0, nu^2 != 1, the convex rule, the unusable inputs: (co, si), C, p bit for
    bit and the seven coefficients bit for bit against the oracle fed with the same sums (the same IEEE operations and the same C
    library); the branch and the cause equal."""
    S, e, nu2 = _table_sums()
    cause, q, rot, branch = H.rotation(S, e)
    cause2, Cp, coef = H.mode_coef(S, q, rot, nu2, cause)
    for i, (name, abc, _, _, want_cause, want_branch, want_rot) in enumerate(ROT_TABLE):
        c0, q0, (co, si), br = O.mode_rotation(S[i], e[i])
        c1, C, p, cf = (c0, 0.0, 0.0, np.zeros(7, np.float32)) if c0 else O.mode_coef(q0, S[i], co, si, nu2[i])
        assert cause2[i] == c1 == want_cause, name
        if want_cause:
            assert (coef[i] == 0).all() and (Cp[i] == 0).all(), name
            continue
        assert branch[i] == br == want_branch, name
        assert (_bits64(rot[i]) == _bits64([co, si])).all() and (_bits64(Cp[i]) == _bits64([C, p])).all(), name
        assert (_bits32(coef[i, :7]) == _bits32(cf)).all(), (name, coef[i], cf)
        assert rot[i, 0] >= 0.0 and abs(rot[i, 0] ** 2 + rot[i, 1] ** 2 - 1.0) < 4e-16, name
        if want_rot is not None:
            assert np.abs(rot[i] - want_rot).max() < 2e-16, (name, rot[i])
        # the eigenvector of the smaller eigenvalue: the Rayleigh quotient is the smaller eigenvalue of [[a, b], [b, c]]
        a, b, c = abc
        lam = np.linalg.eigvalsh(np.array([[a, b], [b, c]]))[0]
        ray = rot[i, 0] ** 2 * a + 2 * rot[i, 0] * rot[i, 1] * b + rot[i, 1] ** 2 * c
        assert abs(ray - lam) < 1e-14 * max(abs(a), abs(b), abs(c)), (name, ray, lam)
        assert abs(Cp[i, 0] - lam / nu2[i]) < 1e-14 * abs(lam / nu2[i]), name
        assert coef[i, O.C_K0] == (1.0 if Cp[i, 0] < 0 else 0.0) and coef[i, O.C_E] == np.float32((-2.0 if Cp[i, 0] < 0 else -1.0) * Cp[i, 1])
    assert {t[5] for t in ROT_TABLE if t[5] is not None} == {O.KEEP, O.SWAP, O.ANGLE}
    # a force sum that is not finite comes before the mode; no free atom: nothing is unusable, nothing rotates
    S2 = S[:3].copy()
    S2[0, O.S_FF], S2[1, O.S_PN], S2[2, O.S_PM] = INF, NAN, NAN
    S2[:, 0] = NAN
    assert H.rotation(S2, e[:3])[0].tolist() == [O.BAD_SUMS] * 3 == [O.mode_rotation(S2[i], e[i])[0] for i in range(3)]
    c, q, r, b = H.rotation(S2, np.full((3, 3), NAN, np.float32), has_free=False)
    assert c.tolist() == [0, 0, 0] and (r == [1.0, 0.0]).all() and (H.mode_coef(S2, q, r, np.zeros(3), c, has_free=False)[2] == 0).all()


def _dyadic_dimers(rng, G, n=5):
    """vectors on a grid of 1/8, forces on a grid of 1/4, delta = 2^-6 (so 1 / delta = 64 exactly): every fp32 product and sum of the
    first launch's terms is exact, the header's sums equal the oracle's and the comparison is about the coefficients alone"""
    N = rng.integers(-8, 9, size=(G, n, 3)).astype(np.float32) / 8
    M = rng.integers(-8, 9, size=(G, n, 3)).astype(np.float32) / 8
    f = rng.integers(-12, 13, size=(G, 3, n, 3)).astype(np.float32) / 4
    return N, M, f


def test_rotation_and_curvature_within_one_ulp_of_the_oracle_on_its_own_sums():
    """The oracle works from the vectors in fp64 with nothing rounded; the header from its fp32 terms, which are exact here.  (co, si)
    and C within 1 fp32 ulp, the branches equal; so are |T| and the partner's branch.  Ties made on purpose: M.HN = -N.HM (b = 0) with
    a < c and a > c, M = 0 (c = 0) and the |T| = 0 dimer, whose partner is the rotated old one."""
    rng = np.random.default_rng(11)
    G, n, delta = 40, 5, 2.0 ** -6
    N, M, f = _dyadic_dimers(rng, G, n)
    fixed = np.array([0, 0, 1, 0, 0], np.uint8)
    # dimers 0, 1: one free atom (two more fixed: dimers share `fixed`, so zero the vectors instead), forces chosen so that b = 0
    for d, (hn, hm) in enumerate([((-2.0, 0, 0), (0, 3.0, 0)), ((2.0, 0, 0), (0, -3.0, 0))]):
        N[d], M[d] = 0, 0
        N[d, 0], M[d, 0] = (1, 0, 0), (0, 1, 0)
        f[d] = 0.25
        f[d, 1, 0] = f[d, 0, 0] - np.array(hn, np.float32) * np.float32(delta)
        f[d, 2, 0] = f[d, 0, 0] - np.array(hm, np.float32) * np.float32(delta)
    M[2] = 0  # no partner: M.HN = c = 0
    # dimer 3: H = diag(-2, 3, 3) on one atom with N its eigenvector -> T = 0 exactly
    N[3], M[3] = 0, 0
    N[3, 0], M[3, 0] = (1, 0, 0), (0, 1, 0)
    f[3] = 0.5
    f[3, 1, 0] = f[3, 0, 0] - np.array((-2.0, 0, 0), np.float32) * np.float32(delta)
    f[3, 2, 0] = f[3, 0, 0] - np.array((0, 3.0, 0), np.float32) * np.float32(delta)
    e = np.zeros((G, 3), np.float32)
    S = H.sums(N, M, f, delta, fixed)
    cause, q, rot, branch = H.rotation(S, e)
    nu2 = H.nu2(N, M, rot, fixed)
    cause, Cp, coef = H.mode_coef(S, q, rot, nu2, cause)
    np_, t, fe, terms = H.project(N, M, f, delta, coef, fixed)
    _, Pm = H.part_sums(np.zeros_like(N), fe, terms, fixed)
    coef, resid, pbranch = H.partner(Pm, coef)
    worst = 0
    for d in range(G):
        r = O.step64(N[d], M[d], e[d], f[d, 0], f[d, 1], f[d, 2], delta, fixed)
        assert (r["S"] == S[d]).all(), d  # exact terms
        assert cause[d] == r["cause"] == 0 and branch[d] == r["branch"], (d, branch[d], r["branch"])
        got = np.array([rot[d, 0], rot[d, 1], Cp[d, 0]], np.float32)
        want = np.array([r["co"], r["si"], r["C"]], np.float32)
        dist = MO.ulp_distance(got, want).max()
        worst = max(worst, int(dist))
        assert dist <= 1, (d, got, want)
        assert abs(nu2[d] - r["nu2"]) <= 1e-14 * r["nu2"] and abs(Cp[d, 1] - r["p"]) <= 1e-6 * (abs(r["p"]) + 1)
        assert pbranch[d] == r["partner"], (d, pbranch[d], r["partner"])
        assert abs(resid[d] - r["resid"]) <= 1e-5 * (r["resid"] + abs(r["C"])), (d, resid[d], r["resid"])
    print("largest distance of (co, si, C) from the oracle on its own sums:", worst, "ulp")
    assert branch[[0, 1, 3]].tolist() == [O.KEEP, O.SWAP, O.KEEP] and (branch[4:] == O.ANGLE).all() and S[2, O.S_C] == 0 == S[2, O.S_B2]
    assert resid[3] == 0.0 and pbranch[3] == O.ROTATED and (pbranch[4:] == O.RESIDUAL).all()
    # the |T| = 0 dimer keeps a defined partner: the old one, still orthonormal to N'
    _, _, N2, M2 = H.atoms(np.ones(G, np.uint8), 0, np.zeros(G, np.uint8), 1, delta, coef, np.zeros((G, 3), np.float32), np_, t, fe,
                           np.zeros((G, 3, n, 3), np.float32), np.zeros_like(N), N, M, fixed)
    assert (N2[3] == N[3]).all() and (M2[3] == M[3]).all()
    free = fixed == 0
    for d in range(4, G):  # the new pair is orthonormal to fp32 accuracy and zero on the fixed atom
        nn, mm, nm = (N2[d, free].astype(np.float64) ** 2).sum(), (M2[d, free].astype(np.float64) ** 2).sum(), (N2[d, free].astype(np.float64) * M2[d, free]).sum()
        assert abs(nn - 1) < 1e-6 and abs(mm - 1) < 1e-6 and abs(nm) < 1e-6, (d, nn, mm, nm)
    assert (N2[:, 2] == 0).all() and (M2[:, 2] == 0).all()


def test_partner_and_controller_equal_the_oracle_bit_for_bit_on_the_headers_sums():
    rng = np.random.default_rng(12)
    G = 64
    Pm = np.abs(rng.normal(size=(G, 6)))
    Pm[:, O.P_TN] = 1e-4 * rng.normal(size=G)
    Pm[:, O.P_RN] = 1e-4 * rng.normal(size=G)
    Pm[:, O.P_NN] = 1.0 + 1e-7 * rng.normal(size=G)
    Pm[::4, O.P_TT] = Pm[::4, O.P_HH] * 2.0 ** -41       # below the floor: the rotated partner
    Pm[::8, O.P_RR] = 0.0                                  # ... which has no length in every second of those
    Pm[1, O.P_TT], Pm[2, O.P_NN], Pm[3, O.P_TT] = NAN, 0.0, 0.0
    coef, resid, branch = H.partner(Pm, np.zeros((G, 10), np.float32))
    seen = set()
    for d in range(G):
        br, c, rs = O.partner_coef(Pm[d])
        seen.add(br)
        assert branch[d] == br and (_bits32(coef[d, 7:]) == _bits32(c)).all(), (d, coef[d], c)
        assert _bits64(resid[d]) == _bits64(rs) or (math.isnan(rs) and math.isnan(resid[d])), d
    assert seen == {O.RESIDUAL, O.ROTATED, O.NONE}
    assert H.partner(Pm, np.zeros((G, 10), np.float32), has_free=False)[2].tolist() == [O.NONE] * G
    # the controller: FIRE unchanged, convergence only with C < 0, translate = 0 touches nothing, no free atom converges at once
    fs = np.array([[0.5, 2.0, 0.3, 1e-8], [0.5, 2.0, 0.3, 1e-8], [-0.5, 2.0, 0.3, 1.0], [0.0, 0.0, 0.0, 0.0], [NAN, 1.0, 1.0, 1.0]])
    Cp = np.array([[-1.0, 0], [1.0, 0], [-1.0, 0], [0.0, 0], [-1.0, 0]])
    for translate, has_free in ((1, True), (0, True), (1, False), (0, False)):
        state = (np.full(5, 0.1), np.full(5, 0.1), np.zeros(5, np.int32), np.full(5, -1, np.int64))
        new, fcoef, ret = H.fire_control(state, fs, Cp, translate, has_free, 7, P)
        for d in range(5):
            s = dict(dt=0.1, alpha=0.1, n_pos=0, converged_at=-1)
            r, c = O.fire(s, P, fs[d], Cp[d, 0], translate, has_free, 7)
            assert ret[d] == r and (_bits32(fcoef[d]) == _bits32(c)).all(), (translate, has_free, d)
            assert (new[0][d], new[1][d], new[2][d], new[3][d]) == (s["dt"], s["alpha"], s["n_pos"], s["converged_at"])
        if translate and has_free:
            assert new[3].tolist() == [7, -1, -1, -1, -1] and ret.tolist() == [MO.FROZEN, MO.MOVING, MO.MOVING, MO.MOVING, MO.UNUSABLE]
        if not translate and has_free:
            assert (new[3] == -1).all() and (fcoef == 0).all() and (new[0] == 0.1).all() and ret[4] == MO.UNUSABLE


# ---- 2. the per-atom operations ----------------------------------------------------------------------------------------------------------
def test_per_atom_operations_are_single_rounded():
    """numpy fp32 rounds every operation: the header's terms, N', T, F_eff, the partner terms, the accept and the move bit for bit"""
    rng = np.random.default_rng(13)
    G, n = 3, 50
    N = rng.normal(size=(G, n, 3)).astype(np.float32)
    M = rng.normal(size=(G, n, 3)).astype(np.float32)
    f = (3 * rng.normal(size=(G, 3, n, 3))).astype(np.float32)
    f[:, 1:] = f[:, :1] + (0.03 * rng.normal(size=(G, 2, n, 3))).astype(np.float32)
    fixed = (rng.uniform(size=n) < 0.15).astype(np.uint8)
    still = (fixed != 0)[None, :, None]
    inv, dl = np.float32(1.0 / DELTA), np.float32(DELTA)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    hn, hm = (f[:, 0] - f[:, 1]) * inv, (f[:, 0] - f[:, 2]) * inv
    ref = np.stack([dot(N, hn), dot(N, hm), dot(M, hn), dot(M, hm), dot(f[:, 0], N), dot(f[:, 0], M),
                    (dot(f[:, 0], f[:, 0]) + dot(f[:, 1], f[:, 1])) + dot(f[:, 2], f[:, 2])], -1)
    ref = np.where(still, np.float32(0), ref).astype(np.float32)
    t7 = H.sum_terms(N, M, f, DELTA, fixed)
    assert (_bits32(t7) == _bits32(ref)).all() and (H.sum_terms(N, M, f, DELTA)[:, fixed != 0] != 0).any()
    S = H.sums(N, M, f, DELTA, fixed)
    for d in range(G):
        exact = np.array([math.fsum(t7[d, :, k].astype(np.float64)) for k in range(7)])
        assert np.abs(S[d, :7] - exact).max() <= 1e-12 * np.abs(t7[d].astype(np.float64)).sum() and S[d, 7] == (fixed == 0).sum()
    coef = np.zeros((G, 10), np.float32)
    coef[:, :7] = rng.uniform(-1, 1, size=(G, 7)).astype(np.float32)
    coef[:, O.C_K0] = [1, 0, 1]
    coef[:, 7:] = rng.uniform(-2, 2, size=(G, 3)).astype(np.float32)
    c = lambda k: coef[:, k, None, None]
    np_, t, fe, terms = H.project(N, M, f, DELTA, coef, fixed)
    np_ref = c(O.C_CN) * N + c(O.C_SN) * M
    hp = c(O.C_CN) * hn + c(O.C_SN) * hm
    r = (-c(O.C_SI)) * N + c(O.C_CO) * M
    t_ref = hp + (-(c(O.C_CC) * np_ref))
    fe_ref = c(O.C_K0) * f[:, 0] + c(O.C_E) * np_ref
    terms_ref = np.stack([dot(t_ref, t_ref), dot(t_ref, np_ref), dot(np_ref, np_ref), dot(r, r), dot(r, np_ref), dot(hp, hp)], -1)
    assert (_bits32(np_) == _bits32(np.where(still, np.float32(0), np_ref))).all()
    assert (_bits32(t) == _bits32(np.where(still, np.float32(0), t_ref))).all()
    assert (_bits32(fe) == _bits32(np.where(still, f[:, 0], fe_ref))).all()
    assert (_bits32(terms) == _bits32(np.where(still, np.float32(0), terms_ref))).all()
    assert (fe[1][fixed == 0] == (coef[1, O.C_E] * np_ref[1])[fixed == 0]).all()  # the convex rule has no F0 in it
    # the accept and the move: dimer 1 frozen, fixed atoms keep x bit for bit and get v = 0, images 1 and 2 rewritten
    pos = (4 * rng.normal(size=(G, 3, n, 3))).astype(np.float32)
    vel = (0.05 * rng.normal(size=(G, n, 3))).astype(np.float32)
    fcoef = rng.uniform(0.1, 1.0, size=(G, 3)).astype(np.float32)
    frozen = np.array([0, 1, 0], np.uint8)
    accept = np.array([1, 0, 1], np.uint8)
    x2, v2, N2, M2 = H.atoms(accept, 1, frozen, 1, DELTA, coef, fcoef, np_, t, fe, pos, vel, N, M, fixed)
    m_ref = (c(O.C_MT) * t + c(O.C_MR) * r) + c(O.C_MN) * np_
    acc = (accept != 0)[:, None, None]
    N_ref = np.where(acc, np.where(still, np.float32(0), np_), N)
    M_ref = np.where(acc, np.where(still, np.float32(0), m_ref), M)
    stop = still | (frozen != 0)[:, None, None]
    fc = fcoef[:, None, :]
    v_ref = np.where(stop, np.float32(0), fc[..., 0:1] * vel + fc[..., 1:2] * fe)
    x0_ref = np.where(stop, pos[:, 0], pos[:, 0] + fc[..., 2:3] * v_ref)
    assert (_bits32(N2) == _bits32(N_ref)).all() and (_bits32(M2) == _bits32(M_ref)).all()
    assert (_bits32(v2) == _bits32(v_ref)).all() and (_bits32(x2[:, 0]) == _bits32(x0_ref)).all()
    assert (_bits32(x2[:, 1]) == _bits32(x0_ref + dl * N_ref)).all() and (_bits32(x2[:, 2]) == _bits32(x0_ref + dl * M_ref)).all()
    assert (x2[0, 0][fixed == 0] != pos[0, 0][fixed == 0]).any() and (_bits32(x2[1, 0]) == _bits32(pos[1, 0])).all()
    x3, v3, _, _ = H.atoms(accept, 1, frozen, 0, DELTA, coef, fcoef, np_, t, fe, pos, vel, N, M, fixed)  # translate = 0
    assert (_bits32(x3[:, 0]) == _bits32(pos[:, 0])).all() and (v3 == 0).all() and (_bits32(x3[:, 1]) == _bits32(pos[:, 0] + dl * N_ref)).all()
    # the FIRE sums are tn_min's terms on F_eff, the partner sums the terms above
    fs, Pm = H.part_sums(vel, fe, terms, fixed)
    free = fixed == 0
    for d in range(G):
        tt = np.stack([dot(fe[d], vel[d]), dot(fe[d], fe[d]), dot(vel[d], vel[d])], -1).astype(np.float64)[free]
        assert np.abs(fs[d, :3] - tt.sum(0)).max() <= 1e-12 * np.abs(tt).sum() and fs[d, 3] == tt[:, 1].max()
        assert np.abs(Pm[d] - terms[d].astype(np.float64).sum(0)).max() <= 1e-12 * np.abs(terms[d]).sum()


# ---- 3. whole searches on the analytic surface -----------------------------------------------------------------------------------------------
CONCAVE, CONVEX = (0.4, 0.3, 0.1), (0.9, 0.1, 0.05)
# steps to convergence found, delta = 0.01, fmax = 1e-3 - the fp32 header and the fp64 oracle agree on every one
STEPS = {(1, CONCAVE, 0): 63, (3, CONCAVE, 0): 68, (3, CONCAVE, 1): 63, (3, CONCAVE, 2): 67, (3, CONCAVE, 3): 55, (3, CONCAVE, 4): 67,
         (3, CONCAVE, 5): 56, (40, CONCAVE, 0): 65, (1, CONVEX, 0): 67}


def _start(n, start, seed, fixed=None, mode=None):
    x0, sites = O.problem(n, start, seed)
    N, M = O.orthonormal(mode, fixed, seed, n)
    N, M = N.astype(np.float32), M.astype(np.float32)
    return x0, N, M, sites


@pytest.mark.parametrize("n,start,seed", sorted(STEPS))
def test_dimer_finds_the_saddle_in_fp32_and_fp64(n, start, seed):
    """The surface of tests/neb_oracle.py (the saddle of atom 0 at (0, A, 0), E = 1, curvature -4 along x) from ONE state and a random
    axis: the concave start for n = 1, 3 (six seeds) and 40, and for n = 1 the convex start, which exercises -p N'.  (Convex starts with
    n >= 3 are left out on purpose: the wells of atoms j >= 1, curvature kappa = 2, are then the lowest mode and the method climbs them
    without end - a property of minimum-mode following, not of this code.)  The header's fp32 run and the fp64 oracle converge at the
    same step; atom 0 ends within position_bound of the saddle, |E - 1| within barrier_bound, |N'_x| of atom 0 > 0.999, and |C + 4|
    within curvature_bound for the oracle and within ten times the oracle's own deviation for the fp32 run."""
    x0, N, M, sites = _start(n, start, seed)
    r32 = H.run(O.images(x0, N, M, DELTA)[None], N[None], M[None], sites, NO.KAPPA, NO.A, P, DELTA, 1, 400)
    r64 = O.run(x0, N, M, sites, P, DELTA, 1, 400)
    d32 = np.abs(r32["pos"][0, 0, 0].astype(np.float64) - NO.SADDLE).max()
    d64 = np.abs(r64["x"][0] - NO.SADDLE).max()
    e32, e64 = float(r32["e"][0, 0]) - 1.0, r64["e"] - 1.0
    c32, c64 = abs(r32["C"][0] + 4.0), abs(r64["C"][-1] + 4.0)
    print(f"n = {n} start {start} seed {seed}: steps {r32['steps']} / {r64['steps']}, distance {d32:.3e} / {d64:.3e} (bound "
          f"{NO.position_bound(n, P['fmax']):.3e}), E - 1 = {e32:.3e} / {e64:.3e} (bound {NO.barrier_bound(n, P['fmax']):.3e}), "
          f"|C + 4| = {c32:.3e} / {c64:.3e} (bound {O.curvature_bound(n, P['fmax'], DELTA):.3e}), |T| = {r32['resid'][0]:.3e}")
    assert 0 < r32["steps"] < 400 and r32["conv"][0] == r32["steps"] and r64["conv"] == r64["steps"]
    assert r32["steps"] == r64["steps"] == STEPS[(n, start, seed)]
    assert d32 < NO.position_bound(n, P["fmax"]) and d64 < NO.position_bound(n, P["fmax"])
    assert abs(e32) < NO.barrier_bound(n, P["fmax"]) and abs(e64) < NO.barrier_bound(n, P["fmax"])
    assert abs(r32["mode"][0, 0, 0]) > 0.999 and abs(r64["N"][0, 0]) > 0.999
    assert r32["C"][0] < 0 and c64 <= O.curvature_bound(n, P["fmax"], DELTA) and c32 <= 10.0 * c64
    # the images the mirror leaves are the midpoint displaced along the final N and M
    assert (_bits32(r32["pos"][0]) == _bits32(O.images(r32["pos"][0, 0], r32["mode"][0], r32["partner"][0], DELTA))).all()
    if start == CONVEX:
        assert r64["C"][0] > 0  # the run did begin in the convex region


def test_two_dimers_run_as_they_do_alone():
    """one controller per dimer: two dimers of 3 atoms in one call converge at their own steps and end with the bits of their runs alone"""
    x0b, Nb, Mb, sites = _start(3, CONCAVE, 0)  # (the sites are seeded: both dimers live on the surface of seed 0)
    rngb = np.random.default_rng(5)
    Nb2, Mb2 = (t.astype(np.float32) for t in O.orthonormal(rngb.normal(size=(3, 3))))
    xb2 = x0b.copy()
    xb2[0] += np.float32(0.05)
    pair = [(O.images(x0b, Nb, Mb, DELTA), Nb, Mb), (O.images(xb2, Nb2, Mb2, DELTA), Nb2, Mb2)]
    alone = [H.run(p[None], n_[None], m_[None], sites, NO.KAPPA, NO.A, P, DELTA, 1, 400) for p, n_, m_ in pair]
    both = H.run(np.stack([p[0] for p in pair]), np.stack([p[1] for p in pair]), np.stack([p[2] for p in pair]), sites, NO.KAPPA, NO.A, P,
                 DELTA, 1, 400)
    assert alone[0]["steps"] != alone[1]["steps"] and both["conv"].tolist() == [alone[0]["steps"], alone[1]["steps"]]
    assert both["steps"] == max(both["conv"])
    for d in range(2):
        for key in ("pos", "mode", "partner"):
            assert (_bits32(both[key][d]) == _bits32(alone[d][key][0])).all(), (d, key)


# ---- 4. the mode search ------------------------------------------------------------------------------------------------------------------
def test_mode_search_finds_the_lowest_mode_without_moving():
    """translate = 0, n = 7, 20 steps from a random axis: the axis overlaps the lowest eigenvector of a fine central-difference Hessian
    of the surface by > 0.9999; C is within 0.06 of the lowest eigenvalue - the forward difference's bias (delta / 2) d^3 E along the
    mode, about 0.05 here - checked on the oracle first; R0 keeps its bits.  (C need not fall monotonically: the forward difference
    is not a symmetric operator.)"""
    n = 7
    x0, N, M, sites = _start(n, CONCAVE, 0)
    w, V = np.linalg.eigh(O.surface_hessian(x0, sites))
    lam, vec = w[0], V[:, 0]
    r64 = O.run(x0, N, M, sites, P, DELTA, 0, 20)
    r32 = H.run(O.images(x0, N, M, DELTA)[None], N[None], M[None], sites, NO.KAPPA, NO.A, P, DELTA, 0, 20)
    o64 = abs(float(r64["N"].reshape(-1) @ vec))
    o32 = abs(float(r32["mode"][0].astype(np.float64).reshape(-1) @ vec))
    print(f"lowest eigenvalue {lam:.5f}; C {r32['C'][0]:.5f} / {r64['C'][-1]:.5f}; overlap {o32:.6f} / {o64:.6f}")
    assert r64["steps"] == 20 and r64["conv"] == -1 and o64 > 0.9999 and abs(r64["C"][-1] - lam) <= 0.06
    assert r32["steps"] == 20 and r32["conv"][0] == -1 and o32 > 0.9999 and abs(r32["C"][0] - lam) <= 0.06
    assert (_bits32(r32["pos"][0, 0]) == _bits32(x0)).all()
    assert (_bits32(r32["pos"][0]) == _bits32(O.images(x0, r32["mode"][0], r32["partner"][0], DELTA))).all()
    # the same graph then translates: from the found mode the search converges onto the saddle
    r = H.run(r32["pos"], r32["mode"], r32["partner"], sites, NO.KAPPA, NO.A, P, DELTA, 1, 400)
    assert 0 < r["steps"] < 400 and np.abs(r["pos"][0, 0, 0] - NO.SADDLE).max() < NO.position_bound(n, P["fmax"])


# ---- 5. fixed atoms ------------------------------------------------------------------------------------------------------------------------
def test_fixed_atoms_and_unusable_dimers():
    """a fixed atom keeps its bits, and N and M stay zero on it; every atom fixed: the dimer converges as it stands; a zero mode, a NaN
    force and a NaN energy are reported by their causes"""
    n = 3
    fixed = np.array([0, 1, 0], np.uint8)
    x0, N, M, sites = _start(n, CONCAVE, 0, fixed)
    assert (N[1] == 0).all() and (M[1] == 0).all()
    r = H.run(O.images(x0, N, M, DELTA)[None], N[None], M[None], sites, NO.KAPPA, NO.A, P, DELTA, 1, 400, fixed)
    r64 = O.run(x0, N, M, sites, P, DELTA, 1, 400, fixed)
    assert 0 < r["steps"] < 400 and r["steps"] == r64["steps"]
    assert (_bits32(r["pos"][0, :, 1]) == _bits32(x0[1])).all() and (r["mode"][0, 1] == 0).all() and (r["partner"][0, 1] == 0).all()
    assert (r["pos"][0, 0, 2] != x0[2]).any() and np.abs(r["pos"][0, 0, 0] - NO.SADDLE).max() < NO.position_bound(n, P["fmax"])
    every = np.ones(n, np.uint8)
    z = np.zeros((1, n, 3), np.float32)
    pos = np.stack([x0, x0, x0])[None]
    r = H.run(pos, z, z, sites, NO.KAPPA, NO.A, P, DELTA, 1, 400, every)
    assert r["steps"] == 0 and r["conv"].tolist() == [0] and (_bits32(r["pos"]) == _bits32(pos)).all()
    assert O.run(x0, z[0], z[0], sites, P, DELTA, 1, 400, every)["conv"] == 0
    x0, N, M, sites = _start(n, CONCAVE, 0)
    assert H.run(pos, z, M[None], sites, NO.KAPPA, NO.A, P, DELTA, 1, 10)["steps"] == -O.BAD_MODE
    assert O.run(x0, z[0], M, sites, P, DELTA, 1, 10)["cause"] == O.BAD_MODE
    bad = O.images(x0, N, M, DELTA)[None].copy()
    bad[0, 1, 2, 0] = NAN  # a NaN position of image 1: its energy and its forces are NaN - the energy is looked at first
    assert H.run(bad, N[None], M[None], sites, NO.KAPPA, NO.A, P, DELTA, 1, 10)["steps"] == -O.BAD_ENERGY
    S = np.array([[1.0, 0, 0, 1, 0, 0, NAN, 3]])
    assert H.rotation(S, np.zeros((1, 3), np.float32))[0].tolist() == [O.BAD_SUMS]


def test_surface_mirror_equals_the_oracle():
    x0, N, M, sites = _start(5, CONCAVE, 3)
    x = O.images(x0, N, M, DELTA)
    e32, f32 = H.surface(x, sites, NO.KAPPA, NO.A)
    e64, f64 = NO.surface(x, sites)
    assert np.abs(e32 - e64).max() <= 2.0 ** -24 * np.abs(e64).max() and np.abs(f32 - f64).max() <= 2.0 ** -24 * np.abs(f64).max()
    H_ = O.surface_hessian(np.array([NO.SADDLE, sites[1]]), sites[:2])
    assert abs(H_[0, 0] + 4.0) < 1e-6 and abs(np.linalg.eigvalsh(H_)[0] + 4.0) < 1e-6  # the curvature along x at the saddle is -4


# ---- 6. the sanitizers -----------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/dimer_host.hip with its own main, host code only (-Xarch_host -fsanitize=address,undefined): every entry of the mirror on
    heap arrays of exact size.  A report makes the program exit non-zero (-fno-sanitize-recover)."""
    exe = str(tmp_path / "dimer_host_san")
    subprocess.check_call([H.hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DDIMER_HOST_MAIN", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", H.SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "steps" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


# ---- 7. the additive ABI ---------------------------------------------------------------------------------------------------------------
DIMER_ENTRIES = (("tmdnet_dimer_workspace_bytes", 3), ("tmdnet_dimer_reset", 6), ("tmdnet_dimer_advance", 38), ("tmdnet_dimer_status", 3))


def test_header_and_bindings_are_additive():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from torchmdnet_amd import _C

    src = open(_C.__file__).read()
    args_of = lambda name: [" ".join(a.split()) for a in re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")]
    for name, n_args in DIMER_ENTRIES:
        assert len(args_of(name)) == n_args, name
        assert name in _C.declared_symbols() and name + ".argtypes" in src
    for name, n_args in (("tmdnet_min_advance", 29), ("tmdnet_neb_advance", 34), ("tmdnet_md_advance", 22)):  # untouched
        assert len(args_of(name)) == n_args, name
    # the arguments of tmdnet_neb_advance in its order: no n_images, mode and partner after vel, the true forces after forces_keep,
    # delta in place of spring_k, the dimer's rows in place of the band's
    neb = [a.replace("neb_ws", "dimer_ws").replace("n_bands", "n_dimers") for a in args_of("tmdnet_neb_advance")]
    dim = args_of("tmdnet_dimer_advance")
    assert dim[:5] == neb[:5] and dim[5:9] == neb[6:10] and dim[9:11] == ["float* mode", "float* partner"]
    assert dim[11:15] == neb[10:14] and dim[15] == "float* true_forces_keep" and dim[16:24] == neb[14:22]
    assert dim[24] == "double delta" and dim[25:32] == neb[23:30]
    assert dim[32:] == ["double* curvature_log_row", "double* rotation_log_row", "double* residual_log_row", "double* quad_log_row",
                        "double* mode_sums_log_row", "float* mode_coef_log_row"]


def test_library_exports_the_dimer_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10
    for name, n_args in DIMER_ENTRIES:
        assert len(getattr(hip_lib, name).argtypes) == n_args, name
    small, large = C.c_size_t(0), C.c_size_t(0)
    assert hip_lib.tmdnet_dimer_workspace_bytes(64, 1, C.byref(small)) == 0 and small.value >= 256 + 64 * 60
    assert hip_lib.tmdnet_dimer_workspace_bytes(1100, 2, C.byref(large)) == 0 and large.value >= 256 + 2 * 1100 * 60 + 2 * 2 * 18 * 8
    for bad in ((64, 0), (-1, 1), (2 ** 31, 1)):
        assert hip_lib.tmdnet_dimer_workspace_bytes(*bad, C.byref(small)) != 0
    # argument checks happen before anything is enqueued: no device is needed to be refused
    assert hip_lib.tmdnet_dimer_reset(None, None, 0, 0.1, 0.1, 1) == 1
    assert hip_lib.tmdnet_dimer_reset(None, C.c_void_p(256), 0, 0.0, 0.1, 1) == 1
    assert hip_lib.tmdnet_dimer_reset(None, C.c_void_p(256), 0, 0.1, 0.1, 2) == 1


def test_capture_dimer_and_module_signatures():
    from torchmdnet_amd import dimer
    from torchmdnet_amd.models.model import TorchMD_Net

    sig = inspect.signature(TorchMD_Net.capture_dimer).parameters
    assert list(sig)[1:] == ["z", "pos", "mode", "box", "q", "steps_per_replay", "fmax", "delta", "translate", "seed", "fire", "fixed", "warmup"]
    defaults = {k: sig[k].default for k in list(sig)[3:]}
    assert defaults == dict(mode=None, box=None, q=None, steps_per_replay=10, fmax=0.05, delta=0.01, translate=True, seed=0, fire=None,
                            fixed=None, warmup=3)
    for name in ("__call__", "check", "reset", "run"):
        assert callable(getattr(dimer.DeviceDimer, name))
    assert list(inspect.signature(dimer.DeviceDimer.run).parameters)[1:] == ["max_steps", "check_every"]
    assert list(inspect.signature(dimer.DeviceDimer.reset).parameters)[1:] == ["pos", "mode", "translate"]
    import torch

    # the host's orthonormalisation: fp64, zero on fixed atoms, seeded, and a zero mode is refused
    fixed = torch.tensor([0, 1, 0, 0], dtype=torch.uint8)
    N, M = dimer.orthonormal_pair(None, 2, 4, fixed, seed=3)
    assert N.dtype == torch.float32 and tuple(N.shape) == (2, 4, 3) and (N[:, 1] == 0).all() and (M[:, 1] == 0).all()
    for d in range(2):
        nn, mm, nm = (N[d].double() ** 2).sum(), (M[d].double() ** 2).sum(), (N[d].double() * M[d].double()).sum()
        assert abs(nn - 1) < 1e-6 and abs(mm - 1) < 1e-6 and abs(nm) < 1e-6
    assert not torch.equal(N[0], N[1]) and torch.equal(dimer.orthonormal_pair(None, 2, 4, fixed, seed=3)[0], N)
    given = torch.zeros(4, 3)
    given[0, 0] = 2.0
    N1, _ = dimer.orthonormal_pair(given, 1, 4, fixed, seed=0)
    assert N1[0, 0, 0] == 1.0 and float(N1.abs().sum()) == 1.0
    with pytest.raises(ValueError):
        dimer.orthonormal_pair(torch.zeros(4, 3), 1, 4, None, seed=0)
    only_fixed = torch.zeros(4, 3)
    only_fixed[1, 2] = 1.0
    with pytest.raises(ValueError):
        dimer.orthonormal_pair(only_fixed, 1, 4, fixed, seed=0)
