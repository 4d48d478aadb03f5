"""The relaxed coordinate scan without a GPU: torchmd-net_amd/csrc/tn_scan_math.h compiled for the host (tests/scan_host.hip through
tests/scan_host_mirror.py) against the independent fp64 numpy restatement tests/scan_oracle.py, the closed-form relaxed profile of the
analytic surface and scipy's SLSQP."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import min_host_mirror as MH
from tests import min_oracle as MO
from tests import scan_host_mirror as H
from tests import scan_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(MO.FIRE, fmax=1e-3)  # ASE's defaults, the bound of the surface runs
EPS32 = 2.0 ** -24            # half an ulp of 1.0f, the relative error of one fp32 rounding
TORSION = [("torsion", 0, 1, 2, 3)]
DRIVE, TOL, MAX_ITER = [0.1], 1e-10, 16


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def molecule(seed, n=9, scale=1.0, shift=0.0):
    """n atoms in general position, about 1.5 apart along a jittered zig-zag (no CV of neighbouring atoms is degenerate)"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 3))
    for a in range(1, n):
        step = np.array([1.2, 0.8 * (-1) ** a, 0.5 * math.sin(1.3 * a)]) + 0.2 * rng.normal(size=3)
        x[a] = x[a - 1] + scale * step
    return (x + shift).astype(np.float32)


# ---- 0. the oracle itself ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", [("distance", 0, 3), ("angle", 1, 2, 4), ("torsion", 0, 1, 2, 3), ("torsion", 5, 2, 7, 1)])
def test_oracle_gradients_match_central_differences(cv):
    x = molecule(1).astype(np.float64)
    s, g = O.cv_value_grad(cv, x)
    num = np.zeros_like(x)
    h = 1e-6
    for a in range(len(x)):
        for k in range(3):
            xp, xm = x.copy(), x.copy()
            xp[a, k] += h
            xm[a, k] -= h
            num[a, k] = O.diff(cv[0], O.cv_value_grad(cv, xp)[0], O.cv_value_grad(cv, xm)[0]) / (2 * h)
    assert np.abs(g - num).max() < 1e-8


def test_surface_mirror_equals_the_oracle():
    sites = np.arange(18, dtype=np.float64).reshape(6, 3) * 0.7 + 2.0
    x = np.stack([O.chain(phi, 6, sites, 0.1 * k) for k, phi in enumerate((0.3, -2.0, 3.0))]).astype(np.float32)
    e, f = H.surface(x, sites, 2.0)
    for g in range(3):
        E, F = O.surface(x[g].astype(np.float64), sites, 2.0)
        assert abs(float(e[g]) - E) <= ulp32(E) and (np.abs(f[g] - F) <= ulp32(F) + 1e-12).all()


# ---- 1. projection and constraint tables -------------------------------------------------------------------------------------------------
CASES = {
    "one torsion": ([("torsion", 0, 1, 2, 3)], None, 0.0),
    "two torsions about one bond": ([("torsion", 0, 1, 2, 3), ("torsion", 4, 1, 2, 5)], None, 0.0),
    "an angle and a distance inside a torsion": ([("torsion", 0, 1, 2, 3), ("angle", 0, 1, 2), ("distance", 2, 3)], None, 0.0),
    "four coupled CVs": ([("torsion", 0, 1, 2, 3), ("angle", 1, 2, 3), ("distance", 0, 3), ("torsion", 1, 2, 3, 4)], None, 0.0),
    "fixed CV atoms": ([("torsion", 0, 1, 2, 3), ("distance", 3, 6)], [1, 0, 0, 0, 0, 0, 1, 0, 0], 0.0),
    "far from the origin": ([("torsion", 0, 1, 2, 3), ("angle", 2, 3, 4)], None, 100.0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_multipliers_and_projection_against_the_oracle(name):
    cvs, fixed, shift = CASES[name]
    D = len(cvs)
    rng = np.random.default_rng(len(name))
    pos = np.stack([molecule(3, shift=shift), molecule(4, shift=shift)])
    vel = rng.normal(size=pos.shape).astype(np.float32) * 0.1
    frc = rng.normal(size=pos.shape).astype(np.float32)
    out = H.project(cvs, pos, vel, frc, fixed)
    rc, distinct = H.tables(cvs, pos.shape[1])
    assert rc == 0 and list(distinct) == sorted({i for cv in cvs for i in cv[1:]})
    for g in range(2):
        x, F, v = (a[g].astype(np.float64) for a in (pos, frc, vel))
        s, grad, lam, mu = O.multipliers(cvs, x, F, v, fixed)
        assert out["why"][g] == 0
        assert np.abs(out["cv"][g, :D] - s).max() < 1e-12 * max(1.0, abs(shift))
        # the header solves by Cholesky in fp64 and rounds once: one fp32 rounding plus the fp64 solves' conditioning
        gf = grad.reshape(D, -1)
        M = gf @ gf.T
        slack = 1e-13 * np.linalg.cond(M) * max(1.0, abs(shift))
        for got, want in ((out["mult"][g, 0, :D], lam), (out["mult"][g, 1, :D], mu)):
            assert (np.abs(got - want) <= EPS32 * np.abs(want) * 1.0001 + slack * np.abs(want).max() + 1e-30).all()
        # every per-atom operation is single-rounded: the correction is fp32(- sum lambda32 g), the projection one fp32 sum
        for h, (u, key) in enumerate(((frc, "fperp"), (vel, "vperp"))):
            c64 = -np.tensordot(out["mult"][g, h, :D].astype(np.float64), grad, 1)
            corr = np.zeros_like(pos[g])
            corr[distinct] = out["corr"][g, :len(distinct), h]
            assert (np.abs(corr - c64) <= ulp32(c64) * 0.5001 + 1e-13 * max(1.0, abs(shift))).all()
            assert np.array_equal(out[key][g], u[g] + corr)  # (numpy adds two fp32 arrays with one rounding)
            others = np.setdiff1d(np.arange(pos.shape[1]), distinct)
            assert np.array_equal(out[key][g][others], u[g][others])
            if fixed is not None:
                still = np.flatnonzero(fixed)
                assert np.array_equal(out[key][g][still], u[g][still])
            # g_d . u_perp = 0 up to the three fp32 roundings: of the multiplier, of the correction and of the sum
            up = out[key][g].astype(np.float64)
            coef = np.abs(out["mult"][g, h, :D].astype(np.float64))
            bound = EPS32 * (np.abs(M) @ coef + (np.abs(gf) * (np.abs(corr.astype(np.float64)) + np.abs(up)).reshape(-1)).sum(1)) * 1.01
            resid = gf @ up.reshape(-1)
            assert (np.abs(resid) <= bound + slack * np.abs(coef).max() * np.abs(M).max()).all(), (name, resid, bound)
            assert np.abs(out["gdot"][g, h, :D] - resid).max() < 1e-12
        # the sums: fp32 terms (tests/min_host_mirror's contract) widened and added
        free = np.ones(pos.shape[1], bool) if fixed is None else np.asarray(fixed) == 0
        fp, vp = out["fperp"][g].astype(np.float64)[free], out["vperp"][g].astype(np.float64)[free]
        want = np.array([(vp * fp).sum(), (fp * fp).sum(), (vp * vp).sum(), (fp * fp).sum(1).max()])
        assert np.allclose(out["sums"][g], want, rtol=1e-6, atol=1e-9)


def test_move_is_single_rounded_and_frozen_points_keep_their_bits():
    rng = np.random.default_rng(5)
    pos, vel, f = (rng.normal(size=(2, 6, 3)).astype(np.float32) for _ in range(3))
    coef = np.array([[0.9, 0.31, 0.17], [0.5, 0.2, 0.1]], np.float32)
    fixed = np.array([0, 0, 1, 0, 0, 0], np.uint8)
    x2, v2 = H.move(np.array([-1, 7]), coef, pos, vel, f, fixed)
    v_want = coef[0, 0] * vel[0] + coef[0, 1] * f[0]  # (fp32 numpy: every product and sum rounded once)
    x_want = pos[0] + coef[0, 2] * v_want
    free = fixed == 0
    assert np.array_equal(v2[0][free], v_want[free]) and np.array_equal(x2[0][free], x_want[free])
    assert np.array_equal(x2[0][~free], pos[0][~free]) and (v2[0][~free] == 0).all()
    assert np.array_equal(x2[1], pos[1]) and (v2[1] == 0).all()


def test_constraint_step_reaches_the_target_and_writes_only_cv_atoms():
    cvs = [("torsion", 0, 1, 2, 3), ("distance", 3, 6)]
    fixed = np.array([1, 0, 0, 0, 0, 0, 0, 0, 0], np.uint8)
    for shift in (0.0, 100.0):
        pos = np.stack([molecule(3, shift=shift), molecule(4, shift=shift)])
        s0 = np.array([O.cv_all(cvs, p.astype(np.float64))[0] for p in pos])
        t_cur = np.zeros((2, 4))
        t_cur[:, :2] = s0
        t_fin = s0 + np.array([[0.5, -0.2], [0.04, 0.3]])
        new, t_new, why2, iters = H.constrain(cvs, pos, np.array([-1, -1]), t_cur, t_fin, [0.1, 0.05], 1e-10, 16, fixed)
        assert (why2 == 0).all() and (iters >= 1).all() and (iters <= 6).all()
        assert np.allclose(t_new[:, :2], s0 + np.array([[0.1, -0.05], [0.04, 0.05]]), atol=1e-15) and t_new[1, 0] == t_fin[1, 0]
        moved = [1, 2, 3, 6]
        rest = np.setdiff1d(np.arange(9), moved)
        assert np.array_equal(new[:, rest], pos[:, rest]) and not np.array_equal(new[:, moved], pos[:, moved])
        for g in range(2):
            x_or, it_or = O.constrain(cvs, pos[g].astype(np.float64), t_new[g, :2], 1e-10, 16, fixed)
            assert it_or == iters[g] and np.array_equal(new[g], x_or.astype(np.float32))
            s = O.cv_all(cvs, new[g].astype(np.float64))[0]
            # after the fp32 rounding: the CV moves by at most |g|_1 times half an ulp of the coordinates
            _, grad = O.cv_all(cvs, new[g].astype(np.float64), fixed)
            bound = (np.abs(grad) * ulp32(new[g])[None] * 0.5).sum((1, 2)) + 1e-10
            assert (np.abs(s - t_new[g, :2]) <= bound).all()
        frozen, t_same, _, _ = H.constrain(cvs, pos, np.array([3, -1]), t_cur, t_fin, [0.1, 0.05], 1e-10, 16, fixed)
        assert np.array_equal(frozen[0], pos[0]) and np.array_equal(t_same[0], t_cur[0])


def test_every_cause_of_an_unusable_point():
    pos = molecule(3)[None]
    zero = np.zeros_like(pos)
    f = np.ones_like(pos)
    assert H.project([("torsion", 0, 1, 2, 3), ("torsion", 0, 1, 2, 3)], pos, zero, f)["why"][0] == 3  # two identical CVs
    line = pos.copy()
    line[0, :4] = [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0.5]]
    assert H.project(TORSION, line, zero, f)["why"][0] == 2  # a collinear torsion
    nan = pos.copy()
    nan[0, 2, 1] = np.nan
    assert H.project(TORSION, nan, zero, f)["why"][0] == 2  # NaN input
    assert H.project(TORSION, pos, zero, f, np.array([1, 1, 1, 1, 0, 0, 0, 0, 0], np.uint8))["why"][0] == 3  # every CV atom fixed
    start = O.chain(1.0)[None].astype(np.float32)
    assert H.run(TORSION, start, [[2.0]], DRIVE, TOL, 1, P, 50)["steps"] == -4  # one correction cannot reach 1e-10
    assert H.run(TORSION, start, [[2.0]], DRIVE, TOL, MAX_ITER, P, 500)["steps"] > 0
    bad = start.copy()
    bad[0, 0, 0] = np.inf  # a position that is not finite: the CV is not
    assert H.run(TORSION, bad, [[2.0]], DRIVE, TOL, MAX_ITER, P, 50)["steps"] == -2
    # a force that is not finite at finite positions is cause 1: on a CV atom through the multiplier, elsewhere through the sums
    nine = np.stack([molecule(3), molecule(4)])
    v9, f9 = np.zeros_like(nine), np.ones_like(nine)
    f9[1, 2, 1] = np.nan
    out = H.project(TORSION, nine, v9, f9)
    assert list(out["why"]) == [0, 1]
    f9 = np.ones_like(nine)
    f9[1, 7, 0] = np.inf
    out = H.project(TORSION, nine, v9, f9)
    assert list(out["why"]) == [0, 0] and np.isfinite(out["sums"][0]).all() and not np.isfinite(out["sums"][1]).all()
    state = (np.full(2, P["dt"]), np.full(2, P["alpha"]), np.zeros(2, np.int32), np.full(2, -1, np.int64))
    t = np.zeros((2, 4))
    after, coef, ret = H.control(state, out["sums"], t, np.ones((2, 1)), 3, P)
    assert list(ret) == [MO.MOVING, MO.UNUSABLE] and (coef[1] == 0).all() and after[0][1] == state[0][1] and after[3][1] == -1
    for cvs in ([], [("distance", 0, 1)] * 5, [("distance", 0, 0)], [("angle", 0, 1, 9)], [("torsion", 0, 1, 2, -1)]):
        assert H.tables(cvs, 9)[0] == 1


@pytest.mark.parametrize("n", [9, 300, 1100, 2500])
def test_sums_in_the_devices_order_of_addition(n):
    """the restatement of the device's reduction (slices, 256 strided threads, the xor tree of a wave, waves and slices in turn): the
    maximum is exact, the three sums lie within the reordering error of n fp64 additions of the plain sum in atom order, and for a
    point that fits one thread each (n <= 256, one slice) the tree is checked by hand against pairwise halving"""
    rng = np.random.default_rng(n)
    f, v = (rng.normal(size=(2, n, 3)).astype(np.float32) for _ in range(2))
    fixed = (rng.random(n) < 0.2).astype(np.uint8)
    assert H.slices(n) == (1 if n <= 1024 else (n + 1023) // 1024)
    tree = H.tree_sums(f, v, fixed)
    terms = np.stack([MH.terms(v[g], f[g], fixed) for g in range(2)]).astype(np.float64)  # the fp32 terms v.f, f.f, v.v; zero on fixed atoms
    assert np.array_equal(tree[:, 3], terms[:, :, 1].max(1))
    assert (np.abs(tree[:, :3] - terms.sum(1)) <= n * 2.0 ** -52 * np.abs(terms).sum(1)).all()
    if n <= 256:
        t = np.zeros((256, 3))
        t[:n] = terms[0]
        w = t.reshape(4, 64, 3)
        for o in (1, 2, 4, 8, 16, 32):
            w = w + w[:, np.arange(64) ^ o]
        want = ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]
        assert np.array_equal(tree[0, :3], want)


def test_torsion_drive_takes_the_short_way_round():
    t, seen = -math.pi + 0.1, []
    for _ in range(3):
        t_or = O.drive("torsion", math.pi - 0.1, t, 0.1)
        t = H.drive("torsion", math.pi - 0.1, t, 0.1)
        assert abs(t - t_or) < 1e-15
        seen.append(t)
    assert abs(abs(seen[0]) - math.pi) < 1e-12 and seen[1] == math.pi - 0.1 and seen[2] == math.pi - 0.1  # two steps, not sixty
    assert H.drive("distance", 2.0, 1.0, 0.05) == 1.05 and H.drive("distance", 1.0, 1.02, 0.05) == 1.0
    assert H.drive("angle", 1.0, 2.0, 0.1) == 1.9


# ---- 2. whole scans on the analytic surface ----------------------------------------------------------------------------------------------
TARGETS = np.linspace(-math.pi + 0.01, 3.0, 8)
_SCANS = {}


def scans():
    """the eight-target scan from one start geometry: the header in fp32 storage, the oracle in fp64 and with fp32 storage (made once)"""
    if not _SCANS:
        x0 = O.chain(1.0)
        _SCANS["x0"] = x0
        _SCANS["host"] = H.run(TORSION, np.repeat(x0[None], 8, 0), TARGETS[:, None], DRIVE, TOL, MAX_ITER, P, 2000)
        _SCANS["o64"] = [O.run(TORSION, x0, [t], DRIVE, TOL, MAX_ITER, P, 2000) for t in TARGETS]
        _SCANS["o32"] = [O.run(TORSION, x0, [t], DRIVE, TOL, MAX_ITER, P, 2000, store32=True) for t in TARGETS]
    return _SCANS


def test_scan_reproduces_the_closed_form_relaxed_profile():
    """Measured with the header (fp32 storage) on these eight targets: steps 59...91, identical in all three runs; |E - E*| <= 1.6e-7;
    |lambda + dE*/dphi| <= 3.3e-4 (header and oracle alike); |s - t| <= 5.7e-8 after the fp32 rounding."""
    S = scans()
    host, E_star, dE_star = S["host"], *O.relaxed_energy(TARGETS)
    assert host["steps"] == max(host["conv"]) and (host["conv"] > 0).all()
    worst = dict(E=0.0, lam_oracle=0.0, lam_host=0.0, cv=0.0)
    for g, t in enumerate(TARGETS):
        o64, o32 = S["o64"][g], S["o32"][g]
        print(f"target {t:+.4f}: steps host {host['conv'][g]} oracle {o64['converged_at']} oracle/fp32 {o32['converged_at']}  "
              f"|E-E*| {abs(float(host['e'][g]) - E_star[g]):.2e}  |lam+dE*| host {abs(float(host['lam'][g, 0]) + dE_star[g]):.2e} "
              f"oracle {abs(o64['lam'][0] + dE_star[g]):.2e}  |s-t| {abs(host['cv'][g, 0] - t):.2e}")
        assert host["conv"][g] == o64["converged_at"] == o32["converged_at"]
        assert host["target"][g, 0] == t and o64["target"][0] == t
        worst["E"] = max(worst["E"], abs(float(host["e"][g]) - E_star[g]), abs(o64["E"] - E_star[g]))
        worst["lam_oracle"] = max(worst["lam_oracle"], abs(o64["lam"][0] + dE_star[g]))
        worst["lam_host"] = max(worst["lam_host"], abs(float(host["lam"][g, 0]) + dE_star[g]))
        worst["cv"] = max(worst["cv"], abs(host["cv"][g, 0] - t))
        assert float(host["fmax"][g]) < P["fmax"]
    print(worst)
    assert worst["E"] <= 1e-6
    assert worst["lam_oracle"] <= 3e-3
    assert worst["lam_host"] <= 3e-3 + 1e-4
    # |x| <= 3: half an ulp of a coordinate is at most 2^-23, and the torsion's gradient has an L1 norm below 4 here
    assert worst["cv"] <= 4 * 2.0 ** -23


@pytest.mark.parametrize("g", [2, 6])
def test_scan_agrees_with_slsqp(g):
    """an independent solver of the same constrained minimum: scipy's SLSQP from the scan's end point, in fp64"""
    from scipy.optimize import minimize

    t = TARGETS[g]
    host = scans()["host"]
    x0 = host["pos"][g].astype(np.float64).reshape(-1)
    energy = lambda x: O.surface(x.reshape(4, 3))[0]
    grad = lambda x: -O.surface(x.reshape(4, 3))[1].reshape(-1)
    cons = dict(type="eq", fun=lambda x: O.diff("torsion", O.cv_value_grad(TORSION[0], x.reshape(4, 3))[0], t),
                jac=lambda x: O.cv_value_grad(TORSION[0], x.reshape(4, 3))[1].reshape(-1))
    res = minimize(energy, x0, jac=grad, constraints=[cons], method="SLSQP", options=dict(ftol=1e-14, maxiter=500))
    assert res.success and abs(res.fun - O.relaxed_energy(t)[0]) < 1e-9
    assert abs(float(host["e"][g]) - res.fun) <= 1e-6


def test_two_points_of_forty_atoms_freeze_at_different_steps_and_end_as_they_do_alone():
    n = 40
    rng = np.random.default_rng(7)
    sites = rng.uniform(4.0, 12.0, size=(n, 3))
    cvs = [("torsion", 0, 1, 2, 3), ("distance", 1, 2)]
    x0 = np.stack([O.chain(1.0, n, sites, 0.02), O.chain(1.0, n, sites, 0.5)]).astype(np.float32)
    t_fin = np.array([[1.3, 1.52], [2.4, 1.45]])
    drive = [0.1, 0.05]
    both = H.run(cvs, x0, t_fin, drive, TOL, MAX_ITER, P, 3000, sites, 2.0)
    assert (both["conv"] > 0).all() and both["conv"][0] != both["conv"][1] and both["steps"] == both["conv"].max()
    for g in range(2):
        alone = H.run(cvs, x0[g:g + 1], t_fin[g:g + 1], drive, TOL, MAX_ITER, P, 3000, sites, 2.0)
        assert alone["conv"][0] == both["conv"][g] and np.array_equal(alone["pos"][0], both["pos"][g])
        assert alone["e"][0] == both["e"][g] and np.array_equal(alone["lam"][0], both["lam"][g])
        o = O.run(cvs, x0[g].astype(np.float64), t_fin[g], drive, TOL, MAX_ITER, P, 3000, sites, 2.0, store32=True)
        assert o["converged_at"] == both["conv"][g]
        assert np.abs(both["cv"][g] - t_fin[g]).max() <= 4 * 2.0 ** -23 * 4  # coordinates of the chain below 4


# ---- 3. the sanitizers -------------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/scan_host.hip with its own main, host code only (-fsanitize=address,undefined): whole scans, fixed atoms and the causes on
    heap arrays of exact size.  A report makes the program exit non-zero (-fno-sanitize-recover)."""
    exe = str(tmp_path / "scan_host_san")
    subprocess.check_call([H.hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DSCAN_HOST_MAIN", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", H.SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "scan_host: ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


# ---- 4. the additive ABI -----------------------------------------------------------------------------------------------------------------
SCAN_ENTRIES = (("tmdnet_scan_workspace_bytes", 3), ("tmdnet_scan_reset", 7), ("tmdnet_scan_advance", 42), ("tmdnet_scan_status", 3))


def test_header_and_bindings_are_additive():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from torchmdnet_amd import _C

    src = open(_C.__file__).read()
    args_of = lambda name: [" ".join(a.split()) for a in re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")]
    for name, n_args in SCAN_ENTRIES:
        assert len(args_of(name)) == n_args, name
        assert name in _C.declared_symbols() and name + ".argtypes" in src
    for name, n_args in (("tmdnet_min_advance", 29), ("tmdnet_neb_advance", 34), ("tmdnet_dimer_advance", 38)):  # untouched
        assert len(args_of(name)) == n_args, name
    # the minimiser's arguments in its order around the scan's own
    mn, sc = args_of("tmdnet_min_advance"), args_of("tmdnet_scan_advance")
    assert sc[0:3] == mn[0:3] and sc[6:12] == mn[6:12] and sc[21:36] == mn[14:29]


def test_library_exports_the_scan_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10
    for name, n_args in SCAN_ENTRIES:
        assert len(getattr(hip_lib, name).argtypes) == n_args, name
    small, large = C.c_size_t(0), C.c_size_t(0)
    assert hip_lib.tmdnet_scan_workspace_bytes(64, 1, C.byref(small)) == 0 and small.value >= 256 + 64 * 24
    assert hip_lib.tmdnet_scan_workspace_bytes(1100, 2, C.byref(large)) == 0 and large.value >= 256 + 2 * 1100 * 24 + 2 * 2 * 4 * 8
    for bad in ((64, 0), (0, 1), (-1, 1), (2 ** 31, 1)):
        assert hip_lib.tmdnet_scan_workspace_bytes(*bad, C.byref(small)) != 0
    # argument checks happen before anything is enqueued: no device is needed to be refused
    assert hip_lib.tmdnet_scan_reset(None, None, 4, 1, 0, 0.1, 0.1) == 1
    assert hip_lib.tmdnet_scan_reset(None, C.c_void_p(256), 4, 1, 0, 0.0, 0.1) == 1
    assert hip_lib.tmdnet_scan_reset(None, C.c_void_p(256), 0, 1, 0, 0.1, 0.1) == 1


def test_capture_scan_and_module_signatures():
    import torch

    from torchmdnet_amd import scan
    from torchmdnet_amd.models.model import TorchMD_Net

    sig = inspect.signature(TorchMD_Net.capture_scan).parameters
    assert list(sig)[1:] == ["z", "pos", "cvs", "targets", "box", "q", "steps_per_replay", "fmax", "drive", "tol", "max_iter", "fire", "fixed",
                             "warmup"]
    defaults = {k: sig[k].default for k in list(sig)[5:]}
    assert defaults == dict(box=None, q=None, steps_per_replay=10, fmax=0.05, drive=None, tol=1e-8, max_iter=16, fire=None, fixed=None, warmup=3)
    for name in ("__call__", "check", "reset", "run", "profile"):
        assert callable(getattr(scan.DeviceScan, name))
    assert list(inspect.signature(scan.DeviceScan.reset).parameters)[1:] == ["pos", "targets"]
    g = scan.grid(-3.0, 3.0, 24)
    assert g.dtype == torch.float64 and tuple(g.shape) == (24, 1) and g[0, 0] == -3.0 and g[-1, 0] == 3.0
    kinds, atoms, distinct = scan.parse_cvs([("torsion", 4, 1, 2, 3), ("distance", 2, 7)], 9)
    assert kinds == [2, 0] and atoms == [[4, 1, 2, 3], [2, 7, -1, -1]] and distinct == [1, 2, 3, 4, 7]
    assert list(H.tables([("torsion", 4, 1, 2, 3), ("distance", 2, 7)], 9)[1]) == distinct  # the C entry builds the same table
    assert scan.parse_drive(None, kinds) == [0.1, 0.05] and scan.parse_drive(0.2, kinds) == [0.2, 0.2]
    fixed = torch.tensor([0, 1, 1, 0, 0, 0, 0, 0, 0])
    for bad in ([], [("distance", 0, 1)] * 5, [("bond", 0, 1)], [("angle", 0, 1)], [("distance", 0, 9)], [("torsion", 0, 1, 2, 1)],
                [("distance", 1, 2)]):
        with pytest.raises(ValueError):
            scan.parse_cvs(bad, 9, fixed)
    for bad in (0.0, -0.1, [0.1, 0.1, 0.1], float("nan")):
        with pytest.raises(ValueError):
            scan.parse_drive(bad, kinds)
