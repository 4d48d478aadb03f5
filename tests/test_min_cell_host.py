"""No GPU: the cell relaxation of the device-resident FIRE minimiser (the tn_min::cell_* statements of csrc/tn_min_math.h, compiled
host-only by tests/min_cell_host_mirror.py) against tests/min_cell_oracle.py - the scheme in fp64 Python floats, written from the
equations.  1. the generalised forces against finite differences of E + p V on a spring crystal, 2. the same through the fp64
TensorNet oracle, 3. the controller table, 4. a whole relaxation in both precisions, 5. the sanitizers, 6. signatures and exports."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import min_cell_host_mirror as H
from tests import min_cell_oracle as CO
from tests import min_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(O.FIRE)  # ASE's defaults, fmax = 0.05
NAN = float("nan")
ONES = [[1.0] * 3] * 3
OPTIONS = [dict(), dict(hydrostatic=True), dict(constant_volume=True), dict(mask=[[1, 0, 0], [0, 1, 0], [0, 0, 0]]),
           dict(mask=[[0, 1, 1], [1, 0, 1], [1, 1, 0]]), dict(mask=[[1, 1, 0], [1, 0, 0], [0, 0, 1]], constant_volume=True)]


def _cp(pressure=0.0, **kw):
    return dict(CO.CELL, pressure=pressure, **kw)


def _bits64(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _bits32(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _finite_difference(enthalpy, xt, D, h=1e-5):
    """central differences of enthalpy(xt, D) -> (-dH/dxt [N,3], -dH/dD [3,3])"""
    gx, gD = np.zeros_like(xt), np.zeros((3, 3))
    for idx in np.ndindex(*xt.shape):
        e = np.zeros_like(xt)
        e[idx] = h
        gx[idx] = -(enthalpy(xt + e, D) - enthalpy(xt - e, D)) / (2 * h)
    for idx in np.ndindex(3, 3):
        e = np.zeros((3, 3))
        e[idx] = h
        gD[idx] = -(enthalpy(xt, D + e) - enthalpy(xt, D - e)) / (2 * h)
    return gx, gD


# ---- 1. the gradient -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pressure", [0.0, 0.35])
def test_generalised_forces_equal_finite_differences_on_the_spring_crystal(pressure):
    """4-atom fcc of springs in a triclinic box, atoms displaced, D != I and not symmetric.  The oracle's Ft and G against central
    differences (h = 1e-5) of E + p V in xt and D, for every option: the option applied to the finite-difference gradient of all nine
    entries.  Measured discrepancy: 2.5e-10 of max |gradient| (p = 0) and 1.9e-10 (p = 0.35), the largest over the options;
    asserted: ten times the larger, 2.5e-9."""
    rng = np.random.default_rng(11)
    x, H0, bonds = CO.crystal()
    D = np.eye(3) + 0.04 * rng.normal(size=(3, 3))
    xt = x + 0.05 * rng.normal(size=x.shape)
    c = 4.0
    worst = 0.0
    for opt in OPTIONS:
        cp = _cp(pressure, **opt)
        full = _cp(pressure)
        Ft, Gc, _ = CO.generalised_forces(xt, H0, D, bonds, cp, c)
        gx, gD = _finite_difference(lambda a, b: CO.generalised_forces(a, H0, b, bonds, full, c)[2], xt, D)
        scale = max(np.abs(gx).max(), np.abs(gD).max())
        err = max(np.abs(Ft - gx).max(), np.abs(c * Gc - CO.project(gD, cp)).max()) / scale
        print(opt, "discrepancy", err)
        worst = max(worst, err)
        assert np.abs(c * Gc).max() > 1e-2 * scale  # the option left something to compare
    assert worst < 2.5e-9, worst
    # the sign and the transpose, spelled out: a wrong one fails by the size of the gradient itself
    Ft, Gc, _ = CO.generalised_forces(xt, H0, D, bonds, _cp(pressure), c)
    assert np.abs(c * Gc - (c * Gc).T).max() > 1e-2 * np.abs(Gc).max() * c  # G is not symmetric at D != I: the transpose matters


# ---- 2. the model's virial convention ------------------------------------------------------------------------------------------------
def test_generalised_forces_equal_finite_differences_through_the_model(golden_dir):
    """tests/virial_oracle.py's fp64 TensorNet on the triclinic periodic fixture: E, F, W at x = xt D^T, box = H0 D^T give Ft = F D and
    G = (W_s - p V I) D^-T, against central differences of E + p V in xt and D.  Measured: 1.7e-10 of max |gradient|; asserted: ten times that, 1.7e-9."""
    from tests import virial_oracle as VO

    tiny = torch.load(os.path.join(golden_dir, "tiny_ref.pt"))
    f = torch.load(os.path.join(golden_dir, "tiny_pbc_ref.pt"))
    args, sd, z, batch = tiny["args"], tiny["state_dict"], f["z"], f["batch"]
    H0 = f["box"].double().numpy().reshape(3, 3)
    rng = np.random.default_rng(2)
    D = np.eye(3) + 0.02 * rng.normal(size=(3, 3))
    xt = f["pos"].double().numpy() @ np.linalg.inv(D).T
    pressure, c = 0.01, float(len(xt))
    cp = _cp(pressure)

    def evaluate(a, b):
        box = torch.from_numpy(H0 @ b.T)
        E, F, W = VO.energy_forces_virial(args, sd, z, torch.from_numpy(a @ b.T), batch, box)
        return float(E.sum()), F.numpy(), W[0].numpy(), box.numpy()

    E, F, W, box = evaluate(xt, D)
    why, Gc, V, _ = CO.cell_force(W, box, D, cp, c)
    assert why == CO.OK
    gx, gD = _finite_difference(lambda a, b: evaluate(a, b)[0] + pressure * abs(np.linalg.det(H0 @ b.T)), xt, D)
    scale = max(np.abs(gx).max(), np.abs(gD).max())
    err = max(np.abs(F @ D - gx).max(), np.abs(c * np.array(Gc).reshape(3, 3) - gD).max()) / scale
    print("discrepancy", err, "scale", scale)
    assert err < 1.7e-9, err
    assert np.abs(gD).max() > 1e-3 * scale


# ---- 3. the controller table -------------------------------------------------------------------------------------------------------------
def _table():
    """name, FIRE state, the atoms' sums, W, V_D scale, cell options, expected return, expected why"""
    W0 = [[0.9, 0.2, -0.1], [0.3, -0.7, 0.05], [0.0, 0.1, 0.4]]
    big = [[60.0, 5.0, 0.0], [5.0, -40.0, 0.0], [0.0, 0.0, 20.0]]
    small = [[1e-3, 0.0, 0.0], [0.0, -2e-3, 0.0], [0.0, 0.0, 1e-3]]
    moving, idle = (0.3, 2.0, 0.5, 0.4), (0.0, 7.0, 0.0, 1.5)
    rows = [
        ("downhill, n_pos below n_min", (0.1, 0.1, 2, -1), moving, W0, 0.05, {}, O.MOVING, 0),
        ("downhill, n_pos equal to n_min", (0.1, 0.1, 5, -1), moving, W0, 0.05, {}, O.MOVING, 0),
        ("downhill, n_pos above n_min", (0.1, 0.1, 6, -1), moving, W0, 0.05, {}, O.MOVING, 0),
        ("downhill, dt reaches dt_max", (0.95, 0.07, 9, -1), (0.003, 0.02, 0.005, 0.004), small, 0.001, {}, O.MOVING, 0),
        ("uphill through the atoms", (0.4, 0.03, 11, -1), (-0.9, 2.0, 0.5, 0.4), W0, 0.05, {}, O.MOVING, 0),
        ("uphill through the cell rows alone", (0.4, 0.03, 11, -1), (0.001, 2.0, 0.5, 0.4), W0, "against", {}, O.MOVING, 0),
        ("first step: v = 0", (0.1, 0.1, 0, -1), idle, W0, 0.0, {}, O.MOVING, 0),
        ("cell rows dominate fmax", (0.1, 0.1, 2, -1), (0.001, 0.004, 0.002, 0.0024), W0, 0.05, {}, O.MOVING, 0),
        ("clamp triggered by the cell rows alone", (0.5, 0.1, 3, -1), (0.01, 0.1, 0.002, 0.02), big, 0.5, {}, O.MOVING, 0),
        ("clamp inactive", (0.05, 0.1, 3, -1), (0.01, 0.1, 0.002, 0.02), small, 0.001, {}, O.MOVING, 0),
        ("converging now: atoms and cell below fmax", (0.3, 0.08, 4, -1), (0.001, 0.004, 0.002, 0.0024), small, 0.01, {}, O.FROZEN, 0),
        ("already converged", (0.3, 0.08, 4, 17), moving, W0, 0.05, {}, O.FROZEN, 0),
        ("already converged, a NaN virial is not looked at", (0.3, 0.08, 4, 17), moving, [[NAN] * 3] * 3, 0.05, {}, O.FROZEN, 0),
        ("hydrostatic", (0.1, 0.1, 2, -1), moving, W0, 0.05, dict(hydrostatic=True), O.MOVING, 0),
        ("constant volume", (0.1, 0.1, 2, -1), moving, W0, 0.05, dict(constant_volume=True), O.MOVING, 0),
        ("pressure", (0.1, 0.1, 2, -1), moving, W0, 0.05, dict(pressure=0.02), O.MOVING, 0),
        ("mask: xy plane only", (0.1, 0.1, 2, -1), moving, W0, 0.05, dict(mask=[[1, 1, 0], [1, 1, 0], [0, 0, 0]]), O.MOVING, 0),
        ("mask: nothing, the atoms converge", (0.1, 0.1, 2, -1), (0.001, 0.004, 0.002, 0.0024), big, 0.0, dict(mask=[[0] * 3] * 3), O.FROZEN, 0),
        ("hydrostatic under pressure and a mask", (0.1, 0.1, 6, -1), moving, W0, 0.05,
         dict(hydrostatic=True, pressure=0.02, mask=[[1, 0, 0], [0, 1, 0], [0, 0, 0]]), O.MOVING, 0),
        ("NaN in W", (0.1, 0.1, 2, -1), moving, [[0.9, NAN, 0.0], [0.3, -0.7, 0.0], [0.0, 0.1, 0.4]], 0.05, {}, O.UNUSABLE, CO.BAD_VIRIAL),
        ("inf in W, masked entry", (0.1, 0.1, 2, -1), moving, [[0.9, 0.0, 0.0], [0.0, -0.7, 0.0], [0.0, 0.0, float("inf")]], 0.05,
         dict(mask=[[1, 0, 0], [0, 1, 0], [0, 0, 0]]), O.UNUSABLE, CO.BAD_VIRIAL),
        ("NaN atom sum", (0.1, 0.1, 2, -1), (NAN, 2.0, 0.5, 0.4), W0, 0.05, {}, O.UNUSABLE, CO.BAD_SUMS),
        ("zero volume", (0.1, 0.1, 2, -1), moving, W0, 0.05, dict(_box="flat"), O.UNUSABLE, CO.BAD_VOLUME),
        ("the move would leave a box that is not finite", (100.0, 0.1, 2, -1), moving, [[-3e38, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], 0.0,
         dict(_max_step=1e300), O.UNUSABLE, CO.BAD_VOLUME),
    ]
    return rows


def _cell_velocity(vscale, VD0, W32, box, D, cp, c):
    """a number: that multiple of a fixed random V_D; "against": V_D = -2 G / c, so that the cell rows alone make vf negative"""
    if vscale == "against":
        return -2.0 * np.array(CO.cell_force(W32, box, D, cp, c)[1])
    return vscale * VD0


def test_controller_with_cell_rows_equals_the_oracle_bit_for_bit():
    """Every branch of the controller's table with the cell rows in the sums, the cell rows dominating fmax, the clamp triggered by the
    cell rows alone, each option and the unusable inputs, plus random cases.  No transcendental but sqrt, no FMA in the x86-64
    baseline: dt, alpha, n_pos, converged_at, the three fp32 coefficients, the next D and V_D (fp64), D32 and the fp32 box are equal
    bit for bit, and so are G / c, the volume, the stress and the sums."""
    rng = np.random.default_rng(5)
    H0 = np.array([[6.0, 0.0, 0.0], [0.8, 6.5, 0.0], [-0.5, 0.4, 7.0]])
    D = np.eye(3) + 0.03 * rng.normal(size=(3, 3))
    VD0 = rng.normal(size=9)
    cases = _table()
    for i in range(200):
        ff, vv = float(10.0 ** rng.uniform(-4, 2)), float(10.0 ** rng.uniform(-6, 1))
        vf = float(rng.uniform(-1, 1) * math.sqrt(ff * vv))
        st = (float(rng.uniform(0.01, 1.0)), float(rng.uniform(0.001, 0.1)), int(rng.integers(0, 12)), -1)
        opt = [dict(), dict(hydrostatic=True), dict(constant_volume=True), dict(pressure=float(rng.uniform(-0.05, 0.05)))][i % 4]
        cases.append((f"random {i}", st, (vf, ff, vv, ff * float(rng.uniform(0.01, 1.0))), (10.0 ** rng.uniform(-2, 1.5) * rng.normal(size=(3, 3))).tolist(),
                      float(10.0 ** rng.uniform(-3, 0)), opt, None, None))
    step = (3 << 32) + 9
    seen = set()
    for name, st, sums, W, vscale, opt, expect, expect_why in cases:
        opt = dict(opt)
        p = dict(P, max_step=opt.pop("_max_step", P["max_step"]))
        flat = opt.pop("_box", None) == "flat"
        cp = _cp(**opt)
        c = 5.0
        Dm = np.eye(3) if "not finite" in name and "random" not in name else D
        box = (H0 @ Dm.T).astype(np.float32)
        if flat:
            box[2] = box[1]
        d32, W32 = Dm.astype(np.float32), np.array(W, np.float32)
        VD = _cell_velocity(vscale, VD0, W32, box, Dm, cp, c)
        s = dict(dt=st[0], alpha=st[1], n_pos=st[2], converged_at=st[3])
        ref = CO.control(s, p, cp, c, sums, W32, box, d32, H0.reshape(-1), Dm.reshape(-1), VD, step)
        state = tuple(np.array([t]) for t in st)
        (dt, alpha, n_pos, conv), o = H.control(state, [sums], W32, box, d32, H0, Dm, VD, [c], p, cp, step)
        assert expect is None or (ref["ret"], ref["why"]) == (expect, expect_why), (name, ref["ret"], ref["why"])
        assert (o["ret"][0], o["why"][0]) == (ref["ret"], ref["why"]), name
        assert _bits64(dt[0]) == _bits64(s["dt"]) and _bits64(alpha[0]) == _bits64(s["alpha"]), name
        assert n_pos[0] == s["n_pos"] and conv[0] == s["converged_at"], name
        assert (_bits32(o["coef"][0]) == _bits32(ref["coef"])).all(), (name, o["coef"], ref["coef"])
        assert (_bits32(o["d32"][0]) == _bits32(ref["d32"])).all() and (_bits32(o["box"][0]) == _bits32(ref["box"])).all(), name
        assert (_bits64(o["D"][0]) == _bits64(ref["D"])).all() and (_bits64(o["VD"][0]) == _bits64(ref["VD"])).all(), name
        if ref["ret"] != O.UNUSABLE and st[3] < 0:
            assert (_bits64(o["Gc"][0]) == _bits64(ref["Gc"])).all() and _bits64(o["V"][0]) == _bits64(ref["V"]), name
            assert (_bits64(o["stress"][0]) == _bits64(ref["stress"])).all() and (_bits64(o["sums"][0]) == _bits64(ref["sums"])).all(), name
        if ref["ret"] == O.UNUSABLE or st[3] >= 0:  # the state is untouched, nothing moves
            assert (dt[0], alpha[0], n_pos[0], conv[0]) == st, name
        if ref["ret"] != O.MOVING:
            assert (o["coef"] == 0).all() and (_bits64(o["D"][0]) == _bits64(Dm.reshape(-1))).all() and (o["VD"] == 0).all(), name
            assert (_bits32(o["box"][0]) == _bits32(box.reshape(-1))).all() and (_bits32(o["d32"][0]) == _bits32(d32.reshape(-1))).all(), name
        else:
            clamped = o["coef"][0][2] < np.float32(s["dt"])
            seen.add(("down" if ref["sums"][0] > 0 else "up", "clamped" if clamped else "free", "grow" if st[2] > P["n_min"] else "hold"))
            assert not (_bits64(o["D"][0]) == _bits64(Dm.reshape(-1))).all() or "mask: nothing" in name, name
    assert len(seen) >= 7, seen
    # what the table is about, spelled out on the oracle
    by = {c[0]: c for c in cases}

    def run(name):
        _, st, sums, W, vscale, opt, _, _ = by[name]
        s = dict(dt=st[0], alpha=st[1], n_pos=st[2], converged_at=st[3])
        box = (H0 @ D.T).astype(np.float32)
        VD = _cell_velocity(vscale, VD0, np.array(W, np.float32), box, D, _cp(**opt), 5.0)
        return s, CO.control(s, P, _cp(**opt), 5.0, sums, np.array(W, np.float32), box, D.astype(np.float32), H0.reshape(-1), D.reshape(-1),
                             VD, step), sums

    s, r, sums = run("cell rows dominate fmax")
    assert math.sqrt(sums[3]) < P["fmax"] < math.sqrt(r["sums"][3]) and r["ret"] == O.MOVING  # the atoms alone would have converged
    s, r, sums = run("clamp triggered by the cell rows alone")
    cv, cf, d = (float(t) for t in r["coef"])
    atoms_only = s["dt"] * math.sqrt(cv * cv * sums[2] + 2 * cv * cf * sums[0] + cf * cf * sums[1])
    vf, ff, vv, _ = r["sums"]
    assert atoms_only < P["max_step"] and d < s["dt"]
    assert abs(d * math.sqrt(cv * cv * vv + 2 * cv * cf * vf + cf * cf * ff) - P["max_step"]) < 1e-6
    s, r, sums = run("uphill through the cell rows alone")
    assert sums[0] > 0 > r["sums"][0] and r["coef"][0] == 0 and s["n_pos"] == 0
    s, r, _ = run("hydrostatic")
    G = np.array(r["Gc"]).reshape(3, 3)
    assert G[0, 0] == G[1, 1] == G[2, 2] != 0 and (G[~np.eye(3, dtype=bool)] == 0).all()
    s, r, _ = run("constant volume")
    assert abs(np.trace(np.array(r["Gc"]).reshape(3, 3))) < 1e-15
    s, r, _ = run("mask: xy plane only")
    G = np.array(r["Gc"]).reshape(3, 3)
    assert (G[2] == 0).all() and (G[:, 2] == 0).all() and (G[:2, :2] != 0).all()


def test_positions_and_generalised_forces_are_single_rounded_operations():
    """x = xt D32^T and Ft = F D32 in the order of the equations, every product and sum rounded to fp32; with D32 = I both are exact,
    which is what makes a fully masked cell equal to the fixed-box run."""
    rng = np.random.default_rng(6)
    n = 200
    batch = rng.integers(0, 3, size=n)
    d32 = (np.eye(3) + 0.05 * rng.normal(size=(3, 3, 3))).astype(np.float32)
    xt, f, vt = (rng.normal(size=(n, 3)).astype(np.float32) * s for s in (6.0, 3.0, 0.05))
    Dm = d32[batch]
    x_ref = np.stack([(xt[:, 0] * Dm[:, a, 0] + xt[:, 1] * Dm[:, a, 1]) + xt[:, 2] * Dm[:, a, 2] for a in range(3)], 1)
    ft_ref = np.stack([(f[:, 0] * Dm[:, 0, b] + f[:, 1] * Dm[:, 1, b]) + f[:, 2] * Dm[:, 2, b] for b in range(3)], 1)
    x = H.positions(batch, d32.reshape(3, 9), xt)
    ft, t = H.terms(batch, d32.reshape(3, 9), vt, f)
    assert (_bits32(x) == _bits32(x_ref)).all() and (_bits32(ft) == _bits32(ft_ref)).all()
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    assert (_bits32(t) == _bits32(np.stack([dot(ft_ref, vt), dot(ft_ref, ft_ref), dot(vt, vt)], 1))).all()
    eye = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (3, 1))
    assert (_bits32(H.positions(batch, eye, xt)) == _bits32(xt)).all() and (_bits32(H.terms(batch, eye, vt, f)[0]) == _bits32(f)).all()
    # a fixed atom: no terms, vt = 0, xt kept, x follows the new D32; a converged molecule: not touched
    fixed = (rng.uniform(size=n) < 0.2).astype(np.uint8)
    coef = rng.uniform(0.1, 1.0, size=(3, 3)).astype(np.float32)
    conv = np.array([-1, 4, -1])
    d32n = (d32 + 0.01).astype(np.float32)
    xt2, vt2, x2 = H.update(batch, conv, fixed, coef, d32.reshape(3, 9), d32n.reshape(3, 9), xt, vt, f, x)
    frozen, pinned = conv[batch] >= 0, (fixed != 0) & (conv[batch] < 0)
    assert (H.terms(batch, d32.reshape(3, 9), vt, f, fixed)[1][fixed != 0] == 0).all()
    assert (_bits32(x2[frozen]) == _bits32(x[frozen])).all() and (_bits32(xt2[frozen]) == _bits32(xt[frozen])).all() and (vt2[frozen] == 0).all()
    assert (_bits32(xt2[pinned]) == _bits32(xt[pinned])).all() and (vt2[pinned] == 0).all()
    assert (_bits32(x2[pinned]) == _bits32(H.positions(batch, d32n.reshape(3, 9), xt)[pinned])).all() and (x2[pinned] != x[pinned]).any()
    free = ~frozen & ~pinned
    c = coef[batch]
    v_ref = c[:, 0:1] * vt + c[:, 1:2] * ft_ref
    xt_ref = xt + c[:, 2:3] * v_ref
    assert (_bits32(vt2[free]) == _bits32(v_ref[free])).all() and (_bits32(xt2[free]) == _bits32(xt_ref[free])).all()
    assert (_bits32(x2[free]) == _bits32(H.positions(batch, d32n.reshape(3, 9), xt_ref)[free])).all()


# ---- 4. a whole relaxation -------------------------------------------------------------------------------------------------------------
def _start():
    x, H0, bonds = CO.crystal()
    rng = np.random.default_rng(8)
    x = 0.95 * (x + 0.03 * rng.normal(size=x.shape))
    return x.astype(np.float32), (0.95 * H0).astype(np.float32), bonds


def _efw(bonds):
    return lambda x, box: CO.crystal_efw(np.asarray(x, np.float64), np.asarray(box, np.float64), bonds)


def test_relaxation_at_zero_pressure_reaches_the_rest_lengths():
    """The crystal compressed by 5 %, in its sheared box, atoms displaced; fmax = 1e-4.  The header's fp32 run and the fp64 oracle both
    converge, and every bond ends at R0 within the bound that tests/min_cell_oracle.py's length_bound derives from fmax and the spring
    constant (2.7e-4 here; measured 2.5e-5)."""
    x, H0, bonds = _start()
    p = dict(P, fmax=1e-4)
    cp, c = _cp(), float(len(x))
    r32 = H.relax(x, H0, _efw(bonds), p, cp, c, 2000)
    r64 = CO.relax(x, H0, bonds, p, cp, c, 2000)
    print("converged at: fp32", r32["converged_at"], "fp64", r64["converged_at"])
    assert r32["status"] == 0 and 0 < r32["converged_at"] < 2000 and 0 < r64["converged_at"] < 2000
    assert abs(r32["converged_at"] - r64["converged_at"]) <= 0.25 * r64["converged_at"] + 5
    for r, xt, D in ((r32, r32["xt"], r32["D"]), (r64, r64["xt"], r64["D"])):
        bound = CO.length_bound(xt, D, H0, bonds, c, p["fmax"])
        L = CO.bond_lengths(r["x"], r["box"] if "box" in r else r["H"], bonds)
        print("max |L - R0|", np.abs(L - CO.R0).max(), "bound", bound)
        assert np.abs(L - CO.R0).max() < bound < 1e-3
    assert abs(np.linalg.det(r32["box"].astype(np.float64)) / np.linalg.det(H0.astype(np.float64)) - 0.95 ** -3) < 1e-3  # the box grew back


def test_relaxation_under_pressure_satisfies_its_own_criterion_in_fp64():
    """The same start at pressure 0.4 (E / length^3; the crystal's bulk modulus is of order k / R0 = 3).  Both runs converge to a
    smaller volume than at p = 0.  The fp32 run's final state, re-evaluated in fp64 at (xt, D), satisfies the criterion it stopped on,
    up to the fp32 rounding of what the run evaluated: the slack that tests/min_cell_oracle.py's criterion_slack derives (a worst
    case, 1.9e-4 here; the run's own fmax and the fp64 one differ by 1.2e-7)."""
    x, H0, bonds = _start()
    p = dict(P, fmax=1e-3)
    cp, c = _cp(0.4), float(len(x))
    r32 = H.relax(x, H0, _efw(bonds), p, cp, c, 2000)
    r64 = CO.relax(x, H0, bonds, p, cp, c, 2000)
    print("converged at: fp32", r32["converged_at"], "fp64", r64["converged_at"])
    assert r32["status"] == 0 and 0 < r32["converged_at"] < 2000 and 0 < r64["converged_at"] < 2000
    V32, V64 = abs(np.linalg.det(r32["box"].astype(np.float64))), abs(np.linalg.det(r64["H"]))
    V_rest = abs(np.linalg.det(CO.crystal()[1]))
    assert V32 < 0.99 * V_rest and abs(V32 / V64 - 1) < 1e-3
    Ft, Gc, _ = CO.generalised_forces(r32["xt"].astype(np.float64), H0.astype(np.float64), r32["D"], bonds, cp, c)
    fmax64 = math.sqrt(max((Ft * Ft).sum(1).max(), (Gc * Gc).sum(1).max()))
    slack = CO.criterion_slack(r32["x"], r32["box"], bonds, c, p["fmax"])
    print("fmax of the run", r32["fmax"], "re-evaluated in fp64", fmax64, "slack", slack)
    assert r32["fmax"] < p["fmax"] and fmax64 < p["fmax"] + slack and slack < p["fmax"]
    # the stress at the end balances the target pressure: -W_s / V = -p I, every entry within |G row| |D column| / V
    _, _, W = CO.crystal_efw(r32["x"].astype(np.float64), r32["box"].astype(np.float64), bonds)
    assert np.abs(-0.5 * (W + W.T) / V32 + 0.4 * np.eye(3)).max() < 1.1 * math.sqrt(3) * (p["fmax"] + slack) * c / V32


# ---- 5. the sanitizers -----------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/min_cell_host.hip with its own main, host code only (-Xarch_host -fsanitize=address,undefined): every entry of the mirror on heap
    arrays of exact size.  A report makes the program exit non-zero (-fno-sanitize-recover)."""
    exe = str(tmp_path / "min_cell_host_san")
    subprocess.check_call([H.hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DMIN_CELL_HOST_MAIN", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", H.SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "steps" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


# ---- 6. signatures and exports ---------------------------------------------------------------------------------------------------------
def test_capture_minimize_takes_cell_after_halo_exchange():
    from torchmdnet_amd import minimize
    from torchmdnet_amd.models.model import TorchMD_Net

    sig = inspect.signature(TorchMD_Net.capture_minimize).parameters
    names = list(sig)
    assert names[names.index("halo_exchange") + 1] == "cell" and names[-1] == "cell" and sig["cell"].default is None
    assert list(inspect.signature(minimize.DeviceMinimizer.reset).parameters)[1:] == ["pos", "box"]
    assert minimize.parse_cell({}) == dict(mask=ONES, hydrostatic=False, constant_volume=False, pressure=0.0, cell_factor=None)
    got = minimize.parse_cell(dict(mask=torch.tensor([[1, 0, 0], [0, 1, 0], [0, 0, 0]]), pressure=2, cell_factor=7))
    assert got["mask"] == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]] and got["pressure"] == 2.0 and got["cell_factor"] == 7.0
    for bad in (dict(scalar_pressure=1.0), dict(mask=[[1, 1, 0], [0, 1, 0], [0, 0, 1]]), dict(mask=[1, 1, 1]), dict(mask=[[2, 0, 0], [0, 1, 0], [0, 0, 1]]),
                dict(hydrostatic=True, constant_volume=True), dict(cell_factor=0.0), dict(cell_factor=-3), dict(pressure=NAN)):
        with pytest.raises(ValueError):
            minimize.parse_cell(bad)


def test_header_and_bindings_declare_the_cell_entries():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from torchmdnet_amd import _C

    src = open(_C.__file__).read()
    for name, n_args in (("tmdnet_min_workspace_bytes_cell", 3), ("tmdnet_min_reset_cell", 12), ("tmdnet_min_advance_cell", 41),
                         ("tmdnet_min_status_cell", 3), ("tmdnet_min_advance", 29)):
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == n_args, name
        assert name in _C.declared_symbols() and name + ".argtypes" in src
    # the first 29 arguments of the cell entry are tmdnet_min_advance's, in its order
    plain = re.search(r"\bint\s+tmdnet_min_advance\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")
    cell = re.search(r"\bint\s+tmdnet_min_advance_cell\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")
    assert [" ".join(a.split()) for a in cell[:29]] == [" ".join(a.split()) for a in plain]


def test_library_exports_the_cell_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10
    assert len(hip_lib.tmdnet_min_advance_cell.argtypes) == 41 and len(hip_lib.tmdnet_min_advance.argtypes) == 29
    plain, cell = C.c_size_t(0), C.c_size_t(0)
    for n, b in ((64, 1), (5000, 2), (300, 40)):
        assert hip_lib.tmdnet_min_workspace_bytes(n, b, C.byref(plain)) == 0 and hip_lib.tmdnet_min_workspace_bytes_cell(n, b, C.byref(cell)) == 0
        assert cell.value >= plain.value + b * (5 * 72 + 5 * 36)
    assert hip_lib.tmdnet_min_workspace_bytes_cell(-1, 1, C.byref(cell)) != 0
    # argument checks happen before anything is enqueued: no device is needed to be refused
    p = C.c_void_p(256)
    assert hip_lib.tmdnet_min_reset_cell(None, None, 4, 1, 0, 0.1, 0.1, p, p, p, p, p) == 1
    assert hip_lib.tmdnet_min_reset_cell(None, p, 4, 1, 0, 0.1, 0.1, None, p, p, p, p) == 1
    assert hip_lib.tmdnet_min_reset_cell(None, p, 4, 0, 0, 0.1, 0.1, p, p, p, p, p) == 1
    assert hip_lib.tmdnet_min_status_cell(None, None, (C.c_uint64 * 3)()) == 1
