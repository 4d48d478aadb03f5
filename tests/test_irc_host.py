"""No GPU: the arithmetic of the device-resident IRC follower (csrc/tn_irc_math.h, compiled host-only by tests/irc_host_mirror.py)
against tests/irc_oracle.py - the scheme in fp64, written from the equations.  1. the single-rounded per-atom operations, 2. the
controller table, 3. whole paths on the analytic surface in both precisions against the exact IRC, 4. the mirror symmetry of the two
directions, 5. the path record, 6. fixed atoms, 7. frozen paths, 8. the additive ABI and the signatures, 9. the sanitizers on a
stand-alone program."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import irc_host_mirror as H
from tests import irc_oracle as O
from tests import min_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
# The integration parameters of the surface runs: capture_irc's defaults for v0 and error, and a largest time step chosen so that
# the end of a path is resolved: a path that finishes by turning uphill has overshot the minimum by at most one step,
# v0 dt_max = 0.004, and ten times that stays below the 0.05 the discrimination between the mass sets needs.
DT, STEP = 0.05, 0.02
PRM = dict(fmax=1e-3, v0=0.02, error=1.5e-3, dt_min=DT / 16, dt_max=0.2, every=1, capacity=1024)
MASS_SETS = ((1.0, 1.0), (1.0, 16.0), (16.0, 1.0))
# fp32 against fp64: every step rounds x (half an ulp of a coordinate below 4: 2^-23) and carries the rounding of v and F through
# dt <= 0.2; four such roundings per step, added linearly over at most 800 steps
F32_BOUND = 800 * 4 * 2.0 ** -23
HALF_SEPARATION = 0.05


def _bits32(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.asarray(a, np.float64).view(np.uint64)


# ---- 1. the per-atom operations ----------------------------------------------------------------------------------------------------------
def test_per_atom_operations_are_single_rounded():
    """numpy fp32 rounds every operation: the start images, the open step, v', x', the terms and the damping bit for bit"""
    rng = np.random.default_rng(21)
    G, n = 3, 50
    f32 = np.float32
    x_ts = (4 * rng.normal(size=(G, n, 3))).astype(f32)
    u = rng.normal(size=(G, n, 3)).astype(f32)
    pos, vel = H.start(x_ts, u, 0.05, 0.02, D=2)
    for d, sigma in ((0, f32(1)), (1, f32(-1))):
        assert (_bits32(pos[d::2]) == _bits32(x_ts + (sigma * f32(0.05)) * u)).all()
        assert (_bits32(vel[d::2]) == _bits32((sigma * f32(0.02)) * u)).all()
    assert (_bits32(H.start(x_ts, u, 0.05, 0.02, D=1, backward=True)[0]) == _bits32(pos[1::2])).all()
    assert (_bits32(H.start(x_ts, u, 0.05, 0.02, D=1)[0]) == _bits32(pos[0::2])).all()
    P = 2 * G
    masses = rng.uniform(1, 20, size=n).astype(f32)
    masses[7] = INF
    fixed = (rng.uniform(size=n) < 0.15).astype(np.uint8)
    fixed[7] = 0
    still = ((fixed != 0) | np.isinf(masses))[None, :, None]
    ca = H.half_inv_mass(masses, 0.7)
    assert ca[7] == 0 and (_bits32(ca) == _bits32((0.7 / (2.0 * masses.astype(np.float64))).astype(f32))).all()
    f, x1, x2, v2, f2 = ((3 * rng.normal(size=(P, n, 3))).astype(f32) for _ in range(5))
    dt, dtp = rng.uniform(0.01, 0.2, size=P).astype(f32), rng.uniform(0.01, 0.2, size=P).astype(f32)
    has2 = np.array([1, 0, 1, 1, 0, 1], np.int32)
    vp, t = H.terms(pos, vel, f, ca, masses, dt, dtp, has2, x1, x2, v2, f2, fixed)
    hk = dt[:, None, None] * ca[None, :, None]
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    vp_ref = vel + hk * f
    T = (dtp + dt)[:, None, None]
    xp_ref = (x2 + T * v2) + (T * T) * (ca[None, :, None] * f2)
    assert (_bits32(H.extrapolate(x2, v2, f2, ca, dtp + dt)) == _bits32(xp_ref)).all()
    dx, ds = pos - xp_ref, pos - x1
    with np.errstate(invalid="ignore"):
        t_ref = np.stack([dot(vp_ref, vp_ref), dot(f, vp_ref), dot(f, f), np.where(has2[:, None] != 0, dot(dx, dx), f32(0)),
                          masses[None] * dot(ds, ds)], -1).astype(f32)
    assert (_bits32(vp) == _bits32(np.where(still, f32(0), vp_ref))).all()
    assert (_bits32(t) == _bits32(np.where(still, f32(0), t_ref))).all()
    c = rng.uniform(0.5, 1.5, size=P).astype(f32)
    assert (_bits32(H.damp(vp_ref, c)) == _bits32(c[:, None, None] * vp_ref)).all()
    # the sums: the fp32 terms widened and added, the maximum of |F|^2, the count of the atoms that move
    paths = H.Paths(pos, vel, masses, PRM, 0.05, fixed, force_scale=0.7)
    paths.fresh, paths.n_acc[:], paths.dt[:], paths.dt_used[:] = False, has2, dt.astype(np.float64), dtp
    paths.x1, paths.x2, paths.v2, paths.f2 = x1, x2, v2, f2
    S = np.zeros((P, 6))
    H.lib().irc_sums(P, n, 0, H._p(pos), H._p(vel), H._p(f), H._p(ca), H._p(masses), H._p(fixed), H._p(paths.dt), H._p(dtp), H._p(has2), H._p(x1),
                     H._p(x2), H._p(v2), H._p(f2), H._p(S))
    mv = ~still[0, :, 0]
    for p in range(P):
        tt = t[p, mv].astype(np.float64)
        exact = np.array([math.fsum(tt[:, k]) for k in range(5)])
        assert np.abs(S[p, [0, 1, 3, 4]] - exact[[0, 1, 3, 4]]).max() <= 1e-12 * np.abs(tt).sum()
        assert S[p, 2] == tt[:, 2].max() and S[p, 5] == mv.sum()
    # the open step is tn_md's: the kick, then the drift, on the atoms that move; the generations shift
    paths.fkeep = f.copy()
    paths.x1, paths.v1, paths.f1 = x1.copy(), x2.copy(), f2.copy()
    paths.conv[1] = 5
    before = (paths.pos.copy(), paths.vel.copy())
    paths.open()
    vh = vel + hk * f
    live = (np.arange(P) != 1)[:, None, None]
    assert (_bits32(paths.vel) == _bits32(np.where(still | ~live, before[1], vh))).all()
    assert (_bits32(paths.pos) == _bits32(np.where(still | ~live, before[0], before[0] + dt[:, None, None] * vh))).all()
    assert (_bits32(paths.x2[0]) == _bits32(x1[0])).all() and (_bits32(paths.x1[0]) == _bits32(before[0][0])).all()
    assert (_bits32(paths.v1[0]) == _bits32(before[1][0])).all() and (_bits32(paths.f1[0]) == _bits32(f[0])).all()
    assert (_bits32(paths.x1[1]) == _bits32(x1[1])).all()  # a finished path keeps its generations


# ---- 2. the controller table --------------------------------------------------------------------------------------------------------------
# name, sums (vv, P, fmax2, D2, ds2, free), energy, n_acc before, start, expected ret, cause, reason, and what dt must do
TABLE = [
    ("the start images", (4e-4, 0.3, 0.01, 0.0, 0.0, 3), 1.0, 0, 1, O.MOVING, 0, 0, "same"),
    ("first step: no generation 2", (4e-4, 0.3, 0.01, 7.0, 1e-4, 3), 1.0, 0, 0, O.MOVING, 0, 0, "same"),
    ("D2 = 0", (4e-4, 0.3, 0.01, 0.0, 1e-4, 3), 1.0, 2, 0, O.MOVING, 0, 0, "same"),
    ("ratio inside the clamps", (4e-4, 0.3, 0.01, (1.5e-3 / 1.2 ** 3) ** 2, 1e-4, 3), 1.0, 2, 0, O.MOVING, 0, 0, "free"),
    ("ratio clamped to 1/2", (4e-4, 0.3, 0.01, 1.0, 1e-4, 3), 1.0, 2, 0, O.MOVING, 0, 0, 0.5),
    ("ratio clamped to 2", (4e-4, 0.3, 0.01, 1e-12, 1e-4, 3), 1.0, 2, 0, O.MOVING, 0, 0, 2.0),
    ("dt clamped to dt_min", (4e-4, 0.3, 0.01, 1.0, 1e-4, 3), 1.0, 2, 0, O.MOVING, 0, 0, "min"),
    ("dt clamped to dt_max", (4e-4, 0.3, 0.01, 1e-12, 1e-4, 3), 1.0, 2, 0, O.MOVING, 0, 0, "max"),
    ("sqrt(fmax2) just below fmax", (4e-4, 0.3, (1e-3 * (1 - 1e-9)) ** 2, 1e-6, 1e-4, 3), 1.0, 2, 0, O.FINISHED, 0, 1, "free"),
    ("sqrt(fmax2) just above fmax", (4e-4, 0.3, (1e-3 * (1 + 1e-9)) ** 2, 1e-6, 1e-4, 3), 1.0, 2, 0, O.MOVING, 0, 0, "free"),
    ("P = 0", (4e-4, 0.0, 0.01, 1e-6, 1e-4, 3), 1.0, 2, 0, O.FINISHED, 0, 2, "free"),
    ("P < 0", (4e-4, -0.2, 0.01, 1e-6, 1e-4, 3), 1.0, 2, 0, O.FINISHED, 0, 2, "free"),
    ("both conditions: reason 1 wins", (4e-4, -0.2, 1e-8, 1e-6, 1e-4, 3), 1.0, 2, 0, O.FINISHED, 0, 1, "free"),
    ("NaN energy", (4e-4, 0.3, 0.01, 1e-6, 1e-4, 3), NAN, 2, 0, O.UNUSABLE, 3, 0, "same"),
    ("infinite energy before NaN forces", (NAN, NAN, NAN, NAN, NAN, 3), INF, 2, 0, O.UNUSABLE, 3, 0, "same"),
    ("NaN P", (4e-4, NAN, 0.01, 1e-6, 1e-4, 3), 1.0, 2, 0, O.UNUSABLE, 1, 0, "same"),
    ("infinite fmax2 before the velocity", (NAN, 0.3, INF, 1e-6, 1e-4, 3), 1.0, 2, 0, O.UNUSABLE, 1, 0, "same"),
    ("NaN vv", (NAN, 0.3, 0.01, 1e-6, 1e-4, 3), 1.0, 2, 0, O.UNUSABLE, 2, 0, "same"),
    ("infinite vv", (INF, 0.3, 0.01, 1e-6, 1e-4, 3), 1.0, 2, 0, O.UNUSABLE, 2, 0, "same"),
    ("vv = 0", (0.0, 0.0, 0.01, 1e-6, 1e-4, 3), 1.0, 2, 0, O.UNUSABLE, 2, 0, "same"),
    ("NaN D2", (4e-4, 0.3, 0.01, NAN, 1e-4, 3), 1.0, 2, 0, O.UNUSABLE, 2, 0, "same"),
    ("NaN D2 without a generation 2 is not looked at", (4e-4, 0.3, 0.01, NAN, 1e-4, 3), 1.0, 0, 0, O.MOVING, 0, 0, "same"),
    ("infinite ds2", (4e-4, 0.3, 0.01, 1e-6, INF, 3), 1.0, 2, 0, O.UNUSABLE, 2, 0, "same"),
    ("all atoms fixed", (0.0, 0.0, 0.0, 0.0, 0.0, 0), NAN, 2, 0, O.FINISHED, 0, 1, "same"),
]


def test_controller_table_equals_the_oracle_bit_for_bit_on_the_headers_sums():
    """Every branch of the controller: c, the arc, the state, the slot, the return value and the cause equal the oracle's on the same
    sums; c and the logged dt are the same IEEE operations and the same C library's cbrt, so they agree bit for bit here - the
    stated allowance for dt is one fp32 ulp."""
    n = len(TABLE)
    dt0 = np.array([DT * 20 if t[8] == "min" else DT for t in TABLE])
    prm = [dict(PRM, dt_min=DT * 15, dt_max=DT * 40) if t[8] == "min" else dict(PRM, dt_max=DT * 1.5) if t[8] == "max" else PRM for t in TABLE]
    seen_ret, seen_cause = set(), set()
    for i, (name, sums, e, n_acc, start, want_ret, want_cause, want_reason, dt_rule) in enumerate(TABLE):
        state = dict(dt=[dt0[i]], arc=[0.75], conv=[-1], reason=[0], n_acc=[n_acc], n_rec=[n_acc + 1])
        new, out, slot, cause, ret = H.control([sums], [e], state, start, 9, prm[i])
        s = dict(dt=float(dt0[i]), arc=0.75, conv=-1, reason=0, n_acc=n_acc, n_rec=n_acc + 1)
        r, c, (cc, du), sl = O.control(s, prm[i], sums, e, bool(start), 9)
        assert ret[0] == r == want_ret and cause[0] == c == want_cause, (name, ret, r, cause, c)
        seen_ret.add(r)
        seen_cause.add(c)
        if r == O.UNUSABLE:  # nothing is touched
            assert new["dt"][0] == dt0[i] and new["arc"][0] == 0.75 and new["conv"][0] == -1 and new["n_acc"][0] == n_acc, name
            continue
        assert (_bits32(out[0]) == _bits32([cc, du])).all(), (name, out, cc, du)
        assert MO.ulp_distance(np.float32(new["dt"][0]), np.float32(s["dt"])) <= 1 and _bits64(new["arc"][0]) == _bits64(s["arc"]), name
        assert (new["conv"][0], new["reason"][0], new["n_acc"][0], new["n_rec"][0], slot[0]) == (s["conv"], s["reason"], s["n_acc"], s["n_rec"], sl), name
        assert new["reason"][0] == want_reason and new["conv"][0] == (9 if want_reason else -1), name
        assert new["n_acc"][0] == (0 if start else n_acc + 1) and slot[0] == n_acc + 1  # every = 1: each accepted step is a frame
        if sums[5] > 0:
            assert out[0, 0] == np.float32(PRM["v0"] / math.sqrt(sums[0])) and out[0, 1] == (0 if start else np.float32(dt0[i])), name
            assert new["arc"][0] == (0.75 if start else 0.75 + math.sqrt(sums[4])), name
        if dt_rule == "same":
            assert new["dt"][0] == dt0[i], name
        elif dt_rule == "min":
            assert new["dt"][0] == prm[i]["dt_min"], name
        elif dt_rule == "max":
            assert new["dt"][0] == prm[i]["dt_max"], name
        elif dt_rule == "free":
            assert prm[i]["dt_min"] < new["dt"][0] < prm[i]["dt_max"] and new["dt"][0] != dt0[i], name
        else:
            assert new["dt"][0] == dt0[i] * dt_rule, name
    assert seen_ret == {O.MOVING, O.FINISHED, O.UNUSABLE} and seen_cause == {0, 1, 2, 3}
    # a finished path is frozen: nothing changes, whatever the sums hold
    state = dict(dt=[DT], arc=[0.75], conv=[4], reason=[2], n_acc=[4], n_rec=[5])
    new, out, slot, cause, ret = H.control([[NAN] * 5 + [3]], [NAN], state, 0, 9, PRM)
    assert ret[0] == O.FROZEN and slot[0] == -1 and cause[0] == 0 and all(new[k][0] == state[k][0] for k in state)
    # every = 3 records steps 0, 3, 6, ... and the finishing step; a full record stops but the count goes on
    for n_acc, fin, want in ((1, False, -1), (2, False, 2), (1, True, 2)):
        state = dict(dt=[DT], arc=[0.0], conv=[-1], reason=[0], n_acc=[n_acc], n_rec=[2])
        sums = (4e-4, -1.0 if fin else 0.3, 0.01, 1e-6, 1e-4, 3)
        new, _, slot, _, _ = H.control([sums], [1.0], state, 0, 9, dict(PRM, every=3))
        assert slot[0] == want and new["n_rec"][0] == (3 if want >= 0 else 2)
    state = dict(dt=[DT], arc=[0.0], conv=[-1], reason=[0], n_acc=[7], n_rec=[4])
    new, _, slot, _, _ = H.control([(4e-4, 0.3, 0.01, 1e-6, 1e-4, 3)], [1.0], state, 0, 9, dict(PRM, capacity=4))
    assert slot[0] == -1 and new["n_rec"][0] == 5


# ---- 3. whole paths on the analytic surface -----------------------------------------------------------------------------------------------
def _problem(n, masses2, seed=0):
    x_ts, u, masses, sites = O.problem(n, *masses2, seed=seed)
    return x_ts, u.astype(np.float32), masses, sites


def _run32(x_ts, u, masses, sites, prm=PRM, fixed=None, max_steps=1000, D=2):
    pos, vel = H.start(x_ts[None], u[None], STEP, prm["v0"], D=D)
    return H.run(pos, vel, masses, sites, O.KAPPA, O.A, prm, DT, max_steps, fixed)


_ORACLE = {}


def _oracle(n, masses2):
    """the fp64 run of one case (forward; the backward one is its mirror image) and its distances from the exact IRC, computed once"""
    if (n, masses2) not in _ORACLE:
        x_ts, u, masses, sites = _problem(n, masses2)
        r = O.run(x_ts, u, 1.0, masses, sites, PRM, DT, STEP, 1000)
        r["dist"] = O.distance_from(O.exact_irc(*masses2), r["frames"][:, 0, 0], r["frames"][:, 1, 1])
        _ORACLE[(n, masses2)] = r
    return _ORACLE[(n, masses2)]


def test_exact_ircs_of_the_mass_sets_are_apart():
    """the condition that makes the path test discriminate: the exact IRCs of the three mass sets lie at least 0.1 apart"""
    for i, a in enumerate(MASS_SETS):
        for b in MASS_SETS[i + 1:]:
            sep = max(O.curve_separation(O.exact_irc(*a), O.exact_irc(*b)), O.curve_separation(O.exact_irc(*b), O.exact_irc(*a)))
            print(f"masses {a} against {b}: the exact IRCs are {sep:.3f} apart")
            assert sep >= 2 * HALF_SEPARATION
    for m in MASS_SETS:
        end = O.exact_irc(*m)[-1]
        assert abs(end[0] - 1) < 1e-3 and abs(end[1]) < 1e-3


@pytest.mark.parametrize("n", [2, 3, 40])
@pytest.mark.parametrize("masses2", MASS_SETS)
def test_paths_follow_the_exact_irc_of_their_masses_in_fp32_and_fp64(n, masses2):
    """From the saddle in both directions: the header's fp32 run and the fp64 oracle finish at the same step with the same reason;
    the end lies within twice the oracle's own |X| - 1 and Y plus the fp32 bound; every recorded point lies within
    max(10 x the oracle's largest distance, the fp32 bound) of the exact IRC of ITS masses, and that bound is below half the smallest
    separation of the exact IRCs - which the oracle alone must satisfy - so a path integrated with other masses fails."""
    x_ts, u, masses, sites = _problem(n, masses2)
    r64 = _oracle(n, masses2)
    r32 = _run32(x_ts, u, masses, sites)
    bound = max(10.0 * r64["dist"].max(), F32_BOUND)
    assert r64["cause"] == 0 and 0 < r64["steps"] < 1000 and r64["reason"] in (1, 2)
    assert bound < HALF_SEPARATION, (bound, "the oracle itself does not resolve the mass sets")
    assert r32["steps"] == r64["steps"] and r32["conv"].tolist() == [r64["steps"]] * 2 and r32["reason"].tolist() == [r64["reason"]] * 2
    k = r32["n_rec"][0]
    assert k == r64["steps"] + 1 == r32["n_rec"][1]
    fr = r32["frames"][:, :k].astype(np.float64)
    curve = O.exact_irc(*masses2)
    d32 = np.stack([O.distance_from(curve, fr[p, :, 0, 0], fr[p, :, 1, 1]) for p in range(2)])
    diff = np.abs(fr[0] - r64["frames"]).max()
    ex, ey = abs(abs(r32["pos"][0, 0, 0]) - 1.0), abs(r32["pos"][0, 1, 1])
    ox, oy = abs(abs(r64["x"][0, 0]) - 1.0), abs(r64["x"][1, 1])
    print(f"n = {n} masses {masses2}: steps {r32['steps']} / {r64['steps']} reason {r32['reason'][0]} / {r64['reason']}, largest distance from "
          f"the exact IRC {d32.max():.3e} / {r64['dist'].max():.3e} (bound {bound:.3e}), fp32 - fp64 {diff:.3e} (bound {F32_BOUND:.3e}), end "
          f"|X| - 1 = {ex:.3e} / {ox:.3e}, Y = {ey:.3e} / {oy:.3e}, arc {r32['arc'][0]:.6f} / {r64['arc']:.6f}")
    assert d32.max() <= bound
    assert diff <= F32_BOUND
    assert ex <= 2.0 * ox + F32_BOUND and ey <= 2.0 * oy + F32_BOUND and ox < 0.01 and oy < 0.01
    assert (fr[0, :, 0, 0] > 0).all() and (fr[1, :, 0, 0] < 0).all()  # forward goes to X = +1, backward to X = -1
    assert abs(r32["arc"][0] - r64["arc"]) <= 1e-5 * r64["arc"]
    # the spectators never leave their sites
    assert (_bits32(r32["pos"][:, 2:]) == _bits32(np.broadcast_to(x_ts[2:], r32["pos"][:, 2:].shape))).all()
    # a path integrated with the masses of another set is told apart
    other = MASS_SETS[(MASS_SETS.index(masses2) + 1) % 3]
    wrong = masses.copy()
    wrong[:2] = other
    rw = _run32(x_ts, u, wrong, sites)
    fw = rw["frames"][0, :rw["n_rec"][0]].astype(np.float64)
    assert O.distance_from(curve, fw[:, 0, 0], fw[:, 1, 1]).max() > bound


# ---- 4. symmetry ------------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_paths_are_mirror_images_bit_for_bit():
    x_ts, u, masses, sites = _problem(3, (1.0, 16.0))
    r = _run32(x_ts, u, masses, sites)
    flip = np.ones((3, 3), np.float32)
    flip[0, 0] = -1
    for key in ("pos", "vel", "forces"):  # (values, so that a zero of either sign equals a zero: sigma = -1 makes the spectators' v0 = -0)
        assert (r[key][0] == flip * r[key][1]).all() and (r[key][0, 0, 0] != 0).all(), key
    k = r["n_rec"][0]
    assert (_bits32(r["frames"][0, :k, 0, 0]) == _bits32(-r["frames"][1, :k, 0, 0])).all()
    assert (_bits32(r["frames"][0, :k, 1:]) == _bits32(r["frames"][1, :k, 1:])).all()
    assert (_bits64(r["frame_s"][0]) == _bits64(r["frame_s"][1])).all() and (_bits32(r["frame_e"][0]) == _bits32(r["frame_e"][1])).all()
    assert (_bits64(r["log"][:, 0]) == _bits64(r["log"][:, 1])).all()
    # one direction alone runs as it does beside the other
    for back in (False, True):
        pos, vel = H.start(x_ts[None], u[None], STEP, PRM["v0"], D=1, backward=back)
        alone = H.run(pos, vel, masses, sites, O.KAPPA, O.A, PRM, DT, 1000)
        assert alone["steps"] == r["steps"] and (_bits32(alone["pos"][0]) == _bits32(r["pos"][int(back)])).all()


# ---- 5. the record -----------------------------------------------------------------------------------------------------------------------
def test_record_every_capacity_and_arc_length():
    x_ts, u, masses, sites = _problem(3, (16.0, 1.0))
    r1 = _run32(x_ts, u, masses, sites)
    r3 = _run32(x_ts, u, masses, sites, dict(PRM, every=3))
    steps = r1["steps"]
    assert r3["steps"] == steps and r1["n_rec"].tolist() == [steps + 1] * 2
    want = list(range(0, steps + 1, 3)) + ([] if steps % 3 == 0 else [steps])
    assert r3["n_rec"].tolist() == [len(want)] * 2
    for key in ("frames", "frame_s", "frame_e"):
        assert (r3[key][:, :len(want)] == r1[key][:, want]).all(), key
    assert (_bits32(r1["frames"][:, steps]) == _bits32(r1["pos"])).all() and (r1["frame_s"][:, steps] == r1["arc"]).all()
    small = _run32(x_ts, u, masses, sites, dict(PRM, capacity=4))
    assert small["steps"] == steps and small["n_rec"].tolist() == [steps + 1] * 2 and (small["n_rec"] > 4).all()  # truncated
    assert (small["frames"] == r1["frames"][:, :4]).all() and (_bits32(small["pos"]) == _bits32(r1["pos"])).all()
    # the arc is the sum of the mass-weighted chords between consecutive frames
    fr = r1["frames"][0, :steps + 1].astype(np.float64)
    chords = np.sqrt((masses[None, :, None] * np.diff(fr, axis=0) ** 2).sum((1, 2)))
    rel = abs(chords.sum() - r1["arc"][0]) / r1["arc"][0]
    print(f"arc {r1['arc'][0]:.9f}, recomputed from the frames {chords.sum():.9f}: relative difference {rel:.2e}")
    assert rel <= 1e-6
    assert (np.diff(r1["frame_s"][0, :steps + 1]) > 0).all() and r1["frame_s"][0, 0] == 0.0
    assert abs(float(r1["frame_e"][0, 0]) - 1.0) < 0.01 and abs(float(r1["frame_e"][0, steps])) < 1e-4  # from the saddle, E = 1, to the minimum


# ---- 6. fixed atoms ------------------------------------------------------------------------------------------------------------------------
def test_fixed_atoms_keep_their_bits_and_leave_the_sums():
    """A spectator held off its site feels a force; fixed, it keeps its bits, and the path of the others is the one they take with
    that spectator free on its site, where it contributes exact zeros.  An atom of infinite mass behaves the same."""
    n = 5
    x_ts, u, masses, sites = _problem(n, (1.0, 16.0))
    ref = _run32(x_ts, u, masses, sites)
    off = x_ts.copy()
    off[3] += np.float32(0.3)
    for how in ("fixed", "infinite mass"):
        fixed = np.array([0, 0, 0, 1, 0], np.uint8) if how == "fixed" else None
        m = masses.copy()
        if how != "fixed":
            m[3] = INF
        r = _run32(off, u, m, sites, fixed=fixed)
        assert r["steps"] == ref["steps"] and (_bits32(r["pos"][:, 3]) == _bits32(off[3])).all() and (r["vel"][:, 3] == 0).all(), how
        keep = [0, 1, 2, 4]
        assert (_bits32(r["pos"][:, keep]) == _bits32(ref["pos"][:, keep])).all() and (_bits64(r["arc"]) == _bits64(ref["arc"])).all(), how
        assert (r["forces"][:, 3] != 0).any()
    # a direction that lives on fixed atoms only cannot be followed; every atom fixed: the path is finished as it stands
    every = np.ones(n, np.uint8)
    pos, vel = H.start(x_ts[None], np.zeros((1, n, 3), np.float32), STEP, PRM["v0"])
    r = H.run(pos, vel, masses, sites, O.KAPPA, O.A, PRM, DT, 50, every)
    assert r["steps"] == 0 and r["conv"].tolist() == [0, 0] and r["reason"].tolist() == [1, 1] and (_bits32(r["pos"]) == _bits32(pos)).all()
    assert O.run(x_ts, np.zeros((n, 3)), 1.0, masses, sites, PRM, DT, STEP, 50, every)["conv"] == 0
    # unusable: zero velocity on free atoms (cause 2), a NaN position (its energy is looked at first: cause 3)
    assert H.run(pos, vel, masses, sites, O.KAPPA, O.A, PRM, DT, 50)["steps"] == -O.BAD_VELOCITY
    assert O.run(x_ts, np.zeros((n, 3)), 1.0, masses, sites, PRM, DT, STEP, 50)["cause"] == O.BAD_VELOCITY
    pos, vel = H.start(x_ts[None], u[None], STEP, PRM["v0"])
    pos[1, 2, 0] = NAN
    assert H.run(pos, vel, masses, sites, O.KAPPA, O.A, PRM, DT, 50)["steps"] == -O.BAD_ENERGY


# ---- 7. frozen paths ---------------------------------------------------------------------------------------------------------------------
def test_a_finished_path_changes_nothing_on_further_steps():
    """two saddles of unequal masses in one call finish at their own steps with the bits of their runs alone; further launches change
    nothing of a finished path; an unusable step puts generation 1 back and writes nothing else"""
    n = 3
    x_ts, u, masses, sites = _problem(n, (1.0, 1.0))
    pos, vel = H.start(x_ts[None], u[None], STEP, PRM["v0"])
    pos[1, 0, 0] -= np.float32(0.05)  # the backward path starts further out: it finishes at another step
    alone = [H.run(pos[p:p + 1], vel[p:p + 1], masses, sites, O.KAPPA, O.A, PRM, DT, 1000) for p in range(2)]
    both = H.run(pos, vel, masses, sites, O.KAPPA, O.A, PRM, DT, 1000)
    assert alone[0]["steps"] != alone[1]["steps"] and both["conv"].tolist() == [alone[0]["steps"], alone[1]["steps"]]
    for p in range(2):
        for key in ("pos", "vel", "forces", "frames", "frame_s", "arc", "dt"):
            assert (both[key][p] == alone[p][key][0]).all(), (p, key)
    paths = H.Paths(pos, vel, masses, dict(PRM, capacity=8), DT)
    first = int(np.argmin(both["conv"]))
    for step in range(int(both["conv"].min()) + 3):
        if step:
            paths.open()
        e, f = H.surface(paths.pos, sites, O.KAPPA, O.A)
        assert paths.close(e, f) == 0
        if paths.conv[first] == step:
            snap = {k: getattr(paths, k)[first].copy() for k in ("pos", "vel", "fkeep", "x1", "x2", "dt", "arc", "n_rec", "frames", "rec")}
    assert paths.conv[first] == both["conv"].min() and paths.step == both["conv"].min() + 2 and paths.conv[1 - first] == -1
    for k, v in snap.items():
        assert (_bits32(getattr(paths, k)[first]) == _bits32(v)).all() if v.dtype == np.float32 else (getattr(paths, k)[first] == v).all(), k
    # an unusable evaluation: nothing is accepted, the moving path is back at generation 1, the finished one untouched
    paths.open()
    e, f = H.surface(paths.pos, sites, O.KAPPA, O.A)
    f[1 - first, 1, 2] = NAN
    before = {k: getattr(paths, k).copy() for k in ("fkeep", "dt", "arc", "n_rec", "n_acc", "conv")}
    assert paths.close(e, f) == O.BAD_FORCES and paths.step == both["conv"].min() + 2
    assert (_bits32(paths.pos[1 - first]) == _bits32(paths.x1[1 - first])).all() and (_bits32(paths.vel[1 - first]) == _bits32(paths.v1[1 - first])).all()
    assert all((getattr(paths, k) == v).all() for k, v in before.items()) and (_bits32(paths.pos[first]) == _bits32(snap["pos"])).all()


# ---- 8. the additive ABI ---------------------------------------------------------------------------------------------------------------
IRC_ENTRIES = (("tmdnet_irc_workspace_bytes", 4), ("tmdnet_irc_reset", 4), ("tmdnet_irc_advance", 34), ("tmdnet_irc_status", 3))


def test_header_and_bindings_are_additive():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from torchmdnet_amd import _C

    src = open(_C.__file__).read()
    args_of = lambda name: [" ".join(a.split()) for a in re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")]
    for name, n_args in IRC_ENTRIES:
        assert len(args_of(name)) == n_args, name
        assert name in _C.declared_symbols() and name + ".argtypes" in src
    for name, n_args in (("tmdnet_min_advance", 29), ("tmdnet_neb_advance", 34), ("tmdnet_dimer_advance", 38), ("tmdnet_md_advance", 22)):  # untouched
        assert len(args_of(name)) == n_args, name
    adv = args_of("tmdnet_irc_advance")
    assert adv[:9] == ["tmdnet_model* m", "void* stream", "void* graph_ws", "void* irc_ws", "int64_t n_atoms", "int64_t n_paths", "int64_t capacity",
                       "int32_t every", "int32_t phase"]
    assert adv[-5:] == ["int64_t* converged_at", "int32_t* reason", "double* step_size", "double* arc_length", "int32_t* n_recorded"]


def test_library_exports_the_irc_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10
    for name, n_args in IRC_ENTRIES:
        assert len(getattr(hip_lib, name).argtypes) == n_args, name
    small, large = C.c_size_t(0), C.c_size_t(0)
    assert hip_lib.tmdnet_irc_workspace_bytes(64, 2, 16, C.byref(small)) == 0 and small.value >= 256 + 2 * 64 * (72 + 16 * 12)
    assert hip_lib.tmdnet_irc_workspace_bytes(1500, 2, 16, C.byref(large)) == 0 and large.value >= 256 + 2 * 1500 * (72 + 16 * 12) + 2 * 2 * 6 * 8
    for bad in ((64, 0, 4), (-1, 1, 4), (2 ** 31, 1, 4), (64, 1, 0)):
        assert hip_lib.tmdnet_irc_workspace_bytes(*bad, C.byref(small)) != 0
    assert hip_lib.tmdnet_irc_workspace_bytes(64, 1, 4, None) == 1
    # argument checks happen before anything is enqueued: no device is needed to be refused
    assert hip_lib.tmdnet_irc_reset(None, None, 0, 0.1) == 1
    assert hip_lib.tmdnet_irc_reset(None, C.c_void_p(256), 0, 0.0) == 1
    assert hip_lib.tmdnet_irc_status(None, None, None) == 1
    p = C.c_void_p(256)
    ok = [None, None, None, p, 4, 2, 8, 1, 2, p, p, p, p, p, p, None, None, 0.05, 0.02, 1e-3, 0.01, 0.1] + [None] * 12
    for i, v in ((3, None), (9, None), (12, None), (13, None), (8, 7), (7, 0), (17, 0.0), (18, -1.0), (19, 0.0), (20, 0.2), (6, 0), (2, p)):
        args = list(ok)
        args[i] = v
        assert hip_lib.tmdnet_irc_advance(*args) == 1, i


def test_capture_irc_and_module_signatures():
    import torch

    from torchmdnet_amd import irc
    from torchmdnet_amd.models.model import TorchMD_Net

    sig = inspect.signature(TorchMD_Net.capture_irc).parameters
    assert list(sig)[1:] == ["z", "pos", "mode", "masses", "dt", "direction", "box", "q", "steps_per_replay", "force_scale", "fmax", "v0", "error",
                             "initial_step", "dt_min", "dt_max", "record", "fixed", "warmup"]
    defaults = {k: sig[k].default for k in list(sig)[6:]}
    assert defaults == dict(direction="both", box=None, q=None, steps_per_replay=10, force_scale=1.0, fmax=0.05, v0=0.02, error=1.5e-3,
                            initial_step=0.05, dt_min=None, dt_max=None, record=dict(every=1, capacity=512), fixed=None, warmup=3)
    for name in ("__call__", "check", "reset", "run", "path"):
        assert callable(getattr(irc.DeviceIRC, name))
    assert list(inspect.signature(irc.DeviceIRC.run).parameters)[1:] == ["max_steps", "check_every"]
    assert list(inspect.signature(irc.DeviceIRC.reset).parameters)[1:] == ["pos", "mode"]
    fixed = torch.tensor([0, 1, 0, 0], dtype=torch.uint8)
    mode = torch.zeros(4, 3)
    mode[0, 0], mode[1, 1], mode[2, 2] = 3.0, 5.0, 4.0
    u = irc.unit_direction(mode, 2, 4, fixed)
    assert u.dtype == torch.float32 and tuple(u.shape) == (2, 4, 3) and (u[:, 1] == 0).all()
    assert torch.equal(u[0], u[1]) and abs(float(u[0, 0, 0]) - 0.6) < 1e-7 and abs(float(u[0, 2, 2]) - 0.8) < 1e-7
    with pytest.raises(ValueError):
        irc.unit_direction(torch.zeros(4, 3), 1, 4, None)
    only_fixed = torch.zeros(4, 3)
    only_fixed[1, 2] = 1.0
    with pytest.raises(ValueError):
        irc.unit_direction(only_fixed, 1, 4, fixed)
    # the record's place in the workspace, as the header states it
    off = irc.record_layout(40, 4, 8)
    assert off == dict(n_recorded=256, frame_s=512, frame_e=768, frames=1024, end=1024 + 4 * 8 * 40 * 12)


# ---- 9. the sanitizers -----------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/irc_host.hip with its own main, host code only (-Xarch_host -fsanitize=address,undefined): every entry of the mirror on
    heap arrays of exact size.  A report makes the program exit non-zero (-fno-sanitize-recover)."""
    exe = str(tmp_path / "irc_host_san")
    subprocess.check_call([H.hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DIRC_HOST_MAIN", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", H.SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "steps" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
