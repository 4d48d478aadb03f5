"""Minima hopping without a GPU: torchmd-net_amd/csrc/tn_hop_math.h compiled for the host (tests/hop_host.hip through
tests/hop_host_mirror.py) against the independent fp64 numpy restatement tests/hop_oracle.py on a 4-atom chain whose three minima
have a closed form, an SVD Kabsch superposition, and the invariants of the feedback."""
import functools
import json
import math
import os

import numpy as np
import pytest

from tests import hop_host_mirror as H
from tests import hop_oracle as O
from torchmdnet_amd import hop as HP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 2, 3)  # the oracle alone finds exactly the three minima within 30 hops for each (test 2 re-checks it)
EPS32 = 2.0 ** -24


def params(**kw):
    return HP.parse_hop(**dict(O.CHAIN_PARAMS, **kw))


def surface32(x):
    """the chain's surface as an engine would hand it over: fp64 at the fp32 positions, rounded once"""
    E, F = O.chain_surface(np.asarray(x, np.float64))
    return np.float32(E), F.astype(np.float32)


def mirror(**kw):
    return H.HostHop(params(**kw), O.CHAIN_START, np.ones(4))


def run_mirror(h, hops, max_steps=20000, log=None):
    """step until the walker has `hops` hops; log rows: phase, outcome, energy, pos AT the evaluation, kT, ediff, ekin"""
    steps = 0
    while h.n_hops[0] < hops and steps < max_steps:
        at = h.pos.copy()
        E, F = surface32(at)
        h.step([E], F)
        steps += 1
        if log is not None:
            log.append((int(h.phase_log[0]), int(h.outcome[0]), float(h.epot[0]), at, float(h.kT[0]), float(h.ediff[0]), float(h.ekin[0])))
    return steps


def ideal_chain(phi):
    """bonds 1.5, angles 110 deg, torsion +-phi"""
    th = O.THETA0
    return np.array([[1.5 * math.cos(th), 1.5 * math.sin(th), 0.0], [0.0, 0.0, 0.0], [1.5, 0.0, 0.0],
                     [1.5 - 1.5 * math.cos(th), 1.5 * math.sin(th) * math.cos(phi), 1.5 * math.sin(th) * math.sin(phi)]])


def gauche():
    """(phi, E) of the gauche minimum of the torsion term, by bisection on its derivative"""
    def dV(p):
        return -0.45 * math.sin(3 * p) - 0.05 * math.sin(p)

    lo, hi = math.radians(50), math.radians(75)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if dV(mid) < 0 else (lo, mid)
    return lo, O.torsion_energy(lo)


@functools.lru_cache(maxsize=None)
def oracle_run(seed, hops=30):
    return O.Walker(O.chain_surface, O.CHAIN_START, np.ones(4), seed=seed, **O.CHAIN_PARAMS).run(hops)


# ---- 1. the surface and the oracle ---------------------------------------------------------------------------------------------------
def test_surface_forces_match_central_differences_and_the_closed_form():
    rng = np.random.default_rng(0)
    x = O.CHAIN_START + 0.1 * rng.standard_normal((4, 3))
    _, F = O.chain_surface(x)
    num = np.zeros_like(x)
    for a in range(4):
        for k in range(3):
            xp, xm = x.copy(), x.copy()
            xp[a, k] += 1e-6
            xm[a, k] -= 1e-6
            num[a, k] = -(O.chain_surface(xp)[0] - O.chain_surface(xm)[0]) / 2e-6
    assert np.abs(F - num).max() < 1e-7
    for phi in (0.3, 1.1, -2.0, math.pi):
        x = ideal_chain(phi)
        assert abs(abs(O.chain_torsion(x)) - abs(phi)) < 1e-12
        assert abs(O.chain_surface(x)[0] - O.torsion_energy(phi)) < 1e-12
    assert abs(O.torsion_energy(math.pi)) < 1e-15 and abs(gauche()[1] - 0.0743) < 1e-4


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_finds_exactly_the_three_minima(seed):
    """2. with Philox, within 30 hops: trans and gauche+-, no duplicate.  The energies of the minima, quenched on to a force of 1e-9,
    match the closed form to 1e-9; as recorded (fmax = 1e-3) they lie within fmax^2 / (2 x the softest curvature, > 0.5) of it."""
    w = oracle_run(seed)
    mins = w.minima()
    phi_g, e_g = gauche()
    assert len(mins) == 3
    tors = [O.chain_torsion(m["pos"]) for m in mins]  # (lowest energy first: trans, then the two gauche minima)
    assert abs(abs(tors[0]) - math.pi) < 0.02 and sorted(round(t / phi_g, 1) for t in tors[1:]) == [-1.0, 1.0]
    for m, e in zip(mins, (0.0, e_g, e_g)):
        assert abs(m["energy"] - e) < 1e-6
        polish = O.Walker(O.chain_surface, m["pos"], np.ones(4), **dict(O.CHAIN_PARAMS, fmax=1e-9))
        while polish.phase == O.QUENCH:
            polish.step()
        assert abs(polish.epot[-1] - e) < 1e-9
    assert w.n["hops"] == w.n["same"] + w.n["known"] + w.n["new"] + w.n["unconverged"] and w.n["accepted"] <= w.n["new"]


# ---- 3. the mirror against the oracle over the first hop -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_mirror_walks_the_oracles_first_hop(seed):
    """The same phases and outcomes step by step until the first hop is classified.  Positions: within 10 x the distance between the
    oracle in fp32 numpy and in fp64 over the same steps (profiles/hop.json records that distance); chaos ends the comparison there."""
    w64 = O.Walker(O.chain_surface, O.CHAIN_START, np.ones(4), seed=seed, **O.CHAIN_PARAMS)
    w32 = O.Walker(O.chain_surface, O.CHAIN_START, np.ones(4), dtype=np.float32, seed=seed, **O.CHAIN_PARAMS)
    h = mirror(seed=seed)
    worst32, worst = 0.0, 0.0
    while w64.n["hops"] < 1:
        w64.step()
        w32.step()
        E, F = surface32(h.pos)
        h.step([E], F)
        assert (int(h.phase_log[0]), int(h.outcome[0])) == (w64.phases[-1], w64.outcomes[-1]), f"step {w64.steps}"
        assert int(h.phase[0]) == w64.phase
        worst32 = max(worst32, float(np.abs(w32.x.astype(np.float64) - w64.x).max()))
        worst = max(worst, float(np.abs(h.pos.astype(np.float64) - w64.x).max()))
    print(f"seed {seed}: {w64.steps} steps, |mirror - fp64| = {worst:.3e}, |fp32 numpy - fp64| = {worst32:.3e}")
    with open(os.path.join(ROOT, "profiles", "hop.json")) as fh:
        recorded = json.load(fh)["first_hop_fp32_vs_fp64"][str(seed)]
    assert worst32 == pytest.approx(recorded, rel=0.5)  # (the record is what this test measures)
    assert worst <= 10.0 * recorded
    assert h.kT[0] == w64.kT and h.ediff[0] == w64.ediff and int(h.n_hops[0]) == 1


# ---- 4. invariants beyond the first hop ----------------------------------------------------------------------------------------------
def test_feedback_is_the_ordered_product_of_the_logged_factors():
    p = params(seed=5)
    h = H.HostHop(p, O.CHAIN_START, np.ones(4))
    log = []
    run_mirror(h, 12, log=log)
    kT, ediff, counts = p["kT0"], p["ediff0"], dict.fromkeys(range(8), 0)
    for _, out, *_ in log:
        counts[out] += 1
        if out == HP.OUT_SAME:
            kT = kT * p["beta1"]
        if out == HP.OUT_KNOWN:
            kT = kT * p["beta2"]
        if out in (HP.OUT_ACCEPTED, HP.OUT_REJECTED):
            kT = kT * p["beta3"]
            ediff = ediff * (p["alpha1"] if out == HP.OUT_ACCEPTED else p["alpha2"])
    assert h.kT[0] == kT and h.ediff[0] == ediff  # exactly: the same fp64 products in the same order
    n = h.counters[0]
    assert n[0] == 12 and n[0] == n[1] + n[2] + n[3] + n[5] and n[4] <= n[3]
    assert (n[1], n[2], n[3], n[4], n[5]) == (counts[2], counts[3], counts[4] + counts[5], counts[4], counts[6])
    assert counts[HP.OUT_START] == 1 and n[6] == n[3] + 1
    # every ring entry is a minimum with the logged energy, and no two entries are the same minimum
    live = int(min(n[6], p["capacity"]))
    for s in range(live):
        E, F = O.chain_surface(h.ring_pos[s].astype(np.float64))
        assert math.sqrt((F * F).sum(1).max()) < p["fmax"] * (1 + 1e-5) and abs(E - h.ring_energy[0, s]) < 4 * EPS32 * max(abs(E), 1.0)
        for t in range(s):
            same = abs(h.ring_energy[0, s] - h.ring_energy[0, t]) < p["energy_tol"] and H.rmsd(h.ring_pos[s], h.ring_pos[t]) < p["rmsd_tol"]
            assert not same
    assert h.best_energy[0] == h.ring_energy[0, :live].min()


def test_an_exhausted_quench_restores_the_walker_bit_for_bit():
    h = mirror(seed=1, opt_steps=3)
    log = []
    run_mirror(h, 1, log=log)
    assert [o for _, o, *_ in log if o] == [HP.OUT_START, HP.OUT_UNCONVERGED]
    assert np.array_equal(h.pos.view(np.uint32), h.minimum_pos.view(np.uint32))
    assert h.kT[0] == 0.3 and h.ediff[0] == 0.1 and h.counters[0, 5] == 1 and h.phase[0] == HP.LAUNCH
    # the quench moved once at the transition out of the escape and twice more; the fourth control found the budget of 3 used up
    assert [ph for ph, *_ in log[-4:]] == [HP.MD, HP.QUENCH, HP.QUENCH, HP.QUENCH]
    assert h.vel.any()  # new velocities are drawn for the next escape


def test_a_full_ring_overwrites_its_oldest_entry_and_best_survives():
    p = params(seed=0, capacity=2)
    h = H.HostHop(p, O.CHAIN_START, np.ones(4))
    recorded = []
    while h.counters[0, 6] < 3 and h.n_hops[0] < 60:
        log = []
        run_mirror(h, int(h.n_hops[0]) + 1, log=log)
        recorded += [(e, x) for _, o, e, x, *_ in log if o in (HP.OUT_START, HP.OUT_ACCEPTED, HP.OUT_REJECTED)]
    assert h.counters[0, 6] == 3 == len(recorded)
    assert h.ring_found[0, 0] > h.ring_found[0, 1]  # slot 0 was written again after slot 1
    assert h.ring_energy[0, 0] == recorded[2][0] and h.ring_energy[0, 1] == recorded[1][0]
    assert np.array_equal(h.ring_pos[0], recorded[2][1]) and np.array_equal(h.ring_pos[1], recorded[1][1])
    best = min(range(3), key=lambda i: recorded[i][0])
    assert h.best_energy[0] == recorded[best][0] and np.array_equal(h.best_pos, recorded[best][1])
    assert best == 0 and h.best_energy[0] < h.ring_energy[0].min()  # the lowest minimum left the ring: only `best` holds it


# ---- 5. the aligned RMSD -------------------------------------------------------------------------------------------------------------
def rotation(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("n", [3, 4, 65])
def test_horn_equals_kabsch(n):
    rng = np.random.default_rng(n)
    for _ in range(20):
        a, b = (rng.standard_normal((n, 3)) * 2).astype(np.float32), (rng.standard_normal((n, 3)) * 2 + 3).astype(np.float32)
        for name, code in HP.ALIGN.items():
            ref = O.kabsch_rmsd(a, b, name)
            assert abs(H.rmsd(a, b, code) - ref) < 1e-10
            assert abs(HP.rmsd(a, b, name) - ref) < 1e-10
    # a rotated and translated copy that fp32 holds exactly (a cyclic permutation of the axes with two signs flipped is a proper
    # rotation; coordinates on a grid of 2^-10): zero to 1e-7
    a = (rng.integers(-2048, 2048, (n, 3)) / 1024.0).astype(np.float32)
    b = (np.stack([-a[:, 1], -a[:, 2], a[:, 0]], 1) + np.array([0.5, -2.0, 1.0])).astype(np.float32)
    assert H.rmsd(a, b) < 1e-7 and HP.rmsd(a, b) < 1e-7
    # a general rotation, rounded to fp32: what the rounding of the copy's coordinates leaves (half an ulp each)
    c = (a.astype(np.float64) @ rotation(rng).T + np.array([0.3, 1.7, -0.9])).astype(np.float32)
    assert H.rmsd(a, c) < 4 * EPS32 * np.abs(c).max() + 1e-7
    assert H.rmsd(a, c, 1) > 0.1  # (translation alone does not superpose them)


def test_mirror_images_stay_distinct_and_collinear_atoms_give_no_nan():
    rng = np.random.default_rng(7)
    a = rng.standard_normal((5, 3)).astype(np.float32)
    m = a * np.array([1.0, 1.0, -1.0], np.float32)
    assert H.rmsd(a, m) > 0.05 and abs(H.rmsd(a, m) - O.kabsch_rmsd(a, m)) < 1e-10
    line = np.outer(np.arange(4.0), [1.0, 2.0, -0.5]).astype(np.float32)
    turned = np.outer(np.arange(4.0), [-0.5, 1.0, 2.0]).astype(np.float32) + np.float32(1.0)
    for x, y in ((line, line), (line, turned), (line, a[:4])):
        r = H.rmsd(x, y)
        assert math.isfinite(r) and abs(r - O.kabsch_rmsd(x, y)) < 1e-7
    assert H.rmsd(line, turned) < 1e-6
    two = a[:2]
    assert abs(H.rmsd(two, two[::-1] + np.float32(2.0)) - O.kabsch_rmsd(two, two[::-1] + 2.0, "translation")) < 1e-10


# ---- 6. the launch ------------------------------------------------------------------------------------------------------------------
def launch_sums(m, d, v):
    return np.concatenate([[m.sum()], (m[:, None] * d).sum(0), (m[:, None] * v).sum(0), (m[:, None] * np.cross(d, v)).sum(0),
                           [(m * d[:, i] * d[:, j]).sum() for i, j in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]])


def test_launch_solve_removes_momentum_and_angular_momentum():
    rng = np.random.default_rng(3)
    n = 7
    m, d, v = rng.uniform(1, 16, n), rng.standard_normal((n, 3)) * 2 + 0.4, rng.standard_normal((n, 3))
    u, w, singular = H.launch_solve(launch_sums(m, d, v))
    assert not singular
    v2 = v - (u.astype(np.float64) + np.cross(w.astype(np.float64), d))
    scale = (m[:, None] * np.abs(v)).sum()  # u and omega are rounded to fp32 once: relative 2^-24 of terms of this size
    assert np.abs((m[:, None] * v2).sum(0)).max() < 8 * EPS32 * scale
    dcm = (m[:, None] * d).sum(0) / m.sum()
    assert np.abs((m[:, None] * np.cross(d - dcm, v2)).sum(0)).max() < 32 * EPS32 * scale * np.abs(d).max()
    # collinear atoms: the inertia tensor is singular, the rotation stays and the flag is raised
    d = np.outer(np.arange(3.0), [1.0, 1.0, 0.0])
    u, w, singular = H.launch_solve(launch_sums(np.ones(3), d, v[:3]))
    assert singular == 1 and not w.any() and np.isfinite(u).all()
    u, w, singular = H.launch_solve(launch_sums(np.ones(3), d, v[:3]), align=1)
    assert singular == 0 and not w.any()


def test_launch_noise_is_its_own_philox_stream():
    from tests import md_oracle as M

    xi = H.noise(seed=11, hop=3, n=5)
    ref = np.array([M.normals(M.philox4x32_10((3, 0, i, 2), (11, 0))) for i in range(5)])
    assert np.abs(xi - ref).max() < 4e-6  # (the fp32 Box-Muller against the fp64 one)
    other = np.array([M.normals(M.philox4x32_10((3, 0, i, 0), (11, 0))) for i in range(5)])
    assert np.abs(xi - other).max() > 0.1


def test_refusals_name_the_parameter():
    for bad in (dict(capacity=0), dict(capacity=65), dict(mdmin=0), dict(dt=0.0), dict(kT0=-1.0), dict(fmax=0.0), dict(rmsd_tol=0.0),
                dict(energy_tol=0.0)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            params(**bad)
    with pytest.raises(ValueError, match="align"):
        params(align="mirror")
    assert params()["align"] == 2 and params(has_box=True)["align"] == 1 and params(has_fixed=True, has_box=True)["align"] == 0


def test_overflow_and_nan_freeze_the_mirror():
    h = mirror(seed=2)
    for _ in range(5):
        E, F = surface32(h.pos)
        h.step([E], F)
    before = h.pos.copy()
    E, F = surface32(h.pos)
    h.step([E], F)
    h.step([E], F, overflowed=True)
    assert h.status() == (6, 1) and np.array_equal(h.pos, before)
    h.step([E], F)
    assert h.status() == (6, 1)
    h = mirror(seed=2)
    E, F = surface32(h.pos)
    h.step([E], F)
    moved = h.pos.copy()
    F[2, 1] = np.nan
    h.step([E], F)
    assert h.status() == (1, 2) and np.array_equal(h.pos, moved)
    # a force that is not finite at a LAUNCH step, whose sums are otherwise of positions and velocities: found before the half-step
    h = mirror(seed=2)
    while h.phase[0] != HP.LAUNCH:
        E, F = surface32(h.pos)
        h.step([E], F)
    step, at, vel = h.status()[0], h.pos.copy(), h.vel.copy()
    E, F = surface32(h.pos)
    F[0, 0] = np.inf
    h.step([E], F)
    assert h.status() == (step, 2) and np.array_equal(h.pos, at) and np.array_equal(h.vel, vel) and h.phase[0] == HP.LAUNCH
