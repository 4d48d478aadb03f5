"""No GPU: the distance constraints of the device-resident MD loop.  csrc/tn_md_cons_math.h, compiled host-only by
tests/md_cons_host_mirror.py, against tests/md_cons_oracle.py (fp64, Newton on the full nonlinear system, a direct solve for the
velocities - no Gauss-Seidel); the host logic of torchmdnet_amd/md.py (clusters, refusals, hydrogen_pairs, ndof); the additive C
ABI."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import md_cons_host_mirror as M
from tests import md_cons_oracle as O
from tests import md_host_mirror as H
from torchmdnet_amd import md as MD
from torchmdnet_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 9.648533e-3
DT, TOL = 2.0, 1e-6
EPS = 2.0 ** -23

ORACLE_X, ORACLE_V = M.ORACLE_X, M.ORACLE_V


def _bits(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def _water():
    a = np.deg2rad(104.52)
    return np.array([[0, 0, 0], [0.9572, 0, 0], [0.9572 * np.cos(a), 0.9572 * np.sin(a), 0]])


def _case(name):
    """-> x [n,3] fp64, mass [n], pairs"""
    if name == "diatomic":
        return np.array([[0.1, 0.2, 0.3], [1.1, 0.2, 0.3]]), np.array([12.0, 1.008]), [(0, 1)]
    if name in ("water", "water_far"):
        x = _water() + (100.0 if name == "water_far" else 0.0) * np.array([1.0, -1.0, 0.7])
        return x, np.array([15.999, 1.008, 1.008]), [(0, 1), (0, 2), (1, 2)]
    if name == "ch4":
        t = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) * 1.09 / np.sqrt(3)
        return np.vstack([np.zeros((1, 3)), t]) + 0.5, np.array([12.011] + [1.008] * 4), [(0, k) for k in range(1, 5)]
    if name == "cube":  # 8 atoms, the 12 edges: the limits of a cluster
        x = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64)
        pairs = [(a, b) for a in range(8) for b in range(a + 1, 8) if abs(np.abs(x[a] - x[b]).sum() - 1) < 1e-9]
        assert len(pairs) == 12
        return x * 1.1, np.linspace(1.0, 16.0, 8), pairs
    if name == "wall":  # one end at m = inf
        return np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([np.inf, 1.008]), [(0, 1)]
    raise KeyError(name)


CASES = ["diatomic", "water", "ch4", "cube", "wall", "water_far"]


def _setup(name, seed=0, kick=1.0):
    x, mass, pairs = _case(name)
    rng = np.random.default_rng(100 + seed)
    n = len(x)
    x = x.astype(np.float32)
    v = (0.02 * rng.normal(size=(n, 3))).astype(np.float32)
    f = [(kick * 2.0 * rng.normal(size=(n, 3))).astype(np.float32) for _ in range(2)]
    v[np.isinf(mass)] = 0.0
    con = MD.prepare_constraints(dict(pairs=torch.tensor(pairs), tol=TOL), torch.from_numpy(x), torch.zeros(n, dtype=torch.long),
                                 torch.from_numpy(mass), 1)
    hk = (0.5 * DT * FS / mass).astype(np.float32)
    w = 1.0 / mass.astype(np.float32).astype(np.float64)
    return x, v, f, mass.astype(np.float32), hk, w, pairs, con


def _residual_x(x, con):
    res, bound = MD.constraint_residuals(torch.from_numpy(np.asarray(x)), con["pairs"], con["lengths"], con["tol"])
    return res.numpy(), bound.numpy()


def _residual_v(x, v, con, dt):
    """-> |r.(v_a - v_b)| and its bound per pair.  The iteration stops with |r.u| dt <= tol d^2 on fp64 velocities; rounding the six
    components to fp32 then changes each by at most 2^-24 |v|, so r.u by at most sum_d |r_d| 2 * 2^-24 max|v| <= sqrt(3) |r| 2^-23
    max|v| < 2 * 2^-23 |r| max|v|:       |r.u| <= tol d^2 / dt + 2 * 2^-23 |r| max|v|."""
    x, v = np.asarray(x, np.float64), np.asarray(v, np.float64)
    p = con["pairs"].numpy()
    r, u = x[p[:, 0]] - x[p[:, 1]], v[p[:, 0]] - v[p[:, 1]]
    d = con["lengths"].numpy()
    vmax = np.maximum(np.abs(v[p[:, 0]]).max(1), np.abs(v[p[:, 1]]).max(1))
    return np.abs((r * u).sum(1)), con["tol"] * d * d / dt + 2 * EPS * np.linalg.norm(r, axis=1) * vmax


@pytest.fixture(scope="module")
def runs():
    """every case once: projection, OPEN, CLOSE by the header, and the oracle on the same fp32 inputs"""
    out = {}
    for k, name in enumerate(CASES):
        x, v, f, mass, hk, w, pairs, con = _setup(name, k)
        d = con["lengths"].numpy()
        p0 = M.advance(0, 0, con, x, v, None, None, mass, DT, tol=TOL)
        a = M.advance(0, 1, con, x, p0["vel"], f[0], hk, mass, DT, tol=TOL)
        b = M.advance(1, 0, con, a["pos"], a["vel"], f[1], hk, mass, DT, tol=TOL, x_keep=a["x_keep"], v_keep=a["v_keep"])
        ox, ov = O.open_step(x, p0["vel"], f[0], hk, DT, w, pairs, d)
        ov2 = O.close_step(a["pos"], a["vel"], f[1], hk, w, pairs)
        out[name] = dict(x=x, v=v, f=f, mass=mass, hk=hk, w=w, pairs=pairs, con=con, p0=p0, a=a, b=b, ox=ox, ov=ov, ov2=ov2,
                         ov0=O.rattle(x, v, w, pairs))
    return out


@pytest.mark.parametrize("name", CASES)
def test_position_residual_after_shake(runs, name):
    """after S every | |r| - d | / d <= tol + 2 * 2^-23 max|x| / d"""
    r = runs[name]
    assert r["a"]["fail"] == 0 and not _bits(r["a"]["pos"], r["x"])
    res, bound = _residual_x(r["a"]["pos"], r["con"])
    print(name, "position residual / bound", (res / bound).max())
    assert (res <= bound).all()
    # without S the drift breaks the constraints by far more than the bound: the test can fail
    free = MD.build_clusters(torch.zeros(0, 2, dtype=torch.long), len(r["x"]))
    free["constraint_d2"] = torch.zeros(0, dtype=torch.float64)
    u = M.advance(0, 1, free, r["x"], r["p0"]["vel"], r["f"][0], r["hk"], r["mass"], DT)
    assert (_residual_x(u["pos"], r["con"])[0] > 100 * bound).any()


@pytest.mark.parametrize("name", CASES)
def test_velocity_residual_after_rattle(runs, name):
    r = runs[name]
    for key, x in (("p0", r["x"]), ("b", r["a"]["pos"])):
        assert r[key]["fail"] == 0
        res, bound = _residual_v(x, r[key]["vel"], r["con"], DT)
        print(name, key, "velocity residual / bound", (res / bound).max())
        assert (res <= bound).all()
    res, bound = _residual_v(r["x"], r["v"], r["con"], DT)  # the velocities as drawn break it by far more: the test can fail
    assert (res > 10 * bound).any()


def test_agreement_with_the_newton_oracle(runs):
    """|header - oracle| in units of max(1, max|x|) for the positions and the half-step velocities (which take up Dx / dt): both
    carry the rounding of x to fp32, which grows with |x|; the projected velocities in absolute terms."""
    ex = ev = 0.0
    for name, r in runs.items():
        scale = max(1.0, float(np.abs(r["x"]).max()))
        dx = np.abs(r["a"]["pos"] - r["ox"]).max() / scale
        dv = max(np.abs(r["a"]["vel"] - r["ov"]).max() / scale, np.abs(r["b"]["vel"] - r["ov2"]).max(),
                 np.abs(r["p0"]["vel"] - r["ov0"]).max())
        print(name, "max |header - oracle|: x", dx, "v", dv)
        ex, ev = max(ex, dx), max(ev, dv)
    print("largest difference to the oracle: x", ex, "v", ev, "asserted", ORACLE_X, ORACLE_V)
    assert ex <= ORACLE_X and ev <= ORACLE_V


@pytest.mark.parametrize("name", [c for c in CASES if c != "wall"])
def test_momentum_of_a_cluster_is_unchanged(runs, name):
    """sum m v is changed neither by S (against the velocities after B alone) nor by R (against B alone), up to n 2^-23 sum |m v|.
    (Not the case with an end of infinite mass: a wall takes up momentum - test_an_end_of_infinite_mass_does_not_move.)"""
    r = runs[name]
    m = r["mass"].astype(np.float64)
    n = len(m)
    _, v_b = H.open_step(r["x"], r["p0"]["vel"], r["f"][0], r["hk"], DT)  # B, A without S
    v_c, _ = H.close_step(r["a"]["vel"], r["f"][1], r["hk"], r["mass"])  # B without R
    for got, ref in ((r["a"]["vel"], v_b), (r["b"]["vel"], v_c), (r["p0"]["vel"], r["v"])):
        pg, pr = (m[:, None] * got).sum(0), (m[:, None] * ref).sum(0)
        assert np.abs(pg - pr).max() <= n * EPS * np.abs(m[:, None] * ref).sum()
        assert not _bits(got, ref)


def test_an_end_of_infinite_mass_does_not_move(runs):
    r = runs["wall"]
    for key in ("p0", "a", "b"):
        assert _bits(r[key]["vel"][0], r["v"][0]) and (r[key]["vel"][0] == 0).all()
    assert _bits(r["a"]["pos"][0], r["x"][0]) and not _bits(r["a"]["pos"][1], r["x"][1])
    assert r["b"]["part"][0] == 0 and r["b"]["part"][1] > 0


def _mixed():
    """two waters, a CH3-like group, and seven atoms in no constraint, interleaved"""
    rng = np.random.default_rng(5)
    x = np.vstack([_water(), rng.normal(size=(2, 3)) + 5, _water() + 9.0, rng.normal(size=(5, 3)) - 5,
                   np.array([[0, 0, 0], [1.09, 0, 0], [0, 1.09, 0], [0, 0, 1.09]]) + 20.0]).astype(np.float32)
    pairs = [(0, 1), (0, 2), (1, 2), (5, 6), (5, 7), (6, 7), (13, 14), (13, 15), (13, 16)]
    n = len(x)
    mass = rng.uniform(1.0, 16.0, n).astype(np.float32)
    mass[9] = np.inf
    v = (0.02 * rng.normal(size=(n, 3))).astype(np.float32)
    v[9] = 0
    f = [(2.0 * rng.normal(size=(n, 3))).astype(np.float32) for _ in range(3)]
    free = np.array([3, 4, 8, 9, 10, 11, 12])
    return x, v, f, mass, pairs, free


@pytest.mark.parametrize("thermostat", [False, True])
def test_free_atoms_are_bit_equal_to_the_unconstrained_mirror(thermostat):
    x, v, f, mass, pairs, free = _mixed()
    n = len(x)
    con = MD.prepare_constraints(dict(pairs=torch.tensor(pairs)), torch.from_numpy(x), torch.zeros(n, dtype=torch.long),
                                 torch.from_numpy(mass), 1)
    assert con["n_bound"] == 3 and con["cluster_atoms"].shape[0] == 4
    hk = (0.5 * DT * FS / mass.astype(np.float64)).astype(np.float32)
    sigma = np.sqrt(0.025 * FS / mass.astype(np.float64)).astype(np.float32) if thermostat else None
    c1, c2, seed = (0.98, float(np.sqrt(1 - 0.98 ** 2)), 77) if thermostat else (1.0, 0.0, 0)
    p0 = M.advance(0, 0, con, x, v, None, None, mass, DT)
    assert _bits(p0["vel"][free], v[free]) and not _bits(p0["vel"], v)
    a = M.advance(0, 1, con, x, p0["vel"], f[0], hk, mass, DT, sigma, c1, c2, seed, 5)
    hx, hv = H.open_step(x, v, f[0], hk, DT)
    assert _bits(a["pos"][free], hx[free]) and _bits(a["vel"][free], hv[free]) and _bits(a["x_keep"], x)
    b = M.advance(1, 1, con, a["pos"], a["vel"], f[1], hk, mass, DT, sigma, c1, c2, seed, 5, x_keep=a["x_keep"], v_keep=a["v_keep"])
    hv1, hke = H.close_step(hv, f[1], hk, mass, sigma, c1, c2, seed, 5)  # the noise is keyed by the atom's own index
    hx2, hv2 = H.open_step(hx, hv1, f[1], hk, DT)
    assert _bits(b["pos"][free], hx2[free]) and _bits(b["vel"][free], hv2[free]) and _bits(b["part"][free], hke[free])
    c = M.advance(1, 0, con, b["pos"], b["vel"], f[2], hk, mass, DT, sigma, c1, c2, seed, 6, x_keep=b["x_keep"], v_keep=b["v_keep"])
    hv3, hke3 = H.close_step(hv2, f[2], hk, mass, sigma, c1, c2, seed, 6)
    assert _bits(c["vel"][free], hv3[free]) and _bits(c["part"][free], hke3[free]) and _bits(c["pos"], b["pos"])
    # a constrained atom: the kinetic term is that of the projected, rounded velocity, by the same expression
    bound = np.setdiff1d(np.arange(n), free)
    _, ke = H.close_step(c["vel"], np.zeros_like(x), np.zeros_like(hk), mass)
    assert _bits(c["part"][bound], ke[bound]) and c["fail"] == 0
    res, lim = _residual_x(c["pos"], con)
    assert (res <= lim).all()
    res, lim = _residual_v(c["pos"], c["vel"], con, DT)
    assert (res <= lim).all()


def test_failure_returns_the_saved_state():
    """max_iter = 1 on a strongly kicked triangle: the fail word, and x_keep / v_keep with all bits intact"""
    x, v, f, mass, hk, w, pairs, con = _setup("water", 9, kick=8.0)
    a = M.advance(0, 1, con, x, v, f[0], hk, mass, DT, tol=TOL, max_iter=1)
    assert a["fail"] == M.FAIL_SHAKE
    assert _bits(a["pos"], x) and _bits(a["vel"], v) and _bits(a["x_keep"], x) and _bits(a["v_keep"], v)
    ok = M.advance(0, 1, con, x, v, f[0], hk, mass, DT, tol=TOL, max_iter=64)
    assert ok["fail"] == 0 and (_residual_x(ok["pos"], con)[0] <= _residual_x(ok["pos"], con)[1]).all()
    # the velocities: CLOSE restores the state saved by the opening half
    b = M.advance(1, 0, con, ok["pos"], ok["vel"], f[1], hk, mass, DT, tol=TOL, max_iter=1, x_keep=ok["x_keep"], v_keep=ok["v_keep"])
    assert b["fail"] == M.FAIL_RATTLE and _bits(b["pos"], x) and _bits(b["vel"], v) and np.isnan(b["part"]).all()
    # a NaN force is a failure too, never "within tolerance"
    f_nan = f[0].copy()
    f_nan[1, 0] = np.nan
    c = M.advance(0, 1, con, x, v, f_nan, hk, mass, DT, tol=TOL)
    assert c["fail"] == M.FAIL_SHAKE and _bits(c["pos"], x) and np.isfinite(c["pos"]).all() and np.isfinite(c["vel"]).all()


def test_standalone_program_under_the_host_sanitizers(tmp_path):
    """tests/md_cons_host.hip with its own main, built with -fsanitize=address,undefined and run as a program of its own"""
    exe = M.build_program(str(tmp_path / "md_cons_host_san"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "md_cons_host: fail 0, forced fail 1" in out.stdout


# ------------------------------------------------------------------------------------------------ host logic
def test_clusters_are_the_connected_components():
    pairs = torch.tensor([[7, 5], [0, 1], [5, 6], [0, 2], [10, 11], [1, 2]])
    t = MD.build_clusters(pairs, 14)
    assert t["n_bound"] == 3
    assert t["cluster_atoms"].tolist() == [[0, 1, 2] + [-1] * 5, [5, 6, 7] + [-1] * 5, [10, 11] + [-1] * 6,
                                           [3, 4, 8, 9, 12, 13, -1, -1]]
    assert t["cluster_offsets"].tolist() == [0, 3, 5, 6, 6]
    assert t["order"].tolist() == [1, 3, 5, 0, 2, 4]  # the caller's order inside a cluster
    assert t["constraint_ends"].tolist() == [[0, 1], [0, 2], [1, 2], [2, 0], [0, 1], [0, 1]]
    every = sorted(a for row in t["cluster_atoms"].tolist() for a in row if a >= 0)
    assert every == list(range(14))
    # nine free atoms: two clusters without constraints
    t = MD.build_clusters(torch.zeros(0, 2, dtype=torch.long), 9)
    assert t["n_bound"] == 0 and t["cluster_atoms"].shape == (2, 8) and t["cluster_offsets"].tolist() == [0, 0, 0]


def test_cluster_limits_and_refusals():
    star = [[0, k] for k in range(1, 8)]  # 8 atoms, 7 constraints: fits
    assert MD.build_clusters(torch.tensor(star), 9)["n_bound"] == 1
    with pytest.raises(ValueError, match="cluster of atom 0 has 9 atoms"):
        MD.build_clusters(torch.tensor(star + [[0, 8]]), 9)
    k6 = [[a, b] for a in range(6) for b in range(a + 1, 6)]  # 6 atoms, 15 constraints
    with pytest.raises(ValueError, match="6 atoms and 15 constraints"):
        MD.build_clusters(torch.tensor(k6), 6)
    batch = torch.tensor([0, 0, 0, 1, 1, 1])
    mass = torch.tensor([12.0, 1.0, float("inf"), float("inf"), 1.0, 1.0])
    for bad, msg in (([[0, 6]], "outside"), ([[-1, 2]], "outside"), ([[1, 1]], "itself"), ([[0, 1], [1, 0]], "duplicate"),
                     ([[2, 3]], "joins molecules 0 and 1"), ([[0, 1], [4, 5], [1, 4]], "joins molecules")):
        with pytest.raises(ValueError, match=msg):
            MD.build_clusters(torch.tensor(bad), 6, batch, mass)
    with pytest.raises(ValueError, match="infinite mass"):
        MD.build_clusters(torch.tensor([[2, 3]]), 6, None, mass)
    with pytest.raises(ValueError, match=r"\[C,2\]"):
        MD.build_clusters(torch.tensor([0, 1, 2]), 6)
    pos = torch.randn(6, 3, generator=torch.Generator().manual_seed(1))
    for bad in (dict(pairs=[[0, 1]], sweeps=3), dict(lengths=[1.0]), dict(pairs=[[0, 1]], tol=0.0), dict(pairs=[[0, 1]], max_iter=0),
                dict(pairs=[[0, 1]], lengths=[1.0, 2.0]), dict(pairs=[[0, 1]], lengths=[-1.0])):
        with pytest.raises(ValueError):
            MD.prepare_constraints(bad, pos, batch, mass, 2)
    with pytest.raises(ValueError, match=r"worst is pair 1 = \(4, 5\)"):  # the positions must satisfy the constraints
        MD.prepare_constraints(dict(pairs=[[0, 1], [4, 5]], lengths=[float((pos[0] - pos[1]).norm()), 0.5]), pos, batch, mass, 2)
    ok = MD.prepare_constraints(dict(pairs=[[0, 1], [4, 5]]), pos, batch, mass, 2)
    assert abs(float(ok["lengths"][1]) - float((pos[4].double() - pos[5].double()).norm())) < 1e-15
    assert ok["tol"] == 1e-6 and ok["max_iter"] == 64
    assert ok["ndof"].tolist() == [3 * 2 - 1, 3 * 2 - 1]  # three per atom of finite mass, minus the molecule's constraints


def test_hydrogen_pairs_water_box():
    z, pos, _ = W.water_box(n_side=2)  # 8 waters
    p = MD.hydrogen_pairs(z, pos)
    assert p.shape == (16, 2) and p.dtype == torch.int64
    assert (z[p[:, 0]] == 8).all() and (z[p[:, 1]] == 1).all() and sorted(p[:, 1].tolist()) == (z == 1).nonzero().reshape(-1).tolist()
    assert ((pos[p[:, 0]] - pos[p[:, 1]]).norm(dim=1) < 1.3).all()
    r = MD.hydrogen_pairs(z, pos, rigid_water=True)
    assert r.shape == (24, 2) and torch.equal(r[:16], p) and (z[r[16:]] == 1).all()
    t = MD.build_clusters(r, z.shape[0])
    assert t["n_bound"] == 8 and t["cluster_atoms"].shape[0] == 8 and (t["cluster_offsets"][1:] - t["cluster_offsets"][:-1] == 3).all()
    con = MD.prepare_constraints(dict(pairs=r), pos, torch.zeros_like(z), torch.where(z == 1, 1.008, 15.999), 1)
    assert con["ndof"].tolist() == [3 * 24 - 24]


def test_hydrogen_pairs_methane_and_ammonia():
    t = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) * 1.09 / np.sqrt(3)
    ch4 = np.vstack([np.zeros((1, 3)), t])
    nh3 = np.array([[0, 0, 0], [0.94, 0, -0.38], [-0.47, 0.81, -0.38], [-0.47, -0.81, -0.38]]) + np.array([0.3, 0.2, 0.9])
    # the two molecules overlap in space: only `batch` keeps an H of one from the heavy atom of the other
    z = torch.tensor([6, 1, 1, 1, 1, 7, 1, 1, 1])
    pos = torch.from_numpy(np.vstack([ch4, nh3])).float()
    batch = torch.tensor([0] * 5 + [1] * 4)
    p = MD.hydrogen_pairs(z, pos, batch, rigid_water=True)
    assert p.tolist() == [[0, 1], [0, 2], [0, 3], [0, 4], [5, 6], [5, 7], [5, 8]]  # no H-H pair: neither is a water
    merged = MD.hydrogen_pairs(z, pos)
    assert merged.shape == (7, 2) and merged.tolist() != p.tolist()
    assert MD.hydrogen_pairs(z, pos, batch, cutoff=1.05).tolist() == [[5, 6], [5, 7], [5, 8]]  # N-H = 1.014, C-H = 1.09 is outside
    con = MD.prepare_constraints(dict(pairs=p), pos, batch, torch.tensor([12.011] + [1.008] * 4 + [14.007] + [1.008] * 3), 2)
    assert con["ndof"].tolist() == [15 - 4, 12 - 3] and con["n_bound"] == 2
    # a hydroxide-like O with one H, and an O with two H and a heavy neighbour inside the cutoff: no rigid water
    z2 = torch.tensor([8, 1, 8, 1, 1, 6])
    pos2 = torch.tensor([[0, 0, 0], [0.96, 0, 0], [5, 0, 0], [5.96, 0, 0], [4.76, 0.93, 0], [5, 0, 1.2]], dtype=torch.float32)
    assert MD.hydrogen_pairs(z2, pos2, rigid_water=True).tolist() == [[0, 1], [2, 3], [2, 4]]


def test_header_is_additive_and_declares_the_constraint_entries():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("tmdnet_md_constraints_workspace_bytes", "tmdnet_md_advance_constrained", "tmdnet_md_advance", "tmdnet_md_status",
                 "tmdnet_md_barostat"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    for name, value in (("TMDNET_MD_OPEN", 0), ("TMDNET_MD_MIDDLE", 1), ("TMDNET_MD_CLOSE", 2), ("TMDNET_MD_PROJECT", 3)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", code), name
    args = re.search(r"\bint\s+tmdnet_md_advance\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(args.split(",")) == 22  # the unconstrained entry keeps its signature
    args = re.search(r"\bint\s+tmdnet_md_advance_constrained\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(args.split(",")) == 22 + 1 + 8
    from torchmdnet_amd import _C

    assert "tmdnet_md_advance_constrained" in _C.declared_symbols()


def test_library_exports_the_constraint_entries(hip_lib):
    import ctypes as C

    assert hasattr(hip_lib, "tmdnet_md_advance_constrained") and hip_lib.tmdnet_abi_version() == 10
    nb = C.c_size_t(0)
    assert hip_lib.tmdnet_md_constraints_workspace_bytes(192, 64, 192, C.byref(nb)) == 0 and nb.value >= 260
    assert hip_lib.tmdnet_md_constraints_workspace_bytes(192, 1, 13, C.byref(nb)) != 0  # more than 12 constraints per cluster
    assert hip_lib.tmdnet_md_constraints_workspace_bytes(-1, 1, 1, C.byref(nb)) != 0


def test_capture_md_keeps_its_signature_and_constraints_come_after_it():
    """``capture_md`` is as it was (tests/test_md_barostat_host.py pins ``barostat`` as its last parameter); the entry that takes
    ``constraints`` has every one of its parameters in its place, with its default, and ``constraints`` after them"""
    from torchmdnet_amd.models.model import TorchMD_Net

    old = inspect.signature(TorchMD_Net.capture_md).parameters
    assert list(old) == ["self", "z", "pos", "vel", "masses", "dt", "batch", "box", "q", "num_systems", "steps_per_replay", "force_scale",
                         "thermostat", "warmup", "atom_weights", "halo_exchange", "barostat"]
    new = inspect.signature(TorchMD_Net.capture_md_constrained).parameters
    assert list(new) == list(old) + ["constraints"] and new["constraints"].default is None
    assert all(new[k].default == old[k].default and new[k].kind == old[k].kind for k in old)
