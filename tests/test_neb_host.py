"""No GPU: the arithmetic of the device-resident nudged elastic band (csrc/tn_neb_math.h, compiled host-only by
tests/neb_host_mirror.py) against tests/neb_oracle.py - the scheme in fp64, written from the equations.  1. the tangent table,
2. the single-rounded per-atom operations, 3. whole band optimisations on the analytic surface in both precisions, 4. the additive
ABI and the signatures, 5. the sanitizers on a stand-alone program."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import neb_host_mirror as H
from tests import neb_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(O.MO.FIRE, fmax=1e-3)  # ASE's defaults, the bound of the surface runs
NAN = float("nan")

# name, the band's five energies, (w+, w-) expected at image 2 (None: the image is unusable), the climber
TABLE = [
    ("rising", [0, 1, 2, 3, 4], (1.0, 0.0), 3),
    ("falling", [4, 3, 2, 1, 0], (0.0, 1.0), 1),
    ("maximum, E_next above E_prev", [0, 1, 3, 2, 0], (2.0, 1.0), 2),
    ("maximum, E_next below E_prev", [0, 2, 3, 1, 0], (1.0, 2.0), 2),
    ("minimum, E_next below E_prev", [0, 3, 1, 2, 0], (1.0, 2.0), 1),
    ("minimum, E_next above E_prev", [0, 2, 1, 3, 0], (2.0, 1.0), 3),
    ("tie with the previous image", [0, 1, 1, 2, 0], (1.0, 0.0), 3),
    ("tie with the next image", [0, 2, 1, 1, 0], (0.0, 1.0), 1),
    ("neighbours tied", [0, 2, 1, 2, 0], (1.0, 1.0), 1),
    ("tied maxima: the lowest index climbs", [0, 3, 1, 3, 0], (2.0, 2.0), 1),
    ("fp32 neighbours", [0, 1, 1 + 2.0 ** -23, 1 + 2.0 ** -22, 0], (1.0, 0.0), 3),
    ("all tied: no tangent", [1, 1, 1, 1, 1], None, 1),
    ("a NaN energy", [0, 1, NAN, 1, 0], None, None),
    ("an infinite endpoint energy", [float("inf"), 1, 2, 1, 0], None, None),
]


def _bits32(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _dyadic_band(rng, G, M=5, n=4):
    """positions on a grid of 1/8, forces on a grid of 1/4: every fp32 product and sum of the path terms is exact, so the header's
    sums equal the oracle's and the comparison is about the coefficients alone"""
    pos = rng.integers(-8, 9, size=(G, M, n, 3)).astype(np.float32) / 8
    f = rng.integers(-12, 13, size=(G, M, n, 3)).astype(np.float32) / 4
    return pos, f


def test_tangent_table_equals_the_oracle():
    """Every branch of the tangent, the climber's choice, climbing on and off, both spring constants, the unusable inputs.  w+ and
    w- equal; s+ and s- within 1 fp32 ulp of the oracle working from its own fp64 sums (measured: 0)."""
    rng = np.random.default_rng(5)
    G = len(TABLE)
    pos, f = _dyadic_band(rng, G + 1)
    pos[G, 1] = pos[G, 2] = pos[G, 3]  # one more band: coincident images under the rising energies
    e = np.array([c[1] for c in TABLE] + [TABLE[0][1]], np.float32)
    fixed = np.array([0, 0, 1, 0], np.uint8)
    sums = H.path_sums(pos, f, fixed)
    worst = 0
    for k in (0.1, 1.0):
        for climb in (0, 1):
            w, s, why, top = H.image_control(e, sums, k, climb)
            for b in range(G + 1):
                name = TABLE[b][0] if b < G else "coincident images"
                S64 = O.path_sums(pos[b], f[b], fixed)
                assert (S64 == sums[b]).all(), name  # exact terms
                for i in (1, 2, 3):
                    cause, wo, so = O.image_control(e[b], i, S64[i], k, climb)
                    assert why[b, i] == cause, (name, i)
                    assert tuple(w[b, i]) == wo, (name, i, w[b, i], wo)
                    d = O.MO.ulp_distance(s[b, i], np.array(so, np.float32)).max()
                    worst = max(worst, int(d))
                    assert d <= 1, (name, i, s[b, i], so)
                    if cause:
                        assert (s[b, i] == 0).all(), name
                    if cause == O.BAD_ENERGY:
                        assert (w[b, i] == 0).all(), name
                if b == G:
                    assert why[b].tolist() == [0, O.BAD_PATH, O.BAD_PATH, 0, 0]  # (rising: tau = d+, and image 3 still has one)
                    continue
                _, _, expect, climber = TABLE[b]
                if climber is None:
                    assert (why[b, 1:4] == O.BAD_ENERGY).all(), name
                    continue
                assert top[b] == climber == O.climber(e[b]), name
                if expect is None:
                    assert why[b, 2] == O.BAD_PATH, name
                else:
                    scale = w[b, 2].max() / max(expect)  # the weights are energy differences: the table states their ratio
                    assert why[b, 2] == 0 and tuple(w[b, 2] / scale) == expect, (name, w[b, 2])
            # endpoints carry nothing
            assert (w[:, [0, 4]] == 0).all() and (s[:, [0, 4]] == 0).all() and (why[:, [0, 4]] == 0).all()
    print("largest distance of s from the oracle on its own sums:", worst, "ulp")
    # climbing changes the climber's coefficients and nobody else's
    _, s0, _, top = H.image_control(e, sums, 0.1, 0)
    _, s1, _, _ = H.image_control(e, sums, 0.1, 1)
    for b in range(G):
        if TABLE[b][3] is None or (H.image_control(e, sums, 0.1, 0)[2][b] != 0).any():
            continue
        for i in (1, 2, 3):
            same = (_bits32(s0[b, i]) == _bits32(s1[b, i])).all()
            assert same == (i != top[b]), (TABLE[b][0], i)


def test_coefficients_equal_the_oracle_bit_for_bit_on_the_headers_sums():
    """Random bands, the oracle fed with the header's sums: no transcendental but sqrt, no FMA in the x86-64 baseline - the header's
    fp64 statements and the oracle's are the same IEEE operations."""
    rng = np.random.default_rng(6)
    G, M, n = 60, 6, 7
    pos = rng.normal(size=(G, M, n, 3)).astype(np.float32)
    f = (3 * rng.normal(size=(G, M, n, 3))).astype(np.float32)
    e = rng.normal(size=(G, M)).astype(np.float32)
    e[::7, 3] = e[::7, 2]  # some exact ties
    sums = H.path_sums(pos, f)
    near = O.path_sums(pos[0], f[0])
    assert np.abs(sums[0] - near).max() < 1e-4 and (sums[0] != near).any()  # fp32 terms: close to, not equal to, the fp64 sums
    branches = set()
    for climb in (0, 1):
        w, s, why, top = H.image_control(e, sums, 0.37, climb)
        assert (why == 0).all()
        for b in range(G):
            assert top[b] == O.climber(e[b])
            for i in range(1, M - 1):
                cause, wo, so = O.image_control(e[b], i, sums[b, i], 0.37, climb)
                assert cause == 0 and tuple(w[b, i]) == wo
                assert (_bits32(s[b, i]) == _bits32(so)).all(), (b, i, s[b, i], so)
                branches.add((wo[0] == 1.0, wo[1] == 1.0, bool(climb) and top[b] == i))
    # rising, falling, extremum; the climber is an extremum or (next to an endpoint) on a slope
    assert {(True, False, False), (False, True, False), (False, False, False), (False, False, True)} <= branches, branches


def test_terms_and_projection_are_single_rounded_operations():
    rng = np.random.default_rng(7)
    G, M, n = 3, 5, 50
    pos = (6 * rng.normal(size=(G, M, n, 3))).astype(np.float32)
    f = (3 * rng.normal(size=(G, M, n, 3))).astype(np.float32)
    fixed = (rng.uniform(size=n) < 0.15).astype(np.uint8)
    inner = np.zeros((G, M, n), bool)
    inner[:, 1:-1] = True
    dp, dm = np.zeros_like(pos), np.zeros_like(pos)
    dp[:, 1:-1] = pos[:, 2:] - pos[:, 1:-1]  # numpy fp32: every operation rounds
    dm[:, 1:-1] = pos[:, 1:-1] - pos[:, :-2]
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    ref = np.stack([dot(dp, dp), dot(dm, dm), dot(dp, dm), dot(f, dp), dot(f, dm)], -1)
    ref = np.where((inner & (fixed == 0))[..., None], ref, np.float32(0)).astype(np.float32)
    t = H.path_terms(pos, f, fixed)
    assert (_bits32(t) == _bits32(ref)).all()
    assert (H.path_terms(pos, f)[:, 1:-1][:, :, fixed != 0] != 0).all()
    s = rng.uniform(-1, 1, size=(G, M, 2)).astype(np.float32)
    fn = H.project(pos, f, s, fixed)
    proj = (f + s[..., 0, None, None] * dp) + s[..., 1, None, None] * dm
    proj = np.where(inner[..., None], np.where((fixed != 0)[:, None], f, proj), np.float32(0)).astype(np.float32)
    assert (_bits32(fn) == _bits32(proj)).all()
    # the update: endpoints, fixed atoms and converged bands keep x bit for bit and get v = 0
    v = (0.05 * rng.normal(size=pos.shape)).astype(np.float32)
    coef = rng.uniform(0.1, 1.0, size=(G, 3)).astype(np.float32)
    conv = np.array([-1, 9, -1])
    x2, v2 = H.move(conv, coef, pos, v, fn, fixed)
    still = ~inner | (fixed != 0)[None, None, :] | (conv >= 0)[:, None, None]
    c = coef[:, None, None, :]
    v_ref = np.where(still[..., None], np.float32(0), c[..., 0:1] * v + c[..., 1:2] * fn)
    x_ref = np.where(still[..., None], pos, pos + c[..., 2:3] * v_ref)
    assert (_bits32(v2) == _bits32(v_ref)).all() and (_bits32(x2) == _bits32(x_ref)).all()
    assert (x2[~still] != pos[~still]).any() and still.sum() > 300
    # the FIRE sums: the fp32 terms of tn_min added per image, the images in image order
    S = H.fire_sums(v, fn, fixed)
    free = (fixed == 0)
    for b in range(G):
        tt = np.stack([dot(fn[b], v[b]), dot(fn[b], fn[b]), dot(v[b], v[b])], -1).astype(np.float64)[1:-1][:, free]
        exact = tt.sum((0, 1))
        assert np.abs(S[b, :3] - exact).max() <= 1e-12 * np.abs(tt).sum() and S[b, 3] == tt[..., 1].max()


# ---- 3. the analytic surface ---------------------------------------------------------------------------------------------------------
# steps to convergence found, k = 0.1, fmax = 1e-3, seed 0 - fp32 header and fp64 oracle agree on every one:
STEPS = {(5, 1): dict(climb=69, plain=81), (7, 3): dict(climb=100, plain=100), (9, 40): dict(climb=204, plain=172)}


@pytest.mark.parametrize("M,n", sorted(STEPS))
def test_climbing_band_finds_the_saddle_in_fp32_and_fp64(M, n):
    """The surface of tests/neb_oracle.py, atom 0 from (-1, 0, 0) to (1, 0, 0), the interior images perturbed.  Both precisions
    converge; the climber's atom 0 is within 2 sqrt(n) fmax / 4 of (0, A, 0) and the barrier within (sqrt(n) fmax)^2 / 4 + fp32
    rounding of 1; without climbing the highest image is NOT within that distance.  Steps found: STEPS above."""
    x, sites = O.problem(M, n)
    r_bound, e_bound = O.position_bound(n, P["fmax"]), O.barrier_bound(n, P["fmax"])
    found = {}
    for name, climb in (("climb", 1), ("plain", 0)):
        s32, c32, x32, e32, top32 = H.run(x, sites, O.KAPPA, O.A, P, 0.1, climb, 400)
        s64, c64, x64, e64, top64 = O.run(x, sites, P, 0.1, climb, 400)
        found[name] = (s32, s64)
        assert 0 < s32 < 400 and 0 < s64 < 400 and c32[0] == s32 and c64[0] == s64
        assert top32[0] == top64[0]
        d32 = np.abs(x32[0, top32[0], 0].astype(np.float64) - O.SADDLE).max()
        d64 = np.abs(x64[0, top64[0], 0] - O.SADDLE).max()
        b32 = float(e32[0, top32[0]]) - float(e32[0, 0]) - 1.0
        b64 = e64[0, top64[0]] - e64[0, 0] - 1.0
        print(f"(M, n) = ({M}, {n}) {name}: steps {s32} / {s64}, distance {d32:.3e} / {d64:.3e} (bound {r_bound:.3e}), "
              f"barrier - 1 = {b32:.3e} / {b64:.3e} (bound {e_bound:.3e})")
        if climb:
            assert d32 < r_bound and d64 < r_bound
            assert abs(b32) < e_bound and abs(b64) < e_bound
        else:
            assert d32 > r_bound and d64 > r_bound  # climbing does something
        # endpoints kept their bits; the images stay ordered along x
        assert (_bits32(x32[0, [0, -1]]) == _bits32(x[0, [0, -1]])).all()
        assert (np.diff(x32[0, :, 0, 0]) > 0).all()
    assert found["climb"][0] == found["climb"][1] == STEPS[(M, n)]["climb"], found
    assert found["plain"][0] == found["plain"][1] == STEPS[(M, n)]["plain"], found


def test_stiffer_springs_fixed_atoms_and_two_bands():
    """k = 1.0 converges as well; a fixed atom keeps its bits in every image; two bands in one call run as they do alone (one
    controller per band), and an unusable band is reported by its cause."""
    xa, sites = O.problem(7, 3, seed=0)
    xb, _ = O.problem(7, 3, seed=2)
    xb[0, :, 1:] = xa[0, :, 1:]  # the same sites for atoms 1, 2; another perturbation of atom 0
    ra = H.run(xa, sites, O.KAPPA, O.A, P, 1.0, 1, 400)
    rb = H.run(xb, sites, O.KAPPA, O.A, P, 1.0, 1, 400)
    both = H.run(np.concatenate([xa, xb]), sites, O.KAPPA, O.A, P, 1.0, 1, 400)
    assert 0 < ra[0] < 400 and 0 < rb[0] < 400 and ra[0] != rb[0]
    assert both[1].tolist() == [ra[0], rb[0]] and both[0] == max(ra[0], rb[0])
    assert (_bits32(both[2][0]) == _bits32(ra[2][0])).all() and (_bits32(both[2][1]) == _bits32(rb[2][0])).all()
    assert np.abs(ra[2][0, ra[4][0], 0] - O.SADDLE).max() < O.position_bound(3, P["fmax"])
    fixed = np.array([0, 1, 0], np.uint8)
    rf = H.run(xa, sites, O.KAPPA, O.A, P, 1.0, 1, 400, fixed)
    assert 0 < rf[0] < 400 and (_bits32(rf[2][0, :, 1]) == _bits32(xa[0, :, 1])).all() and (rf[2][0, 1:-1, 2] != xa[0, 1:-1, 2]).any()
    assert rf[0] == O.run(xa, sites, P, 1.0, 1, 400, fixed)[0]
    every = H.run(xa, sites, O.KAPPA, O.A, P, 1.0, 1, 400, np.ones(3, np.uint8))  # no degree of freedom: converged as it stands
    assert every[0] == 0 and every[1].tolist() == [0] and (_bits32(every[2]) == _bits32(xa)).all()
    assert O.run(xa, sites, P, 1.0, 1, 400, np.ones(3, np.uint8))[0] == 0
    assert H.image_control(np.zeros((1, 5), np.float32), np.zeros((1, 5, 5)), 0.1, 0, has_free=False)[2].tolist() == [[0] * 5]
    assert H.image_control(np.zeros((1, 5), np.float32), np.zeros((1, 5, 5)), 0.1, 0)[2].tolist() == [[0, 2, 2, 2, 0]]
    bad = xa.copy()
    bad[0, 2] = bad[0, 3] = bad[0, 4]
    assert H.run(bad, sites, O.KAPPA, O.A, P, 1.0, 0, 10)[0] == -O.BAD_PATH
    bad = xa.copy()
    bad[0, 3, 0, 1] = NAN
    assert H.run(bad, sites, O.KAPPA, O.A, P, 1.0, 0, 10)[0] == -O.BAD_ENERGY


def test_surface_mirror_equals_the_oracle():
    x, sites = O.problem(6, 5, seed=3)
    e32, f32 = H.surface(x, sites, O.KAPPA, O.A)
    e64, f64 = O.surface(x, sites)
    assert np.abs(e32 - e64).max() <= 2.0 ** -24 * np.abs(e64).max() and np.abs(f32 - f64).max() <= 2.0 ** -24 * np.abs(f64).max()
    e, f = O.surface(O.SADDLE[None], np.zeros((1, 3)))
    assert e == 1.0 and (f == 0).all()
    h = 1e-6
    for d in range(3):  # the forces are the gradient
        xp, xm = x.astype(np.float64), x.astype(np.float64)
        xp[0, 2, 0, d] += h
        xm[0, 2, 0, d] -= h
        assert abs(-(O.surface(xp, sites)[0][0, 2] - O.surface(xm, sites)[0][0, 2]) / (2 * h) - f64[0, 2, 0, d]) < 1e-7


# ---- 4. the additive ABI ---------------------------------------------------------------------------------------------------------------
NEB_ENTRIES = (("tmdnet_neb_workspace_bytes", 4), ("tmdnet_neb_reset", 6), ("tmdnet_neb_advance", 34), ("tmdnet_neb_status", 3))


def test_header_and_bindings_are_additive():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from torchmdnet_amd import _C

    src = open(_C.__file__).read()
    for name, n_args in NEB_ENTRIES:
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == n_args, name
        assert name in _C.declared_symbols() and name + ".argtypes" in src
    for name, n_args in (("tmdnet_min_advance", 29), ("tmdnet_min_advance_cell", 41), ("tmdnet_md_advance", 22)):  # untouched
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == n_args, name
    # the arguments of tmdnet_min_advance in its order, batch and the two sizes replaced, spring_k after fmax, the new rows last
    strip = lambda a: " ".join(a.split())
    plain = [strip(a) for a in re.search(r"\bint\s+tmdnet_min_advance\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")]
    neb = [strip(a) for a in re.search(r"\bint\s+tmdnet_neb_advance\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")]
    kept = [a for a in plain if a not in ("int64_t n_atoms", "int64_t n_mol", "const int64_t* batch")]
    kept = [a.replace("min_ws", "neb_ws") for a in kept]
    assert neb[:4] == kept[:4] and neb[4:7] == ["int64_t n_atoms_per_image", "int64_t n_images", "int64_t n_bands"]
    assert neb[7:22] == kept[4:19] and neb[22] == "double spring_k" and neb[23:30] == kept[19:]
    assert neb[30:] == ["double* path_sums_log_row", "double* weights_log_row", "float* tangent_coef_log_row", "int32_t* climber_log_row"]


def test_library_exports_the_band_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10
    for name, n_args in NEB_ENTRIES:
        assert len(getattr(hip_lib, name).argtypes) == n_args, name
    small, large = C.c_size_t(0), C.c_size_t(0)
    assert hip_lib.tmdnet_neb_workspace_bytes(64, 7, 1, C.byref(small)) == 0 and small.value >= 256 + 7 * 64 * 36
    assert hip_lib.tmdnet_neb_workspace_bytes(1100, 3, 2, C.byref(large)) == 0 and large.value >= 256 + 6 * 1100 * 36 + 6 * 2 * 72
    for bad in ((64, 2, 1), (64, 7, 0), (-1, 7, 1)):
        assert hip_lib.tmdnet_neb_workspace_bytes(*bad, C.byref(small)) != 0
    # argument checks happen before anything is enqueued: no device is needed to be refused
    assert hip_lib.tmdnet_neb_reset(None, None, 0, 0.1, 0.1, 0) == 1
    assert hip_lib.tmdnet_neb_reset(None, C.c_void_p(256), 0, 0.0, 0.1, 0) == 1
    assert hip_lib.tmdnet_neb_reset(None, C.c_void_p(256), 0, 0.1, 0.1, 2) == 1


def test_capture_neb_and_module_signatures():
    from torchmdnet_amd import neb
    from torchmdnet_amd.models.model import TorchMD_Net

    sig = inspect.signature(TorchMD_Net.capture_neb).parameters
    assert list(sig)[1:] == ["z", "images", "box", "q", "steps_per_replay", "fmax", "spring", "climb", "fire", "fixed", "warmup"]
    defaults = {k: sig[k].default for k in list(sig)[3:]}
    assert defaults == dict(box=None, q=None, steps_per_replay=10, fmax=0.05, spring=0.1, climb=False, fire=None, fixed=None, warmup=3)
    assert neb.parse_neb(None) == dict(spring=0.1, climb=False)
    assert neb.parse_neb(dict(spring=2, climb=1)) == dict(spring=2.0, climb=True)
    for bad in (dict(spring=0.0), dict(spring=-1.0), dict(spring=NAN), dict(k=0.1)):
        with pytest.raises(ValueError):
            neb.parse_neb(bad)
    import torch

    a, b = torch.zeros(4, 3), torch.ones(4, 3)
    path = neb.interpolate(a, b, 5)
    assert tuple(path.shape) == (5, 4, 3) and torch.equal(path[0], a) and torch.equal(path[-1], b)
    assert torch.allclose(path[2], torch.full((4, 3), 0.5)) and path.dtype == a.dtype
    with pytest.raises(ValueError):
        neb.interpolate(a, b, 2)
    with pytest.raises(ValueError):
        neb.interpolate(a, torch.ones(5, 3), 4)
    for name in ("__call__", "check", "reset", "run", "barrier"):
        assert callable(getattr(neb.DeviceNEB, name))
    assert list(inspect.signature(neb.DeviceNEB.run).parameters)[1:] == ["max_steps", "check_every"]
    assert list(inspect.signature(neb.DeviceNEB.reset).parameters)[1:] == ["images", "climb"]


# ---- 5. the sanitizers -----------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/neb_host.hip with its own main, host code only (-Xarch_host -fsanitize=address,undefined): every entry of the mirror on
    heap arrays of exact size.  A report makes the program exit non-zero (-fno-sanitize-recover)."""
    exe = str(tmp_path / "neb_host_san")
    subprocess.check_call([H.hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DNEB_HOST_MAIN", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", H.SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "steps" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
