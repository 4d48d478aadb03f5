"""No GPU: the anisotropic cell barostat of the device-resident MD loop (csrc/tn_md_cell_math.h, compiled host-only by
tests/md_cell_host_mirror.py) against tests/md_cell_oracle.py - the scheme in numpy fp64 with scipy's matrix exponential and an
independent pure-Python Philox4x32-10 -, the isotropic barostat's oracle, two ensembles of an ideal gas, the refusals of the Python
layer and the additive C ABI."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import md_baro_oracle as OB
from tests import md_cell_host_mirror as HC
from tests import md_cell_oracle as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 9.648533e-3


# ---- 1. the move against the oracle -------------------------------------------------------------------------------------------------
def _boxes():
    cubic = np.eye(3) * 7.0
    ortho = np.diag([6.0, 7.5, 9.0])
    tri_lower = np.array([[7.0, 0.0, 0.0], [1.2, 6.5, 0.0], [-0.8, 1.5, 8.0]])
    tri_full = np.array([[7.0, 0.6, -0.4], [1.2, 6.5, 0.9], [-0.8, 1.5, 8.0]])
    return {"cubic": cubic, "orthorhombic": ortho, "triclinic-lower": tri_lower, "triclinic-full": tri_full}


def _virials():
    sym = np.array([[0.9, 0.25, -0.15], [0.25, -0.4, 0.3], [-0.15, 0.3, 0.6]])
    asym = sym + 1e-3 * np.array([[0.0, 1.0, -2.0], [-1.0, 0.0, 0.5], [2.0, -0.5, 0.0]])
    return {"symmetric": sym, "asymmetric": asym}


def _state_list():
    """23 hand-made states: every box with every coupling, both virials, every axis, kT = 0 and kT > 0"""
    out = []
    for b, box in _boxes().items():
        for k, coupling in enumerate(OC.COUPLINGS):
            out.append((b, "symmetric" if k % 2 else "asymmetric", coupling, 2, 0.025))
    for axis in range(3):
        out.append(("orthorhombic", "symmetric", "semi-isotropic", axis, 0.025))
        out.append(("triclinic-lower", "asymmetric", "semi-isotropic", axis, 0.0))
    out += [("cubic", "symmetric", "anisotropic", 2, 0.0), ("triclinic-full", "asymmetric", "anisotropic", 0, 0.0),
            ("triclinic-lower", "symmetric", "diagonal", 1, 0.0), ("cubic", "asymmetric", "diagonal", 2, 0.0),
            ("orthorhombic", "asymmetric", "anisotropic", 1, 0.0)]
    return out


def _atoms(seed=3, n=9):
    rng = np.random.default_rng(seed)
    return np.zeros(n, np.int64), rng.uniform(1.0, 16.0, n).astype(np.float32), (0.02 * rng.normal(size=(n, 3))).astype(np.float32)


@pytest.mark.parametrize("state", _state_list(), ids=lambda s: "-".join(str(t) for t in s))
def test_move_agrees_with_the_oracle(state):
    bname, wname, coupling, axis, kT = state
    box, W = _boxes()[bname][None].astype(np.float32), _virials()[wname][None].astype(np.float32)
    batch, mass, vel = _atoms()
    kt = HC.ktensor(batch, mass, vel, 1)
    Kt = OC.ktensor(batch, mass, vel, 1)
    assert np.abs(kt - OC.six(Kt)).max() < 1e-14 * np.abs(Kt).max()
    P0, a, seed, step = 2e-3, 0.9, 0x0123456789ABCDEF, (3 << 32) + 41
    got = HC.move(box, W, kt, FS, P0, kT, a, coupling, axis, seed, step)
    ref = OC.moves(box, W, Kt, FS, P0, kT, a, coupling, axis, seed, step)
    assert got["flag"][0] == 0
    assert abs(got["V"][0] - ref["V"][0]) < 1e-12 * ref["V"][0] and np.abs(got["P"] - ref["P"]).max() < 1e-12 * np.abs(ref["P"]).max()
    for k in ("D", "mu", "nu", "L", "Q"):
        assert np.abs(got[k] - ref[k]).max() < 1e-12, k
    assert np.abs(got["Mx"] - np.eye(3)).max() > 1e-4  # the move is not trivial
    ref64 = dict(Mx=ref["mu"] @ ref["Q"].transpose(0, 2, 1), Mv=ref["nu"] @ ref["Q"].transpose(0, 2, 1), Mf=ref["Q"].transpose(0, 2, 1),
                 box=ref["L"])
    for k in ("Mx", "Mv", "Mf", "box"):
        ok = OC.close_to_oracle(got[k], ref64[k])
        print(k, "max ulp distance", OC.ulp_distance(got[k], ref64[k].astype(np.float32)).max())
        assert ok.all(), (k, got[k], ref64[k])
    L, Q = got["L"][0], got["Q"][0]
    if coupling == "anisotropic" or bname != "triclinic-full":  # the new box is lower triangular, exactly
        assert (np.triu(got["box"][0], 1) == 0).all()
    assert np.abs(Q @ Q.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Q) - 1.0) < 1e-14
    if coupling == "anisotropic":
        assert (np.triu(L, 1) == 0).all() and (np.diag(L) > 0).all()
        assert np.abs(L @ Q - box[0].astype(np.float64) @ got["mu"][0]).max() < 1e-13
    else:
        off = ~np.eye(3, dtype=bool)
        assert (got["Mf"][0] == np.eye(3, dtype=np.float32)).all() and (got["Mx"][0][off] == 0).all() and (got["Mv"][0][off] == 0).all()
        d = np.diag(got["D"][0])
        if coupling == "semi-isotropic":
            others = [i for i in range(3) if i != axis]
            assert d[others[0]] == d[others[1]] and d[others[0]] != d[axis]
    # mu nu^T = I: nu is the inverse transpose, from the same routine
    assert np.abs(got["mu"][0] @ got["nu"][0].T - np.eye(3)).max() < 1e-14
    if kT > 0.0:  # the noise entered: another seed, another step, another matrix
        assert (HC.move(box, W, kt, FS, P0, kT, a, coupling, axis, seed + 1, step)["Mx"] != got["Mx"]).any()
        assert (HC.move(box, W, kt, FS, P0, kT, a, coupling, axis, seed, step + 1)["Mx"] != got["Mx"]).any()


def test_matrix_exponential_and_projection():
    rng = np.random.default_rng(11)
    for scale in (1e-6, 1e-2, 0.3, 2.0, 9.0):
        A = scale * rng.normal(size=(3, 3))
        E, ref = HC.expm(A), OC.expm(A)
        assert np.abs(E - ref).max() < 2e-14 * max(1.0, np.abs(ref).max()), scale
    assert (HC.expm(np.zeros((3, 3))) == np.eye(3)).all()
    # the projections are Frobenius-orthogonal: <D_f - Pi D_f, Pi D_f> = 0 and Pi Pi = Pi, and they keep the trace
    Df = rng.normal(size=(3, 3))
    for coupling in OC.COUPLINGS:
        for axis in range(3):
            D = OC.project(Df, coupling, axis)
            assert abs(((Df - D) * D).sum()) < 1e-14 and np.abs(OC.project(D, coupling, axis) - D).max() < 1e-15
            assert abs(np.trace(D) - np.trace(Df)) < 1e-14


def test_noise_counter_layout():
    """key = the 64-bit seed (low word first), counter = (step low, step high, molecule, 4 + row): apart from every other stream"""
    from tests import md_host_mirror as H
    from tests import md_baro_host_mirror as HB
    from tests import md_oracle as O

    seed, step = 0x0123456789ABCDEF, (5 << 32) + 77
    mols = np.array([0, 1, 999, 2 ** 31 + 3], np.uint32)
    got = HC.noise(seed, step, mols)
    ref32 = np.stack([OC.noise(seed, step, int(m)) for m in mols])
    ref64 = np.stack([OC.noise_f64(seed, step, int(m)) for m in mols])
    assert np.abs(got - ref64).max() < 1e-5 and np.abs(got - ref32).max() < 1e-6
    assert (got == got.astype(np.float32)).all()
    for r in range(3):
        w = O.philox4x32_10((77, 5, 999, 4 + r), (0x89ABCDEF, 0x01234567))
        assert np.abs(np.array(O.normals(w)) - got[2, r]).max() < 1e-5
    assert np.abs(got[:, 0, 0] - H.noise(seed, step, mols)[:, 0]).min() > 1e-4  # the atoms' stream (0)
    assert np.abs(got[:, :, 0] - HB.noise(seed, step, mols)[:, None]).min() > 1e-4  # the isotropic barostat's (1)
    assert len({round(float(t), 6) for t in got.reshape(-1)}) == got.size  # 36 different numbers
    # the tags are documented next to the others
    txt = open(os.path.join(ROOT, "torchmd-net_amd", "csrc", "tn_md_cell_math.h")).read()
    assert re.search(r"kCellNoiseTag\s*=\s*4u", txt) and "3 + 256 draw" in txt


def test_scaling_is_three_rounded_products_and_two_sums():
    rng = np.random.default_rng(7)
    batch = np.repeat(np.arange(3), [3, 0, 5])
    f32 = np.float32
    x, v, f = (rng.normal(size=(8, 3)).astype(f32) * s for s in (6.0, 0.05, 2.0))
    M = (np.eye(3)[None, None] + 0.01 * rng.normal(size=(3, 3, 3, 3))).astype(f32)
    x2, v2, f2 = HC.scale(batch, M[:, 0], M[:, 1], M[:, 2], False, x, v, f)
    for got, src, k in ((x2, x, 0), (v2, v, 1), (f2, f, 2)):
        Mk = M[batch, k]  # [n,3,3]
        ref = ((src[:, 0, None] * Mk[:, 0, :]) + (src[:, 1, None] * Mk[:, 1, :])) + (src[:, 2, None] * Mk[:, 2, :])
        assert (got.view(np.uint32) == ref.astype(f32).view(np.uint32)).all(), k
    x3, v3, f3 = HC.scale(batch, M[:, 0], M[:, 1], M[:, 2], True, x, v, f)
    d = np.einsum("mkaa->mka", M)
    assert (x3.view(np.uint32) == (x * d[batch, 0]).view(np.uint32)).all() and (v3.view(np.uint32) == (v * d[batch, 1]).view(np.uint32)).all()
    assert (f3.view(np.uint32) == f.view(np.uint32)).all()


# ---- 2. consistency with the isotropic barostat -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling", OC.COUPLINGS)
def test_hydrostatic_weak_coupling_equals_the_isotropic_barostat(coupling):
    """kT = 0, a cubic box and P = p I: every coupling gives Mx = exp(-a (P0 - p) / 3) I, the isotropic oracle's mu"""
    side, P0, a = 7.0, 1e-3, 40.0
    box = (np.eye(3) * side).astype(np.float32)[None]
    V = side ** 3
    for p in (0.0, 2.5e-3, 4e-4):
        ekin = np.float32(1.5 * p * V)  # force_scale 1, W = 0: P = 2 K / 3 V
        kt = np.array([[float(ekin) / 3, 0, 0, float(ekin) / 3, 0, float(ekin) / 3]])
        got = HC.move(box, np.zeros((1, 3, 3), np.float32), kt, 1.0, P0, 0.0, a, coupling, 1)
        _, P, d, mu, nu = OB.move(box[0], np.zeros((3, 3)), ekin, 1.0, P0, 0.0, a)
        assert got["flag"][0] == 0 and abs(got["P"][0, 0, 0] - P) < 1e-15
        for i in range(3):
            assert OB.ulp_distance(got["Mx"][0, i, i], mu) <= 1 and OB.ulp_distance(got["Mv"][0, i, i], nu) <= 1
        off = ~np.eye(3, dtype=bool)
        assert (got["Mx"][0][off] == 0).all() and (got["Mf"][0] == np.eye(3, dtype=np.float32)).all()
        assert OB.ulp_distance(got["box"][0, 0, 0], np.float32(side * math.exp(d / 3.0))) <= 1


# ---- 3. the ideal-gas ensemble: V ~ Gamma(N + 1, kT / P0) in every mode -------------------------------------------------------------------
@pytest.mark.parametrize("coupling", ["anisotropic", "diagonal"])
def test_ideal_gas_samples_the_npt_ensemble(coupling):
    e = OB.ENSEMBLE
    side = (e["n"] * e["kT"] / e["P0"]) ** (1.0 / 3.0)
    ref, _ = OC.ideal_gas(e["R"], e["n"], e["steps"], e["dt"], e["friction"], e["kT"], e["P0"], 1.0 / e["P0"], e["tau"], np.eye(3) * side,
                          coupling, seed=3)
    m_ref, s_ref = OB.ensemble_bounds(ref)
    print(coupling, "oracle: mean / ((N+1) kT/P0) =", m_ref, " relative sd * sqrt(N+1) =", s_ref)
    assert abs(m_ref - 1.0) < 0.01 and abs(s_ref - 1.0) < 0.05  # the oracle alone
    box, x, v, hk, mass, sigma, c1, c2 = OB.ensemble_state()
    vol, _ = HC.ideal_gas(box, x, v, hk, mass, sigma, e["dt"], c1, c2, 2024, 1.0, e["P0"], e["kT"], 1.0 / e["P0"], e["tau"], 77, e["steps"],
                          coupling)
    assert np.isfinite(vol).all()
    m, s = OB.ensemble_bounds(vol)
    print(coupling, "header: mean / ((N+1) kT/P0) =", m, " relative sd * sqrt(N+1) =", s)
    assert abs(m - 1.0) < 0.01 and abs(s - 1.0) < 0.05


# ---- 4. the per-axis ensemble, exactly solvable (parameters, theory and bounds: tests/md_cell_oracle.py) ------------------------------------
@pytest.mark.parametrize("coupling", ["diagonal", "semi-isotropic"])
def test_per_axis_ensemble_is_gaussian_in_the_log_lengths(coupling):
    e = OC.PER_AXIS
    axis = 2
    _, ref = OC.ideal_gas(e["R"], e["n"], e["steps"], e["dt"], e["friction"], e["kT"], e["P0"], e["compressibility"], e["tau"],
                          np.eye(3) * 400.0 ** (1.0 / 3.0), coupling, axis, seed=5, kappa=e["kappa"], eps0=e["eps0"])
    r_ref = OC.per_axis_ratios(ref, coupling, axis)
    print(coupling, "oracle: (mean, variance) / theory =", r_ref)
    for m, s in r_ref:
        assert abs(m - 1.0) < 0.05 and abs(s - 1.0) < 0.05  # the oracle alone
    box, x, v, hk, mass, sigma, c1, c2 = OC.per_axis_state()
    _, length = HC.ideal_gas(box, x, v, hk, mass, sigma, e["dt"], c1, c2, 2024, 1.0, e["P0"], e["kT"], e["compressibility"], e["tau"], 77,
                             e["steps"], coupling, axis, e["kappa"], e["eps0"])
    assert np.isfinite(length).all()
    r = OC.per_axis_ratios(length, coupling, axis)
    print(coupling, "header: (mean, variance) / theory =", r)
    for m, s in r:
        assert abs(m - 1.0) < 0.05 and abs(s - 1.0) < 0.05
    if coupling == "semi-isotropic":  # the coupled pair moves as one
        assert (length[:, :, 0] == length[:, :, 1]).all() and (length[-1, :, 0] != length[-1, :, 2]).any()


# ---- 5. unusable moves and refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling", OC.COUPLINGS)
def test_unusable_moves_are_flagged(coupling):
    box = np.tile(np.diag([6.0, 7.0, 8.0]).astype(np.float32), (6, 1, 1))
    W = np.zeros((6, 3, 3), np.float32)
    kt = np.tile(np.array([0.1, 0.0, 0.0, 0.1, 0.0, 0.1]), (6, 1))
    box[1, 2] = box[1, 1]          # V = 0
    W[2, 1, 1] = np.nan            # a NaN in the virial
    W[3, 0, 0] = np.inf
    box[4, 0, 0] = -6.0            # a left-handed box: det (h mu) < 0
    kt[5, 3] = np.nan              # a NaN kinetic tensor
    got = HC.move(box, W, kt, 1.0, 1e-3, 0.025, 0.5, coupling, 2, 1, 1)
    assert list(got["flag"]) == [0, 1, 1, 1, 1, 1]
    # an exponent that overflows fp32: the matrices are not finite
    W2 = np.zeros((1, 3, 3), np.float32)
    W2[0] = np.eye(3) * 1e9
    assert HC.move(box[:1], W2, kt[:1], 1.0, 1e-3, 0.0, 50.0, coupling)["flag"][0] == 1


def test_python_layer_refuses_before_anything_is_staged():
    from torchmdnet_amd import md
    from torchmdnet_amd.models.model import TorchMD_Net

    names = list(inspect.signature(TorchMD_Net.capture_md_cell).parameters)
    assert names[:8] == ["self", "z", "pos", "vel", "masses", "dt", "batch", "box"] and "barostat" in names and "thermostat" in names
    for absent in ("constraints", "bias", "atom_weights", "halo_exchange"):
        assert absent not in names
    assert list(inspect.signature(TorchMD_Net.capture_md).parameters)[14:] == ["atom_weights", "halo_exchange", "barostat"]  # untouched
    full = md.parse_cell_barostat(dict(pressure=1.0, tau=100.0, compressibility=4.5e-5), dict(friction=0.1, kT=0.025, seed=9))
    assert full == dict(pressure=1.0, tau=100.0, compressibility=4.5e-5, kT=0.025, seed=9, coupling="anisotropic", axis=2)
    ok = dict(pressure=1.0, tau=1.0, compressibility=1.0, kT=0.0)
    assert md.parse_cell_barostat(dict(ok, coupling="semi-isotropic", axis=0), None)["axis"] == 0
    assert md.CELL_COUPLINGS == {"anisotropic": 0, "diagonal": 1, "semi-isotropic": 2}
    for bad in (dict(pressure=1.0, tau=1.0, compressibility=1.0), dict(ok, beta=2), dict(ok, tau=0.0), dict(ok, coupling="isotropic"),
                dict(ok, coupling="semi-isotropic", axis=3), dict(ok, axis=-1), dict(ok, axis=1.5), dict(tau=1.0, compressibility=1.0, kT=0.1),
                dict(ok, kT=-1.0), dict(ok, compressibility=float("nan"))):
        with pytest.raises(ValueError):
            md.parse_cell_barostat(bad, None)
    with pytest.raises(ValueError, match="barostat"):
        md.parse_cell_barostat(None, None)
    assert issubclass(md.DeviceCellMD, md.DeviceMD)
    for name in ("volume", "pressure_tensor", "scale"):
        assert name in (md.DeviceCellMD.__doc__ or "")


def test_capture_md_cell_refusals_without_a_gpu():
    """what is refused before the device is touched, in the style of tests/test_capture_host.py: a model without static shapes, a bad
    barostat dict"""
    import torch

    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    z, pos = torch.tensor([8, 1, 1]), torch.randn(3, 3)
    vel, mass, box = torch.zeros(3, 3), torch.ones(3), torch.eye(3) * 9.0
    baro = dict(pressure=0.0, tau=1.0, compressibility=1.0, kT=0.01)
    model = create_model(dict(W.TINY_ARGS, static_shapes=True))
    with pytest.raises(ValueError, match="unknown"):
        model.capture_md_cell(z, pos, vel, mass, 0.01, box=box, barostat=dict(baro, beta=1.0))
    with pytest.raises(ValueError, match="coupling"):
        model.capture_md_cell(z, pos, vel, mass, 0.01, box=box, barostat=dict(baro, coupling="shear"))
    with pytest.raises(ValueError, match="barostat"):
        model.capture_md_cell(z, pos, vel, mass, 0.01, box=box)
    with pytest.raises(RuntimeError, match="static_shapes"):
        create_model(dict(W.TINY_ARGS)).capture_md_cell(z, pos, vel, mass, 0.01, box=box, barostat=baro)
    tn2 = create_model(dict(W.TINY_ARGS, static_shapes=True, model="tensornet2", output_model="ScalarPlusWeightedCoulomb", q_dim=4,
                            q_weights=[1.0, 1.0, 1.0]))
    with pytest.raises(NotImplementedError, match="TensorNet2"):
        tn2.capture_md_cell(z, pos, vel, mass, 0.01, box=box, barostat=baro)


# ---- 6. the additive ABI ----------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_are_additive():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    for name, value in (("TMDNET_CELL_ANISOTROPIC", 0), ("TMDNET_CELL_DIAGONAL", 1), ("TMDNET_CELL_SEMI_ISOTROPIC", 2)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", txt), name
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("tmdnet_md_barostat_cell_workspace_bytes", "tmdnet_md_barostat_cell"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    args = lambda name: re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")
    assert len(args("tmdnet_md_barostat")) == 27 and len(args("tmdnet_md_advance")) == 22  # untouched
    assert len(args("tmdnet_md_barostat_cell")) == 30
    from torchmdnet_amd import _C

    declared = _C.declared_symbols()
    assert "tmdnet_md_barostat_cell" in declared and "tmdnet_md_barostat_cell_workspace_bytes" in declared
    src = open(_C.__file__).read()
    assert "tmdnet_md_barostat_cell.argtypes" in src and "tmdnet_md_barostat_cell_workspace_bytes.argtypes" in src
    import __graft_entry__ as ge

    assert "tn_md_cell.hip" in ge.HIP_SOURCES


def test_library_exports_the_cell_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10
    assert len(hip_lib.tmdnet_md_barostat_cell.argtypes) == 30 and len(hip_lib.tmdnet_md_barostat.argtypes) == 27
    nb, nb2 = C.c_size_t(0), C.c_size_t(0)
    assert hip_lib.tmdnet_md_barostat_cell_workspace_bytes(100, 3, C.byref(nb)) == 0 and nb.value >= 3 * (27 * 4 + 6 * 8)
    assert hip_lib.tmdnet_md_barostat_cell_workspace_bytes(5000, 2, C.byref(nb2)) == 0 and nb2.value > nb.value  # the slice sums
    assert hip_lib.tmdnet_md_barostat_cell_workspace_bytes(-1, 1, C.byref(nb)) != 0
    assert hip_lib.tmdnet_md_barostat_cell_workspace_bytes(1, -1, C.byref(nb)) != 0


# ---- 7. the sanitizers ------------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/md_cell_host.hip with its own main, host code only (-Xarch_host -fsanitize=address,undefined): every entry of the mirror on
    heap arrays of exact size.  A report makes the program exit non-zero (-fno-sanitize-recover)."""
    exe = HC.build_program(str(tmp_path / "md_cell_host_san"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "bad 0" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
