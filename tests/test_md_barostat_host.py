"""No GPU: the barostat arithmetic of the device-resident MD loop (csrc/tn_md_math.h, compiled host-only by
tests/md_baro_host_mirror.py) against tests/md_baro_oracle.py - the scheme in fp64 Python floats, an independent pure-Python
Philox4x32-10 -, the NPT ensemble of an ideal gas, and the additive C ABI."""
import math
import os
import re

import numpy as np
import pytest

from tests import md_baro_host_mirror as HB
from tests import md_baro_oracle as OB
from tests import md_host_mirror as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _molecules(n=257, seed=5):
    """n molecules: triclinic boxes (volumes of a few hundred), random virials and kinetic energies around P V ~ 1"""
    rng = np.random.default_rng(seed)
    box = (np.eye(3)[None] * rng.uniform(5.0, 9.0, size=(n, 3))[:, None, :] + rng.uniform(-1.5, 1.5, size=(n, 3, 3))).astype(np.float32)
    W = rng.normal(size=(n, 3, 3)).astype(np.float32)
    ekin = rng.uniform(0.0, 2.0, size=n).astype(np.float32)
    return box, W, ekin


@pytest.mark.parametrize("kT", [0.0, 0.025])
def test_move_agrees_with_the_oracle(kT):
    box, W, ekin = _molecules()
    fs, P0, a, seed, step = 9.648533e-3, 1e-3, 0.7, 0x0123456789ABCDEF, (3 << 32) + 41
    V, P, mu, nu, flag = HB.move(box, W, ekin, fs, P0, kT, a, seed, step)
    Vo, Po, muo, nuo = OB.moves(box, W, ekin, fs, P0, kT, a, seed, step)
    assert (flag == 0).all()
    assert np.abs(V - np.abs(np.linalg.det(box.astype(np.float64)))).max() < 1e-12 * V.max()
    # the oracle's pressure from numpy's determinant and trace: the formula, not the order of operations
    P_np = (2.0 * ekin.astype(np.float64) / fs + np.trace(W.astype(np.float64), axis1=1, axis2=2)) / (3.0 * np.abs(np.linalg.det(box.astype(np.float64))))
    assert np.abs(P - P_np).max() < 1e-12 * np.abs(P_np).max()
    assert (V == Vo).all() and (P == Po).all()  # fp64, the same order of operations
    print("kT", kT, "mu in", mu.min(), mu.max(), "max ulp distance", OB.ulp_distance(mu, muo).max(), OB.ulp_distance(nu, nuo).max())
    assert np.abs(mu - 1).max() > 1e-3  # the moves are not trivial
    assert OB.ulp_distance(mu, muo).max() <= 1 and OB.ulp_distance(nu, nuo).max() <= 1
    if kT == 0.0:  # no noise: the same fp64 operations and the same libm on both sides
        assert (mu.view(np.uint32) == muo.view(np.uint32)).all() and (nu.view(np.uint32) == nuo.view(np.uint32)).all()
    else:  # the noise entered: another seed, another step, other factors
        assert (HB.move(box, W, ekin, fs, P0, kT, a, seed + 1, step)[2] != mu).mean() > 0.9
        assert (HB.move(box, W, ekin, fs, P0, kT, a, seed, step + 1)[2] != mu).mean() > 0.9
    # mu nu = 1 up to the two roundings
    assert np.abs(mu.astype(np.float64) * nu.astype(np.float64) - 1.0).max() < 2.0 ** -22


def test_scaling_is_one_rounded_product():
    box, W, ekin = _molecules(n=5, seed=6)
    rng = np.random.default_rng(7)
    batch = np.repeat(np.arange(5), [3, 0, 7, 1, 4])
    x, v = rng.normal(size=(15, 3)).astype(np.float32) * 6, rng.normal(size=(15, 3)).astype(np.float32) * 0.05
    _, _, mu, nu, _ = HB.move(box, W, ekin, 1.0, 1e-3, 0.025, 0.3, 9, 2)
    b2, x2, v2 = HB.scale(batch, mu, nu, box, x, v)
    assert (b2.view(np.uint32) == (box * mu[:, None, None]).view(np.uint32)).all()
    assert (x2.view(np.uint32) == (x * mu[batch][:, None]).view(np.uint32)).all()
    assert (v2.view(np.uint32) == (v * nu[batch][:, None]).view(np.uint32)).all()


def test_noise_counter_layout():
    """key = the 64-bit seed (low word first), counter = (step low, step high, molecule, 1): apart from the atoms' stream (0)"""
    seed, step = 0x0123456789ABCDEF, (5 << 32) + 77
    mols = np.array([0, 1, 999, 2 ** 31 + 3], np.uint32)
    got = HB.noise(seed, step, mols)
    ref32 = np.array([OB.noise(seed, step, int(m)) for m in mols])
    ref64 = np.array([OB.noise_f64(seed, step, int(m)) for m in mols])
    assert np.abs(got - ref64).max() < 1e-5 and np.abs(got - ref32).max() < 1e-6
    assert (got == got.astype(np.float32)).all()  # a widened fp32 value
    atoms = H.noise(seed, step, mols)[:, 0]  # the atom stream for equal indices: other numbers
    assert np.abs(got - atoms).min() > 1e-3
    assert np.abs(HB.noise(seed, step + 1, mols) - got).min() > 0
    # with the layout spelled out
    from tests import md_oracle as O

    w = O.philox4x32_10((77, 5, 999, 1), (0x89ABCDEF, 0x01234567))
    assert abs(O.normals(w)[0] - got[2]) < 1e-5


def test_sign_and_flags():
    box = np.tile(np.diag([6.0, 7.0, 8.0]).astype(np.float32), (4, 1, 1))
    V = 336.0
    W = np.zeros((4, 3, 3), np.float32)
    ekin = np.array([0.0, 1.5 * V * 1e-3, 3.0 * V * 1e-3, 0.3 * V * 1e-3], np.float32)  # P = 0, P0, 2 P0, 0.2 P0 (force_scale 1)
    _, P, mu, nu, flag = HB.move(box, W, ekin, 1.0, 1e-3, 0.0, 50.0)
    assert (flag == 0).all() and np.allclose(P, [0.0, 1e-3, 2e-3, 2e-4], rtol=1e-6)
    assert mu[0] < 1 < nu[0] and mu[2] > 1 > nu[2] and mu[3] < 1  # P < P0 compresses, P > P0 expands
    assert abs(mu[1] - 1) < 1e-6
    assert abs(float(mu[0]) - math.exp(-50.0 * 1e-3 / 3)) < 1e-7
    # the virial enters with the sign of section 12: tr W > 0 is outward pressure
    W[0] = np.diag([1.0, 1.0, 1.0]).astype(np.float32)
    assert HB.move(box, W, ekin, 1.0, 1e-3, 0.0, 50.0)[2][0] > 1
    # unusable moves: a flat box, a NaN or an infinity from the virial, a NaN kinetic energy
    bad_box = box.copy()
    bad_box[1, 2] = bad_box[1, 1]
    W2 = np.zeros((4, 3, 3), np.float32)
    W2[2, 1, 1] = np.nan
    W2[3, 0, 0] = np.inf
    assert list(HB.move(bad_box, W2, ekin, 1.0, 1e-3, 0.025, 50.0, 1, 1)[4]) == [0, 1, 1, 1]
    ekin2 = ekin.copy()
    ekin2[0] = np.nan
    assert list(HB.move(box, np.zeros((4, 3, 3), np.float32), ekin2, 1.0, 1e-3, 0.025, 50.0, 1, 1)[4]) == [1, 0, 0, 0]


# ---- the ensemble (parameters, bounds and their basis: tests/md_baro_oracle.py) ------------------------------------------------------
ENSEMBLE, ensemble_bounds, ensemble_state = OB.ENSEMBLE, OB.ensemble_bounds, OB.ensemble_state


def test_ideal_gas_samples_the_npt_ensemble():
    e = ENSEMBLE
    ref = OB.ideal_gas(e["R"], e["n"], e["steps"], e["dt"], e["friction"], e["kT"], e["P0"], 1.0 / e["P0"], e["tau"],
                       e["n"] * e["kT"] / e["P0"], seed=3)
    m_ref, s_ref = ensemble_bounds(ref)
    print("oracle: mean / ((N+1) kT/P0) =", m_ref, " relative sd * sqrt(N+1) =", s_ref)
    assert abs(m_ref - 1.0) < 0.01 and abs(s_ref - 1.0) < 0.05  # the oracle alone
    box, x, v, hk, mass, sigma, c1, c2 = ensemble_state()
    vol = HB.ideal_gas(box, x, v, hk, mass, sigma, e["dt"], c1, c2, 2024, 1.0, e["P0"], e["kT"], 1.0 / e["P0"], e["tau"], 77, e["steps"])
    assert np.isfinite(vol).all()
    m, s = ensemble_bounds(vol)
    print("header: mean / ((N+1) kT/P0) =", m, " relative sd * sqrt(N+1) =", s)
    assert abs(m - 1.0) < 0.01 and abs(s - 1.0) < 0.05


# ---- the additive ABI -------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_are_additive():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("tmdnet_md_barostat_workspace_bytes", "tmdnet_md_barostat"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    args = re.search(r"\bint\s+tmdnet_md_barostat\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(args.split(",")) == 27
    args = re.search(r"\bint\s+tmdnet_md_advance\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(args.split(",")) == 22  # untouched
    from torchmdnet_amd import _C

    declared = _C.declared_symbols()
    assert "tmdnet_md_barostat" in declared and "tmdnet_md_barostat_workspace_bytes" in declared
    src = open(_C.__file__).read()
    assert "tmdnet_md_barostat.argtypes" in src and "tmdnet_md_barostat_workspace_bytes.argtypes" in src


def test_library_exports_the_barostat_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10
    assert len(hip_lib.tmdnet_md_barostat.argtypes) == 27
    nb = C.c_size_t(0)
    assert hip_lib.tmdnet_md_barostat_workspace_bytes(3, C.byref(nb)) == 0 and nb.value >= 24
    assert hip_lib.tmdnet_md_barostat_workspace_bytes(-1, C.byref(nb)) != 0


def test_capture_md_and_md_module_signatures():
    import inspect

    from torchmdnet_amd import md
    from torchmdnet_amd.models.model import TorchMD_Net

    names = list(inspect.signature(TorchMD_Net.capture_md).parameters)
    assert names[14:] == ["atom_weights", "halo_exchange", "barostat"]
    assert inspect.signature(TorchMD_Net.capture_md).parameters["barostat"].default is None
    assert "box" in inspect.signature(md.DeviceMD.reset).parameters
    assert md.BAR_IN_EV_PER_A3 == 6.2415091e-7
    full = md.parse_barostat(dict(pressure=1.0, tau=100.0, compressibility=4.5e-5), dict(friction=0.1, kT=0.025, seed=9))
    assert full == dict(pressure=1.0, tau=100.0, compressibility=4.5e-5, kT=0.025, seed=9)
    assert md.parse_barostat(dict(pressure=1.0, tau=1.0, compressibility=1.0, kT=0.0), None)["seed"] == 0
    for bad in (dict(pressure=1.0, tau=1.0, compressibility=1.0), dict(pressure=1.0, tau=1.0, compressibility=1.0, kT=0.1, beta=2),
                dict(pressure=1.0, tau=0.0, compressibility=1.0, kT=0.1), dict(tau=1.0, compressibility=1.0, kT=0.1)):
        with pytest.raises(ValueError):
            md.parse_barostat(bad, None)
