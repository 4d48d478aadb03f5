"""No GPU: the per-atom arithmetic of the device-resident MD loop (csrc/tn_md_math.h, compiled host-only by tests/md_host_mirror.py)
against tests/md_oracle.py - the fp64 scheme, its fp32 op-by-op mirror and an independent pure-Python Philox4x32-10 -, and the
additive C ABI."""
import os
import re

import numpy as np
import pytest

from tests import md_host_mirror as H
from tests import md_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# known answers of Philox4x32-10 (counter, key, result), recomputed from an independent implementation
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.fixture(scope="module")
def words():
    """3 * 10^5 / 3 Philox calls of the header: one call gives the three normals of one atom"""
    n = 100_000
    rng = np.random.default_rng(11)
    counters = rng.integers(0, 2 ** 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    keys = rng.integers(0, 2 ** 32, size=(n, 2), dtype=np.uint64).astype(np.uint32)
    return counters, keys, H.philox(counters, keys)


def test_philox_known_answers():
    for counter, key, want in KAT:
        assert O.philox4x32_10(counter, key) == want
        got = H.philox(np.array([counter], np.uint32), np.array([key], np.uint32))[0]
        assert tuple(int(w) for w in got) == want, [hex(int(w)) for w in got]


def test_philox_header_equals_pure_python(words):
    counters, keys, out = words
    for i in range(1000):
        assert tuple(int(w) for w in out[i]) == O.philox4x32_10(counters[i], keys[i]), i


def test_uniform_map():
    w = np.array([0, 1, 255, 256, 0xFFFFFFFF, 0xFFFFFF00, 0x80000000, 0x7FFFFFFF, 0x12345678, 0x9ABCDEF0], np.uint32)
    u = H.uniform(w)
    assert [float(x) for x in u] == [O.uniform(x) for x in w]
    below = (w >> 8) < 2 ** 23  # 24 significant bits: the fp32 value is the real number ((r >> 8) + 0.5) 2^-24
    assert [float(x) for x in u[below]] == [((int(x) >> 8) + 0.5) * 2.0 ** -24 for x in w[below]]
    assert u.min() == 2.0 ** -25 and u.max() <= 1.0  # never 0: the logarithm is finite


def test_normals_agree_with_fp64_and_are_standard(words):
    _, _, out = words
    xi = H.normals(out)
    assert np.isfinite(xi).all() and np.abs(xi).max() <= 5.89
    ref = np.array([O.normals(w) for w in out[:20000]])
    err = np.abs(xi[:20000] - ref).max()
    print("normals: max |fp32 - fp64| =", err)
    assert err < 1e-5
    flat = xi.astype(np.float64).ravel()  # 3 * 10^5 samples: standard errors 1.8e-3 (mean) and 2.6e-3 (variance)
    assert flat.size == 300_000
    print("normals: mean", flat.mean(), "variance", flat.var())
    assert abs(flat.mean()) < 0.01 and abs(flat.var() - 1.0) < 0.01
    for d in range(3):
        assert abs(xi[:, d].mean()) < 0.02 and abs(xi[:, d].var() - 1.0) < 0.02, d
    assert abs(np.corrcoef(xi[:, 0], xi[:, 1])[0, 1]) < 0.02


def test_noise_counter_layout():
    """key = the 64-bit seed (low word first), counter = (step low, step high, atom, 0)"""
    seed, step = 0x0123456789ABCDEF, (5 << 32) + 77
    atoms = np.array([0, 1, 999, 2 ** 31 + 3], np.uint32)
    got = H.noise(seed, step, atoms)
    ref = np.array([O.noise(seed, step, int(a)) for a in atoms])
    assert np.abs(got - ref).max() < 1e-5
    assert np.abs(H.noise(seed, step + 1, atoms) - got).min() > 0  # another step: other numbers


def _inputs(n=257, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 3)).astype(np.float32) * 5
    v = rng.normal(size=(n, 3)).astype(np.float32) * 0.05
    f = rng.normal(size=(n, 3)).astype(np.float32) * 3
    mass = rng.uniform(1.0, 40.0, size=n).astype(np.float32)
    dt, fs = 0.5, 9.648533e-3
    hk = (0.5 * dt * fs / mass.astype(np.float64)).astype(np.float32)
    sigma = np.sqrt(0.025 * fs / mass.astype(np.float64)).astype(np.float32)
    return x, v, f, mass, hk, sigma, dt


def test_step_arithmetic_nve():
    x, v, f, mass, hk, _, dt = _inputs()
    v1, ke = H.close_step(v, f, hk, mass)
    v1_32, ke_32 = O.close_step_f32(v, f, hk, mass)
    assert (v1.view(np.uint32) == v1_32.view(np.uint32)).all() and (ke.view(np.uint32) == ke_32.view(np.uint32)).all()
    v1_64, ke_64 = O.close_step(v, f, hk, mass)
    assert np.abs(v1 - v1_64).max() <= 1e-6 * np.abs(v1_64).max()
    assert np.abs(ke - ke_64).max() <= 1e-6 * np.abs(ke_64).max()
    x2, v2 = H.open_step(x, v1, f, hk, dt)
    x2_32, v2_32 = O.open_step_f32(x, v1, f, hk, dt)
    assert (x2.view(np.uint32) == x2_32.view(np.uint32)).all() and (v2.view(np.uint32) == v2_32.view(np.uint32)).all()
    x2_64, v2_64 = O.open_step(x, v1, f, hk, dt)
    assert np.abs(x2 - x2_64).max() <= 1e-6 * np.abs(x2_64).max()
    assert np.abs(v2 - v2_64).max() <= 1e-6 * np.abs(v2_64).max()


def test_step_arithmetic_langevin():
    _, v, f, mass, hk, sigma, _ = _inputs(seed=4)
    c1 = float(np.exp(-0.01 * 0.5))
    c2 = float(np.sqrt(1 - c1 * c1))
    seed, step = 2024, 12345678901
    xi32 = H.noise(seed, step, np.arange(len(v)))
    v1, ke = H.close_step(v, f, hk, mass, sigma, c1, c2, seed, step)
    # op by op in fp32 on the header's own noise: bit for bit
    v1_32, ke_32 = O.close_step_f32(v, f, hk, mass, xi32, c1, c2, sigma)
    assert (v1.view(np.uint32) == v1_32.view(np.uint32)).all() and (ke.view(np.uint32) == ke_32.view(np.uint32)).all()
    # fp64 with the pure-Python generator: the whole chain (c1, c2 as the fp32 values the kernel receives)
    v1_64, ke_64 = O.close_step(v, f, hk, mass, O.noise_array(seed, step, len(v)), float(np.float32(c1)), float(np.float32(c2)), sigma)
    assert np.abs(v1 - v1_64).max() <= 1e-6 * np.abs(v1_64).max()
    assert np.abs(ke - ke_64).max() <= 1e-6 * np.abs(ke_64).max()


def test_frozen_atoms_keep_their_bits():
    x, v, f, mass, hk, sigma, dt = _inputs(n=16)
    mass[::4] = np.inf
    hk[::4] = 0.0
    sigma[::4] = 0.0
    v[::4] = 0.0
    v1, ke = H.close_step(v, f, hk, mass, sigma, 0.9, float(np.sqrt(1 - 0.81)), 7, 3)
    x2, v2 = H.open_step(x, v1, f, hk, dt)
    assert (x2[::4].view(np.uint32) == x[::4].view(np.uint32)).all()
    assert (v2[::4] == 0).all() and (ke[::4] == 0).all() and np.isfinite(ke).all()


def test_header_is_additive():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("tmdnet_md_workspace_bytes", "tmdnet_md_reset", "tmdnet_md_advance", "tmdnet_md_status"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    for name in ("TMDNET_MD_OPEN", "TMDNET_MD_MIDDLE", "TMDNET_MD_CLOSE"):
        assert re.search(r"#define\s+" + name + r"\b", code), name
    args = re.search(r"\bint\s+tmdnet_energy_forces\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(args.split(",")) == 14
    from torchmdnet_amd import _C

    declared = _C.declared_symbols()
    assert "tmdnet_md_advance" in declared and "tmdnet_md_status" in declared


def test_library_exports_the_md_entries(hip_lib):
    import ctypes as C

    for name in ("tmdnet_md_workspace_bytes", "tmdnet_md_reset", "tmdnet_md_advance", "tmdnet_md_status"):
        assert hasattr(hip_lib, name), name
    assert hip_lib.tmdnet_abi_version() == 10
    small, large = C.c_size_t(0), C.c_size_t(0)
    assert hip_lib.tmdnet_md_workspace_bytes(64, 1, C.byref(small)) == 0
    assert hip_lib.tmdnet_md_workspace_bytes(10 ** 6, 1, C.byref(large)) == 0
    assert small.value >= 256 + 64 * 28 and large.value >= 256 + 28 * 10 ** 6
    assert hip_lib.tmdnet_md_workspace_bytes(-1, 1, C.byref(small)) != 0


def test_capture_md_signature():
    import inspect

    from torchmdnet_amd.models.model import TorchMD_Net

    names = list(inspect.signature(TorchMD_Net.capture_md).parameters)
    assert names[:14] == ["self", "z", "pos", "vel", "masses", "dt", "batch", "box", "q", "num_systems", "steps_per_replay",
                          "force_scale", "thermostat", "warmup"]
