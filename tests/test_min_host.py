"""No GPU: the arithmetic of the device-resident FIRE minimiser (csrc/tn_min_math.h, compiled host-only by
tests/min_host_mirror.py) against tests/min_oracle.py - the controller in fp64 Python floats, written from the equations -, a
whole minimisation of harmonic wells in both precisions, and the additive C ABI."""
import math
import os
import re

import numpy as np
import pytest

from tests import min_host_mirror as H
from tests import min_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(O.FIRE)  # ASE's defaults, fmax = 0.05

NAN, INF = float("nan"), float("inf")
# name, (dt, alpha, n_pos, converged_at), (vf, ff, vv, fmax2), expected return
CASES = [
    ("downhill, n_pos below n_min", (0.1, 0.1, 2, -1), (0.3, 2.0, 0.5, 0.4), O.MOVING),
    ("downhill, n_pos equal to n_min", (0.1, 0.1, 5, -1), (0.3, 2.0, 0.5, 0.4), O.MOVING),
    ("downhill, n_pos above n_min", (0.1, 0.1, 6, -1), (0.3, 2.0, 0.5, 0.4), O.MOVING),
    ("downhill, dt reaches dt_max", (0.95, 0.07, 9, -1), (0.003, 0.02, 0.005, 0.004), O.MOVING),
    ("downhill, dt already dt_max", (1.0, 0.05, 30, -1), (0.003, 0.02, 0.005, 0.004), O.MOVING),
    ("uphill", (0.4, 0.03, 11, -1), (-0.2, 2.0, 0.5, 0.4), O.MOVING),
    ("vf exactly zero counts as uphill", (0.4, 0.03, 11, -1), (0.0, 2.0, 0.5, 0.4), O.MOVING),
    ("clamp active", (0.5, 0.1, 3, -1), (40.0, 900.0, 3.0, 90.0), O.MOVING),
    ("clamp active after an uphill step", (0.5, 0.1, 3, -1), (-40.0, 900.0, 3.0, 90.0), O.MOVING),
    ("clamp inactive", (0.05, 0.1, 3, -1), (0.01, 0.1, 0.002, 0.02), O.MOVING),
    ("ff zero while fmax2 is not (inconsistent sums: mix = 0)", (0.1, 0.1, 2, -1), (0.3, 0.0, 0.5, 0.4), O.MOVING),
    ("vv zero: the first step", (0.1, 0.1, 0, -1), (0.0, 7.0, 0.0, 1.5), O.MOVING),
    ("vv zero with vf > 0 (inconsistent sums: mix = 0)", (0.1, 0.1, 0, -1), (0.2, 7.0, 0.0, 1.5), O.MOVING),
    ("already converged", (0.3, 0.08, 4, 17), (0.3, 2.0, 0.5, 0.4), O.FROZEN),
    ("already converged, NaN sums are not looked at", (0.3, 0.08, 4, 17), (NAN, NAN, NAN, NAN), O.FROZEN),
    ("converging now", (0.3, 0.08, 4, -1), (0.001, 0.004, 0.002, 0.0024), O.FROZEN),
    ("just above fmax", (0.3, 0.08, 4, -1), (0.001, 0.004, 0.002, 0.0026), O.MOVING),
    ("no atoms", (0.1, 0.1, 0, -1), (0.0, 0.0, 0.0, 0.0), O.FROZEN),
    ("NaN vf", (0.1, 0.1, 2, -1), (NAN, 2.0, 0.5, 0.4), O.UNUSABLE),
    ("NaN ff", (0.1, 0.1, 2, -1), (0.3, NAN, 0.5, 0.4), O.UNUSABLE),
    ("inf vv", (0.1, 0.1, 2, -1), (0.3, 2.0, INF, 0.4), O.UNUSABLE),
    ("inf fmax2", (0.1, 0.1, 2, -1), (0.3, 2.0, 0.5, INF), O.UNUSABLE),
]


def _bits64(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_controller_equals_the_oracle_bit_for_bit():
    """No transcendental in the controller, no FMA in the x86-64 baseline: the header's fp64 statements and the oracle's are the
    same IEEE operations.  Random sums on top of the table."""
    rng = np.random.default_rng(3)
    cases = list(CASES)
    for i in range(400):
        ff = float(10.0 ** rng.uniform(-4, 3))
        vv = float(10.0 ** rng.uniform(-6, 2))
        vf = float(rng.uniform(-1, 1) * math.sqrt(ff * vv))
        st = (float(rng.uniform(0.01, 1.0)), float(rng.uniform(0.001, 0.1)), int(rng.integers(0, 12)), -1)
        cases.append((f"random {i}", st, (vf, ff, vv, ff * float(rng.uniform(0.01, 1.0))), None))
    step = (7 << 32) + 5
    state = tuple(np.array([c[1][k] for c in cases]) for k in range(4))
    sums = np.array([c[2] for c in cases])
    (dt, alpha, n_pos, conv), coef, ret = H.control(state, sums, P, step)
    seen = set()
    for i, (name, st, sm, expect) in enumerate(cases):
        s = dict(dt=st[0], alpha=st[1], n_pos=st[2], converged_at=st[3])
        r, c = O.control(s, P, *sm, step)
        assert expect is None or r == expect, name
        assert ret[i] == r, name
        assert _bits64(dt[i]) == _bits64(s["dt"]) and _bits64(alpha[i]) == _bits64(s["alpha"]), name
        assert n_pos[i] == s["n_pos"] and conv[i] == s["converged_at"], name
        assert (coef[i].view(np.uint32) == np.array(c, np.float32).view(np.uint32)).all(), (name, coef[i], c)
        if r == O.MOVING:
            clamped = coef[i][2] < np.float32(s["dt"])
            seen.add(("down" if sm[0] > 0 else "up", "clamped" if clamped else "free", "grow" if st[2] > P["n_min"] else "hold"))
        if r != O.MOVING:
            assert (coef[i] == 0).all(), name
        if r == O.UNUSABLE or st[3] >= 0:  # the state is untouched
            assert (dt[i], alpha[i], n_pos[i], conv[i]) == st, name
    assert len(seen) >= 7, seen  # every branch combination that exists was taken
    # what the table is about, spelled out
    by = {c[0]: i for i, c in enumerate(cases)}
    assert dt[by["downhill, n_pos equal to n_min"]] == 0.1 and dt[by["downhill, n_pos above n_min"]] == 0.1 * 1.1
    assert alpha[by["downhill, n_pos above n_min"]] == 0.1 * 0.99 and n_pos[by["downhill, n_pos above n_min"]] == 7
    assert dt[by["downhill, dt reaches dt_max"]] == 1.0 and dt[by["downhill, dt already dt_max"]] == 1.0
    i = by["uphill"]
    assert (dt[i], alpha[i], n_pos[i]) == (0.2, 0.1, 0) and coef[i][0] == 0 and coef[i][1] == np.float32(0.2)
    assert conv[by["converging now"]] == step and conv[by["no atoms"]] == step and conv[by["already converged"]] == 17
    i = by["clamp active"]  # the move of the whole molecule is max_step long: d |v_new| = max_step
    cv, cf, d = (float(t) for t in coef[i])
    vf, ff, vv, _ = cases[i][2]
    assert abs(d * math.sqrt(cv * cv * vv + 2 * cv * cf * vf + cf * cf * ff) - P["max_step"]) < 1e-6
    i = by["vv zero: the first step"]
    assert coef[i][0] == 0 and coef[i][1] == np.float32(0.05) and n_pos[i] == 0


def test_terms_and_update_are_single_rounded_operations():
    rng = np.random.default_rng(4)
    n = 300
    batch = rng.integers(0, 4, size=n)
    v, f, x = (rng.normal(size=(n, 3)).astype(np.float32) * s for s in (0.05, 3.0, 6.0))
    fixed = (rng.uniform(size=n) < 0.1).astype(np.uint8)
    t = H.terms(v, f, fixed)
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]  # numpy fp32: every operation rounds
    ref = np.where((fixed != 0)[:, None], np.float32(0), np.stack([dot(f, v), dot(f, f), dot(v, v)], 1))
    assert (t.view(np.uint32) == ref.astype(np.float32).view(np.uint32)).all()
    assert (H.terms(v, f)[fixed != 0] != 0).all()
    coef = rng.uniform(0.1, 1.0, size=(4, 3)).astype(np.float32)
    conv = np.array([-1, 12, -1, -1])
    x2, v2 = H.update(batch, conv, fixed, coef, x, v, f)
    c = coef[batch]
    still = (fixed != 0) | (conv[batch] >= 0)
    v_ref = np.where(still[:, None], np.float32(0), c[:, 0:1] * v + c[:, 1:2] * f)
    x_ref = np.where(still[:, None], x, x + c[:, 2:3] * v_ref)
    assert (v2.view(np.uint32) == v_ref.view(np.uint32)).all() and (x2.view(np.uint32) == x_ref.view(np.uint32)).all()
    assert still.sum() > 60 and (x2[~still] != x[~still]).any()


@pytest.mark.parametrize("interleave", [False, True])
def test_wells_converge_at_the_same_step_in_fp32_and_fp64(interleave):
    """Molecules of 1, 3, 40, 64 and 1 500 atoms in harmonic wells, fmax = 1e-3: the header's fp32 run and the fp64 oracle freeze
    every molecule at the same step, and at the minimum."""
    p = dict(P, fmax=1e-3)
    batch, kspring, x0, x = O.wells_problem(interleave=interleave)
    steps32, conv32, x32, dt32 = H.wells(batch, 5, kspring, x0, x, p, 1000)
    steps64, conv64, x64 = O.wells(batch, 5, kspring, x0, x, p, 1000)
    print("converged at: fp32", conv32.tolist(), "fp64", conv64.tolist())
    assert (conv32 > 0).all() and steps32 == conv32.max() < 1000
    assert conv32.tolist() == conv64.tolist() and steps32 == steps64
    assert len(set(conv32.tolist())) > 1 and (dt32 != dt32[0]).any()  # every molecule its own controller
    resid = np.abs(kspring[:, None] * (x32 - x0))
    assert resid.max() < 1e-3 and np.abs(x32 - x64).max() < 1e-3
    # a fixed atom keeps its bits and does not hold up the convergence of its molecule
    fixed = np.zeros(len(batch), np.uint8)
    fixed[::97] = 1
    steps_f, conv_f, x_f, _ = H.wells(batch, 5, kspring, x0, x, p, 1000, fixed)
    assert (conv_f >= 0).all() and (x_f[fixed != 0].view(np.uint32) == x[fixed != 0].view(np.uint32)).all()
    assert conv_f.tolist() == O.wells(batch, 5, kspring, x0, x, p, 1000, fixed)[1].tolist()
    # stopped early: max_steps steps taken, the large molecule still open
    steps_s, conv_s, _, _ = H.wells(batch, 5, kspring, x0, x, p, 40)
    assert steps_s == 40 and conv_s[4] == -1 and conv_s[3] == conv32[3]


# ---- the additive ABI -------------------------------------------------------------------------------------------------------------
def test_header_and_bindings_are_additive():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from torchmdnet_amd import _C

    src = open(_C.__file__).read()
    for name, n_args in (("tmdnet_min_workspace_bytes", 3), ("tmdnet_min_reset", 5), ("tmdnet_min_advance", 29), ("tmdnet_min_status", 3)):
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == n_args, name
        assert name in _C.declared_symbols() and name + ".argtypes" in src
    args = re.search(r"\bint\s+tmdnet_md_advance\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(args.split(",")) == 22  # untouched
    assert [int(re.search(r"#define\s+TMDNET_MIN_" + n + r"\s+(\d+)", txt).group(1)) for n in ("OPEN", "MIDDLE", "CLOSE")] == [0, 1, 2]


def test_library_exports_the_minimiser_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10
    assert len(hip_lib.tmdnet_min_advance.argtypes) == 29
    small, large = C.c_size_t(0), C.c_size_t(0)
    assert hip_lib.tmdnet_min_workspace_bytes(64, 1, C.byref(small)) == 0 and small.value >= 256 + 2 * 64 * 12 + 44 + 32
    assert hip_lib.tmdnet_min_workspace_bytes(5000, 2, C.byref(large)) == 0 and large.value >= 256 + 2 * 5000 * 12 + 2 * 44 + 2 * 3 * 32
    assert hip_lib.tmdnet_min_workspace_bytes(-1, 1, C.byref(small)) != 0
    # argument checks happen before anything is enqueued: no device is needed to be refused
    assert hip_lib.tmdnet_min_reset(None, None, 0, 0.1, 0.1) == 1
    assert hip_lib.tmdnet_min_reset(None, C.c_void_p(256), 0, 0.0, 0.1) == 1


def test_capture_minimize_and_module_signatures():
    import inspect

    from torchmdnet_amd import minimize
    from torchmdnet_amd.models.model import TorchMD_Net

    sig = inspect.signature(TorchMD_Net.capture_minimize).parameters
    assert list(sig)[1:12] == ["z", "pos", "batch", "box", "q", "num_systems", "steps_per_replay", "fmax", "fire", "fixed", "warmup"]
    assert (sig["steps_per_replay"].default, sig["fmax"].default, sig["fire"].default, sig["warmup"].default) == (10, 0.05, None, 3)
    assert minimize.FIRE_DEFAULTS == {k: v for k, v in O.FIRE.items() if k != "fmax"}  # ASE's
    assert minimize.parse_fire(None) == minimize.FIRE_DEFAULTS
    assert minimize.parse_fire(dict(dt=0.05, n_min=3)) == dict(minimize.FIRE_DEFAULTS, dt=0.05, n_min=3)
    for bad in (dict(timestep=0.1), dict(dt=0.0), dict(f_dec=1.5), dict(max_step=-1.0), dict(n_min=-1)):
        with pytest.raises(ValueError):
            minimize.parse_fire(bad)
    for name in ("__call__", "check", "reset", "run"):
        assert callable(getattr(minimize.DeviceMinimizer, name))
    assert list(inspect.signature(minimize.DeviceMinimizer.run).parameters)[1:] == ["max_steps", "check_every"]
