"""The committee pass without a GPU: the header's reduction (csrc/tn_committee_math.h, compiled host-only by
tests/committee_host_mirror.py) against the float64 definitions of tests/committee_oracle.py, its corner cases, the refusals of the
host objects (CPU-resident models: nothing is launched to refuse) and the C ABI's declarations.

Bound: 4 fp32 ulps of the float64 value.  The header sums in fp64 and rounds every output once (half an ulp); the slack is for the
order of the fp64 additions, which differs from numpy's.  An exact zero stays exactly zero.  Every test here fails on a tree
without the committee: the header, the mirror and the methods do not exist."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import committee_host_mirror as H
from tests import committee_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, _case = O.SIZES, O.synthetic


@pytest.mark.parametrize("unsorted", [False, True], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("M", [2, 3, 7, 16])
def test_mirror_against_oracle(M, unsorted):
    E, F, batch, B = _case(M, 10 + M, unsorted)
    got, want = H.reduce(E, F, batch, B), O.reduce(E, F, batch, B)
    worst = O.check(got, want, batch, B)
    print("worst ulps", worst)
    assert got["max_atom"][3] == -1 and got["max_deviation"][3] == 0.0  # the molecule without atoms
    assert got["energy"].dtype == np.float32 and got["max_atom"].dtype == np.int64
    # no batch vector: one molecule
    one, ref = H.reduce(E[:, :1], F, None, 1), O.reduce(E[:, :1], F, None, 1)
    O.check(one, ref, None, 1)
    # atoms outside [0, B) join no molecule, and still get their own mean, spread and deviation
    bad = batch.copy()
    bad[::7], bad[3::11] = -1, B
    O.check(H.reduce(E, F, bad, B), O.reduce(E, F, bad, B), bad, B)


def test_cancellation_in_the_energies():
    """M = 3 energies 1e5 + {0, 1e-2, 2e-2}.  fp32 has a spacing of 2^-7 at 1e5, so the members' fp32 energies are 1e5 + {0, 1, 3} 2^-7
    and their spread is 1.19e-2, not 1e-2: the header is held to 4 ulps of the float64 spread of the fp32 values it is given, and to
    1e-2 within what the rounding of the inputs moved it.  With offsets {0, 2, 4} 2^-7, which fp32 holds, the spread is 2^-6 to the
    bit.  A one-pass sum x^2 - M mean^2 in fp32 misses both entirely; that is shown here, not assumed."""
    for offsets, exact in (((0.0, 1e-2, 2e-2), None), ((0.0, 2.0 ** -6, 2.0 ** -5), 2.0 ** -6)):
        E = (1e5 + np.array(offsets)).astype(np.float32).reshape(3, 1)
        F = np.zeros((3, 1, 3), np.float32)
        got, want = H.reduce(E, F, None, 1), O.reduce(E, F, None, 1)
        u = float(O.ulps(got["energy_std"], want["energy_std"]).max())
        print("offsets", offsets, "sE", got["energy_std"][0], "float64", want["energy_std"][0], "ulps", u)
        assert u <= 4.0
        assert float(O.ulps(got["energy"], want["energy"]).max()) <= 4.0
        # 1e-2 up to the rounding of the inputs: each moved by at most half a spacing, 2^-8
        assert abs(float(got["energy_std"][0]) - np.std(offsets, ddof=1)) <= 2.0 ** -8
        if exact is not None:
            assert got["energy_std"][0] == np.float32(exact)
        x = E[:, 0]
        one_pass = np.float32(0)
        for v in x:
            one_pass += v * v
        one_pass = (one_pass - np.float32(3) * (x.sum(dtype=np.float32) / np.float32(3)) ** 2) / np.float32(2)
        with np.errstate(invalid="ignore"):
            assert not abs(np.sqrt(one_pass) - want["energy_std"][0]) <= 0.5 * want["energy_std"][0]


@pytest.mark.parametrize("M", [2, 3, 16])
def test_identical_members_have_no_spread(M):
    E1, F1, batch, B = _case(2, 3)
    E, F = np.repeat(E1[:1], M, axis=0), np.repeat(F1[:1], M, axis=0)
    got = H.reduce(E, F, batch, B)
    assert np.array_equal(got["forces"].view(np.int32), F1[0].view(np.int32))
    assert np.array_equal(got["energy"].view(np.int32), E1[0].view(np.int32))
    for k in ("energy_std", "forces_std", "deviation", "max_deviation"):
        assert np.all(got[k] == 0.0) and not np.signbit(got[k]).any(), k
    # all deviations tie at 0: the first atom of every molecule with atoms
    first = [int(np.flatnonzero(batch == m)[0]) if s else -1 for m, s in enumerate(SIZES)]
    assert got["max_atom"].tolist() == first
    assert not H.gate_fires(0.0, 0.0)  # thresholds of 0 flag nothing on identical members


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_value_that_is_not_finite_wins_the_maximum_and_fires_the_gate(value):
    E, F, batch, B = _case(3, 5)
    i = int(np.flatnonzero(batch == 4)[40])
    F[1, i, 2] = value
    got, want = H.reduce(E, F, batch, B), O.reduce(E, F, batch, B)
    assert got["deviation"][i] == np.inf and got["max_deviation"][4] == np.inf and got["max_atom"][4] == i
    assert H.gate_fires(got["max_deviation"][4], 1e30) and H.gate_fires(got["max_deviation"][4], np.float32(3.4e38))
    keep = np.arange(len(batch)) != i
    assert float(O.ulps(got["deviation"][keep], want["deviation"][keep]).max()) <= 4.0
    # the comparison is !(D <= threshold): a NaN on either side fires, a finite D below the threshold does not
    assert H.gate_fires(np.nan, 1.0) and H.gate_fires(1.0, np.nan) and H.gate_fires(2.0, 1.0)
    assert not H.gate_fires(1.0, 1.0) and not H.gate_fires(0.5, 1.0)
    # a deviation that overflows fp32 from finite inputs is +inf as well
    F[:, i, :] = 0.0
    F[0, i, :], F[1, i, :] = 3e38, -3e38  # every component's spread is 3e38: d = sqrt(3) 3e38 is above the largest fp32
    assert H.reduce(E, F, batch, B)["deviation"][i] == np.inf


def test_ties_pick_the_lowest_index():
    M, N = 3, 200
    rng = np.random.default_rng(9)
    F = np.zeros((M, N, 3), np.float32)
    F[0, :, 0] = 1.0  # every atom: the same spread
    batch = rng.integers(0, 3, size=N).astype(np.int64)
    got = H.reduce(np.zeros((M, 3), np.float32), F, batch, 3)
    assert len(set(got["deviation"].tolist())) == 1 and got["deviation"][0] > 0
    assert got["max_atom"].tolist() == [int(np.flatnonzero(batch == m)[0]) for m in range(3)]
    # two atoms above the rest, equal to the bit: the lower index, whichever comes first in memory
    F[0, 150, 0] = F[0, 20, 0] = 2.0
    batch[:] = 0
    assert H.reduce(np.zeros((M, 1), np.float32), F, batch, 1)["max_atom"][0] == 20


def test_member_count_limits():
    assert H.max_members() == 16
    E, F, batch, B = _case(2, 1)
    assert H.reduce(np.repeat(E[:1], 17, 0), np.repeat(F[:1], 17, 0), batch, B) is None
    assert H.reduce(E[:1], F[:1], batch, B) is None


def test_host_program_under_the_sanitizers(tmp_path):
    """the stand-alone program of tests/committee_host.hip with -fsanitize=address,undefined: nothing is loaded into Python"""
    exe = H.build_program(str(tmp_path / "committee_host"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("committee_host ok") and out.stdout.split()[-3:] == ["-1", "1", "0"], out.stdout


# ------------------------------------------------------------------------------------------------ the host objects
def _members(n, **over):
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    out = []
    for s in range(n):
        torch.manual_seed(s + 1)
        out.append(create_model(dict(W.TINY_ARGS, static_shapes=True, **over)))
    return out


def test_refusals_need_no_gpu():
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.committee import DeviceCommitteeMD, parse_gate
    from torchmdnet_amd.md import DeviceMD
    from torchmdnet_amd.models.model import Ensemble, create_model

    assert issubclass(DeviceCommitteeMD, DeviceMD)
    z, pos, batch = W.synthetic_batch(n_mol=2, n_atoms=7)
    vel, mass = torch.zeros_like(pos), torch.ones(len(z))
    calls = {
        "committee": lambda e, **kw: e.committee(z, pos, batch, **kw),
        "capture": lambda e, **kw: e.capture(z, pos, batch, **kw),
        "capture_md": lambda e, **kw: e.capture_md(z, pos, vel, mass, 0.5, batch, **kw),
    }
    good = _members(2)
    for name, call in calls.items():
        with pytest.raises(ValueError, match="2 to 16 members.*has 1"):
            call(Ensemble(good[:1]))
        with pytest.raises(ValueError, match="2 to 16 members.*has 17"):
            call(Ensemble([good[0]] * 17))
        with pytest.raises(ValueError, match="different devices"):
            call(Ensemble([good[0], copy.deepcopy(good[1]).to("meta")]))
        head = create_model(dict(W.TINY_ARGS, static_shapes=True, output_model="DipoleMoment", derivative=False))
        with pytest.raises(NotImplementedError, match="member 1 has output_model DipoleMoment.*scalar head"):
            call(Ensemble([good[0], head]))
        train = copy.deepcopy(good[1])
        train.parameter_gradients = True
        with pytest.raises(NotImplementedError, match="member 1.*parameter_gradients=True"):
            call(Ensemble([good[0], train]))
        for kw in (dict(atom_weights=torch.ones(len(z))), dict(halo_exchange=lambda *a: None)):
            with pytest.raises(NotImplementedError, match="atom weights or the halo exchange"):
                call(Ensemble(good), **kw)
        dynamic = _members(2, )[1]
        dynamic.representation_model.static_shapes = False
        if name == "committee":  # eager: dynamic shapes are served; without a GPU the call ends at the device check, after the refusals
            with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
                call(Ensemble([good[0], dynamic]))
        else:
            with pytest.raises(ValueError, match="member 1 was created without static_shapes=True"):
                call(Ensemble([good[0], dynamic]))
    md = calls["capture_md"]
    for kw, what in ((dict(barostat=dict(pressure=0.0, tau=1.0, compressibility=1.0, kT=0.0)), "a barostat"),
                     (dict(constraints=dict(pairs=torch.tensor([[0, 1]]))), "constraints"),
                     (dict(bias=dict(cvs=[("distance", 0, 1)])), "a bias"),
                     (dict(temperatures=[0.02, 0.03]), "replica exchange"),
                     (dict(thermostat=dict(kind="csvr", kT=0.02, tau=10.0)), "a global thermostat")):
        with pytest.raises(NotImplementedError, match=f"Ensemble.capture_md has no HIP path with {what}"):
            md(Ensemble(good), **kw)
    for gate, msg in ((dict(flag=1.0), "unknown keys"), (dict(stop_above=float("nan")), "must not be NaN")):
        with pytest.raises(ValueError, match=msg):
            md(Ensemble(good), gate=gate)
    assert parse_gate(None) == (0, 0.0, 0.0) and parse_gate(dict(flag_above=None, stop_above=2)) == (2, 0.0, 2.0)
    assert parse_gate(dict(flag_above=0.5, stop_above=0.0)) == (3, 0.5, 0.0)
    assert "Langevin" in Ensemble.capture_md.__doc__ and "global thermostat" in Ensemble.capture_md.__doc__


def test_header_and_bindings_are_additive(hip_lib):
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt) and hip_lib.tmdnet_abi_version() == 10
    assert re.search(r"#define\s+TMDNET_COMMITTEE_MAX_MEMBERS\s+16\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from torchmdnet_amd import _C

    src = open(_C.__file__).read()
    for name, n in (("tmdnet_committee_workspace_bytes", 3), ("tmdnet_committee_reset", 3), ("tmdnet_committee_reduce", 19),
                    ("tmdnet_committee_latch", 8), ("tmdnet_committee_status", 3)):
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == n, name
        assert name in _C.declared_symbols() and name + ".argtypes" in src
        assert len(getattr(hip_lib, name).argtypes) == n
    body = re.search(r"typedef struct \{([^}]*)\} tmdnet_committee_gate;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in _C.CommitteeGate._fields_]
    assert (_C.COMMITTEE_MAX_MEMBERS, _C.COMMITTEE_FLAG, _C.COMMITTEE_STOP) == (16, 1, 2) == (H.max_members(), 1, 2)
    # invalid arguments are refused before any launch: no device is needed to see it
    import ctypes as C

    nb = C.c_size_t(0)
    assert hip_lib.tmdnet_committee_workspace_bytes(10, 2, C.byref(nb)) == _C.OK and nb.value >= 256 + 2 * 12
    assert hip_lib.tmdnet_committee_workspace_bytes(-1, 2, C.byref(nb)) == _C.ERR_INVALID
    assert hip_lib.tmdnet_committee_workspace_bytes(10, 2, None) == _C.ERR_INVALID
    one = (C.c_void_p * 16)(*([8] * 16))  # non-null entries that nothing dereferences: every call below is refused first
    ws, p = C.c_void_p(8), C.c_void_p(8)
    red = lambda M, e=one, f=one, n=4, b=1, w=ws, gate=None: hip_lib.tmdnet_committee_reduce(
        None, w, 1 << 20, M, e, f, n, b, None, p, p, p, p, p, p, p, None, None, gate)
    assert red(1) == red(17) == red(0) == _C.ERR_INVALID
    assert red(2, e=None) == red(2, f=None) == red(2, w=None) == red(2, n=-1) == red(2, b=-1) == _C.ERR_INVALID
    null = (C.c_void_p * 16)(8, 0, *([8] * 14))
    assert red(2, e=null) == red(3, f=null) == _C.ERR_INVALID
    for g in (_C.CommitteeGate(4, 0, 0, 8, 8, 8, 8, 8), _C.CommitteeGate(1, 0, 0, None, 8, 8, 8, 8),
              _C.CommitteeGate(1, 0, 0, 8, 8, 8, 8, None), _C.CommitteeGate(2, 0, float("nan"), 8, None, None, None, None)):
        assert red(2, gate=C.byref(g)) == _C.ERR_INVALID
        assert hip_lib.tmdnet_committee_latch(None, ws, 4, 1, None, p, p, C.byref(g)) == _C.ERR_INVALID
    assert hip_lib.tmdnet_committee_latch(None, ws, 4, 1, None, p, p, None) == _C.ERR_INVALID
    assert hip_lib.tmdnet_committee_reduce(None, ws, 16, 2, one, one, 4, 1, None, p, p, p, p, p, p, p, None, None, None) == _C.ERR_WORKSPACE
    assert hip_lib.tmdnet_committee_status(None, None, None) == _C.ERR_INVALID
    assert hip_lib.tmdnet_committee_reset(None, None, 1) == _C.ERR_INVALID
