"""No GPU: collective-variable restraints and metadynamics of the device-resident MD loop (csrc/tn_bias_math.h, compiled host-only by
tests/md_bias_host_mirror.py) against tests/md_bias_oracle.py - torch autograd in fp64 on other formulas, Python integers for the hill
bookkeeping -, the bias forces against central differences of the oracle's energy, the sampling protocol of the double well, the
host-side refusals and the additive C ABI.  Recorded deviations and bounds: profiles/md_bias.json (section "host"); a bound is ten
times the recorded deviation, and never below ten units in the last place of fp64 (another libm may round exp or atan2 the other
way)."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import md_bias_host_mirror as HM
from tests import md_bias_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
REC = O.recorded()["host"]


def _bound(key):
    return 10.0 * max(REC[key], EPS)


# ---- collective variables ---------------------------------------------------------------------------------------------------------
def test_cvs_and_gradients_equal_the_autograd_oracle():
    worst_s = worst_g = 0.0
    for name, kind, x in O.cv_cases():
        s, g = HM.cv([kind], x[None])
        so, go = O.cv(kind, x)
        n = {"distance": 2, "angle": 3, "torsion": 4}[kind]
        ds, dg = abs(s[0] - so) / max(abs(so), 1.0), np.abs(g[0, :n] - go[:n]).max() / np.abs(go[:n]).max()
        print(f"{name:34s} s = {s[0]: .15f}  value dev {ds:.2e}  gradient dev {dg:.2e}")
        worst_s, worst_g = max(worst_s, ds), max(worst_g, dg)
        assert (g[0, n:] == 0).all()  # slots the kind does not use
    print("largest", worst_s, worst_g, "recorded", REC["cv_value_rel_dev"], REC["cv_gradient_rel_dev"])
    assert worst_s <= _bound("cv_value_rel_dev") and worst_g <= _bound("cv_gradient_rel_dev")


def test_the_torsion_has_the_iupac_sign_and_range():
    for phi in (0.3, -0.3, 2.9, -2.9, math.pi / 2):
        s, _ = HM.cv(["torsion"], O.torsion_geometry(phi)[None])
        assert abs(s[0] - phi) < 1e-6, (phi, s[0])  # (fp32 coordinates of the construction)
    x = O.torsion_geometry(math.pi)
    x[3, 1] = 0.0  # exactly trans: +pi, not -pi
    s, _ = HM.cv(["torsion"], x[None])
    assert s[0] == math.pi
    s, _ = HM.cv(["angle"], O.angle_geometry(math.radians(10))[None])
    assert abs(s[0] - math.radians(10)) < 1e-6


def test_gradients_sum_to_zero_and_exert_no_torque():
    """Translation and rotation invariance of every CV.  The bounds come from fp64 rounding: a gradient component carries a relative
    error of at most 16 u (u = 2^-53: two cross products, a dot product and a quotient in sequence), so the sum of n vectors is
    zero within 16 u n max|g|, and the torque sum_a x_a x g_a - a sum of 2 n products of size max|x| max|g| per component - within
    16 u 2 n max|x| max|g|, plus the rounding of that sum itself, 2 n u max|x| max|g|; asserted with 64 u n in place of 34 u n."""
    u = 2.0 ** -53
    for name, kind, x in O.cv_cases():
        _, g = HM.cv([kind], x[None])
        n = {"distance": 2, "angle": 3, "torsion": 4}[kind]
        g, xx = g[0, :n], x[:n].astype(np.float64)
        gm, xm = np.abs(g).max(), np.abs(xx).max()
        assert np.abs(g.sum(0)).max() <= 16 * u * n * gm, name
        assert np.abs(np.cross(xx, g).sum(0)).max() <= 64 * u * n * xm * gm, name


def test_diff_wraps_torsions_only():
    pi = math.pi
    a = np.array([pi - 0.1, -pi + 0.1, 0.3, pi, -3.0, 3.0, 0.0, 7.0])
    b = np.array([-pi + 0.1, pi - 0.1, -0.2, 0.0, 3.0, -3.0, 0.0, -7.0])
    got = HM.diff("torsion", a, b)
    want = np.array([O.diff("torsion", x, y) for x, y in zip(a, b)])
    assert np.abs(got - want).max() < 4 * EPS * 2 * pi and (got > -pi).all() and (got <= pi).all()
    assert abs(got[0] + 0.2) < 1e-15 and abs(got[1] - 0.2) < 1e-15 and got[3] == pi
    for kind in ("distance", "angle"):
        assert (HM.diff(kind, a, b) == a - b).all()


# ---- bias forces against central differences --------------------------------------------------------------------------------------
def _chain(seed=3, n=6):
    rng = np.random.default_rng(seed)
    base = np.array([[1.0, 0.2, 0.0], [0.0, 0.0, 0.0], [0.1, 0.0, 1.4], [0.9, 0.8, 1.9], [1.2, 1.9, 2.6], [2.5, 2.0, 3.1]])
    return (base[:n] + 0.1 * rng.standard_normal((n, 3))).astype(np.float32)


def _forces_vs_central_difference(x, cvs, restraints=(), hills=None):
    """The mirror's fp32 bias force against -dE/dx of the oracle's energy by central differences (step 1e-5 in fp64).  Tolerance: the
    force is rounded to fp32 once, 2^-24 max|f|; the central difference carries h^2 |E'''| / 6 and u E / h, both below 1e-8 (1 +
    max|f|) for the energies (<= 10) and stiffnesses (<= 30) used here."""
    D = len(cvs)
    kappa, center = np.zeros((1, D)), np.zeros((1, D))
    for c, _, k, s0 in restraints:
        kappa[0, c], center[0, c] = k, s0
    metad, H = None, 0
    if hills is not None:
        H = len(hills["heights"])
        metad = dict(cvs=hills["cvs"], sigma=hills["sigma"], height=0.0, pace=1, kT=1.0)
    wk = HM.Walkers(1, x.shape[0], cvs, [(c, k) for c, k, _, _ in restraints], kappa, center, metad, W=1, H=H, step0=0, base=H)
    if hills is not None:
        wk.hills[0, :wk.dm, :] = np.asarray(hills["centres"]).T
        wk.hills[0, wk.dm, :] = hills["heights"]
    out = wk.launch(0, x, np.zeros_like(x), deposit=0)
    assert wk.status[0] == 0
    want = O.minus_central_difference(x, cvs, restraints, hills)
    e = O.bias_energy(x.astype(np.float64), cvs, restraints, hills)
    assert abs((out["restraint"][0] + out["bias"][0]) - e) <= 1e-13 * max(1.0, abs(e))
    fm = np.abs(want).max()
    tol = 2.0 ** -24 * fm + 1e-8 * (1.0 + fm)
    got = out["forces"].astype(np.float64)
    print("max|f|", fm, "deviation", np.abs(got - want).max(), "tolerance", tol)
    assert np.abs(got - want).max() <= tol
    named = sorted({i for c in cvs for i in c[1:]})
    assert (got[[i for i in range(x.shape[0]) if i not in named]] == 0).all()
    assert (out["bias_forces"][0].astype(np.float64) == got[named]).all()
    return out, fm


@pytest.mark.parametrize("kind", ["harmonic", "upper", "lower"])
def test_restraint_forces_equal_minus_the_central_difference(kind):
    x = _chain()
    cvs = [("distance", 0, 1), ("angle", 1, 2, 3), ("torsion", 1, 2, 3, 4), ("distance", 4, 0)]  # atoms 1..4 are shared
    s = HM.Walkers(1, 6, cvs).launch(0, x, np.zeros_like(x))["cv"][0]  # the values themselves
    # centres on either side of the value: a one-sided kind is active on one of them only
    res = [(0, kind, 30.0, s[0] - 0.2), (1, kind, 12.0, s[1] + 0.3), (2, kind, 8.0, s[2] - 0.4), (3, kind, 5.0, s[3] + 0.25)]
    out, fm = _forces_vs_central_difference(x, cvs, res)
    active = {"harmonic": [1, 1, 1, 1], "upper": [1, 0, 1, 0], "lower": [0, 1, 0, 1]}[kind]
    want = sum(0.5 * k * (0.2, 0.3, 0.4, 0.25)[c] ** 2 for (c, _, k, _), on in zip(res, active) if on)
    assert abs(out["restraint"][0] - want) < 1e-12 and fm > 1.0


def test_torsion_wrap_around_restraint():
    """centre pi - 0.1, value -pi + 0.1: the difference is +0.2 through the branch cut, not -2 pi + 0.2"""
    x = O.torsion_geometry(-math.pi + 0.1)
    cvs = [("torsion", 0, 1, 2, 3)]
    out, _ = _forces_vs_central_difference(x, cvs, [(0, "harmonic", 10.0, math.pi - 0.1)])
    assert abs(out["cv"][0, 0] - (-math.pi + 0.1)) < 1e-6
    assert abs(out["restraint"][0] - 0.5 * 10.0 * 0.2 ** 2) < 1e-5


def test_two_dimensional_hills_with_a_periodic_dimension():
    x = O.torsion_geometry(math.pi - 0.15)
    x = np.concatenate([x, x[:2] + np.float32(3.0)])  # two atoms in no CV
    cvs = [("distance", 0, 3), ("torsion", 0, 1, 2, 3)]
    d0 = float(np.linalg.norm(x[0].astype(np.float64) - x[3].astype(np.float64)))
    rng = np.random.default_rng(8)
    # centres across the cut: most of the weight near -pi, seen from a walker near +pi
    centres = np.stack([d0 + 0.2 * rng.standard_normal(40), -math.pi + 0.3 * rng.random(40)], 1)
    centres[::5, 1] = math.pi - 0.3 * rng.random(8)
    hills = dict(cvs=[0, 1], sigma=[0.25, 0.3], centres=centres.tolist(), heights=rng.uniform(0.2, 1.0, 40).tolist())
    out, fm = _forces_vs_central_difference(x, cvs, [(0, "upper", 4.0, d0 - 0.1)], hills)
    assert out["bias"][0] > 1.0 and fm > 0.5  # the hills across the cut are felt


# ---- hill bookkeeping -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dm", [1, 2])
@pytest.mark.parametrize("W", [1, 3])
def test_hill_bookkeeping_over_200_deposits(W, dm):
    """step0 = 7, hill_base = 5: visible count and written slot at every step equal the oracle as Python integers (asserted inside),
    bias energies and heights against the oracle's own lists (fp64, math.fsum)"""
    dev_V, dev_h = O.run_bookkeeping(HM, W, dm)
    print("V dev", dev_V, "height dev", dev_h, "recorded", REC["hill_energy_rel_dev"], REC["hill_height_rel_dev"])
    assert dev_V <= _bound("hill_energy_rel_dev") and dev_h <= _bound("hill_height_rel_dev")


def test_plain_metadynamics_and_the_height_formula():
    assert HM.height(0.3, 5.0, 1.0, None) == 0.3 == O.height(0.3, 5.0, 1.0, None)
    for V in (0.0, 0.7, 30.0):
        assert abs(HM.height(0.3, V, 0.8, 6.0) - O.height(0.3, V, 0.8, 6.0)) <= 4 * EPS * 0.3


def test_a_full_list_drops_the_deposit_and_writes_nothing_out_of_range():
    W, H, base, step0, pace = 3, 7, 2, 4, 2
    rng = np.random.default_rng(5)
    wk = HM.Walkers(6, 4, O.BOOK_CVS, metad=dict(cvs=[0], sigma=[0.2], height=0.5, pace=pace, kT=1.0, bias_factor=4.0), W=W, H=H,
                    step0=step0, base=base)
    wk.hills[:] = -7.0
    wk.hills[:, :, :base] = 0.4
    written = set()
    for n in range(step0, step0 + 10):
        wk.launch(n, O.book_positions(rng, 6), np.zeros((24, 3), np.float32))
        for w in range(W):
            s = O.slot(n, step0, pace, W, w, base, H)
            assert HM.slot(n, step0, pace, W, w, base, H) == s < H
            written |= {s} if s >= 0 else set()
        assert HM.visible(n + 1, step0, pace, W, base, H) == O.visible(n + 1, step0, pace, W, base, H) <= H
    assert written == {2, 3, 4, 5, 6}  # the deposit after step 8 keeps walker 0 and 1 only... slots 5, 6; walker 2 is dropped
    assert (wk.hills[:, :, 2:] != -7.0).all() and (wk.hills[:, :, :base] == 0.4).all() and wk.status[0] == 0
    assert HM.slot(step0 + 3, step0, pace, W, 2, base, H) == -1 and HM.visible(10 ** 12, step0, pace, W, base, H) == H


def test_a_non_finite_cv_gives_status_4_and_leaves_forces_and_hills_alone():
    rng = np.random.default_rng(6)
    cvs = [("distance", 0, 1), ("angle", 0, 1, 2), ("torsion", 0, 1, 2, 3)]
    for case in ("coincident", "collinear", "nan"):
        wk = HM.Walkers(4, 4, cvs, [(0, "harmonic")], np.full((4, 3), 3.0), np.full((4, 3), 1.0),
                        dict(cvs=[0], sigma=[0.2], height=0.5, pace=1, kT=1.0), W=2, H=8)
        pos = O.book_positions(rng, 4)
        if case == "coincident":
            pos[4] = pos[5]  # walker 1
        elif case == "collinear":
            pos[4:8] = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], np.float32)
        else:
            pos[6, 1] = np.nan
        f0 = rng.standard_normal((16, 3)).astype(np.float32)
        out = wk.launch(0, pos, f0)
        assert wk.status[0] == 4, case
        assert (out["forces"][4:8].view(np.uint32) == f0[4:8].view(np.uint32)).all()  # the walker's forces keep their bits
        assert np.isnan(wk.hills[0, :, 1]).all() and np.isnan(out["cv"][1]).all()  # no hill in its slot, no log row
        assert np.isfinite(out["forces"]).all() and not np.isnan(wk.hills[0, :, 0]).any()  # the others ran
        keep = wk.hills.copy()
        again = wk.launch(0, O.book_positions(rng, 4), f0)  # frozen: the launch returns at once
        assert (again["forces"].view(np.uint32) == f0.view(np.uint32)).all() and np.isnan(again["cv"]).all()
        assert np.array_equal(wk.hills, keep, equal_nan=True)
    wk = HM.Walkers(2, 4, cvs)
    out = wk.launch(0, O.book_positions(rng, 2), np.ones((8, 3), np.float32), overflow=1)  # an overflowed evaluation: nothing
    assert wk.status[0] == 0 and (out["forces"] == 1).all() and np.isnan(out["cv"]).all()


# ---- the sampling protocol --------------------------------------------------------------------------------------------------------
def test_well_tempered_metadynamics_recovers_the_double_well():
    """four walkers sharing one hill list on U(r) = 8 ((r - 2)^2 / 0.25 - 1)^2 under the loop's own Langevin step: free_energy(r)
    against U(r) - 2 kT ln r.  Bounds: mean + 4 standard deviations of the fp64 oracle's error over 8 seeds at the same length
    (profiles/md_bias.json)."""
    e, rec = O.SAMPLING, REC["sampling"]
    assert rec["protocol"] == e and abs(rec["exact_basin_difference"] - O.exact_basin_difference()) < 1e-12
    assert abs(O.exact_basin_difference() + 0.991) < 1e-3
    H = (e["steps"] // e["pace"]) * e["W"]
    c, h, status, x = HM.sample(e["B"], e["W"], e["steps"], e["r0"], e["dt"], e["friction"], e["mirror_seed"], e["sigma"], e["h0"], e["kT"],
                                e["gamma"], e["pace"], H)
    assert status == 0 and c.shape == (1, H) and (h > 0).all() and (h <= e["h0"]).all()
    rms, basin = O.sampling_errors(c[0], h[0])
    print("rms", rms, "bound", rec["rms_bound"], "basin difference", basin, "exact", rec["exact_basin_difference"], "bound",
          rec["basin_error_bound"])
    assert c.min() < 1.6 and c.max() > 2.4  # both basins were visited
    assert rms <= rec["rms_bound"]
    assert abs(basin - rec["exact_basin_difference"]) <= rec["basin_error_bound"]


# ---- the stand-alone program under the sanitizers ---------------------------------------------------------------------------------
def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """a host build with its own main (never loaded into Python) under -fsanitize=address,undefined"""
    exe = str(tmp_path / "md_bias_host")
    HM.build_program(exe, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "md_bias_host: ok 1" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert "visible 8 slot 3 " in r.stdout  # min(8, 2 + 3 * 3); 2 + 0 * 3 + 1


# ---- host-side refusals -----------------------------------------------------------------------------------------------------------
def test_prepare_bias_tables_and_refusals():
    import torch

    from torchmdnet_amd import md

    batch = torch.repeat_interleave(torch.arange(4), 6)
    cvs = [("distance", 0, 1), ("angle", 1, 2, 3), ("torsion", 2, 3, 4, 5), ("distance", 5, 0)]
    metad = dict(cvs=[2, 0], sigma=[0.3, 0.1], height=0.2, pace=5, kT=0.6, bias_factor=8.0, walkers_per_group=2, capacity=10)
    b = md.prepare_bias(dict(cvs=cvs, restraints=[dict(cv=1, kind="upper", kappa=2.0, center=[1.0, 1.1, 1.2, 1.3])], metad=metad), batch, 24, 4)
    kinds, atoms, distinct, offsets, entries = HM.tables(cvs)
    assert b["kinds"].tolist() == kinds.tolist() and b["atoms"].tolist() == atoms.tolist() and b["distinct"].tolist() == distinct.tolist()
    assert b["offsets"].tolist() == offsets.tolist() and b["entries"].tolist() == entries.tolist() and b["mol_start"].tolist() == [0, 6, 12, 18]
    assert b["res_kind"].tolist() == [0, 2, 0, 0] and b["center"][:, 1].tolist() == [1.0, 1.1, 1.2, 1.3] and (b["kappa"][:, 1] == 2).all()
    assert (b["dm"], b["mcv"], b["sigma"], b["W"], b["H"], b["gamma"]) == (2, (2, 0), (0.3, 0.1), 2, 10, 8.0)
    assert md.prepare_bias(dict(cvs=cvs, metad=dict(metad, bias_factor=None, cvs=[1], sigma=[0.2])), batch, 24, 4)["gamma"] == 0.0

    def refuse(match, cvs=cvs, batch=batch, **over):
        with pytest.raises(ValueError, match=match):
            md.prepare_bias(dict(dict(cvs=cvs), **over), batch, 24, 4)

    refuse("outside its molecule", cvs=[("distance", 0, 6)])
    refuse("outside its molecule", cvs=[("angle", -1, 0, 1)])
    refuse("twice", cvs=[("torsion", 0, 1, 2, 1)])
    refuse("at most 8", cvs=[("distance", 0, 1)] * 9)
    refuse("takes 3 atoms", cvs=[("angle", 0, 1)])
    refuse("kind", cvs=[("rmsd", 0, 1)])
    refuse("sorted", batch=batch.flip(0))
    refuse("1 or 2", metad=dict(metad, cvs=[0, 1, 2], sigma=[0.1] * 3))
    refuse("1 or 2", metad=dict(metad, cvs=[], sigma=[]))
    refuse("positive widths", metad=dict(metad, sigma=[0.3, 0.0]))
    refuse("positive widths", metad=dict(metad, sigma=[0.3, -1.0]))
    refuse("pace", metad=dict(metad, pace=0))
    refuse("bias_factor", metad=dict(metad, bias_factor=1.0))
    refuse("bias_factor", metad=dict(metad, bias_factor=0.5))
    refuse("whole number of groups", metad=dict(metad, walkers_per_group=3))
    refuse("capacity", metad=dict(metad, capacity=1))
    refuse("distinct indices", metad=dict(metad, cvs=[0, 0]))
    refuse("two restraints", restraints=[dict(cv=0, kappa=1.0, center=1.0), dict(cv=0, kappa=1.0, center=1.0)])
    refuse("one per walker", restraints=[dict(cv=0, kappa=[1.0, 2.0], center=1.0)])
    refuse("unknown keys", virial=True)


def test_capture_md_biased_signature():
    from torchmdnet_amd import md
    from torchmdnet_amd.models.model import TorchMD_Net

    base = list(inspect.signature(TorchMD_Net.capture_md).parameters)
    names = list(inspect.signature(TorchMD_Net.capture_md_biased).parameters)
    assert names[:len(base)] == base and names[len(base):] == ["constraints", "bias"]  # capture_md's parameters in its order
    assert base[14:] == ["atom_weights", "halo_exchange", "barostat"]  # capture_md itself is untouched
    assert issubclass(md.DeviceBiasedMD, md.DeviceMD)
    assert list(inspect.signature(md.DeviceBiasedMD.reset).parameters)[1:] == ["pos", "vel", "step", "hills"]
    for k in ("n_hills", "hills", "bias_potential", "free_energy"):
        assert hasattr(md.DeviceBiasedMD, k), k


# ---- the additive ABI -------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_exports_agree():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    counts = {"tmdnet_md_bias_workspace_bytes": 6, "tmdnet_md_bias_reset": 4, "tmdnet_md_bias": 36, "tmdnet_md_advance": 22,
              "tmdnet_md_exchange": 22, "tmdnet_md_status": 3}
    from torchmdnet_amd import _C

    src = open(_C.__file__).read()
    for name, n in counts.items():
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == n, name
        assert name in _C.declared_symbols() and name + ".argtypes" in src
    assert "status 2, 3 and 4" in txt  # tmdnet_md_status documents the new status


def test_library_exports_the_bias_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10
    assert len(hip_lib.tmdnet_md_bias.argtypes) == 36 and len(hip_lib.tmdnet_md_bias_workspace_bytes.argtypes) == 6
    assert len(hip_lib.tmdnet_md_bias_reset.argtypes) == 4
    nb = C.c_size_t(0)
    assert hip_lib.tmdnet_md_bias_workspace_bytes(6, 4, 2, 3, 100, C.byref(nb)) == 0 and nb.value >= 256 + 2 * 3 * 100 * 8
    assert hip_lib.tmdnet_md_bias_workspace_bytes(6, 4, 0, 1, 0, C.byref(nb)) == 0 and nb.value >= 256  # restraints only
    for bad in ((6, 9, 1, 1, 10), (6, 0, 0, 1, 0), (6, 4, 3, 1, 10), (6, 1, 2, 1, 10), (6, 4, 1, 4, 10), (6, 4, 1, 3, 2), (0, 4, 1, 1, 10),
                (6, 4, 1, 0, 10)):
        assert hip_lib.tmdnet_md_bias_workspace_bytes(*bad, C.byref(nb)) == 1, bad
    assert hip_lib.tmdnet_md_bias_reset(None, None, 0, 0) == 1
    # refusals need no device: they return before anything is enqueued
    one = C.c_void_p(256)
    ok = [None, None, None, one, one, 72, 6, 1, one, one, 4, one, one, one, 7, one, one, one, one, one, one, 2, 2, 0, 0.3, 0.2, 0.1, 1.0, 6.0, 2,
          3, 8, None, None, None, None]
    for pos, bad in ((3, None), (4, None), (8, None), (9, None), (11, None), (12, None), (13, None), (15, None), (16, None), (17, None),
                     (18, None), (19, None), (20, None), (5, 0), (6, 0), (10, 0), (10, 9), (14, 0), (14, 33), (21, 3), (21, -1), (22, 4), (23, 2),
                     (24, 0.0), (25, -1.0), (26, -0.1), (27, 0.0), (28, 1.0), (28, 0.5), (29, 0), (30, 4), (30, 0), (31, 2)):
        a = list(ok)
        a[pos] = bad
        assert hip_lib.tmdnet_md_bias(*a) == 1, (pos, bad)
