"""No GPU: the observer of the device-resident MD loop.  csrc/tn_observe_math.h, compiled host-only by tests/observe_host_mirror.py,
against tests/observe_oracle.py (numpy fp64 and Python integers, written independently); the exact fp32 mirror of the histogram
against the oracle on the hand-built cases of tests/observe_cases.py, whose margin condition makes the device comparison exact; the
stand-alone program under the sanitizers; the host-side refusals, the signature and the additive C ABI."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import observe_cases as CS
from tests import observe_host_mirror as HM
from tests import observe_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the header against the oracle -------------------------------------------------------------------------------------------------------
def test_sample_and_slot_arithmetic_over_a_counter_that_crosses_2_to_the_32():
    for s0, S in ((0, 1), (5, 4), (2 ** 32 - 9, 3), (2 ** 32 - 1, 1), (2 ** 40 + 3, 7)):
        seen = 0
        for s in range(max(s0 - 3, 0), s0 + 60):
            j = HM.sample_index(s, s0, S)
            assert j == O.sample_index(s, s0, S), (s, s0, S)
            assert HM.samples_at(s, s0, S) == O.samples_at(s, s0, S)
            if j >= 0:
                assert j == seen and HM.sample_step(j, s0, S) == O.sample_step(j, s0, S) == s
                for cap in (1, 3, 256):
                    assert HM.ring_slot(j, cap) == O.ring_slot(j, cap)
                seen += 1
        assert seen == 59 // S
    assert HM.sample_index(7, 7, 1) == -1 and HM.sample_index(3, 7, 1) == -1  # s0 itself and the steps before it are no samples
    big = 2 ** 33 + 5
    assert HM.ring_slot(big, 7) == big % 7 and HM.sample_index(2 ** 34, 0, 2) == 2 ** 33 - 1


def test_per_lag_sample_counts():
    for n in (0, 1, 5, 256, 1000):
        for l in (0, 1, 4, 5, 255):
            assert HM.lag_samples(n, l) == O.lag_samples(n, l) == max(n - l, 0)


def test_the_bin_of_a_distance_equals_np_histogram_away_from_the_edges():
    rng = np.random.default_rng(0)
    for r_max, bins in ((3.5, 7), (4.0, 1024), (2.75, 1), (6.0, 100)):
        d = rng.uniform(0.0, 1.2 * r_max, 20000)
        dr = r_max / bins
        d = d[np.abs(d / dr - np.round(d / dr)) * dr > 1e-5 * np.maximum(d, 1e-3)]  # the margin condition of the cases
        d32 = d.astype(np.float32)
        got = HM.bins_of(d32 * d32, r_max, bins)
        inside = d < r_max
        assert (got[~inside] == -1).all() and (got[inside] >= 0).all()
        want = np.histogram(d[inside], bins=bins, range=(0.0, r_max))[0]
        assert (np.bincount(got[inside], minlength=bins) == want).all()
        assert (got[inside] == np.minimum(np.floor(d[inside] / dr), bins - 1)).all()
    # the last bin takes what rounding pushes onto the upper edge, and r_max itself is outside
    r2, inv = HM.constants(3.5, 7)
    assert HM.bins_of(np.array([np.nextafter(r2, np.float32(0))]), 3.5, 7)[0] == 6
    assert HM.bins_of(np.array([r2, np.float32(np.inf), np.float32(np.nan)]), 3.5, 7).tolist() == [-1, -1, -1]
    assert HM.bins_of(np.array([0.0], np.float32), 3.5, 7)[0] == 0


def test_pair_types_count_a_pair_once_in_either_orientation():
    pairs = [(None, None), (8, 8), (1, 8), (6, 1)]
    z = np.array([8, 1, 6, 7])
    m = HM.masks(z, pairs)
    for i in range(4):
        for j in range(4):
            got = HM.pair_types(int(m[i]), int(m[j]))
            for p, (a, b) in enumerate(pairs):
                fits = lambda zz, s: s is None or zz == s  # noqa: E731
                want = (fits(z[i], a) and fits(z[j], b)) or (fits(z[i], b) and fits(z[j], a))
                assert bool((got >> (2 * p)) & 1) == want, (i, j, p)
            assert got & ~0x55 == 0
    assert HM.pair_types(0xffffffff, 0xffffff00) == 0  # the group bits above bit 7 are no selectors


def test_normalisation_and_same_selector_pair_counts():
    z = np.array([8, 1, 1, 8, 1, 8, 1, 1])
    for a, b in ((None, None), (8, 8), (1, 8), (8, None)):
        na, nb, npairs = O.pair_counts(z, a, b)
        assert HM.pair_count(na, nb, a == b) == npairs
    assert O.pair_counts(z, 8, 8)[2] == 3 and O.pair_counts(z, None, None)[2] == 28 and O.pair_counts(z, 1, 8)[2] == 15
    counts = np.array([0, 3, 10, 7, 1, 0, 2])
    for vol in (None, 321.5):
        want = O.rdf_g(counts, 4, 15, 3.5, vol)
        got = [HM.rdf_value(int(c), 4, 15.0, b, 7, 3.5, vol) for b, c in enumerate(counts)]
        assert np.abs(np.array(got) - want).max() <= 4 * 2.0 ** -52 * want.max()
    # the package's own normalisation (torch, host)
    import torch

    from torchmdnet_amd import observe

    r, g = observe.normalize_rdf(torch.tensor(counts)[None, None], 4, [[5]], [[3]], [False], 3.5, [321.5])
    assert np.abs(g[0, 0].numpy() - O.rdf_g(counts, 4, 15, 3.5, 321.5)).max() <= 4 * 2.0 ** -52 * want.max()
    assert np.allclose(r.numpy(), (np.arange(7) + 0.5) * 0.5, rtol=0, atol=1e-15)
    _, g = observe.normalize_rdf(torch.tensor(counts)[None, None], 4, [[3]], [[3]], [True], 3.5, None)
    assert np.abs(g[0, 0].numpy() - O.rdf_g(counts, 4, 3, 3.5, None)).max() <= 1e-15


# ---- the hand-built cases: margins, and the fp32 mirror against the fp64 oracle ------------------------------------------------------------
@pytest.mark.parametrize("name", ["five", "sixty_four", "three_hundred"])
def test_cases_keep_their_margin_and_mirror_equals_oracle(name):
    c = CS.case(name)
    n = len(c["z"])
    q = np.round(c["pos"].astype(np.float64) * 64.0) / 64.0
    assert np.abs(c["pos"] - q).max() <= 0.25 + 1e-6  # multiples of 2^-6 plus the jitter
    for bins in c["bins"]:
        _, _, rel = O.edge_margin(c["z"], c["pos"], c["box"], CS.PAIRS, c["r_max"], bins)
        assert len(rel) and rel.min() >= CS.MARGIN, (bins, rel.min())
        want = O.rdf_counts(c["z"], c["pos"], c["box"], CS.PAIRS, c["r_max"], bins)
        got = HM.rdf_counts(c["z"], c["pos"], c["box"], 1, np.zeros(n, np.int64), 1, CS.PAIRS, c["r_max"], bins)[0]
        print(name, bins, "pairs counted", want.sum(1).tolist(), "smallest margin", rel.min())
        assert (got.astype(np.int64) == want).all()
        assert want[0].sum() >= want[1].sum() + want[2].sum() > 0  # the wildcard holds the other two and every type has pairs


def test_the_batch_of_three_mirror_equals_oracle_per_molecule():
    c = CS.batch_of_three()
    got = HM.rdf_counts(c["z"], c["pos"], c["box"], 2, c["batch"], 3, CS.PAIRS, c["r_max"], 7)
    for m in range(3):
        k = c["batch"] == m
        _, _, rel = O.edge_margin(c["z"][k], c["pos"][k], c["box"][m], CS.PAIRS, c["r_max"], 7)
        assert rel.min() >= CS.MARGIN
        assert (got[m].astype(np.int64) == O.rdf_counts(c["z"][k], c["pos"][k], c["box"][m], CS.PAIRS, c["r_max"], 7)).all()
    assert got.sum() > 0 and np.diff(c["batch"]).min() >= 0


def test_the_300_atom_case_has_the_three_tile_pairs():
    from torchmdnet_amd import observe

    assert observe.tile_table([300]).tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 1]]
    assert observe.tile_table([5, 64, 300]).tolist() == [[0, 0, 0], [1, 0, 0], [2, 0, 0], [2, 0, 1], [2, 1, 1]]
    assert observe.tile_table([256]).tolist() == [[0, 0, 0]] and len(observe.tile_table([257, 0, 513])) == 3 + 6


def test_borderline_share_of_thermal_distances_is_below_the_bound_of_the_gpu_test():
    """The GPU test compares the device with the mirror on the loop's own frames, which keep no margin: it allows two counts per pair
    whose fp64 distance is within 1e-6 relative of an edge and fails when those exceed 0.5 % of the counted pairs.  Expected share for
    distances spread over the bins: 2e-6 d / dr <= 2e-6 bins.  Checked here on random coordinates for the bin counts that test uses."""
    rng = np.random.default_rng(5)
    pos = rng.uniform(0, 12.0, (192, 3)).astype(np.float32)
    box = np.diag([12.0, 12.0, 12.0]).astype(np.float32)
    for bins in (64, 256):
        _, _, rel = O.edge_margin(np.ones(192), pos, box, [(None, None)], 6.0, bins)
        _, _, d = O.nearest_image_distances(pos, box)
        share = (rel < 1e-6).sum() / max((d < 6.0).sum(), 1)
        print("bins", bins, "borderline share", share, "expected below", 2e-6 * bins)
        assert share <= 4 * 2e-6 * bins < 0.005


# ---- MSD and VACF oracles are consistent with their definition --------------------------------------------------------------------------
def test_oracle_sums_on_a_case_with_a_known_answer():
    z, batch = np.array([8, 1, 1, 8]), np.array([0, 0, 1, 1])
    x0 = np.zeros((4, 3))
    frames = np.stack([x0 + 1.0, x0 + 2.0])  # every atom moves by (1,1,1) per sample
    s, _ = O.msd_sums(z, batch, 2, [None, 8], x0, frames)
    assert s[0].tolist() == [[6.0, 3.0], [6.0, 3.0]] and s[1].tolist() == [[24.0, 12.0], [24.0, 12.0]]
    v = np.stack([np.full((4, 3), 1.0), np.full((4, 3), -2.0), np.full((4, 3), 3.0)])
    acc, mag = O.vacf_sums(z, batch, 2, [None], v, 3)
    assert acc[0, 0].tolist() == [6 * (1 + 4 + 9), 6 * (-2 - 6), 6 * 3] and mag[0, 0, 1] == 6 * 8
    assert O.sum_bound(10, 3.0) == 10 * 2.0 ** -52 * 3.0


# ---- the stand-alone program under the sanitizers -----------------------------------------------------------------------------------------
def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """a host build with its own main (never loaded into Python) under -fsanitize=address,undefined"""
    exe = str(tmp_path / "observe_host")
    HM.build_program(exe, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "observe_host: ok 1" in r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert "samples 13 bins 0 1 2 6 -1 -1 total 4" in r.stdout


# ---- host-side refusals, each before anything is staged -----------------------------------------------------------------------------------
def test_prepare_observe_tables_and_refusals():
    import torch

    from torchmdnet_amd import observe

    z = torch.tensor([8, 1, 1] * 8)
    batch = torch.repeat_interleave(torch.arange(2), 12)
    box = torch.diag(torch.tensor([10.0, 11.0, 12.0]))
    full = dict(every=2, frames=dict(capacity=3, velocities=True), rdf=dict(pairs=[(None, None), (8, 8), (1, 8)], r_max=5.0, bins=64),
                msd=dict(groups=[None, 8], capacity=10), vacf=dict(lags=4, groups=[1]))
    p = observe.prepare_observe(full, z, batch, box, 2, 8)
    assert p["mask"].tolist() == HM.masks(z.numpy(), full["rdf"]["pairs"], [None, 8], [1]).astype(np.int64).tolist()
    assert p["mol_start"].tolist() == [0, 12, 24] and p["tiles"].tolist() == [[0, 0, 0], [1, 0, 0]]
    assert p["n_a"].tolist() == [[12, 4, 8]] * 2 and p["n_b"].tolist() == [[12, 4, 4]] * 2
    assert p["msd_sizes"].tolist() == [[12, 4]] * 2 and p["vacf_sizes"].tolist() == [[8]] * 2
    assert p["spec"]["frames"] == dict(capacity=3, velocities=True) and p["spec"]["every"] == 2

    def refuse(match, K=8, z=z, batch=batch, box=box, **over):
        ob = {k: v for k, v in dict(full, **over).items() if v is not None}
        with pytest.raises(ValueError, match=match):
            observe.prepare_observe(ob, z, batch, box, 2, K)

    refuse("must divide steps_per_replay", K=7)
    refuse("must divide steps_per_replay", every=3)
    refuse("at least 1", every=0)
    refuse("at least one observable", frames=None, rdf=None, msd=None, vacf=None)
    refuse("1 to 4 pair types", rdf=dict(pairs=[(1, 1)] * 5, r_max=5.0, bins=64))
    refuse("1 to 4 pair types", rdf=dict(pairs=[], r_max=5.0, bins=64))
    refuse("1 to 4 groups", msd=dict(groups=[1, 2, 3, 4, 5], capacity=4))
    refuse("1 to 4 groups", vacf=dict(groups=[], lags=4))
    refuse("bins must be 1..1024", rdf=dict(pairs=[(1, 1)], r_max=5.0, bins=1025))
    refuse("lags must be 1..256", vacf=dict(groups=[None], lags=257))
    refuse("half the smallest box height", rdf=dict(pairs=[(1, 1)], r_max=5.01, bins=64))
    refuse("half the smallest box height", box=torch.tensor([[10.0, 0, 0], [0, 11.0, 0], [0, 10.0, 12.0]]))  # sheared: height < 10
    refuse("sorted batch", batch=batch.flip(0))
    refuse("capacity", frames=dict(capacity=0))
    refuse("capacity", msd=dict(groups=[None], capacity=0))
    refuse("unknown keys", structure_factor=dict())
    refuse("unknown keys", rdf=dict(pairs=[(1, 1)], r_max=5.0, bins=8, cutoff=3.0))
    refuse("atomic number or None", msd=dict(groups=["O"], capacity=4))
    with pytest.raises(ValueError, match="needs observe=dict"):
        observe.parse_observe(None, 8)
    # an unsorted batch is refused for the histogram only; every box of a batch is checked
    ok = {k: v for k, v in full.items() if k != "rdf"}
    assert observe.prepare_observe(ok, z, batch.flip(0), box, 2, 8)["tiles"] is None
    with pytest.raises(ValueError, match="half the smallest box height"):
        observe.prepare_observe(full, z, batch, torch.stack([box, 0.9 * box]), 2, 8)
    assert observe.box_heights(torch.tensor([[10.0, 0, 0], [0, 11.0, 0], [0, 10.0, 12.0]]))[0, 1] < 8.5
    # reset(observables="keep") continues the sums on an unchanged state only
    with pytest.raises(ValueError, match="keep"):
        observe.refuse_keep(torch.zeros(24, 3), None, 16, 16)
    with pytest.raises(ValueError, match="keep"):
        observe.refuse_keep(None, torch.zeros(24, 3), 16, 16)
    with pytest.raises(ValueError, match="keep"):
        observe.refuse_keep(None, None, 0, 16)
    observe.refuse_keep(None, None, 16, 16)


def test_capture_md_observed_signature():
    from torchmdnet_amd import md
    from torchmdnet_amd.models.model import TorchMD_Net

    names = list(inspect.signature(TorchMD_Net.capture_md_observed).parameters)
    assert names == ["self", "z", "pos", "vel", "masses", "dt", "batch", "box", "q", "num_systems", "steps_per_replay", "force_scale",
                     "thermostat", "warmup", "constraints", "observe"]
    assert "barostat" not in names and "bias" not in names  # not accepted as keywords
    base = list(inspect.signature(TorchMD_Net.capture_md).parameters)
    assert base[14:] == ["atom_weights", "halo_exchange", "barostat"]  # capture_md itself is untouched
    assert list(inspect.signature(md.DeviceMD.reset).parameters)[1:] == ["pos", "vel", "step", "box", "observables"]
    assert inspect.signature(md.DeviceMD.reset).parameters["observables"].default == "clear"
    for k in ("n_samples", "frames", "rdf", "msd", "vacf"):
        assert hasattr(md.DeviceMD, k) and hasattr(md.DeviceGlobalMD, k), k
    assert "leapfrog" in md.DeviceMD.vacf.__doc__.lower() and "without a box" in md.DeviceMD.rdf.__doc__.lower()


# ---- the additive ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_exports_agree():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)  # additive: the revision stays
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from torchmdnet_amd import _C

    src = open(_C.__file__).read()
    for name, n in {"tmdnet_md_observe_workspace_bytes": 4, "tmdnet_md_observe_start": 7, "tmdnet_md_observe": 17}.items():
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == n, name
        assert name in _C.declared_symbols() and name + ".argtypes" in src
    fields = re.search(r"typedef struct \{([^}]*)\} tmdnet_md_observe_spec;", code, flags=re.S).group(1)
    names = re.findall(r"\b(\w+);", fields)
    assert names == [f[0] for f in _C.ObserveSpec._fields_]
    assert (_C.OBSERVE_MAX_TYPES, _C.OBSERVE_MAX_BINS, _C.OBSERVE_MAX_LAGS, _C.OBSERVE_TILE) == (4, 1024, 256, 256)
    hdr = open(os.path.join(ROOT, "torchmd-net_amd", "csrc", "tn_observe_math.h")).read()
    for k, v in (("kMaxTypes", 4), ("kMaxBins", 1024), ("kMaxLags", 256), ("kTile", 256)):
        assert re.search(r"constexpr int " + k + r" = " + str(v) + r";", hdr), k


def test_library_exports_the_observe_entries(hip_lib):
    import ctypes as C

    from torchmdnet_amd import _C

    assert hip_lib.tmdnet_abi_version() == 10
    assert len(hip_lib.tmdnet_md_observe.argtypes) == 17 and len(hip_lib.tmdnet_md_observe_start.argtypes) == 7
    sp = _C.ObserveSpec(every=2, frame_capacity=3, frame_velocities=1, n_pair_types=2, bins=100, r_max2=9.0, inv_dr=33.0, n_msd_groups=1,
                        n_vacf_groups=2, lags=8, msd_capacity=50)
    nb = C.c_size_t(0)
    assert hip_lib.tmdnet_md_observe_workspace_bytes(300, 3, C.byref(sp), C.byref(nb)) == 0
    up = lambda n: (n + 255) & ~255  # noqa: E731
    want = 256 + 2 * up(3 * 300 * 12) + up(3 * 2 * 100 * 8) + up(300 * 12) + up(50 * 3 * 8) + up(8 * 300 * 12) + up(3 * 2 * 8 * 8) + 256
    assert nb.value == want
    only = _C.ObserveSpec(every=1, n_msd_groups=1, msd_capacity=4, bins=999, lags=999)  # sizes of what is off are ignored
    assert hip_lib.tmdnet_md_observe_workspace_bytes(10, 1, C.byref(only), C.byref(nb)) == 0 and nb.value == 256 + 256 + 256 + 256

    def bad(**over):
        s = _C.ObserveSpec(every=2, frame_capacity=3, n_pair_types=2, bins=100, r_max2=9.0, inv_dr=33.0, n_msd_groups=1, n_vacf_groups=2,
                           lags=8, msd_capacity=50)
        for k, v in over.items():
            setattr(s, k, v)
        return s

    for over in (dict(every=0), dict(n_pair_types=5), dict(bins=1025), dict(bins=0), dict(lags=257), dict(lags=0), dict(n_msd_groups=5),
                 dict(n_vacf_groups=-1), dict(msd_capacity=0), dict(r_max2=0.0), dict(inv_dr=float("nan")), dict(frame_capacity=-1),
                 dict(frame_capacity=0, n_pair_types=0, n_msd_groups=0, n_vacf_groups=0)):
        assert hip_lib.tmdnet_md_observe_workspace_bytes(300, 3, C.byref(bad(**over)), C.byref(nb)) == 1, over
    assert hip_lib.tmdnet_md_observe_workspace_bytes(0, 3, C.byref(sp), C.byref(nb)) == 1
    assert hip_lib.tmdnet_md_observe_workspace_bytes(300, 3, None, C.byref(nb)) == 1
    # refusals need no device: they return before anything is enqueued
    one = C.c_void_p(256)
    assert hip_lib.tmdnet_md_observe_start(None, None, 300, 3, C.byref(sp), 0, one) == 1
    assert hip_lib.tmdnet_md_observe_start(None, one, 300, 3, C.byref(sp), 0, None) == 1  # the MSD needs origins
    ok = [None, None, None, one, one, 300, 3, C.byref(sp), one, one, one, one, 2, one, one, one, 5]
    for pos, val in ((3, None), (4, None), (7, None), (8, None), (9, None), (10, None), (12, 0), (12, 3), (13, None), (14, None),
                     (15, None), (16, -1), (2, one), (5, 0), (6, 0), (7, C.byref(bad(bins=2000)))):
        a = list(ok)
        a[pos] = val
        assert hip_lib.tmdnet_md_observe(*a) == 1, (pos, val)
    a = list(ok)
    a[11], a[12] = None, 1  # a box mode without a box
    assert hip_lib.tmdnet_md_observe(*a) == 1
