"""No GPU: temperature replica exchange of the device-resident MD loop (csrc/tn_remd_math.h, compiled host-only by
tests/remd_host_mirror.py) against tests/remd_oracle.py - the scheme in Python integers and fp64 floats, an independent Philox -, the
acceptance statistics on exact canonical energies, the sampling protocol of the harmonic well, and the additive C ABI."""
import math
import os
import re

import numpy as np
import pytest

from tests import md_baro_host_mirror as HB
from tests import md_host_mirror as H
from tests import md_oracle as MO
from tests import remd_host_mirror as HR
from tests import remd_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_enumeration():
    for R in (2, 3, 4, 5, 8, 33):
        for a in (0, 1, 2, 7, 2 ** 40, 2 ** 40 + 1):
            assert HR.pairs(a, R) == O.pairs(a, R) == [s for s in range(R - 1) if s % 2 == a % 2], (R, a)
    assert HR.pairs(1, 2) == [] and HR.pairs(0, 2) == [0]  # R = 2: odd attempts have no pair
    assert HR.pairs(0, 5) == [0, 2] and HR.pairs(1, 5) == [1, 3]  # odd R: slot 4, then slot 0, idles


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("R", [2, 3, 5, 8])
def test_decisions_slots_and_logs_equal_the_oracle(G, R):
    """200 attempts on random energies: every decision, slot, holder, log row and counter.  The seeds are such that the oracle alone
    reports no pair with |u - exp D| within 4 fp64 ulp (asserted: nothing is skipped)."""
    every, seed = 7, 0x0123456789ABCDEF + 1000 * G + R
    rng = np.random.default_rng(100 * G + R)
    kT = np.sort(rng.uniform(0.5, 3.0, size=R))
    if R == 5:
        kT = kT[[0, 3, 1, 4, 2]]  # the ladder need not be monotonic
    beta = 1.0 / kT
    mir, ora = HR.Ladders(G, R, beta, every, seed), O.Ladders(G, R, beta, every, seed)
    accepted = 0
    for a in range(1, 201):
        n = a * every + (3 if a % 5 == 0 else 0)  # a = n // every also off the multiples
        epot = rng.gamma(6.0, kT.mean(), size=G * R).astype(np.float32)
        slot_o, acc_o = ora.attempt(n, epot)
        slot_m, acc_m = mir.attempt(n, epot)
        assert (acc_m == acc_o).all() and (slot_m == slot_o).all(), (a, acc_m, acc_o)
        assert (mir.slot == slot_o).all() and (mir.holder == np.array(ora.holder)).all()
        assert (mir.accept == acc_o).all()
        O.check_inverse(mir.slot, mir.holder, G, R)
        accepted += int(acc_o.sum())
    assert ora.undecidable == []
    assert (mir.counters[0] == ora.attempts).all() and (mir.counters[1] == ora.accepts).all()
    tried = sum(len(O.pairs(a, R)) for a in range(1, 201)) * G
    assert mir.counters[0].sum() == tried and 0 < accepted < tried  # both outcomes occur
    assert not (mir.slot == np.tile(np.arange(R), G)).all() or R == 2


def test_uniform_counter_layout():
    """key = the 64-bit seed (low word first), counter = (n low, n high, g (R - 1) + s, 2): apart from the atoms' (0) and the
    barostat's (1) streams"""
    seed, step = 0x0123456789ABCDEF, (5 << 32) + 77
    idx = np.array([0, 1, 999, 2 ** 31 + 3], np.uint32)
    got = HR.uniform(seed, step, idx)
    for k, i in enumerate(idx):
        w = MO.philox4x32_10((77, 5, int(i), 2), (0x89ABCDEF, 0x01234567))
        assert float(got[k]) == MO.uniform(w[0])  # exact: the fp32 value widened
        for other in (0, 1):  # the same (seed, step, index) in the other streams: other words
            assert MO.philox4x32_10((77, 5, int(i), other), (0x89ABCDEF, 0x01234567))[0] != w[0]
    assert got[2] == np.float32(O.uniform(seed, step, 999 // 7, 999 % 7, 8))  # g (R - 1) + s with R = 8
    # against the header's own other streams, through their first uniform: the atoms' xi and the barostat's xi differ from
    # the Box-Muller map of this stream's words
    xi_atoms = H.noise(seed, step, idx)[:, 0]
    xi_baro = HB.noise(seed, step, idx)
    words = H.philox(np.array([[77, 5, int(i), 2] for i in idx], np.uint32), np.tile(np.array([0x89ABCDEF, 0x01234567], np.uint32), (4, 1)))
    xi_here = H.normals(words)[:, 0]
    assert np.abs(xi_here - xi_atoms).min() > 1e-4 and np.abs(xi_here - xi_baro).min() > 1e-4
    assert (H.uniform(words[:, 0]) == got).all()
    assert (HR.uniform(seed, step + 1, idx) != got).all() and (HR.uniform(seed + 1, step, idx) != got).all()
    assert (got > 0).all() and (got <= 1).all()


def test_edge_cases_of_the_decision():
    u1 = np.float32(1.0)  # the largest u there is: only D >= 0 accepts
    E = np.array([3.0, -2.0, 0.0, 1e30], np.float32)
    # equal energies, any temperatures; equal temperatures, any energies: D = 0
    assert (HR.decide(1.0, 0.5, E, E, u1) == 1).all()
    assert (HR.decide(0.7, 0.7, E, E[::-1].copy(), u1) == 1).all()
    # the cold slot (larger beta) holds the higher energy: D > 0
    assert (HR.decide(1.0, 0.5, E + 1.0, E, u1)[:3] == 1).all()
    # D < 0: by u
    assert HR.decide(1.0, 0.5, [0.0], [2.0], np.float32(0.36))[0] == 1 and HR.decide(1.0, 0.5, [0.0], [2.0], np.float32(0.37))[0] == 0
    assert abs(math.exp(-1.0) - 0.3679) < 1e-4
    # NaN or +-inf energies on either side reject (D = NaN, or D = -inf, or inf - inf); never an error
    nan, inf = np.float32("nan"), np.float32("inf")
    for Ei, Ej in ((nan, 1.0), (1.0, nan), (nan, nan), (inf, inf), (-inf, -inf), (-inf, 1.0), (1.0, inf)):
        assert HR.decide(1.0, 0.5, [Ei], [Ej], np.float32(2.0 ** -25))[0] == 0, (Ei, Ej)
        assert O.decide(1.0, 0.5, Ei, Ej, 2.0 ** -25)[0] is False or not O.decide(1.0, 0.5, Ei, Ej, 2.0 ** -25)[0]
    # equal temperatures with an infinite energy: 0 * inf = NaN, a rejection
    assert HR.decide(0.7, 0.7, [inf], [1.0], u1)[0] == 0
    # a full attempt on NaN energies: nothing moves, the attempt is counted
    lad = HR.Ladders(2, 3, [1.0, 0.8, 0.5], 4, 9)
    slot_log, acc = lad.attempt(8, np.full(6, np.nan, np.float32))
    assert (acc == 0).all() and (slot_log == np.tile(np.arange(3), 2)).all() and (lad.holder == np.arange(3)).all()
    assert lad.counters[0].tolist() == [[1, 0], [1, 0]] and lad.counters[1].sum() == 0


def test_atoms_follow_the_decisions():
    """the per-atom launch: accepted replicas' velocities are one rounded product with up / down, their sigma rows the table rows
    of the new slots; everything else keeps its bits; an atom of infinite mass keeps sigma = 0 and its zero velocity"""
    G, R, n, every, seed = 2, 3, 5, 4, 77
    kT = np.array([1.0, 1.5, 2.5])
    mass = np.array([1.0, 12.0, np.inf, 16.0, 1.008])
    beta, table, up, down = HR.tables(kT, mass, 9.648533e-3)
    assert (table[:, 2] == 0).all()
    rng = np.random.default_rng(3)
    for step in (4, 8):  # one attempt in each parity
        lad = HR.Ladders(G, R, beta, every, seed)
        epot = np.array([5.0, 1.0, 0.5, 9.0, 9.5, 0.1], np.float32)  # ladder 0: (0,1) D > 0; ladder 1: (1,2) D > 0
        vel = rng.normal(size=(G * R * n, 3)).astype(np.float32)
        vel[2::n] = 0.0
        sigma0 = table[lad.slot].reshape(-1)
        before = lad.slot.copy()
        slot_log, acc = lad.attempt(step, epot)
        v2, s2 = lad.atoms(step, vel, sigma0, table, up, down)
        assert acc.sum() >= 1
        for b in range(G * R):
            rows = slice(b * n, (b + 1) * n)
            new, old = int(lad.slot[b]), int(before[b])
            if new == old:
                assert (v2[rows].view(np.uint32) == vel[rows].view(np.uint32)).all() and (s2[rows] == sigma0[rows]).all()
            else:
                f = up[old] if new == old + 1 else down[new]
                assert (v2[rows].view(np.uint32) == (vel[rows] * f).view(np.uint32)).all()
                assert (s2[rows].view(np.uint32) == table[new].view(np.uint32)).all()
        assert (v2[2::n] == 0).all() and (s2[2::n] == 0).all()


def test_acceptance_on_exact_canonical_energies():
    """Energies of two slots from the exact canonical law of a d-dimensional harmonic well, Gamma(d/2, kT): over 20 000 attempts the
    empirical acceptance of the mirror agrees with the oracle's mean of min(1, exp D) on the same draws within 4 binomial standard
    errors."""
    d, kT, N = 12, np.array([1.0, 1.4]), 20000
    beta = 1.0 / kT
    rng = np.random.default_rng(2024)
    E = np.stack([rng.gamma(d / 2, kT[0], size=N), rng.gamma(d / 2, kT[1], size=N)], 1).astype(np.float32)
    lad = HR.Ladders(1, 2, beta, 1, 31337)
    acc, p = np.zeros(N), np.zeros(N)
    for k in range(N):
        n = 2 * k  # even attempts: the one pair of R = 2 is tried
        i, j = int(lad.holder[0, 0]), int(lad.holder[0, 1])
        p[k] = O.probability(beta[0], beta[1], E[k, 0], E[k, 1])
        e = np.empty(2, np.float32)
        e[i], e[j] = E[k, 0], E[k, 1]  # the holder of slot 0 gets the cold draw
        acc[k] = lad.attempt(n, e)[1][0, 0]
    se = math.sqrt(p.mean() * (1 - p.mean()) / N)
    print("acceptance", acc.mean(), "expected", p.mean(), "standard error", se)
    assert 0.2 < p.mean() < 0.8
    assert abs(acc.mean() - p.mean()) < 4 * se
    assert lad.counters[0, 0, 0] == N and lad.counters[1, 0, 0] == acc.sum()


def test_harmonic_well_is_sampled_canonically_at_every_slot():
    """the protocol and the bounds of tests/remd_oracle.py (SAMPLING, sampling_statistics) on the host mirror; the GPU test runs the
    same protocol through the C entries"""
    e = O.SAMPLING
    x, v = O.sampling_state()
    r = HR.harmonic(e["G"], e["R"], e["n"], e["attempts"], e["every"], x, v, np.ones(e["n"]), e["kT"], e["dt"], e["friction"], e["seed"], e["k"])
    stats = O.sampling_statistics(r["epot"], r["ekin"], r["slot_log"], r["accept_log"], e["kT"], e["n"])
    for name in ("epot", "ekin", "acceptance"):
        for row in stats[name]:
            print(name, row)
    O.assert_sampling(stats)
    O.check_inverse(r["slot"], r["holder"], e["G"], e["R"])
    # the decisions of the run are the oracle's on the logged energies
    ora = O.Ladders(e["G"], e["R"], 1.0 / np.asarray(e["kT"]), e["every"], e["seed"])
    for a in range(200):
        slot_o, acc_o = ora.attempt((a + 1) * e["every"], r["epot"][a])
        assert (slot_o == r["slot_log"][a]).all() and (acc_o == r["accept_log"][a]).all(), a
    assert ora.undecidable == []


# ---- the additive ABI -------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_exports_agree():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("tmdnet_md_exchange_workspace_bytes", "tmdnet_md_exchange"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    args = re.search(r"\bint\s+tmdnet_md_exchange\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(args.split(",")) == 22
    assert len(re.search(r"\bint\s+tmdnet_md_exchange_workspace_bytes\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")) == 3
    assert len(re.search(r"\bint\s+tmdnet_md_advance\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")) == 22  # untouched
    assert len(re.search(r"\bint\s+tmdnet_md_barostat\s*\((.*?)\)\s*;", code, flags=re.S).group(1).split(",")) == 27
    from torchmdnet_amd import _C

    declared = _C.declared_symbols()
    assert "tmdnet_md_exchange" in declared and "tmdnet_md_exchange_workspace_bytes" in declared
    src = open(_C.__file__).read()
    assert "tmdnet_md_exchange.argtypes" in src and "tmdnet_md_exchange_workspace_bytes.argtypes" in src


def test_library_exports_the_exchange_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10
    assert len(hip_lib.tmdnet_md_exchange.argtypes) == 22 and len(hip_lib.tmdnet_md_exchange_workspace_bytes.argtypes) == 3
    nb = C.c_size_t(0)
    assert hip_lib.tmdnet_md_exchange_workspace_bytes(6, 3, C.byref(nb)) == 0 and nb.value >= 4
    for n_mol, ladder in ((6, 1), (7, 3), (0, 2), (-2, 2)):
        assert hip_lib.tmdnet_md_exchange_workspace_bytes(n_mol, ladder, C.byref(nb)) != 0, (n_mol, ladder)
    # refusals need no device: they return before anything is enqueued
    one = C.c_void_p(256)
    ok = [None, None, None, one, one, 30, 6, 3, 2, one, one, one, one, one, one, one, 0, one, one, None, None, None]
    for pos, bad in ((7, 1), (6, 7), (5, 31), (8, 0), (3, None), (4, None), (9, None), (10, None), (11, None), (12, None), (13, None), (14, None),
                     (15, None), (17, None), (18, None)):
        a = list(ok)
        a[pos] = bad
        assert hip_lib.tmdnet_md_exchange(*a) == 1, (pos, bad)


def test_capture_remd_and_md_module_signatures():
    import inspect

    import torch

    from torchmdnet_amd import md
    from torchmdnet_amd.models.model import TorchMD_Net

    names = list(inspect.signature(TorchMD_Net.capture_remd).parameters)
    assert names[1:8] == ["z", "pos", "vel", "masses", "dt", "temperatures", "exchange_every"]
    for k in ("box", "q", "steps_per_replay", "force_scale", "thermostat", "warmup", "barostat", "constraints", "atom_weights", "halo_exchange"):
        assert k in names, k
    assert issubclass(md.DeviceREMD, md.DeviceMD)
    assert list(inspect.signature(md.DeviceREMD.reset).parameters)[1:] == ["pos", "vel", "step", "slots"]
    for k in ("by_slot", "acceptance", "attempts", "accepts"):
        assert hasattr(md.DeviceREMD, k), k
    lad = md.geometric_ladder(0.5, 4.0, 4)
    assert lad.dtype == torch.float64 and torch.allclose(lad, torch.tensor([0.5, 1.0, 2.0, 4.0], dtype=torch.float64), rtol=1e-14)
    with pytest.raises(ValueError):
        md.geometric_ladder(0.5, 4.0, 1)
    # capture_md's own signature is untouched
    assert list(inspect.signature(TorchMD_Net.capture_md).parameters)[14:] == ["atom_weights", "halo_exchange", "barostat"]
