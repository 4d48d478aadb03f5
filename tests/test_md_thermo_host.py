"""No GPU: the global thermostats of the device-resident MD loop (csrc/tn_md_thermo_math.h compiled for the host,
tests/md_thermo_host_mirror.py) against the independent fp64 specification (tests/md_thermo_oracle.py).

1. alpha, reservoir and chain state against the oracle   2. the counter layout   3. exact cases   4. the canonical ensemble
5. the conserved energy   6. the failure protocol   7. refusals and signatures   8. the header under the host sanitizers"""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import md_oracle as O
from tests import md_thermo_host_mirror as M
from tests import md_thermo_oracle as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KT, TAU, DT = 0.025, 5.0, 0.5
SIZES = (1, 2, 3, 4, 9, 189)  # N - 1 = 0, odd and even, and the shape-1 boundary of the gamma deviate (N = 3, 4)


# ---- 1. against the oracle --------------------------------------------------------------------------------------------------------
def test_csvr_alpha_and_reservoir_agree_with_the_oracle():
    """K from 0.01 Kbar to 100 Kbar, four steps (one past 2^32), two seeds, five molecules.  The relative differences are measured
    and printed; the asserted bounds are ten times the values measured when the test was written (T.BOUNDS)."""
    wa = wr = 0.0
    for N in SIZES:
        Kbar = 0.5 * N * KT
        ekin = np.array([0.01, 0.3, 1.0, 3.0, 100.0]) * Kbar
        for step in (0, 1, 7, 2 ** 33 + 5):
            for seed in (0, 2 ** 40 + 3):
                bad, alpha, _, res, flags = M.moves(M.CSVR, ekin, [N] * 5, KT, TAU, DT, seed, step)
                assert bad == 0 and not flags.any()
                for m in range(5):
                    a2, _, K = T.csvr(ekin[m], N, KT, TAU, DT, seed, step, m)
                    wa = max(wa, abs(float(alpha[m]) - math.sqrt(a2)) / math.sqrt(a2))
                    wr = max(wr, abs(res[m] + (a2 - 1.0) * K) / Kbar)
    print("csvr: largest relative difference of alpha", wa, "(bound", T.BOUNDS["csvr"]["alpha"], ") of the reservoir / Kbar", wr,
          "(bound", T.BOUNDS["csvr"]["reservoir"], ")")
    assert wa <= T.BOUNDS["csvr"]["alpha"] and wr <= T.BOUNDS["csvr"]["reservoir"]


def _chain_start(B, Mc, nonzero):
    chain = np.zeros((B, 2, Mc))
    if nonzero:
        chain[:, 0, :] = 0.1 * np.arange(1, Mc + 1)
        chain[:, 1, :] = 0.02 * np.cos(np.arange(Mc))[None, :]
    return chain


def test_chain_agrees_with_the_oracle_over_200_moves():
    """M in {1, 3, 8}, substeps in {1, 2, 5}, from zero and from non-zero chain state, 200 consecutive moves of four molecules; the
    kinetic energy follows alpha^2 and an outside modulation, so the chains are driven both ways.  The oracle runs on its own state."""
    wa = wr = wc = 0.0
    ndof = [9, 3, 189, 1]
    for Mc in (1, 3, 8):
        for sub in (1, 2, 5):
            for nonzero in (0, 1):
                chain = _chain_start(4, Mc, nonzero)
                orc = [T.Chain(ndof[m], KT, TAU, Mc, chain[m, 0], chain[m, 1]) for m in range(4)]
                ekin = np.array([0.5 * n * KT * f for n, f in zip(ndof, (0.3, 1.0, 2.5, 1.0))], np.float32)
                res = np.zeros(4)
                for n in range(200):
                    bad, alpha, chain, res, _ = M.moves(M.NHC, ekin, ndof, KT, TAU, DT, 0, n, Mc, sub, chain, res)
                    assert bad == 0
                    for m in range(4):
                        orc[m].move(ekin[m], DT, sub)
                        wa = max(wa, abs(float(alpha[m]) - orc[m].s) / orc[m].s)
                        wr = max(wr, abs(res[m] - orc[m].energy()) / max(abs(orc[m].energy()), ndof[m] * KT))
                        wc = max(wc, T.rel(chain[m, 0], orc[m].xi, 1.0), T.rel(chain[m, 1], orc[m].v, 1.0 / TAU))
                    ekin = (ekin * alpha * alpha * np.float32(1.0 + 0.3 * math.sin(0.7 * n))).astype(np.float32)
    b = T.BOUNDS["nose-hoover"]
    print("chain: largest relative difference of alpha", wa, "(bound", b["alpha"], ") reservoir", wr, "(bound", b["reservoir"],
          ") chain state", wc, "(bound", b["chain"], ")")
    assert wa <= b["alpha"] and wr <= b["reservoir"] and wc <= b["chain"]


def test_bounds_are_ten_times_the_measured_values():
    for kind, meas in T.MEASURED.items():
        for key, v in meas.items():
            want = max(10.0 * v, 2.0 ** -23) if key == "alpha" else 10.0 * v
            assert T.BOUNDS[kind][key] == want, (kind, key)


# ---- 2. the counter layout ----------------------------------------------------------------------------------------------------------
def test_draws_use_word_3_tags_3_plus_256_j_only():
    known = {(0, 0, 0, 0): (0x4D7B25FC, 0xD75EE2F1, 0x26BC1F97, 0xC64D811C),
             (2 ** 40 + 11, 2 ** 33 + 5, 7, 1): (0x8030E92D, 0x23732B62, 0x25093EE9, 0xB742AE66),
             (123456789, 41, 4095, 64): (0x9ABEFD64, 0xFE11BFE4, 0x42D8B371, 0x94A29970)}
    for (seed, step, mol, draw), w in known.items():
        assert M.words(seed, step, mol, draw) == w
        assert O.philox4x32_10((step & 0xFFFFFFFF, step >> 32, mol, 3 + 256 * draw), (seed & 0xFFFFFFFF, seed >> 32)) == w
        assert T.counter(step, mol, draw)[3] % 256 == 3  # never the atoms' (0), the barostat's (1) or the exchange's (2)


def test_alpha_is_a_function_of_seed_step_and_molecule():
    N, ekin = 9, np.float32(0.07)
    base = M.moves(M.CSVR, [ekin] * 6, [N] * 6, KT, TAU, DT, 5, 12)[1]
    # molecule 3 alone (a batch of one, told its index), and in a larger batch: the same bits
    one = M.moves(M.CSVR, [ekin], [N], KT, TAU, DT, 5, 12, mols=[3])[1]
    big = M.moves(M.CSVR, [ekin] * 40, [N] * 40, KT, TAU, DT, 5, 12)[1]
    assert one[0] == base[3] == big[3] and (big[:6] == base).all()
    assert len(set(base.tolist())) == 6  # another molecule: another alpha
    assert M.moves(M.CSVR, [ekin], [N], KT, TAU, DT, 5, 13, mols=[3])[1][0] != base[3]  # another step
    assert M.moves(M.CSVR, [ekin], [N], KT, TAU, DT, 6, 12, mols=[3])[1][0] != base[3]  # another seed
    # K steps per replay do not enter: a run of 6 steps equals 2 runs of 3 continued at step0 = 3
    rng = np.random.default_rng(1)
    x, v = rng.normal(size=(6, 3)).astype(np.float32), rng.normal(size=(6, 3)).astype(np.float32)
    hk, mass = np.full(6, 0.05, np.float32), np.ones(6, np.float32)
    a = M.run(M.CSVR, x, v, hk, mass, [9, 9], 0.1, 0.0, KT, 1.0, 6, seed=9)
    b = M.run(M.CSVR, x, v, hk, mass, [9, 9], 0.1, 0.0, KT, 1.0, 3, seed=9)
    # (free flight: the force is zero, so the OPEN of the second run is the opening half that the first run's last step left out)
    c = M.run(M.CSVR, b["x"], b["v"], hk, mass, [9, 9], 0.1, 0.0, KT, 1.0, 3, seed=9, step0=3)
    assert (np.concatenate([b["scale"], c["scale"]]) == a["scale"]).all() and (c["v"] == a["v"]).all() and (c["x"] == a["x"]).all()


# ---- 3. exact cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,Mc", [(M.CSVR, 0), (M.NHC, 3)])
def test_no_kinetic_energy_or_no_degrees_of_freedom_is_never_scaled(kind, Mc):
    chain, res = np.full((3, 2, Mc), 0.25), np.array([1.0, 2.0, 3.0])
    bad, alpha, ch, r, flags = M.moves(kind, [0.0, 0.3, np.nan], [9, 0, 0], KT, TAU, DT, 1, 2, Mc, 2, chain, res)
    assert bad == 0 and not flags.any() and (alpha == 1.0).all() and (ch == chain).all() and (r == res).all()


def test_chain_at_rest_at_the_target_temperature_gives_exactly_one():
    for Mc in (1, 3, 8):
        for sub in (1, 2, 5):
            N, kT = 8, 0.125  # 2 K = N kT = 1 exactly in fp32 and fp64
            bad, alpha, ch, _, _ = M.moves(M.NHC, [0.5], [N], kT, 4.0, 1.0, 0, 0, Mc, sub)
            assert bad == 0 and alpha[0] == 1.0 and ch[0, 1, 0] == 0.0 and ch[0, 0, 0] == 0.0


def test_tau_far_below_dt_forgets_the_kinetic_energy():
    """c = exp(-dt / tau) = 0: K' = alpha^2 K = (Kbar / N) (R1^2 + S) whatever K was.  alpha carries one fp32 rounding (2^-24
    relative), so alpha^2 K two, on either side: 4 * 2^-24, and the fp32 K itself is exact here (powers of two times 0.07)."""
    for N in SIZES:
        K = np.float32(0.07) * np.array([1.0, 4.0, 0.25, 64.0], np.float32)
        out = []
        for k in K:
            bad, alpha, _, _, _ = M.moves(M.CSVR, [k], [N], KT, 1e-3 * DT, DT, 3, 4)
            assert bad == 0
            out.append(float(alpha[0]) ** 2 * float(k))
        assert max(out) / min(out) - 1.0 <= 4 * 2.0 ** -24 + 1e-12, (N, out)


def test_scaling_is_one_rounded_product_and_skips_infinite_mass():
    rng = np.random.default_rng(3)
    v = rng.normal(size=(50, 3)).astype(np.float32)
    batch = rng.integers(0, 4, size=50)
    alpha = np.array([0.9371, 1.0, 1.0625001, 3.1e-3], np.float32)
    hk = np.full(50, 0.01, np.float32)
    hk[[4, 17]] = 0.0  # infinite mass
    got = M.scale(batch, alpha, hk, v)
    want = np.float32(v) * np.float32(alpha)[batch][:, None]
    want[[4, 17]] = v[[4, 17]]
    assert (got.view(np.int32) == want.view(np.int32)).all()


# ---- 4. the ensemble --------------------------------------------------------------------------------------------------------------
def _free_molecules(ndof):
    """4 096 molecules with `ndof` degrees of freedom at K = Kbar: three atoms (N = 9), or a diatomic along x with ndof = 2"""
    e = T.ENSEMBLE
    n = 3 if ndof == 9 else 2
    v = np.zeros((e["B"] * n, 3), np.float32)
    if ndof == 9:
        v[:] = math.sqrt(e["kT"])  # 0.5 m v^2 = kT / 2 per component
    else:
        v[:, 0] = math.sqrt(e["kT"])  # two atoms moving along x: K = 2 * kT / 2
    return n, v


@pytest.mark.parametrize("ndof", [9, 2])
def test_csvr_samples_the_canonical_kinetic_energy(ndof):
    """Zero forces, tau = dt, 32 steps from K = Kbar: alpha^2 K of the last step is Gamma(N / 2, scale kT) distributed, exactly for any
    dt.  Kolmogorov-Smirnov distance below 0.042 (4 096 samples, 1e-6 level); the seed is one for which the oracle alone is below
    0.021."""
    e = T.ENSEMBLE
    d_oracle = T.ks_distance(T.ensemble(ndof), ndof)
    n, v = _free_molecules(ndof)
    N = e["B"] * n
    r = M.run(M.CSVR, np.zeros((N, 3), np.float32), v, np.full(N, 0.5 * e["dt"], np.float32), np.ones(N, np.float32), [ndof] * e["B"],
              e["dt"], 0.0, e["kT"], e["tau"], e["steps"], seed=e["seed"])
    sample = r["scale"][-1].astype(np.float64) ** 2 * r["ekin"][-1].astype(np.float64)
    d = T.ks_distance(sample, ndof)
    print("N =", ndof, "KS distance: header", d, "oracle", d_oracle, "mean K / Kbar", sample.mean() / (0.5 * ndof * e["kT"]))
    assert d_oracle < e["oracle_bound"]
    assert d < e["bound"]


# ---- 5. the conserved energy --------------------------------------------------------------------------------------------------------
def _oscillators():
    rng = np.random.default_rng(5)
    R, n, kappa = 4, 16, 1.0
    mass = (1.0 + 3.0 * rng.uniform(size=R * n)).astype(np.float32)  # periods from 2 pi to 4 pi: the phases do not stay aligned
    dt = 2.0 * math.pi / 50.0  # a fiftieth of the shortest period
    x = (math.sqrt(KT / kappa) * rng.normal(size=(R * n, 3))).astype(np.float32)
    v = (np.sqrt(KT / mass)[:, None] * rng.normal(size=(R * n, 3))).astype(np.float32)
    hk = (0.5 * dt / mass.astype(np.float64)).astype(np.float32)
    return dict(x=x, v=v, hk=hk, mass=mass, ndof=[3 * n] * R, dt=dt, kappa=kappa, kT=KT, tau=20.0 * dt, steps=2000)


@pytest.mark.parametrize("kind,Mc,sub", [(M.CSVR, 0, 1), (M.NHC, 3, 2)])
def test_conserved_energy_does_not_drift(kind, Mc, sub):
    """Independent harmonic atoms, dt = period / 50, 2 000 steps.  The drift of epot + kinetic_after + reservoir - its mean over the
    last 200 steps against its mean over the first 200, four periods each, so that the bounded oscillation of the integrator's energy
    error averages out - is at most twice the peak-to-peak fluctuation of epot + ekin in the same run without a thermostat, while the
    kinetic energy itself wanders by more than ten times that: a dead thermostat cannot pass."""
    o = _oscillators()
    nve = M.run(M.NONE, **o)
    E = nve["epot"] + nve["ekin"]
    p2p = E.max(0) - E.min(0)
    r = M.run(kind, seed=11, M=Mc, substeps=sub, **o)
    after = r["scale"].astype(np.float64) ** 2 * r["ekin"]
    cons = r["epot"] + after + r["reservoir_log"]
    drift = np.abs(cons[-200:].mean(0) - cons[:200].mean(0))
    wander = after.max(0) - after.min(0)
    print("NVE peak-to-peak", p2p, "drift of the conserved energy", drift, "largest excursion", np.abs(cons - cons[0]).max(0),
          "kinetic energy wanders by", wander)
    assert (drift <= 2.0 * p2p).all()
    assert (wander > 10.0 * p2p).all()
    assert (r["scale"] != 1.0).mean() > 0.9  # (a chain's factor may round to 1 in a step where its first velocity crosses zero)


# ---- 6. failure -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,Mc", [(M.CSVR, 0), (M.NHC, 3)])
def test_a_nan_kinetic_energy_flags_the_block_and_writes_nothing(kind, Mc):
    chain, res = np.full((4, 2, Mc), 0.25), np.array([1.0, 2.0, 3.0, 4.0])
    bad, alpha, ch, r, flags = M.moves(kind, [0.1, np.nan, 0.1, 0.1], [9] * 4, KT, TAU, DT, 0, 3, Mc, 2, chain, res)
    assert bad == 1 and flags.tolist() == [0, 1, 0, 0]
    assert np.isnan(alpha).all() and (ch == chain).all() and (r == res).all()  # alpha keeps the mirror's fill: never written
    assert M.moves(kind, [0.1, np.inf], [9, 9], KT, TAU, DT, 0, 3, Mc, 2)[0] == 1  # an infinite kinetic energy is unusable too


# ---- 7. refusals and signatures -----------------------------------------------------------------------------------------------------
def test_refusals_need_no_gpu():
    from torchmdnet_amd import md
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    ok = dict(kind="csvr", kT=0.025, tau=10.0)
    nh = dict(kind="nose-hoover", kT=0.025, tau=10.0)
    full = md.parse_global_thermostat(nh)
    assert (full["chain"], full["substeps"], full["ndof"]) == (3, 2, None)
    assert md.parse_global_thermostat(dict(ok, seed=-1))["seed"] == 2 ** 64 - 1
    bad = [None, dict(ok, kind="berendsen"), dict(kT=0.025, tau=1.0), dict(ok, friction=1.0), dict(ok, chain=3), dict(nh, seed=1),
           dict(ok, tau=0.0), dict(ok, tau=-1.0), dict(ok, kT=0.0), dict(ok, kT=float("nan")), dict(kind="csvr", kT=1.0),
           dict(kind="csvr", tau=1.0), dict(nh, chain=0), dict(nh, chain=9), dict(nh, substeps=0), dict(ok, ndof=-1),
           dict(ok, ndof=torch.tensor([3, -2])), dict(ok, ndof=2.5)]
    model = create_model(dict(W.TINY_ARGS, static_shapes=True))
    z, pos, batch = W.synthetic_batch(n_mol=2, n_atoms=5)
    vel, mass = torch.zeros_like(pos), torch.ones(len(z))
    for th in bad:
        with pytest.raises(ValueError):
            md.parse_global_thermostat(th)
        with pytest.raises(ValueError):  # through the public method, on CPU tensors: refused before anything is staged
            model.capture_md_global(z, pos, vel, mass, 0.1, batch=batch, thermostat=th)
    with pytest.raises(ValueError, match="one per molecule"):
        md.stage_ndof(torch.tensor([1, 2, 3]), torch.tensor([3, 3]), 2)
    assert md.stage_ndof(torch.tensor([5]), torch.tensor([3, 3]), 2).tolist() == [5, 5]
    assert md.stage_ndof(None, torch.tensor([3, 6]), 2).tolist() == [3, 6]
    # what _capture_inputs refuses stays refused
    with pytest.raises(ValueError, match="steps_per_replay"):
        model.capture_md_global(z, pos, vel, mass, 0.1, batch=batch, thermostat=ok, steps_per_replay=0)
    with pytest.raises(RuntimeError, match="static_shapes"):
        create_model(dict(W.TINY_ARGS)).capture_md_global(z, pos, vel, mass, 0.1, batch=batch, thermostat=ok)
    with pytest.raises(NotImplementedError, match="output_model"):
        create_model(dict(W.TINY_ARGS, static_shapes=True, output_model="DipoleMoment")).capture_md_global(
            z, pos, vel, mass, 0.1, batch=batch, thermostat=ok)
    with pytest.raises(RuntimeError, match="AMD GPU"):  # and a valid request on CPU tensors reaches the device check, no fallback
        model.capture_md_global(z, pos, vel, mass, 0.1, batch=batch, thermostat=ok)
    # no barostat, bias or exchange parameter
    names = list(inspect.signature(type(model).capture_md_global).parameters)
    assert names == ["self", "z", "pos", "vel", "masses", "dt", "batch", "box", "q", "num_systems", "steps_per_replay", "force_scale",
                     "warmup", "thermostat", "constraints"]
    assert issubclass(md.DeviceGlobalMD, md.DeviceMD)
    for name in ("kinetic_after", "conserved"):
        assert callable(getattr(md.DeviceGlobalMD, name))


def test_header_and_bindings_are_additive():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("tmdnet_md_thermostat_workspace_bytes", "tmdnet_md_thermostat"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    for name, n in (("tmdnet_md_thermostat", 25), ("tmdnet_md_advance", 22), ("tmdnet_md_barostat", 27)):
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == n, name
    assert re.search(r"5: a move of a global thermostat", txt)  # status 5 is documented at tmdnet_md_status
    from torchmdnet_amd import _C

    declared = _C.declared_symbols()
    assert "tmdnet_md_thermostat" in declared and "tmdnet_md_thermostat_workspace_bytes" in declared
    src = open(_C.__file__).read()
    assert "tmdnet_md_thermostat.argtypes" in src and "tmdnet_md_thermostat_workspace_bytes.argtypes" in src


def test_library_exports_the_thermostat_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10
    assert len(hip_lib.tmdnet_md_thermostat.argtypes) == 25
    nb = C.c_size_t(0)
    assert hip_lib.tmdnet_md_thermostat_workspace_bytes(3, 3, C.byref(nb)) == 0 and nb.value >= 3 * 4 + 3 * 8 + 3 * 2 * 3 * 8
    assert hip_lib.tmdnet_md_thermostat_workspace_bytes(3, 0, C.byref(nb)) == 0
    assert hip_lib.tmdnet_md_thermostat_workspace_bytes(3, 9, C.byref(nb)) != 0
    assert hip_lib.tmdnet_md_thermostat_workspace_bytes(-1, 3, C.byref(nb)) != 0


def test_capture_md_keeps_its_signature():
    from torchmdnet_amd.models.model import TorchMD_Net

    p = inspect.signature(TorchMD_Net.capture_md).parameters
    assert list(p) == ["self", "z", "pos", "vel", "masses", "dt", "batch", "box", "q", "num_systems", "steps_per_replay", "force_scale",
                       "thermostat", "warmup", "atom_weights", "halo_exchange", "barostat"]
    assert (p["steps_per_replay"].default, p["force_scale"].default, p["warmup"].default, p["thermostat"].default) == (10, 1.0, 3, None)


# ---- 8. sanitizers ----------------------------------------------------------------------------------------------------------------
def test_standalone_program_under_the_host_sanitizers(tmp_path):
    """tests/md_thermo_host.hip with its own main (alpha for every size and chain of case 1, the exact cases, the failure protocol),
    built with -fsanitize=address,undefined and run as a program of its own"""
    exe = M.build_program(str(tmp_path / "md_thermo_host_san"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "wrong 0, forced fail 1" in out.stdout
