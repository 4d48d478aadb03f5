"""-m gpu: the global thermostats of the device-resident MD loop (csrc/tn_md_thermo.hip: k_md_thermo_factor, k_md_thermo_scale;
TorchMD_Net.capture_md_global).

1. the C entry on a plain force buffer, against the host mirror of the same header and a torch mirror of the scaling
2. through the model: bit-identical to capture() + a torch mirror that takes every step's alpha from the device, which the fp64
   oracle confirms; the same bits whatever K and from run to run
3. the canonical ensemble of tests/test_md_thermo_host.py on the device
4. with constraints   5. status 5   6. overflow   7. reset(step=)"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import md_thermo_host_mirror as M
from tests import md_thermo_oracle as T
from tests.test_gpu_md_constraints import _res_v, _res_x
from tests.test_gpu_md_loop import CLOSE, FS, OPEN, _bits, _model, _Raw, _setup, _system
from torchmdnet_amd import md as MD

pytestmark = pytest.mark.gpu

KINDS = {"csvr": dict(kind="csvr", code=M.CSVR, chain=0, substeps=1), "nose-hoover": dict(kind="nose-hoover", code=M.NHC, chain=3, substeps=2)}


def _np(t):
    return t.detach().cpu().numpy()


def _up(n):
    return (n + 255) & ~255


# ------------------------------------------------------------------------------------------------ 1. the C entry
class _RawT(_Raw):
    """tmdnet_md_thermostat on tensors of the test's own, graph_ws = NULL (no model: the forces are whatever the buffer holds)"""

    def __init__(self, lib, pos, vel, mass, batch, n_mol, dt, ndof, th, force_scale=1.0):
        super().__init__(lib, pos, vel, mass, batch, n_mol, dt, force_scale=force_scale)
        self.th, self.fs = th, force_scale
        self.ndof = torch.as_tensor(ndof, dtype=torch.int32).cuda()
        nb = C.c_size_t(0)
        assert lib.tmdnet_md_thermostat_workspace_bytes(n_mol, th["chain"], C.byref(nb)) == 0
        self.tws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        off = (-self.tws.data_ptr()) % 256
        r0 = off + _up(4 * n_mol)
        c0 = r0 + _up(8 * n_mol)
        self.alpha = self.tws[off:off + 4 * n_mol].view(torch.float32)
        self.reservoir = self.tws[r0:r0 + 8 * n_mol].view(torch.float64)
        self.chain = self.tws[c0:c0 + 16 * n_mol * th["chain"]].view(torch.float64).view(n_mol, 2, th["chain"])

    def thermostat(self, open_next, forces, rows=(None, None), expect=0, **over):
        p = self._p
        a = dict(self.th, ekin=self.ekin, ndof=self.ndof, tws=self.tws)
        a.update(over)
        rc = self.L.tmdnet_md_thermostat(None, self._s(), None, p(self.ws), p(a["tws"]), self.n, self.n_mol, a["code"], int(open_next),
                                         p(self.pos), p(self.vel), p(forces), p(self.hk), self.dt, p(self.batch), p(a["ekin"]), p(a["ndof"]),
                                         a["kT"], a["tau"], a["chain"], a["substeps"], self.fs, a["seed"], p(rows[0]), p(rows[1]))
        assert rc == expect, rc


def _five_molecules():
    """1, 2, 3, 8 and 63 atoms; the molecule of 3 is frozen entirely (infinite masses), one atom of the molecule of 8 has infinite
    mass and a velocity of its own"""
    g = torch.Generator().manual_seed(33)
    sizes = [1, 2, 3, 8, 63]
    n = sum(sizes)
    batch = torch.repeat_interleave(torch.arange(5), torch.tensor(sizes))
    pos = 2.0 * torch.randn(n, 3, generator=g)
    vel = 0.05 * torch.randn(n, 3, generator=g)
    mass = 1.0 + 15.0 * torch.rand(n, generator=g)
    mass[3:6] = float("inf")
    mass[8] = float("inf")
    ndof = [3, 6, 0, 21, 189]
    return [t.cuda() for t in (pos, vel, mass, batch)], ndof


@pytest.mark.parametrize("kind", list(KINDS))
def test_c_entry_against_the_host_mirror_and_a_torch_mirror_of_the_scaling(hip_lib, kind):
    (pos, vel, mass, batch), ndof = _five_molecules()
    dt, kT, B = 0.5, 0.025, 5
    th = dict(KINDS[kind], kT=kT, tau=10.0 * dt, seed=2 ** 40 + 17)
    fused = _RawT(hip_lib, pos, vel, mass, batch, B, dt, ndof, th, force_scale=FS)
    split = _RawT(hip_lib, pos, vel, mass, batch, B, dt, ndof, th, force_scale=FS)
    hk, dt_t = fused.hk[:, None], torch.tensor(dt, device="cuda")
    free = (fused.hk != 0)[:, None]
    kappa = 30.0  # f = -kappa (x - x0): bounded motion on a force buffer of the test's own
    force = lambda md: torch.mul(md.pos - pos, -kappa)
    bound = T.BOUNDS[kind]
    wa = wr = wc = 0.0
    chain_m, res_m = np.zeros((B, 2, th["chain"])), np.zeros(B)
    f = force(fused)
    fused.advance(OPEN, f)
    split.advance(OPEN, f)
    for s in range(64):
        f = force(fused)
        rows = (torch.full((B,), float("nan"), device="cuda"), torch.full((B,), float("nan"), dtype=torch.float64, device="cuda"))
        fused.advance(CLOSE, f)
        split.advance(CLOSE, f)
        x_c, v_c, res_before = fused.pos.clone(), fused.vel.clone(), _np(fused.reservoir).copy()
        fused.thermostat(1, f, rows)
        split.thermostat(0, None)
        split.advance(OPEN, f)
        alpha = fused.alpha.clone()
        assert _bits(rows[0], alpha) and torch.equal(rows[1], fused.reservoir)
        # the host mirror of the same header, fed the device's kinetic energies
        if kind == "csvr":  # per move, as the host measured it: from the device's reservoir of the step before
            bad, a_m, _, res_m, _ = M.moves(M.CSVR, _np(fused.ekin), ndof, kT, th["tau"], dt, th["seed"], s, reservoir=res_before,
                                            force_scale=FS)
            scale_r = np.maximum(0.5 * np.array(ndof) * kT, 1e-300)
        else:  # consecutive moves on the mirror's own state
            bad, a_m, chain_m, res_m, _ = M.moves(M.NHC, _np(fused.ekin), ndof, kT, th["tau"], dt, 0, s, th["chain"], th["substeps"],
                                                  chain_m, res_m, force_scale=FS)
            scale_r = np.maximum(np.abs(res_m), np.maximum(np.array(ndof) * kT, 1e-300))
            wc = max(wc, T.rel(_np(fused.chain)[:, 0], chain_m[:, 0], 1.0), T.rel(_np(fused.chain)[:, 1], chain_m[:, 1], 1.0 / th["tau"]))
        assert bad == 0
        wa = max(wa, float(np.max(np.abs(_np(alpha).astype(np.float64) - a_m) / a_m)))
        wr = max(wr, float(np.max(np.abs(_np(fused.reservoir) - res_m) / scale_r)))
        # given alpha: one rounded product per component (atoms of infinite mass are left out), then B, A of the next step
        v_s = torch.where(free, torch.mul(v_c, alpha[batch][:, None]), v_c)
        v_o = torch.add(v_s, torch.mul(hk, f))
        x_o = torch.add(x_c, torch.mul(dt_t, v_o))
        assert _bits(fused.vel, v_o) and _bits(fused.pos, x_o), s
        # the fused opening half is the unfused scaling followed by tmdnet_md_advance(OPEN)
        assert _bits(split.vel, fused.vel) and _bits(split.pos, fused.pos) and torch.equal(split.tws, fused.tws), s
        assert alpha[2].item() == 1.0 and (alpha[[0, 1, 3, 4]] != 1.0).any()
    print(kind, "device against the host mirror over 64 moves: alpha", wa, "(bound", bound["alpha"], ") reservoir", wr, "(bound",
          bound["reservoir"], ") chain", wc, "(bound", bound.get("chain"), ")")
    assert wa <= bound["alpha"] and wr <= bound["reservoir"] and wc <= bound.get("chain", 0.0)
    assert fused.status() == (0, 64, 0)
    # the frozen molecule kept its velocities; the infinite-mass atom kept its velocity while its molecule was scaled
    assert _bits(fused.vel[3:6], vel[3:6]) and _bits(fused.vel[8], vel[8]) and not _bits(fused.vel[9], vel[9])
    assert fused.reservoir[2].item() == 0.0 and (fused.chain[2] == 0).all()


def test_c_entry_refusals_and_the_failure_protocol(hip_lib):
    (pos, vel, mass, batch), ndof = _five_molecules()
    th = dict(KINDS["nose-hoover"], kT=0.025, tau=5.0, seed=1)
    md = _RawT(hip_lib, pos, vel, mass, batch, 5, 0.5, ndof, th)
    zero = torch.zeros_like(pos)
    md.advance(OPEN, zero)
    md.advance(CLOSE, zero)
    p1, v1 = md.pos.clone(), md.vel.clone()
    for over in (dict(code=2), dict(tau=0.0), dict(kT=0.0), dict(chain=0), dict(chain=9), dict(substeps=0), dict(ekin=None), dict(ndof=None),
                 dict(tws=None)):
        md.thermostat(0, zero, expect=1, **over)
    md.thermostat(1, None, expect=1)  # the opening half needs the forces
    assert _bits(md.vel, v1) and md.status() == (0, 1, 0) and (md.tws == 0).all()
    # a NaN kinetic energy in molecule 1: status 5, nothing written for any molecule, every later launch returns at once
    md.ekin[1] = float("nan")
    rows = (torch.full((5,), 7.0, device="cuda"), torch.full((5,), 7.0, dtype=torch.float64, device="cuda"))
    md.thermostat(1, zero, rows)
    assert md.status() == (5, 1, 5)  # TMDNET_ERR_STATE, one step completed, status 5
    assert _bits(md.vel, v1) and _bits(md.pos, p1) and (md.tws == 0).all() and (rows[0] == 7.0).all() and (rows[1] == 7.0).all()
    md.ekin[1] = 0.1
    md.thermostat(0, zero, rows)
    md.advance(OPEN, zero)
    assert _bits(md.vel, v1) and _bits(md.pos, p1) and (md.tws == 0).all() and md.status() == (5, 1, 5)
    md.reset(0)
    md.thermostat(0, zero, rows)
    assert md.status() == (0, 0, 0) and not _bits(md.vel, v1) and (rows[0] != 7.0).all()


# ------------------------------------------------------------------------------------------------ 2. through the model
def _thermostat_for(kind, vel, mass, ndof, dt, seed=2 ** 40 + 9, factor=2.0):
    """kT a factor above the system's own temperature, so that the thermostat visibly heats; tau = 10 dt"""
    ke = 0.5 * float((mass.double()[:, None] * vel.double() ** 2).sum())
    th = dict(kind=kind, kT=factor * 2.0 * ke / float(sum(ndof)), tau=10.0 * dt)
    if kind == "csvr":
        th["seed"] = seed
    return th


def _run(model, inputs, vel, mass, dt, K, replays, th, **kw):
    z, pos, batch, box, q = inputs
    md = model.capture_md_global(z, pos, vel, mass, dt, batch=batch, box=box, q=q, steps_per_replay=K, thermostat=th, **kw)
    names = ("epot", "ekin", "scale", "reservoir")
    logs = {k: [] for k in names}
    for _ in range(replays):
        md()
        for k in names:
            logs[k].append(getattr(md, k).clone())
    assert md.check() == K * replays == md.steps_done
    return md, {k: torch.cat(v) for k, v in logs.items()}


def _confirm_alpha(logs, ndof, th, dt, steps, force_scale=1.0, step0=0):
    """every alpha of the device against the fp64 oracle fed the device's kinetic energies -> largest relative difference"""
    ekin, scale = _np(logs["ekin"]), _np(logs["scale"]).astype(np.float64)
    worst = 0.0
    chains = [T.Chain(n, th["kT"], th["tau"], th.get("chain", 3)) for n in ndof]
    for s in range(steps):
        for m, n in enumerate(ndof):
            if th["kind"] == "csvr":
                a = math.sqrt(T.csvr(ekin[s, m], n, th["kT"], th["tau"], dt, th.get("seed", 0), step0 + s, m, force_scale)[0])
            else:
                chains[m].move(ekin[s, m], dt, th.get("substeps", 2), force_scale)
                a = chains[m].s
            worst = max(worst, abs(scale[s, m] - a) / a)
    return worst


def _mirror(replay, pos0, vel0, mass, batch, dt, scale):
    """capture() + the scheme in torch, every product and every sum its own rounded kernel; alpha of every step is the device's.
    -> pos, vel, forces, epot [steps,B], and the kinetic energy before every move in fp64 [steps,B]"""
    hk = (0.5 * dt / mass.double()).float()[:, None]
    dt_t = torch.tensor(dt, dtype=torch.float32, device="cuda")
    pos, vel = pos0.clone(), vel0.clone()
    f = replay(pos)[1].clone()
    epot, ke = [], []
    for s in range(scale.shape[0]):
        vel = torch.add(vel, torch.mul(hk, f))
        pos = torch.add(pos, torch.mul(dt_t, vel))
        e, f = (t.clone() for t in replay(pos))
        vel = torch.add(vel, torch.mul(hk, f))
        epot.append(e.view(-1))
        ke.append(torch.zeros(scale.shape[1], dtype=torch.float64, device="cuda").index_add_(0, batch, 0.5 * mass.double() * (vel.double() ** 2).sum(1)))
        vel = torch.mul(vel, scale[s][batch][:, None])
    return pos, vel, f, torch.stack(epot), torch.stack(ke)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("arch", ["tensornet", "equivariant-transformer", "tensornet2"])
def test_global_md_is_bit_identical_to_capture_plus_torch_mirror(hip_lib, arch, kind):
    """16 steps of the ragged three-molecule batch.  Positions, velocities, forces and epot: the mirror's bits.  ekin is summed in the
    reduction kernel's own order, which no torch sum reproduces: it agrees with the mirror's fp64 sum to (n + 5) 2^-24 (five rounded
    operations per term, at most n = 20 positive terms per molecule) and is bit-identical from K to K and from run to run."""
    model, replay, inputs, vel, mass, dt = _setup(arch, "ragged")
    z, pos, batch, box, q = inputs
    ndof = [21, 36, 60]
    th = _thermostat_for(kind, vel, mass, ndof, dt)
    md, logs = _run(model, inputs, vel, mass, dt, 8, 2, th)
    assert md.ndof.tolist() == ndof == md.thermostat_ndof.tolist()
    p_ref, v_ref, f_ref, e_ref, ke_ref = _mirror(replay, pos, vel, mass, batch, dt, logs["scale"])
    assert _bits(md.pos, p_ref) and _bits(md.vel, v_ref) and _bits(md.forces, f_ref) and _bits(logs["epot"], e_ref)
    assert ((logs["ekin"].double() - ke_ref).abs() / ke_ref).max().item() <= 25 * 2.0 ** -24
    worst = _confirm_alpha(logs, ndof, th, dt, 16)
    print(arch, kind, "largest relative difference of a device alpha from the oracle:", worst, "scale", logs["scale"][:, 0].tolist())
    assert worst <= T.BOUNDS[kind]["alpha"]
    assert (logs["scale"] != 1.0).all()
    if kind == "nose-hoover":  # kT is twice the start's: the first move of a chain at rest heats (CSVR does so on average only)
        assert (logs["scale"][0] > 1.0).all()
    # the public bookkeeping
    assert torch.equal(md.kinetic_after(), md.scale.double() ** 2 * md.ekin.double())
    assert torch.equal(md.conserved(), md.epot.double() + md.kinetic_after() / md.force_scale + md.reservoir)
    assert torch.equal(md.reservoir[-1], md._reservoir_now) and md.chain.shape == (3, 2, 3 if kind == "nose-hoover" else 0)
    # the same bits whatever the number of steps per launch, and from run to run
    for K, replays in ((1, 16), (16, 1), (8, 2)):
        md2, logs2 = _run(model, inputs, vel, mass, dt, K, replays, th)
        assert _bits(md2.pos, md.pos) and _bits(md2.vel, md.vel) and _bits(md2.forces, md.forces), (K, replays)
        for k in ("epot", "ekin", "scale"):
            assert _bits(logs2[k], logs[k]), (K, replays, k)
        assert torch.equal(logs2["reservoir"], logs["reservoir"]) and torch.equal(md2.chain, md.chain), (K, replays)
    if kind == "csvr":
        other, lo = _run(model, inputs, vel, mass, dt, 8, 2, dict(th, seed=5))
        assert not _bits(lo["scale"], logs["scale"]) and not _bits(other.vel, md.vel)
        assert len(set(logs["scale"][0].tolist())) == 3  # every molecule its own noise


def test_ndof_of_the_caller_and_molecules_that_are_never_scaled(hip_lib):
    model, replay, inputs, vel, mass, dt = _setup("tensornet", "ragged")
    z, pos, batch, box, q = inputs
    th = dict(_thermostat_for("csvr", vel, mass, [21, 36, 60], dt), ndof=torch.tensor([18, 0, 57]))
    v0 = vel.clone()
    v0[batch == 2] = 0.0  # molecule 2 starts at rest, but gains kinetic energy from the forces: scaled from the first step on
    md, logs = _run(model, inputs, v0, mass, dt, 4, 1, th)
    assert md.thermostat_ndof.tolist() == [18, 0, 57] and md.ndof.tolist() == [21, 36, 60]
    assert (logs["scale"][:, 1] == 1.0).all() and (logs["reservoir"][:, 1] == 0.0).all() and (logs["scale"][:, [0, 2]] != 1.0).all()
    assert _confirm_alpha(logs, [18, 0, 57], th, dt, 4) <= T.BOUNDS["csvr"]["alpha"]
    with pytest.raises(ValueError, match="one per molecule"):
        model.capture_md_global(z, pos, vel, mass, dt, batch=batch, q=q, thermostat=dict(th, ndof=[1, 2]))
    with pytest.raises(ValueError, match="chain"):
        model.capture_md_global(z, pos, vel, mass, dt, batch=batch, q=q, thermostat=dict(kind="nose-hoover", kT=1.0, tau=1.0, chain=9))


# ------------------------------------------------------------------------------------------------ 3. the ensemble
@pytest.mark.parametrize("ndof", [9, 2])
def test_csvr_samples_the_canonical_kinetic_energy_on_the_device(hip_lib, ndof):
    """The case, the seed and the bound of tests/test_md_thermo_host.py::test_csvr_samples_the_canonical_kinetic_energy"""
    e = T.ENSEMBLE
    n = 3 if ndof == 9 else 2
    B, N = e["B"], e["B"] * n
    v = torch.zeros(N, 3)
    if ndof == 9:
        v[:] = math.sqrt(e["kT"])
    else:
        v[:, 0] = math.sqrt(e["kT"])
    batch = torch.repeat_interleave(torch.arange(B), n).cuda()
    zero = torch.zeros(N, 3, device="cuda")
    th = dict(KINDS["csvr"], kT=e["kT"], tau=e["tau"], seed=e["seed"])
    md = _RawT(hip_lib, zero, v.cuda(), torch.ones(N).cuda(), batch, B, e["dt"], [ndof] * B, th)
    scale = torch.full((e["steps"], B), float("nan"), device="cuda")
    ekin = []
    md.advance(OPEN, zero)
    for s in range(e["steps"]):
        md.advance(CLOSE, zero)
        ekin.append(md.ekin.clone())
        md.thermostat(1, zero, (scale[s], None))
    assert md.status() == (0, e["steps"], 0)
    assert abs(ekin[0][0].item() / (0.5 * ndof * e["kT"]) - 1.0) < 1e-6  # the start is K = Kbar
    sample = _np(scale[-1]).astype(np.float64) ** 2 * _np(ekin[-1]).astype(np.float64)
    d = T.ks_distance(sample, ndof)
    print("N =", ndof, "KS distance on the device:", d, "mean K / Kbar", sample.mean() / (0.5 * ndof * e["kT"]))
    assert d < e["bound"]


# ------------------------------------------------------------------------------------------------ 4. with constraints
@pytest.mark.parametrize("kind", list(KINDS))
def test_rigid_water_under_a_global_thermostat(hip_lib, kind):
    """The box, dt and force scale of tests/test_gpu_md_constraints.py::test_rigid_water_stays_rigid_over_64_steps_at_2_fs, 32 steps:
    the residual bounds of DESIGN.md section 13 after every replay, ndof net of the constraints, alpha confirmed by the oracle."""
    model = _model("tensornet", max_num_neighbors=128)
    z, pos, batch, box = (t.cuda() for t in _system("water192"))
    q = torch.zeros(1, device="cuda")
    mass = torch.where(z == 1, 1.008, 12.0).float()
    vel = 0.005 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    pairs = MD.hydrogen_pairs(z, pos, rigid_water=True)
    _, f0 = model.capture(z, pos, batch, box, q=q)(pos)
    fs = FS * 0.2 / float(f0.abs().max())
    th = _thermostat_for(kind, vel, mass, [384], 2.0)
    th["kT"] /= fs  # the unit of E
    logs = {k: [] for k in ("ekin", "scale")}
    md = model.capture_md_global(z, pos, vel, mass, 2.0, batch=batch, box=box, q=q, steps_per_replay=8, force_scale=fs, thermostat=th,
                                 constraints=dict(pairs=pairs))
    assert md.ndof.tolist() == [3 * 192 - 192] == md.thermostat_ndof.tolist()
    for _ in range(4):
        md()
        assert _res_x(md.pos, md.constraints) <= 1 and _res_v(md.pos, md.vel, md.constraints, 2.0) <= 1
        for k in logs:
            logs[k].append(getattr(md, k).clone())
    assert md.check() == 32 and (md.pos - pos).abs().max().item() > 0.05
    logs = {k: torch.cat(v) for k, v in logs.items()}
    worst = _confirm_alpha(logs, [384], th, 2.0, 32, force_scale=fs)
    print(kind, "rigid water: largest relative difference of alpha from the oracle", worst, "scale", logs["scale"][:, 0].tolist())
    assert worst <= T.BOUNDS[kind]["alpha"] and (logs["scale"] != 1.0).all()
    # the constrained loop without the thermostat goes elsewhere
    nve = model.capture_md_constrained(z, pos, vel, mass, 2.0, batch=batch, box=box, q=q, steps_per_replay=8, force_scale=fs,
                                       constraints=dict(pairs=pairs))
    nve(4)
    assert nve.check() == 32 and not _bits(nve.vel, md.vel)


# ------------------------------------------------------------------------------------------------ 5. status 5
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_nan_velocity_is_reported_as_the_thermostat(hip_lib, kind):
    model, replay, inputs, vel, mass, dt = _setup("tensornet", "ragged")
    z, pos, batch, box, q = inputs
    th = _thermostat_for(kind, vel, mass, [21, 36, 60], dt)
    md = model.capture_md_global(z, pos, vel, mass, dt, batch=batch, q=q, steps_per_replay=2, thermostat=th)
    md()
    assert md.check() == 2
    ref = [t.clone() for t in (md.pos, md.vel)]
    md.vel[9, 0] = float("nan")  # an atom of molecule 1: its kinetic energy is NaN after the next closing half
    md()
    with pytest.raises(RuntimeError, match="thermostat: the " + kind):
        md.check()
    host = (C.c_uint64 * 2)()
    assert hip_lib.tmdnet_md_status(None, C.c_void_p(md._ws.data_ptr()), host) == 5 and (int(host[0]), int(host[1])) == (3, 5)
    state = (md.pos, md.vel, md.forces, md.epot, md.ekin, md.scale, md.reservoir, md._thermo_ws)
    keep = [t.clone() for t in state]
    assert torch.isnan(md.ekin[0, 1]) and torch.isfinite(md.pos[batch != 1]).all()
    md(2)  # frozen at the closed step 3, bit for bit
    with pytest.raises(RuntimeError, match="thermostat"):
        md.check()
    for t, k in zip(state, keep):
        assert torch.equal(t.view(torch.uint8), k.view(torch.uint8))
    md.reset(pos=pos, vel=vel)
    md()
    assert md.check() == 2 and _bits(md.pos, ref[0]) and _bits(md.vel, ref[1])


# ------------------------------------------------------------------------------------------------ 6. overflow
def test_overflow_freezes_the_state_and_applies_no_scaling(hip_lib):
    """The case of tests/test_gpu_md_loop.py::test_overflow_freezes_the_state_at_the_last_valid_step under a global thermostat"""
    model = _model("tensornet", max_num_neighbors=72)
    z, pos, batch, box = (t.cuda() for t in _system("water192"))
    box = box.clone()
    box0 = box.clone()
    q = torch.zeros(1, device="cuda")
    vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    mass = torch.where(z == 1, 1.008, 12.0).float()
    th = _thermostat_for("csvr", vel, mass, [576], 0.01)
    md = model.capture_md_global(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, steps_per_replay=4, thermostat=th)
    md()
    assert md.check() == 4 and (md.scale != 1.0).all()
    box.mul_(0.85)
    md.pos.mul_(0.85)
    state = (md.pos, md.vel, md.forces, md.epot, md.ekin, md.scale, md.reservoir, md._thermo_ws)
    keep = [t.clone() for t in state]
    host = (C.c_uint64 * 2)()
    for _ in range(2):  # the overflowing replay and one more
        md()
        with pytest.raises(RuntimeError, match="max_num_pairs"):
            md.check()
        assert hip_lib.tmdnet_md_status(None, C.c_void_p(md._ws.data_ptr()), host) == 3 and (int(host[0]), int(host[1])) == (4, 1)
        for t, k in zip(state, keep):
            assert torch.equal(t.view(torch.uint8), k.view(torch.uint8))
    box.copy_(box0)
    md.reset(pos=pos, vel=vel)
    md()
    assert md.check() == 4 and not _bits(md.pos, keep[0])


# ------------------------------------------------------------------------------------------------ 7. reset(step=)
def test_reset_to_a_step_reproduces_the_trajectory_and_empties_the_thermostat(hip_lib):
    model, replay, inputs, vel, mass, dt = _setup("tensornet", "ragged")
    z, pos, batch, box, q = inputs
    th = _thermostat_for("csvr", vel, mass, [21, 36, 60], dt)
    md = model.capture_md_global(z, pos, vel, mass, dt, batch=batch, q=q, steps_per_replay=4, thermostat=th)
    md(2)
    p8, v8 = md.pos.clone(), md.vel.clone()
    md()
    p12, v12, s12, r12, k12 = (t.clone() for t in (md.pos, md.vel, md.scale, md.reservoir, md.ekin))
    assert md.check() == 12
    md.reset(pos=p8, vel=v8, step=8)  # the noise is a function of (seed, step, molecule): steps 9..12 again
    assert (md._thermo_ws == 0).all() and md.steps_done == 8
    md()
    assert md.check() == 12 and _bits(md.pos, p12) and _bits(md.vel, v12) and _bits(md.scale, s12) and _bits(md.ekin, k12)
    # the reservoir counts from the reset: its first entry is -(alpha^2 - 1) K of step 9 alone, and the differences are the run's
    # (alpha^2 in fp64 there, the rounded alpha here: 2 * 2^-24 alpha^2 K apart at the most)
    a2K = _np(s12[0]).astype(np.float64) ** 2 * _np(k12[0]).astype(np.float64)
    assert (np.abs(_np(md.reservoir[0]) + (a2K - _np(k12[0]).astype(np.float64))) <= 2.0 ** -22 * a2K).all()
    assert np.abs(_np(md.reservoir[-1] - md.reservoir[0]) - _np(r12[-1] - r12[0])).max() <= 1e-12 * np.abs(_np(r12)).max() + 1e-18
    md.reset(pos=p8, vel=v8, step=0)  # another step: another trajectory
    md()
    assert not _bits(md.scale, s12)
    # a chain is part of the state: a reset puts it to rest, so the run from the start comes again
    nh = _thermostat_for("nose-hoover", vel, mass, [21, 36, 60], dt)
    md = model.capture_md_global(z, pos, vel, mass, dt, batch=batch, q=q, steps_per_replay=4, thermostat=nh)
    md(2)
    p, v, c = md.pos.clone(), md.vel.clone(), md.chain.clone()
    assert (c != 0).any()
    md.reset(pos=pos, vel=vel)
    assert (md.chain == 0).all() and (md._reservoir_now == 0).all()
    md(2)
    assert _bits(md.pos, p) and _bits(md.vel, v) and torch.equal(md.chain, c)
