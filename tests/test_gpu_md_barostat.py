"""-m gpu: the barostat of the device-resident MD loop (csrc/tn_md.hip: k_md_baro, k_md_scale; TorchMD_Net.capture_md(barostat=)).

1. the raw entries, no model: tmdnet_md_advance(CLOSE) then tmdnet_md_barostat on synthetic forces and virials
2. the NPT ensemble of an ideal gas through the raw entries (the bounds of tests/test_md_barostat_host.py)
3. through the model: K steps per graph launch are bit-identical to capture(virial=True) + a torch mirror that evaluates the scheme
   one rounded operation at a time and takes every step's factors from the device, which the fp64 oracle confirms within 1 ulp
4. direction, overflow under NPT, refusals"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import md_baro_oracle as OB
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

OPEN, MIDDLE, CLOSE = 0, 1, 2
FS = 9.648533e-3


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _np(t):
    return t.detach().cpu().numpy()


def _factors(ws, n_mol):
    """(mu32, nu32) [n_mol] each of the last move, from the barostat's scratch (tmdnet_md_barostat_workspace_bytes: 256-aligned)"""
    off = (-ws.data_ptr()) % 256
    f = ws[off:off + 8 * n_mol].view(torch.float32)
    return f[:n_mol].clone(), f[n_mol:].clone()


# ------------------------------------------------------------------------------------------------ 1. the raw entries
class _Raw:
    """The C entries on tensors of the test's own, graph_ws = NULL (no model: forces and virial are whatever the buffers hold)."""

    def __init__(self, lib, pos, vel, mass, batch, n_mol, dt, box, force_scale=1.0, sigma=None, c1=1.0, c2=0.0, seed=0):
        self.L, self.n, self.n_mol, self.dt, self.fs = lib, pos.shape[0], n_mol, dt, force_scale
        self.pos, self.vel, self.box = pos.clone().contiguous(), vel.clone().contiguous(), box.clone().contiguous()
        self.mass = mass.float().contiguous()
        self.hk = (0.5 * dt * force_scale / mass.double()).float().contiguous()
        self.sigma, self.c1, self.c2, self.seed, self.batch = sigma, c1, c2, seed, batch
        nb = C.c_size_t(0)
        assert lib.tmdnet_md_workspace_bytes(self.n, n_mol, C.byref(nb)) == 0
        self.ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        assert lib.tmdnet_md_barostat_workspace_bytes(n_mol, C.byref(nb)) == 0
        self.baro_ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        self.ekin = torch.full((n_mol,), float("nan"), device="cuda")
        self.reset(0)

    @staticmethod
    def _s():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def reset(self, step):
        assert self.L.tmdnet_md_reset(self._s(), self._p(self.ws), step) == 0

    def advance(self, phase, forces):
        p = self._p
        rc = self.L.tmdnet_md_advance(None, self._s(), None, p(self.ws), self.n, self.n_mol, phase, p(self.pos), p(self.vel), p(forces),
                                      None, p(self.hk), p(self.mass), p(self.sigma), self.dt, self.c1, self.c2, self.seed, p(self.batch),
                                      None, None, p(self.ekin))
        assert rc == 0, rc

    def barostat(self, open_next, forces, virial, baro, rows=(None, None, None), box_mode=2, expect=0, **over):
        p = self._p
        a = dict(box=self.box, virial=virial, ekin=self.ekin, **baro)
        a.update(over)
        rc = self.L.tmdnet_md_barostat(None, self._s(), None, p(self.ws), p(self.baro_ws), self.n, self.n_mol, int(open_next), p(self.pos),
                                       p(self.vel), p(forces), p(self.hk), self.dt, p(self.batch), p(a["box"]), box_mode, p(a["virial"]),
                                       p(a["ekin"]), a["pressure"], a["kT"], a["compressibility"], a["tau"], self.fs, a["seed"],
                                       p(rows[0]), p(rows[1]), p(rows[2]))
        assert rc == expect, rc

    def status(self):
        host = (C.c_uint64 * 2)()
        rc = self.L.tmdnet_md_status(self._s(), self._p(self.ws), host)
        return rc, int(host[0]), int(host[1])


def _triclinic(n, g, side=30.0):
    return (torch.diag_embed(side + 4.0 * torch.rand(n, 3, generator=g)) + 2.0 * (torch.rand(n, 3, 3, generator=g) - 0.5)).float()


def _ragged_1000(n_mol=3):
    g = torch.Generator().manual_seed(21)
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor([300, 333, 367]))
    pos = 10 * torch.randn(1000, 3, generator=g)
    vel = 0.05 * torch.randn(1000, 3, generator=g)
    f1 = 3 * torch.randn(1000, 3, generator=g)
    mass = 1.0 + 39.0 * torch.rand(1000, generator=g)
    box = _triclinic(n_mol, g)
    vir = 300.0 * torch.randn(n_mol, 3, 3, generator=g)
    return [t.cuda() for t in (pos, vel, f1, mass, batch, box, vir)]


# K = ekin / FS is a few thousand, V about 3e4: P about 0.05; a = 0.5 moves the volume by some 1e-3 per step, the noise by 1e-3
RAW_BARO = dict(pressure=0.05, kT=0.025, compressibility=10.0, tau=10.0, seed=2 ** 40 + 11)


@pytest.mark.parametrize("open_next", [0, 1])
def test_raw_move_equals_oracle_and_torch_mirror(hip_lib, open_next):
    pos, vel, f1, mass, batch, box, vir = _ragged_1000()
    dt = 0.5
    md = _Raw(hip_lib, pos, vel, mass, batch, 3, dt, box, force_scale=FS)
    rows = [torch.full((3,), float("nan"), device="cuda") for _ in range(3)]
    md.advance(CLOSE, f1)
    md.barostat(open_next, f1, vir, RAW_BARO, rows)
    assert md.status() == (0, 1, 0)
    hk, dt_t = md.hk[:, None], torch.tensor(dt, device="cuda")
    v1 = torch.add(vel, torch.mul(hk, f1))
    mu, nu = _factors(md.baro_ws, 3)
    assert _bits(rows[2], mu)
    a = RAW_BARO["compressibility"] * dt / RAW_BARO["tau"]
    Vo, Po, muo, nuo = OB.moves(_np(box), _np(vir), _np(md.ekin), FS, RAW_BARO["pressure"], RAW_BARO["kT"], a, RAW_BARO["seed"], 0)
    print("mu", _np(mu), "oracle", muo, "P", _np(rows[1]), "V", _np(rows[0]))
    assert OB.ulp_distance(_np(mu), muo).max() <= 1 and OB.ulp_distance(_np(nu), nuo).max() <= 1
    assert np.abs(_np(mu) - 1).min() > 1e-5  # every molecule really moved
    assert OB.ulp_distance(_np(rows[0]), Vo.astype(np.float32)).max() <= 1 and OB.ulp_distance(_np(rows[1]), Po.astype(np.float32)).max() <= 1
    # given the factors: one rounded product per entry
    x_s, v_s = torch.mul(pos, mu[batch][:, None]), torch.mul(v1, nu[batch][:, None])
    assert _bits(md.box, torch.mul(box, mu[:, None, None]))
    if open_next:  # then B, A of the next step on the scaled state, with the same force
        v_s = torch.add(v_s, torch.mul(hk, f1))
        x_s = torch.add(x_s, torch.mul(dt_t, v_s))
    assert _bits(md.pos, x_s) and _bits(md.vel, v_s)


def test_raw_empty_molecule_and_one_shared_box(hip_lib):
    pos, vel, f1, mass, batch, box, vir = _ragged_1000(n_mol=4)  # molecule 3 has a box and a virial but no atoms
    md = _Raw(hip_lib, pos, vel, mass, batch, 4, 0.5, box, force_scale=FS)
    rows = [torch.full((4,), float("nan"), device="cuda") for _ in range(3)]
    md.advance(CLOSE, f1)
    md.barostat(1, f1, vir, RAW_BARO, rows)
    assert md.status() == (0, 1, 0) and md.ekin[3].item() == 0
    for t in (md.pos, md.vel, md.box, *rows):
        assert torch.isfinite(t).all()
    assert not _bits(md.box[3], box[3])
    # box_mode 1: one [3,3] box, one molecule, no batch vector
    one = _Raw(hip_lib, pos, vel, mass, None, 1, 0.5, box[0], force_scale=FS)
    one.advance(CLOSE, f1)
    one.barostat(0, None, vir[:1], RAW_BARO, box_mode=1)
    mu, nu = _factors(one.baro_ws, 1)
    v1 = torch.add(vel, torch.mul(one.hk[:, None], f1))
    assert _bits(one.box, torch.mul(box[0], mu)) and _bits(one.pos, torch.mul(pos, mu)) and _bits(one.vel, torch.mul(v1, nu))


def test_raw_nan_in_the_virial_latches_status_2(hip_lib):
    pos, vel, f1, mass, batch, box, vir = _ragged_1000()
    md = _Raw(hip_lib, pos, vel, mass, batch, 3, 0.5, box, force_scale=FS)
    rows = [torch.full((3,), 7.0, device="cuda") for _ in range(3)]
    md.advance(CLOSE, f1)
    v1 = md.vel.clone()
    bad = vir.clone()
    bad[1, 2, 2] = float("nan")
    md.barostat(1, f1, bad, RAW_BARO, rows)
    assert md.status() == (5, 1, 2)  # TMDNET_ERR_STATE, one step completed, status 2
    assert _bits(md.box, box) and _bits(md.pos, pos) and _bits(md.vel, v1)
    assert all((r == 7.0).all() for r in rows)
    md.barostat(0, f1, vir, RAW_BARO, rows)  # frozen until a reset
    md.advance(OPEN, f1)
    assert _bits(md.box, box) and _bits(md.pos, pos) and _bits(md.vel, v1) and md.status() == (5, 1, 2)
    flat = box.clone()
    flat[2, 1] = flat[2, 0]  # a box without volume
    md2 = _Raw(hip_lib, pos, vel, mass, batch, 3, 0.5, flat, force_scale=FS)
    md2.advance(CLOSE, f1)
    md2.barostat(0, f1, vir, RAW_BARO)
    assert md2.status() == (5, 1, 2) and _bits(md2.box, flat) and _bits(md2.pos, pos)


def test_raw_refusals(hip_lib):
    pos, vel, f1, mass, batch, box, vir = _ragged_1000()
    md = _Raw(hip_lib, pos, vel, mass, batch, 3, 0.5, box, force_scale=FS)
    md.advance(CLOSE, f1)
    v1 = md.vel.clone()
    md.barostat(0, f1, vir, RAW_BARO, box_mode=0, expect=1)
    md.barostat(0, f1, vir, RAW_BARO, box_mode=1, expect=1)  # one shared box for three molecules
    md.barostat(0, f1, vir, RAW_BARO, expect=1, tau=0.0)
    md.barostat(0, f1, vir, RAW_BARO, expect=1, compressibility=0.0)
    md.barostat(0, f1, vir, RAW_BARO, expect=1, kT=-1.0)
    md.barostat(0, f1, None, RAW_BARO, expect=1)  # no virial
    md.barostat(0, f1, vir, RAW_BARO, expect=1, box=None)
    md.barostat(0, f1, vir, RAW_BARO, expect=1, ekin=None)
    assert _bits(md.box, box) and _bits(md.pos, pos) and _bits(md.vel, v1) and md.status() == (0, 1, 0)


# ------------------------------------------------------------------------------------------------ 2. the ensemble
def test_ideal_gas_samples_the_npt_ensemble_on_the_device(hip_lib):
    """The case and the two bounds of tests/test_md_barostat_host.py::test_ideal_gas_samples_the_npt_ensemble, per-replica boxes."""
    e = OB.ENSEMBLE
    box, x, v, hk, mass, sigma, c1, c2 = OB.ensemble_state()
    R, n, steps = e["R"], e["n"], e["steps"]
    t = lambda a: torch.from_numpy(a).cuda()
    batch = torch.repeat_interleave(torch.arange(R), n).cuda()
    md = _Raw(hip_lib, t(x), t(v), t(mass), batch, R, e["dt"], t(box), force_scale=1.0, sigma=t(sigma), c1=c1, c2=c2, seed=2024)
    assert _bits(md.hk, t(hk))
    zero, vir = torch.zeros(R * n, 3, device="cuda"), torch.zeros(R, 3, 3, device="cuda")
    baro = dict(pressure=e["P0"], kT=e["kT"], compressibility=1.0 / e["P0"], tau=e["tau"], seed=77)
    vol = torch.full((steps, R), float("nan"), device="cuda")
    md.advance(OPEN, zero)
    for s in range(steps):
        md.advance(CLOSE, zero)
        md.barostat(1, zero, vir, baro, (vol[s], None, None))
    assert md.status() == (0, steps, 0)
    vol = _np(vol)
    assert np.isfinite(vol).all()
    m, s = OB.ensemble_bounds(vol)
    print("device: mean / ((N+1) kT/P0) =", m, " relative sd * sqrt(N+1) =", s)
    assert abs(m - 1.0) < 0.01 and abs(s - 1.0) < 0.05


# ------------------------------------------------------------------------------------------------ 3. through the model
_models = {}


def _model(arch, **over):
    from torchmdnet_amd.models.model import create_model

    key = (arch, tuple(sorted(over.items())))
    if key not in _models:
        torch.manual_seed(4)
        if arch == "tensornet":
            args = dict(W.TINY_ARGS, static_shapes=True)
        elif arch == "equivariant-transformer":
            args = dict(W.ET_TINY_ARGS, static_shapes=True)
        else:
            args = dict(W.TINY_ARGS, static_shapes=True, model="tensornet2", output_model="ScalarPlusWeightedCoulomb", q_dim=4,
                        q_weights=[1.0, 1.0, 1.0])
        _models[key] = create_model(dict(args, **over)).to("cuda")
    return _models[key]


def _water(replicas=1):
    """192-atom periodic water box; replicas = 2: two copies with their own boxes [2,3,3], the second 2 % larger"""
    z, pos, box = W.water_box(n_side=4)
    if replicas == 1:
        return z.cuda(), pos.cuda(), torch.zeros_like(z).cuda(), box.cuda()
    n = z.shape[0]
    batch = torch.cat([torch.zeros(n, dtype=torch.long), torch.ones(n, dtype=torch.long)])
    return torch.cat([z, z]).cuda(), torch.cat([pos, 1.02 * pos]).cuda(), batch.cuda(), torch.stack([box, 1.02 * box]).cuda()


def _setup(arch, replicas=1, **over):
    model = _model(arch, **over)
    z, pos, batch, box = _water(replicas)
    n_mol = replicas
    q = torch.zeros(n_mol, device="cuda") if arch != "equivariant-transformer" else None
    vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()  # (other numbers for the second replica)
    mass = torch.where(z == 1, 1.008, 12.0).float()
    return model, (z, pos, batch, box, q), vel, mass


def _pressure(model, inputs, vel, mass):
    """-> P [B], V [B], dt: the system's own pressure at the start (force_scale 1) and the dt rule of tests/test_gpu_md.py"""
    z, pos, batch, box, q = inputs
    n_mol = int(batch.max()) + 1
    _, f, w = model.energy_forces_virial(z, pos, batch, box, q)
    ke = torch.zeros(n_mol, dtype=torch.float64, device="cuda").index_add_(0, batch, 0.5 * mass.double() * (vel.double() ** 2).sum(1))
    vol = torch.linalg.det(box.double()).abs().reshape(-1)
    P = (2.0 * ke + w.double().diagonal(dim1=1, dim2=2).sum(1)) / (3.0 * vol)
    dt = min(0.05, 0.02 * (12.0 / max(float(f.abs().max()), 1e-6)) ** 0.5)
    return P.cpu(), vol.cpu(), dt


def _baro_for(P, vol, dt, direction, drive=1e-3, amp=5e-4, far=1.0, kT=None, seed=99):
    """Barostat parameters from the system's own pressure, so that the volume visibly moves whatever the random weights give:
    P0 = P -+ far * max|P|: the first deterministic step is d = +-drive (direction +1: expand), and kT is set for a noise amplitude of
    `amp` per step (kT = 0: none).  tau = 10 dt."""
    scale = far * max(float(P.abs().max()), 1e-4)
    a = drive / scale
    if kT is None:
        kT = amp * amp * float(vol.mean()) / (2.0 * a)
    return dict(pressure=float(P.mean()) - direction * scale, tau=10.0 * dt, compressibility=10.0 * a, kT=kT, seed=seed)


def _run(model, inputs, vel, mass, dt, K, replays, baro, thermostat=None, collect_nu=False):
    """-> md, logs: epot, ekin, volume, pressure, scale [K * replays, B] (and nu with K = 1)"""
    z, pos, batch, box, q = inputs
    md = model.capture_md(z, pos, vel, mass, dt, batch=batch, box=box.clone(), q=q, steps_per_replay=K, thermostat=thermostat,
                          barostat=baro)
    names = ("epot", "ekin", "volume", "pressure", "scale")
    logs = {k: [] for k in names + ("nu",)}
    for _ in range(replays):
        md()
        for k in names:
            logs[k].append(getattr(md, k).clone())
        if collect_nu:
            assert K == 1
            logs["nu"].append(_factors(md._baro_ws, md.n_mol)[1][None])
    assert md.check() == K * replays == md.steps_done
    return md, {k: torch.cat(v) for k, v in logs.items() if v}


def _device_noise(hip_lib, n, seed, steps):
    """xi [steps, n, 3] of the loop's O step, the device's own bits: v = 0, F = 0, c1 = 0, c2 = sigma = 1 leaves v = xi"""
    zero, one = torch.zeros(n, 3, device="cuda"), torch.ones(n, device="cuda")
    out = []
    for s in range(steps):
        raw = _Raw(hip_lib, zero, zero, one, None, 1, 1.0, torch.eye(3, device="cuda"), sigma=one, c1=0.0, c2=1.0, seed=seed)
        raw.reset(s)
        raw.advance(CLOSE, zero)
        out.append(raw.vel.clone())
    return torch.stack(out)


def _mirror(model, inputs, vel0, mass, dt, steps, baro, logs, thermostat=None, xi=None):
    """capture(virial=True) + the scheme in torch, every product and every sum its own rounded kernel; the factors of every step are
    the device's (logs), checked against the fp64 oracle fed the mirror's own box and virial and the device's kinetic energy."""
    z, pos0, batch, box0, q = inputs
    box = box0.clone()
    replay = model.capture(z, pos0, batch, box, q=q, virial=True)
    hk = (0.5 * dt / mass.double()).float()[:, None]
    dt_t = torch.tensor(dt, dtype=torch.float32, device="cuda")
    if thermostat is not None:
        c1 = math.exp(-thermostat["friction"] * dt)
        c1_t, c2_t = (torch.tensor(c, dtype=torch.float32, device="cuda") for c in (c1, math.sqrt(1.0 - c1 * c1)))
        sigma = torch.sqrt(thermostat["kT"] / mass.double()).float()[:, None]
    a = baro["compressibility"] * float(np.float32(dt)) / baro["tau"]
    pos, vel = pos0.clone(), vel0.clone()
    f = replay(pos)[1].clone()
    epot, vols, worst = [], [], 0
    for s in range(steps):
        vel = torch.add(vel, torch.mul(hk, f))
        pos = torch.add(pos, torch.mul(dt_t, vel))
        e, f, w = (t.clone() for t in replay(pos))
        vel = torch.add(vel, torch.mul(hk, f))
        if thermostat is not None:
            vel = torch.add(torch.mul(c1_t, vel), torch.mul(torch.mul(c2_t, sigma), xi[s]))
        epot.append(e.view(-1))
        mu, nu = logs["scale"][s], logs["nu"][s]
        Vo, _, muo, nuo = OB.moves(_np(box).reshape(-1, 3, 3), _np(w), _np(logs["ekin"][s]), 1.0, baro["pressure"], baro["kT"], a,
                                   baro["seed"], s)
        worst = max(worst, int(OB.ulp_distance(_np(mu), muo).max()), int(OB.ulp_distance(_np(nu), nuo).max()))
        vols.append(torch.from_numpy(Vo.astype(np.float32)))
        torch.mul(box, mu.view(-1, 1, 1) if box.dim() == 3 else mu, out=box)
        pos = torch.mul(pos, mu[batch][:, None])
        vel = torch.mul(vel, nu[batch][:, None])
    print("mirror: largest distance of a device factor from the oracle:", worst, "ulp")
    assert worst <= 1
    return pos, vel, box, f, torch.stack(epot), torch.stack(vols).cuda()


CASES = {
    "tensornet": dict(arch="tensornet"),
    "equivariant-transformer": dict(arch="equivariant-transformer"),
    "tensornet-langevin": dict(arch="tensornet", thermostat=dict(friction=2.0, kT=0.01, seed=2 ** 40 + 5)),
    "tensornet-cell-list": dict(arch="tensornet", cell_list=True),
    "tensornet-two-replicas": dict(arch="tensornet", replicas=2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_npt_is_bit_identical_to_capture_plus_torch_mirror(hip_lib, case):
    c = CASES[case]
    model, inputs, vel, mass = _setup(c["arch"], c.get("replicas", 1))
    th = c.get("thermostat")
    keep = model.cell_list_min_atoms
    if c.get("cell_list"):
        model.cell_list_min_atoms = 1  # the cell list runs, on a box that changes every step
    try:
        P, vol, dt = _pressure(model, inputs, vel, mass)
        baro = _baro_for(P, vol, dt, +1)
        print(case, "P", P.tolist(), "V", vol.tolist(), "dt", dt, baro)
        md, logs = _run(model, inputs, vel, mass, dt, 1, 16, baro, th, collect_nu=True)
        if c.get("cell_list"):
            assert model.cell_grid(inputs[0].shape[0], 1)[3] == 1
        xi = _device_noise(hip_lib, inputs[0].shape[0], th["seed"], 16) if th else None
        p_ref, v_ref, b_ref, f_ref, e_ref, vol_ref = _mirror(model, inputs, vel, mass, dt, 16, baro, logs, th, xi)
        v_end = float(torch.linalg.det(md.box.double()).abs().reshape(-1)[0])
        print("V_16 / V_0 - 1 =", v_end / float(vol[0]) - 1.0, "scale", logs["scale"][:, 0].tolist())
        assert abs(v_end / float(vol[0]) - 1.0) > 1e-4  # the volume visibly moved
        assert _bits(md.pos, p_ref) and _bits(md.vel, v_ref) and _bits(md.box, b_ref) and _bits(md.forces, f_ref)
        assert _bits(logs["epot"], e_ref) and _bits(logs["volume"], vol_ref)
        # the same bits whatever the number of steps per launch, and from run to run
        for K, replays in ((8, 2), (16, 1), (1, 16)):
            md2, logs2 = _run(model, inputs, vel, mass, dt, K, replays, baro, th)
            assert _bits(md2.pos, md.pos) and _bits(md2.vel, md.vel) and _bits(md2.box, md.box) and _bits(md2.forces, md.forces), (K, replays)
            for k in ("epot", "ekin", "volume", "pressure", "scale"):
                assert _bits(logs2[k], logs[k]), (K, replays, k)
        # reset with the first box: the same trajectory again
        md2.reset(pos=inputs[1], vel=vel, box=inputs[3])
        md2(16)
        assert _bits(md2.pos, md.pos) and _bits(md2.box, md.box) and md2.check() == 16
        if c.get("replicas", 1) == 2:  # the replicas are independent: own box, own noise
            assert not _bits(logs["scale"][:, 0], logs["scale"][:, 1])
    finally:
        model.cell_list_min_atoms = keep


def test_seed_matters_and_no_barostat_is_todays_loop(hip_lib):
    model, inputs, vel, mass = _setup("tensornet")
    z, pos, batch, box, q = inputs
    P, vol, dt = _pressure(model, inputs, vel, mass)
    baro = _baro_for(P, vol, dt, +1)
    a, la = _run(model, inputs, vel, mass, dt, 8, 2, baro)
    b, lb = _run(model, inputs, vel, mass, dt, 8, 2, dict(baro, seed=100))
    assert not _bits(a.pos, b.pos) and not _bits(a.box, b.box) and not _bits(la["scale"], lb["scale"])
    # the caller's own box object is the one the graph scales
    mine = box.clone()
    md = model.capture_md(z, pos, vel, mass, dt, batch=batch, box=mine, q=q, steps_per_replay=8, barostat=baro)
    assert md.box is mine
    md(2)
    assert _bits(mine, a.box) and not _bits(mine, box)
    # barostat=None: the NVE loop as it was - against capture() + the torch mirror of tests/test_gpu_md_loop.py
    nve = model.capture_md(z, pos, vel, mass, dt, batch=batch, box=box, q=q, steps_per_replay=8)
    nve(2)
    assert nve.check() == 16 and not hasattr(nve, "volume")
    replay = model.capture(z, pos, batch, box, q=q)
    hk, dt_t = (0.5 * dt / mass.double()).float()[:, None], torch.tensor(dt, dtype=torch.float32, device="cuda")
    x, v = pos.clone(), vel.clone()
    f = replay(x)[1].clone()
    for _ in range(16):
        v = torch.add(v, torch.mul(hk, f))
        x = torch.add(x, torch.mul(dt_t, v))
        f = replay(x)[1].clone()
        v = torch.add(v, torch.mul(hk, f))
    assert _bits(nve.pos, x) and _bits(nve.vel, v) and _bits(nve.forces, f) and _bits(nve.box, box)


# ------------------------------------------------------------------------------------------------ 4. direction
@pytest.mark.parametrize("direction", [+1, -1])
def test_weak_coupling_moves_the_volume_towards_the_target(hip_lib, direction):
    """kT = 0, P0 twenty times the system's own |P| below (above) it: the volume grows (shrinks) in every one of 16 steps."""
    model, inputs, vel, mass = _setup("tensornet")
    P, vol, dt = _pressure(model, inputs, vel, mass)
    baro = _baro_for(P, vol, dt, direction, far=20.0, kT=0.0)
    md, logs = _run(model, inputs, vel, mass, dt, 16, 1, baro)
    v = torch.cat([logs["volume"][:, 0].double().cpu(), torch.linalg.det(md.box.double()).abs().reshape(-1).cpu()])
    print("direction", direction, "V", v.tolist(), "P", logs["pressure"][:, 0].tolist(), "P0", baro["pressure"])
    assert v.numel() == 17 and (direction * (v[1:] - v[:-1]) > 0).all()
    assert (direction * (logs["scale"][:, 0] - 1.0) > 0).all()
    assert abs(float(v[0]) / float(vol[0]) - 1.0) < 1e-6


# ------------------------------------------------------------------------------------------------ 5. overflow under NPT
def test_overflow_under_npt_freezes_box_and_state(hip_lib):
    """The case of tests/test_gpu_md_loop.py::test_overflow_freezes_the_state_at_the_last_valid_step with a barostat: box and
    positions scaled by 0.85 between two replays, max_num_neighbors = 72."""
    model, inputs, vel, mass = _setup("tensornet", max_num_neighbors=72)
    z, pos, batch, box0, q = inputs
    P, vol, _ = _pressure(model, inputs, vel, mass)
    baro = _baro_for(P, vol, 0.01, +1)
    md = model.capture_md(z, pos, vel, mass, 0.01, batch=batch, box=box0.clone(), q=q, steps_per_replay=4, barostat=baro)
    md()
    assert md.check() == 4 and not _bits(md.box, box0)
    md.box.mul_(0.85)
    md.pos.mul_(0.85)
    state = (md.box, md.pos, md.vel, md.forces, md.epot, md.ekin, md.volume, md.pressure, md.scale)
    keep = [t.clone() for t in state]
    host = (C.c_uint64 * 2)()
    for _ in range(3):  # the overflowing replay and two more
        md()
        with pytest.raises(RuntimeError, match="max_num_pairs"):
            md.check()
        assert hip_lib.tmdnet_md_status(None, C.c_void_p(md._ws.data_ptr()), host) == 3 and (int(host[0]), int(host[1])) == (4, 1)
        for t, k in zip(state, keep):
            assert _bits(t, k)
    md.reset(pos, vel, box=box0)
    assert _bits(md.box, box0)
    md()
    assert md.check() == 4 and not _bits(md.box, box0) and not _bits(md.pos, keep[1])


def test_a_nan_kinetic_energy_is_reported_as_the_barostat(hip_lib):
    model, inputs, vel, mass = _setup("tensornet")
    z, pos, batch, box, q = inputs
    P, vol, dt = _pressure(model, inputs, vel, mass)
    md = model.capture_md(z, pos, vel, mass, dt, batch=batch, box=box.clone(), q=q, steps_per_replay=2, barostat=_baro_for(P, vol, dt, +1))
    md()
    assert md.check() == 2
    md.masses[5] = float("nan")  # the buffer the graph reads: reaches the kinetic energy of the next step, and with it the pressure
    box_before, pos_before = md.box.clone(), md.pos.clone()
    md()
    with pytest.raises(RuntimeError, match="barostat"):
        md.check()
    host = (C.c_uint64 * 2)()
    assert hip_lib.tmdnet_md_status(None, C.c_void_p(md._ws.data_ptr()), host) == 5 and (int(host[0]), int(host[1])) == (3, 2)
    assert _bits(md.box, box_before) and torch.isfinite(md.pos).all() and not _bits(md.pos, pos_before)  # step 3 ran, its move did not
    md.masses[5] = mass[5]
    md.reset(pos, vel, box=box)
    md()
    assert md.check() == 2


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_model_and_earlier_graphs_as_they_were(hip_lib):
    model, inputs, vel, mass = _setup("tensornet")
    z, pos, batch, box, q = inputs
    baro = dict(pressure=0.0, tau=1.0, compressibility=1.0, kT=0.01)
    replay = model.capture(z, pos, batch, box, q=q)
    e0, f0 = (t.clone() for t in replay(pos))
    nve = model.capture_md(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, steps_per_replay=2)
    nve()
    p0, v0 = nve.pos.clone(), nve.vel.clone()
    with pytest.raises(ValueError, match="box"):  # no box (the model is not periodic by itself)
        model.capture_md(z, pos, vel, mass, 0.01, batch=batch, q=q, barostat=baro)
    two = torch.cat([batch, batch + 1])
    with pytest.raises(NotImplementedError, match="own box"):  # one shared box, two molecules
        model.capture_md(torch.cat([z, z]), torch.cat([pos, pos]), torch.cat([vel, vel]), torch.cat([mass, mass]), 0.01, batch=two, box=box,
                         q=torch.zeros(2, device="cuda"), barostat=baro)
    with pytest.raises(ValueError, match="unknown"):
        model.capture_md(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, barostat=dict(baro, beta=1.0))
    with pytest.raises(ValueError, match="kT"):  # no thermostat to take kT from
        model.capture_md(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, barostat=dict(pressure=0.0, tau=1.0, compressibility=1.0))
    with pytest.raises(ValueError):
        model.capture_md(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, barostat=dict(baro, tau=0.0))
    with pytest.raises(NotImplementedError, match="TensorNet2"):
        _model("tensornet2").capture_md(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, barostat=baro)
    # what capture_md refuses anyway, it refuses with a barostat too
    with pytest.raises(ValueError):
        model.capture_md(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, steps_per_replay=0, barostat=baro)
    with pytest.raises(NotImplementedError):
        model.capture_md(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, atom_weights=torch.ones(z.shape[0], device="cuda"), barostat=baro)
    # the graphs captured before the refusals replay the same bits
    e1, f1 = replay(pos)
    assert _bits(e1, e0) and _bits(f1, f0)
    nve.reset(pos, vel)
    nve()
    assert _bits(nve.pos, p0) and _bits(nve.vel, v0)
    # kT and seed default to the thermostat's
    md = model.capture_md(z, pos, vel, mass, 0.01, batch=batch, box=box.clone(), q=q, steps_per_replay=1,
                          thermostat=dict(friction=1.0, kT=0.02, seed=5), barostat=dict(pressure=0.0, tau=1.0, compressibility=1e-3))
    assert md.barostat["kT"] == 0.02 and md.barostat["seed"] == 5
