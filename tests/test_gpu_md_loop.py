"""-m gpu: the device-resident MD loop (csrc/tn_md.hip, TorchMD_Net.capture_md).

1. the integrator alone: tmdnet_md_advance on a synthetic force buffer, no graph workspace
2. NVE through the model: K steps per graph launch are bit-identical to capture() + a torch mirror that evaluates the scheme one
   rounded operation at a time (torch.mul, then torch.add - never addcmul, which fuses)
3. energy conservation from the in-graph logs, with the bounds of tests/test_gpu_md.py
4. Langevin through the model: a function of (seed, step, atom) only
5. overflow: the state freezes at the last valid step
6. refusals"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import md_host_mirror as H
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

OPEN, MIDDLE, CLOSE = 0, 1, 2
FS = 9.648533e-3


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. the integrator alone
class _Raw:
    """The C entries on tensors of the test's own, graph_ws = NULL (no model: the forces are whatever `forces` holds)."""

    def __init__(self, lib, pos, vel, mass, batch, n_mol, dt, force_scale=1.0, kT=None, friction=0.0, seed=0):
        self.L, self.n, self.n_mol, self.dt = lib, pos.shape[0], n_mol, dt
        self.pos, self.vel = pos.clone().contiguous(), vel.clone().contiguous()
        m64 = mass.double()
        self.mass = mass.float().contiguous()
        self.hk = (0.5 * dt * force_scale / m64).float().contiguous()
        self.sigma = None if kT is None else torch.sqrt(kT * force_scale / m64).float().contiguous()
        self.c1 = math.exp(-friction * dt)
        self.c2 = math.sqrt(1.0 - self.c1 ** 2)
        self.seed, self.batch = seed, batch
        nb = C.c_size_t(0)
        assert lib.tmdnet_md_workspace_bytes(self.n, n_mol, C.byref(nb)) == 0
        self.ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
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

    def status(self):
        host = (C.c_uint64 * 2)()
        rc = self.L.tmdnet_md_status(self._s(), self._p(self.ws), host)
        return rc, int(host[0]), int(host[1])


def _ragged_1000():
    g = torch.Generator().manual_seed(21)
    sizes = [300, 333, 367]
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes))
    pos = 10 * torch.randn(1000, 3, generator=g)
    vel = 0.05 * torch.randn(1000, 3, generator=g)
    f0, f1 = 3 * torch.randn(1000, 3, generator=g), 3 * torch.randn(1000, 3, generator=g)
    mass = 1.0 + 39.0 * torch.rand(1000, generator=g)
    return [t.cuda() for t in (pos, vel, f0, f1, mass, batch)]


def test_one_step_equals_the_torch_mirror_bit_for_bit(hip_lib):
    pos, vel, f0, f1, mass, batch = _ragged_1000()
    dt = 0.5
    md = _Raw(hip_lib, pos, vel, mass, batch, 3, dt, force_scale=FS)
    md.advance(OPEN, f0)
    hk, dt_t = md.hk[:, None], torch.tensor(dt, device="cuda")
    v_half = torch.add(vel, torch.mul(hk, f0))
    x_new = torch.add(pos, torch.mul(dt_t, v_half))
    assert _bits(md.vel, v_half) and _bits(md.pos, x_new)
    md.advance(CLOSE, f1)
    v_new = torch.add(v_half, torch.mul(hk, f1))
    assert _bits(md.vel, v_new) and _bits(md.pos, x_new)
    ref = torch.zeros(3, dtype=torch.float64, device="cuda").index_add_(0, batch, 0.5 * mass.double() * (v_new.double() ** 2).sum(1))
    err = ((md.ekin.double() - ref).abs() / ref).max().item()
    print("ekin rel err vs fp64:", err)
    assert err < 1e-5
    assert md.status() == (0, 1, 0)
    # the fused launch: close step 1 and open step 2 with the same force, two kicks as two additions
    md2 = _Raw(hip_lib, pos, vel, mass, batch, 3, dt, force_scale=FS)
    md2.advance(OPEN, f0)
    md2.advance(MIDDLE, f1)
    v_3half = torch.add(v_new, torch.mul(hk, f1))
    assert _bits(md2.vel, v_3half) and _bits(md2.pos, torch.add(x_new, torch.mul(dt_t, v_3half))) and _bits(md2.ekin, md.ekin)
    # one molecule, no batch vector: the unfiltered range
    md3 = _Raw(hip_lib, pos, vel, mass, None, 1, dt, force_scale=FS)
    md3.advance(OPEN, f0)
    md3.advance(CLOSE, f1)
    assert abs(md3.ekin.item() - ref.sum().item()) < 1e-5 * ref.sum().item() and _bits(md3.vel, v_new)


def test_kinetic_energy_slices_of_a_large_molecule(hip_lib):
    """5 000 atoms in 2 molecules (2 500 each > 1 024: three slices and the finishing kernel), interleaved, filtered by `batch`."""
    g = torch.Generator().manual_seed(5)
    n = 5000
    batch = (torch.arange(n) % 2).cuda()
    vel, mass = (0.05 * torch.randn(n, 3, generator=g)).cuda(), (1.0 + 10 * torch.rand(n, generator=g)).cuda()
    zero = torch.zeros(n, 3, device="cuda")
    md = _Raw(hip_lib, zero, vel, mass, batch, 2, 0.5)
    md.advance(OPEN, zero)
    md.advance(CLOSE, zero)
    ref = torch.zeros(2, dtype=torch.float64, device="cuda").index_add_(0, batch, 0.5 * mass.double() * (vel.double() ** 2).sum(1))
    assert ((md.ekin.double() - ref).abs() / ref).max().item() < 1e-5
    first = md.ekin.clone()
    md.advance(OPEN, zero)
    md.advance(CLOSE, zero)
    assert _bits(md.ekin, first) and md.status() == (0, 2, 0)  # fixed order: the same bits


def test_langevin_equilibrates_to_kT(hip_lib):
    n, kT, dt = 4096, 0.025, 1.0
    g = torch.Generator().manual_seed(9)
    mass = (1.0 + 15.0 * torch.rand(n, generator=g)).cuda()
    zero = torch.zeros(n, 3, device="cuda")
    md = _Raw(hip_lib, zero, zero, mass, None, 1, dt, force_scale=FS, kT=kT, friction=0.1, seed=1234)
    md.advance(OPEN, zero)
    for _ in range(199):
        md.advance(MIDDLE, zero)
    md.advance(CLOSE, zero)
    assert md.status() == (0, 200, 0)
    ratio = mass.double()[:, None] * md.vel.double() ** 2 / (kT * FS)  # 12 288 samples of chi^2_1: relative sd of the mean 1.3 %
    print("<m v^2> / (kT force_scale): all", ratio.mean().item(), "per axis", ratio.mean(0).tolist())
    assert abs(ratio.mean().item() - 1.0) < 0.06
    assert abs(md.ekin.item() / (1.5 * n * kT * FS) - 1.0) < 0.06


def test_noise_follows_the_callers_index(hip_lib):
    n, dt, seed = 600, 1.0, 77
    g = torch.Generator().manual_seed(10)
    mass = (1.0 + 15.0 * torch.rand(n, generator=g)).cuda()
    perm = torch.randperm(n, generator=g).cuda()
    zero = torch.zeros(n, 3, device="cuda")

    def xi_of(m, step0):
        md = _Raw(hip_lib, zero, zero, m, None, 1, dt, kT=1.0, friction=0.5, seed=seed)
        md.reset(step0)
        md.advance(OPEN, zero)
        md.advance(CLOSE, zero)
        return md.vel / (md.c2 * md.sigma[:, None])  # v = (c2 sigma) xi from v = 0, F = 0

    a, b = xi_of(mass, 40), xi_of(mass[perm], 40)
    assert (a - b).abs().max().item() < 1e-5  # the atoms moved to other indices, the noise stayed with the index
    assert (a[perm] - b).abs().max().item() > 1.0
    host = torch.from_numpy(H.noise(seed, 40, np.arange(n))).cuda()  # the same header on the host: the same counter layout
    assert (a - host).abs().max().item() < 1e-5
    assert (xi_of(mass, 41) - a).abs().max().item() > 1.0  # the step enters the counter


def test_frozen_atoms_keep_x_and_v(hip_lib):
    pos, vel, f0, f1, mass, batch = _ragged_1000()
    frozen = torch.arange(0, 1000, 7, device="cuda")
    mass = mass.clone()
    mass[frozen] = float("inf")
    vel = vel.clone()
    vel[frozen] = 0.0
    md = _Raw(hip_lib, pos, vel, mass, batch, 3, 0.5, force_scale=FS, kT=0.025, friction=0.1, seed=3)
    assert (md.hk[frozen] == 0).all() and (md.sigma[frozen] == 0).all()
    md.advance(OPEN, f0)
    md.advance(MIDDLE, f1)
    md.advance(CLOSE, f0)
    assert _bits(md.pos[frozen], pos[frozen]) and _bits(md.vel[frozen], vel[frozen])
    assert torch.isfinite(md.ekin).all() and not _bits(md.pos, pos)


# ------------------------------------------------------------------------------------------------ 2. NVE bit-identity
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


def _system(name):
    """-> z, pos, batch, box (CPU)"""
    if name == "mol40":  # the molecule of tests/test_gpu_md.py
        z, pos, batch = W.synthetic_batch(n_mol=1, n_atoms=40, first_seed=31)
        return z % 8 + 1, pos, batch, None
    if name == "ragged":
        zs, ps, bs = [], [], []
        for m, n in enumerate([7, 12, 20]):
            z, p = W.synthetic_molecule(40 + m, n)
            zs.append(torch.from_numpy(z))
            ps.append(torch.from_numpy(p) + 3.0 * m)
            bs.append(torch.full((n,), m, dtype=torch.long))
        return torch.cat(zs), torch.cat(ps), torch.cat(bs), None
    z, pos, box = W.water_box(n_side=4)  # 192 atoms, periodic
    return z, pos, torch.zeros_like(z), box


def _setup(arch, name):
    model = _model(arch)
    z, pos, batch, box = (None if t is None else t.cuda() for t in _system(name))
    n_mol = int(batch.max()) + 1
    q = torch.zeros(n_mol, device="cuda") if arch != "equivariant-transformer" else None
    vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    mass = torch.where(z == 1, 1.008, 12.0).float() if name != "mol40" else torch.full((z.shape[0],), 12.0, device="cuda")
    replay = model.capture(z, pos, batch, box, q=q)
    _, f0 = replay(pos)
    dt = min(0.05, 0.02 * (12.0 / max(float(f0.abs().max()), 1e-6)) ** 0.5)  # the dt rule of tests/test_gpu_md.py
    return model, replay, (z, pos, batch, box, q), vel, mass.cuda(), dt


def _mirror(replay, pos0, vel0, mass, dt, steps, force_scale=1.0):
    """capture() + the scheme in torch, every product and every sum its own rounded kernel.  -> pos, vel, forces, epot [steps,B]"""
    hk = (0.5 * dt * force_scale / mass.double()).float()[:, None]
    dt_t = torch.tensor(dt, dtype=torch.float32, device="cuda")
    pos, vel = pos0.clone(), vel0.clone()
    _, f = replay(pos)
    f = f.clone()
    epot = []
    for _ in range(steps):
        vel = torch.add(vel, torch.mul(hk, f))
        pos = torch.add(pos, torch.mul(dt_t, vel))
        e, f = replay(pos)
        e, f = e.clone(), f.clone()
        vel = torch.add(vel, torch.mul(hk, f))
        epot.append(e.view(-1))
    return pos, vel, f, torch.stack(epot)


def _run(model, inputs, vel, mass, dt, K, replays, **kw):
    z, pos, batch, box, q = inputs
    md = model.capture_md(z, pos, vel, mass, dt, batch=batch, box=box, q=q, steps_per_replay=K, **kw)
    epot, ekin = [], []
    for _ in range(replays):
        md()
        epot.append(md.epot.clone())
        ekin.append(md.ekin.clone())
    assert md.check() == K * replays == md.steps_done
    return md, torch.cat(epot), torch.cat(ekin)


@pytest.mark.parametrize("arch,name", [("tensornet", "mol40"), ("equivariant-transformer", "mol40"), ("tensornet2", "mol40"),
                                       ("tensornet", "ragged"), ("tensornet", "water192")])
def test_nve_is_bit_identical_to_capture_plus_torch_mirror(hip_lib, arch, name):
    model, replay, inputs, vel, mass, dt = _setup(arch, name)
    pos = inputs[1]
    p_ref, v_ref, f_ref, e_ref = _mirror(replay, pos, vel, mass, dt, 16)
    assert (p_ref - pos).abs().max().item() > 4 * dt * 0.02  # the atoms really moved
    md, epot, ekin = _run(model, inputs, vel, mass, dt, 8, 2)
    assert _bits(md.pos, p_ref) and _bits(md.vel, v_ref) and _bits(md.forces, f_ref) and _bits(epot, e_ref)
    ke = torch.zeros(epot.shape[1], dtype=torch.float64, device="cuda").index_add_(0, inputs[2], 0.5 * mass.double() * (v_ref.double() ** 2).sum(1))
    assert ((ekin[-1].double() - ke).abs() / ke).max().item() < 1e-5
    # the same bits whatever the number of steps per launch, and from run to run
    for K, replays in ((1, 16), (16, 1), (8, 2)):
        md2, epot2, ekin2 = _run(model, inputs, vel, mass, dt, K, replays)
        assert _bits(md2.pos, p_ref) and _bits(md2.vel, v_ref) and _bits(md2.forces, f_ref), (K, replays)
        assert _bits(epot2, e_ref) and _bits(ekin2, ekin), (K, replays)
    # reset: back to the start, the same trajectory again
    md2.reset(pos=pos, vel=vel)
    md2(2)
    assert _bits(md2.pos, p_ref) and _bits(md2.vel, v_ref) and md2.check() == 16


# ------------------------------------------------------------------------------------------------ 3. energy conservation
@pytest.mark.parametrize("arch", ["tensornet", "equivariant-transformer", "tensornet2"])
def test_nve_energy_conservation_from_the_in_graph_logs(hip_lib, arch):
    model, replay, inputs, vel, mass, dt = _setup(arch, "mol40")
    pos = inputs[1]
    md1, ep1, ek1 = _run(model, inputs, vel, mass, dt, 40, 3)  # 120 steps
    md2, ep2, ek2 = _run(model, inputs, vel, mass, dt / 2, 40, 6)  # 240 steps
    tot1, tot2 = (ep1.double() + ek1.double()).sum(1).cpu(), (ep2.double() + ek2.double()).sum(1).cpu()
    kin = 0.5 * 12.0 * float((vel * vel).sum())
    fl1, fl2 = float(tot1.std()), float(tot2.std())
    drift1 = abs(float(tot1[-20:].mean() - tot1[:20].mean()))
    print("drift", drift1, "kin", kin, "fluctuation", fl1, fl2)
    assert (md1.pos - pos).abs().max().item() > 10 * dt * 0.02  # the atoms really moved
    assert drift1 < 0.02 * max(kin, float(tot1.abs().mean()) * 1e-3), (drift1, kin)
    assert fl2 < 0.6 * fl1 + 1e-7 * abs(float(tot1.mean())), (fl1, fl2)  # O(dt^2): ~0.25x, fp32 noise floor aside


# ------------------------------------------------------------------------------------------------ 4. Langevin through the model
def test_langevin_depends_on_seed_step_and_atom_only(hip_lib):
    model, replay, inputs, vel, mass, dt = _setup("tensornet", "ragged")
    th = dict(friction=2.0, kT=0.01, seed=2 ** 40 + 5)
    a, ea, ka = _run(model, inputs, vel, mass, dt, 4, 4, thermostat=th)
    b, eb, kb = _run(model, inputs, vel, mass, dt, 4, 4, thermostat=th)
    assert _bits(a.pos, b.pos) and _bits(a.vel, b.vel) and _bits(ea, eb) and _bits(ka, kb)
    c, ec, kc = _run(model, inputs, vel, mass, dt, 16, 1, thermostat=th)
    assert _bits(a.pos, c.pos) and _bits(a.vel, c.vel) and _bits(a.forces, c.forces) and _bits(ea, ec) and _bits(ka, kc)
    d, _, _ = _run(model, inputs, vel, mass, dt, 4, 4, thermostat=dict(th, seed=6))
    assert not _bits(a.vel, d.vel) and not _bits(a.pos, d.pos)
    nve, _, _ = _run(model, inputs, vel, mass, dt, 4, 4)
    assert not _bits(a.vel, nve.vel)


# ------------------------------------------------------------------------------------------------ 5. overflow
def test_overflow_freezes_the_state_at_the_last_valid_step(hip_lib):
    """192-atom periodic box, about 52 neighbours per atom inside 5 A: max_num_neighbors = 72 holds it; scaled by 0.85 (box and
    positions in place, between two replays) it holds about 85 and the first evaluation of the second replay overflows."""
    model = _model("tensornet", max_num_neighbors=72)
    z, pos, batch, box = (t.cuda() for t in _system("water192"))
    box = box.clone()
    box0 = box.clone()
    q = torch.zeros(1, device="cuda")
    vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    mass = torch.where(z == 1, 1.008, 12.0).float()
    md = model.capture_md(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, steps_per_replay=4)
    md()
    assert md.check() == 4
    box.mul_(0.85)
    md.pos.mul_(0.85)
    keep = [t.clone() for t in (md.pos, md.vel, md.forces, md.epot, md.ekin)]
    md()
    with pytest.raises(RuntimeError, match="max_num_pairs"):
        md.check()
    host = (C.c_uint64 * 2)()
    assert hip_lib.tmdnet_md_status(None, C.c_void_p(md._ws.data_ptr()), host) == 3 and (int(host[0]), int(host[1])) == (4, 1)
    for t, k in zip((md.pos, md.vel, md.forces, md.epot, md.ekin), keep):
        assert _bits(t, k)
    md()  # frozen: nothing moves
    with pytest.raises(RuntimeError, match="max_num_pairs"):
        md.check()
    assert hip_lib.tmdnet_md_status(None, C.c_void_p(md._ws.data_ptr()), host) == 3 and (int(host[0]), int(host[1])) == (4, 1)
    for t, k in zip((md.pos, md.vel, md.forces, md.epot, md.ekin), keep):
        assert _bits(t, k)
    # the model evaluates eagerly afterwards, and the loop runs again after a reset at a geometry that fits
    box.copy_(box0)
    E, F = model(z, pos, batch, box=box, q=q)
    assert torch.isfinite(E).all() and torch.isfinite(F).all()
    md.reset(pos=pos, vel=vel)
    md()
    assert md.check() == 4 and not _bits(md.pos, keep[0])


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_model_as_it_was(hip_lib):
    from torchmdnet_amd.models.model import create_model

    model = _model("tensornet")
    z, pos, batch, _ = (None if t is None else t.cuda() for t in _system("ragged"))
    vel, mass = torch.zeros_like(pos), torch.full((z.shape[0],), 12.0, device="cuda")
    replay = model.capture(z, pos, batch)
    e0, f0 = (t.clone() for t in replay(pos))
    y0, g0 = model(z, pos, batch)
    with pytest.raises(ValueError):
        model.capture_md(z, pos, vel, mass, 0.01, batch=batch, steps_per_replay=0)
    with pytest.raises(NotImplementedError):
        model.capture_md(z, pos, vel, mass, 0.01, batch=batch, atom_weights=torch.ones(z.shape[0], device="cuda"))
    with pytest.raises(NotImplementedError):
        model.capture_md(z, pos, vel, mass, 0.01, batch=batch, halo_exchange=lambda *a: None)
    model.parameter_gradients = True
    try:
        with pytest.raises(NotImplementedError):
            model.capture_md(z, pos, vel, mass, 0.01, batch=batch)
    finally:
        model.parameter_gradients = False
    with pytest.raises(ValueError):
        model.capture_md(z, pos, vel, mass[:-1], 0.01, batch=batch)
    torch.manual_seed(0)
    with pytest.raises(NotImplementedError):
        create_model(dict(W.TINY_ARGS, static_shapes=True, output_model="DipoleMoment")).to("cuda").capture_md(
            z, pos, vel, mass, 0.01, batch=batch)
    with pytest.raises(RuntimeError, match="static_shapes"):
        create_model(dict(W.TINY_ARGS)).to("cuda").capture_md(z, pos, vel, mass, 0.01, batch=batch)
    e1, f1 = replay(pos)  # the graph captured before the refusals is still valid, and gives the same bits
    y1, g1 = model(z, pos, batch)
    assert _bits(e1, e0) and _bits(f1, f0) and _bits(y1, y0) and _bits(g1, g0)
