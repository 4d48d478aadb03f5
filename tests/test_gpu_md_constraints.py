"""-m gpu: SHAKE / RATTLE distance constraints in the device-resident MD loop (csrc/tn_md_cons.hip, capture_md_constrained(constraints=)).

1. the C entries alone, forces from a buffer: residual bounds at every step, the host mirror, free atoms bit-identical to
   tmdnet_md_advance, the kinetic energy, a molecule of two slices, an interleaved batch
2. through the model, K = 1: a mirror and the Newton oracle restarted from the device's previous state
3. the same bits whatever K, and from run to run
4. the constraints hold over a trajectory (rigid water, dt = 2 fs)
5. the projection at capture and at reset
6. status 3   7. overflow   8. refusals"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import md_cons_host_mirror as M
from tests import md_cons_oracle as O
from tests.test_gpu_md_loop import FS, _bits, _model, _Raw, _setup, _system
from torchmdnet_amd import md as MD

pytestmark = pytest.mark.gpu

OPEN, MIDDLE, CLOSE, PROJECT = 0, 1, 2, 3
EPS = 2.0 ** -23


def _res_x(pos, con):
    res, bound = MD.constraint_residuals(pos, con["pairs"], con["lengths"], con["tol"])
    return float((res / bound).max())


def _res_v(pos, vel, con, dt):
    """|r.(v_a - v_b)| <= tol d^2 / dt + 2 * 2^-23 |r| max|v| (derived in tests/test_md_constraints_host.py) -> largest ratio"""
    x, v, p = pos.double().cpu(), vel.double().cpu(), con["pairs"]
    r, u = x[p[:, 0]] - x[p[:, 1]], v[p[:, 0]] - v[p[:, 1]]
    d = con["lengths"]
    vmax = torch.maximum(v[p[:, 0]].abs().amax(1), v[p[:, 1]].abs().amax(1))
    return float(((r * u).sum(1).abs() / (con["tol"] * d * d / dt + 2 * EPS * r.norm(dim=1) * vmax)).max())


# ------------------------------------------------------------------------------------------------ 1. the C entries alone
class _RawC(_Raw):
    """tmdnet_md_advance_constrained on tensors of the test's own, graph_ws = NULL"""

    def __init__(self, lib, con, *args, **kw):
        self.con = con
        self.tables = [con[k].cuda().contiguous() for k in ("cluster_atoms", "cluster_offsets", "constraint_ends", "constraint_d2")]
        nb = C.c_size_t(0)
        assert lib.tmdnet_md_constraints_workspace_bytes(args[0].shape[0], self.tables[0].shape[0], self.tables[2].shape[0], C.byref(nb)) == 0
        self.cons_ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        super().__init__(lib, *args, **kw)

    def advance(self, phase, forces, max_iter=None):
        p, t = self._p, self.tables
        rc = self.L.tmdnet_md_advance_constrained(
            None, self._s(), None, p(self.ws), p(self.cons_ws), self.n, self.n_mol, phase, p(self.pos), p(self.vel), p(forces), None,
            p(self.hk), p(self.mass), p(self.sigma), self.dt, self.c1, self.c2, self.seed, p(self.batch), None, None, p(self.ekin),
            t[0].shape[0], t[2].shape[0], p(t[0]), p(t[1]), p(t[2]), p(t[3]), self.con["tol"], max_iter or self.con["max_iter"])
        assert rc == 0, rc


def _part(md):
    """the per-atom kinetic terms in the MD workspace: header 256 B, x_keep, v_keep (12 n bytes each, padded to 256), then part"""
    a256 = lambda b: (b + 255) & ~255
    off = (-md.ws.data_ptr()) % 256 + 256 + 2 * a256(12 * md.n)
    return md.ws[off:off + 4 * md.n].view(torch.float32).clone()


def _waters_and_free(n_mol=2, waters=3, free=5, seed=3, shuffle=False):
    """n_mol molecules of `waters` rigid waters and `free` atoms in no constraint -> pos, vel, forces (5), mass, batch, pairs"""
    g = torch.Generator().manual_seed(seed)
    a = math.radians(104.52)
    w = torch.tensor([[0, 0, 0], [0.9572, 0, 0], [0.9572 * math.cos(a), 0.9572 * math.sin(a), 0]])
    pos, mass, batch, pairs = [], [], [], []
    for m in range(n_mol):
        for k in range(waters):
            b = sum(len(p) for p in pos)
            q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
            pos.append(w @ q.T + 4 * torch.randn(1, 3, generator=g))
            mass += [15.999, 1.008, 1.008]
            pairs += [[b, b + 1], [b, b + 2], [b + 1, b + 2]]
        pos.append(4 * torch.randn(free, 3, generator=g))
        mass += (1.0 + 15 * torch.rand(free, generator=g)).tolist()
        batch += [m] * (3 * waters + free)
    pos, mass, batch, pairs = torch.cat(pos), torch.tensor(mass), torch.tensor(batch), torch.tensor(pairs)
    n = pos.shape[0]
    if shuffle:  # an interleaved, unsorted batch vector
        perm = torch.randperm(n, generator=g)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(n)
        pos, mass, batch, pairs = pos[perm], mass[perm], batch[perm], inv[pairs]
    vel = 0.02 * torch.randn(n, 3, generator=g)
    forces = [2.0 * torch.randn(n, 3, generator=g) for _ in range(5)]
    return pos, vel, forces, mass, batch, pairs


@pytest.mark.parametrize("thermostat", [False, True])
@pytest.mark.parametrize("shuffle", [False, True])
def test_c_entries_against_mirror_and_unconstrained_loop(hip_lib, thermostat, shuffle):
    pos, vel, forces, mass, batch, pairs = _waters_and_free(shuffle=shuffle)
    n, dt = pos.shape[0], 2.0
    if shuffle:
        assert (batch[1:] < batch[:-1]).any()
    con = MD.prepare_constraints(dict(pairs=pairs), pos, batch, mass, 2)
    free = torch.tensor(sorted(set(range(n)) - set(pairs.reshape(-1).tolist())), dtype=torch.long)
    bound = torch.tensor(sorted(set(pairs.reshape(-1).tolist())), dtype=torch.long)
    assert len(free) == 10 and con["n_bound"] == 6
    kw = dict(force_scale=FS, kT=0.025, friction=0.01, seed=99) if thermostat else dict(force_scale=FS)
    dev = [t.cuda() for t in (pos, vel, mass, batch)]
    fc = [f.cuda() for f in forces]
    md = _RawC(hip_lib, con, *dev, 2, dt, **kw)
    ref = _Raw(hip_lib, *dev, 2, dt, **kw)  # tmdnet_md_advance on the same buffers
    md.advance(PROJECT, None)
    assert _res_v(md.pos, md.vel, con, dt) <= 1 and _bits(md.vel[free], dev[1][free]) and _bits(md.pos, dev[0])
    assert not _bits(md.vel[bound], dev[1][bound])
    # the host mirror on the same inputs, launch by launch
    h = M.advance(0, 0, con, pos.numpy(), vel.numpy(), None, None, mass.numpy(), dt)
    args = dict(sigma=None if md.sigma is None else md.sigma.cpu().numpy(), c1=md.c1, c2=md.c2, seed=md.seed)
    hk = md.hk.cpu().numpy()
    worst_x = worst_v = 0.0
    for k, phase in enumerate([OPEN, MIDDLE, MIDDLE, MIDDLE, CLOSE]):
        md.advance(phase, fc[k])
        ref.advance(phase, fc[k])
        h = M.advance(phase != OPEN, phase != CLOSE, con, h["pos"], h["vel"], forces[k].numpy(), hk, mass.numpy(), dt, step=k - 1,
                      x_keep=h["x_keep"], v_keep=h["v_keep"], **args)
        assert h["fail"] == 0
        assert _bits(md.pos[free], ref.pos[free]) and _bits(md.vel[free], ref.vel[free]), phase
        scale = max(1.0, float(md.pos.abs().max()))
        worst_x = max(worst_x, float((md.pos.cpu() - torch.from_numpy(h["pos"])).abs().max()) / scale)
        worst_v = max(worst_v, float((md.vel.cpu() - torch.from_numpy(h["vel"])).abs().max()))
        assert _res_x(md.pos, con) <= 1, (phase, k)
        if phase != OPEN:
            assert _bits(_part(md)[free], _part(ref)[free])
            assert md.status() == (0, k, 0) and ref.status() == (0, k, 0)
    print("largest |device - host mirror|: x", worst_x, "v", worst_v, "margin", M.ORACLE_X, M.ORACLE_V)
    assert worst_x <= M.ORACLE_X and worst_v <= M.ORACLE_V
    assert _res_v(md.pos, md.vel, con, dt) <= 1 and not _bits(md.pos[bound], ref.pos[bound])
    # ekin is the fixed-order sum of the per-atom terms: tmdnet_md_advance reduces the same terms from the same velocities
    zero = torch.zeros_like(md.pos)
    again = _Raw(hip_lib, md.pos, md.vel, dev[2], dev[3], 2, dt)
    again.advance(OPEN, zero)
    again.advance(CLOSE, zero)
    assert _bits(_part(again), _part(md)) and _bits(again.ekin, md.ekin) and torch.isfinite(md.ekin).all()
    # MIDDLE = CLOSE, then OPEN: the velocity residual at every full step
    two = _RawC(hip_lib, con, *dev, 2, dt, **kw)
    two.advance(PROJECT, None)
    two.advance(OPEN, fc[0])
    for k in (1, 2, 3):
        two.advance(CLOSE, fc[k])
        assert _res_v(two.pos, two.vel, con, dt) <= 1, k
        two.advance(OPEN, fc[k])
        assert _res_x(two.pos, con) <= 1, k
    two.advance(CLOSE, fc[4])
    assert _bits(two.pos, md.pos) and _bits(two.vel, md.vel) and _bits(two.ekin, md.ekin)


def test_a_molecule_of_two_kinetic_energy_slices(hip_lib):
    """1 100 atoms in ONE molecule (> 1 024: two slices and the finishing kernel): 300 rigid waters and 200 free atoms"""
    pos, vel, forces, mass, batch, pairs = _waters_and_free(n_mol=1, waters=300, free=200, seed=6)
    assert pos.shape[0] == 1100
    con = MD.prepare_constraints(dict(pairs=pairs), pos, batch, mass, 1)
    assert con["cluster_atoms"].shape[0] == 325
    dev = [t.cuda() for t in (pos, vel, mass)]
    md = _RawC(hip_lib, con, *dev, None, 1, 2.0, force_scale=FS)
    md.advance(PROJECT, None)
    md.advance(OPEN, forces[0].cuda())
    md.advance(MIDDLE, forces[1].cuda())
    md.advance(CLOSE, forces[2].cuda())
    assert md.status() == (0, 2, 0) and _res_x(md.pos, con) <= 1 and _res_v(md.pos, md.vel, con, 2.0) <= 1
    zero = torch.zeros_like(md.pos)
    again = _Raw(hip_lib, md.pos, md.vel, dev[2], None, 1, 2.0)
    again.advance(OPEN, zero)
    again.advance(CLOSE, zero)
    assert _bits(again.ekin, md.ekin) and _bits(_part(again), _part(md))
    ref = (0.5 * mass.double() * (md.vel.double().cpu() ** 2).sum(1)).sum()
    assert abs(float(md.ekin) - float(ref)) < 1e-5 * float(ref)


# ------------------------------------------------------------------------------------------------ 2. through the model, K = 1
def _oracle_step(con, x0, v0, f0, f1, hk, mass, dt):
    """One NVE step of every cluster with constraints by the Newton oracle (tests/md_cons_oracle.py: no Gauss-Seidel, none of the
    header's statements), fp64 numpy on the device's fp32 state: B, A, S from (x0, v0, f0), then B, R with the forces f1 of the
    device's evaluation -> atoms [n_bound atoms], x, v"""
    atoms, off = con["cluster_atoms"].numpy(), con["cluster_offsets"].numpy()
    ends, d = con["constraint_ends"].numpy(), np.sqrt(con["constraint_d2"].numpy())
    idx, xs, vs = [], [], []
    for c in range(con["n_bound"]):
        a = atoms[c][atoms[c] >= 0]
        pairs, dc = ends[off[c]:off[c + 1]], d[off[c]:off[c + 1]]
        w = 1.0 / mass[a].astype(np.float64)
        x, v = O.open_step(x0[a], v0[a], f0[a], hk[a], dt, w, pairs, dc)
        idx.append(a)
        xs.append(x)
        vs.append(O.close_step(x, v, f1[a], hk[a], w, pairs))
    return np.concatenate(idx), np.concatenate(xs), np.concatenate(vs)


def _constrained(arch, name):
    model, replay, inputs, vel, mass, dt = _setup(arch, name)
    z, pos, batch = inputs[0], inputs[1], inputs[2]
    if name == "mol40":
        pairs = MD.hydrogen_pairs(z, pos, batch, cutoff=1.6)
        assert pairs.shape[0] >= 3
    else:
        pairs = MD.hydrogen_pairs(z, pos, batch, rigid_water=True)
        assert pairs.shape[0] == 192
    return model, replay, inputs, vel, mass, dt, pairs


@pytest.mark.parametrize("arch,name", [("tensornet", "mol40"), ("equivariant-transformer", "mol40"), ("tensornet2", "mol40"),
                                       ("tensornet", "water192")])
def test_k1_replays_against_a_mirror_restarted_from_the_device_state(hip_lib, arch, name):
    model, replay, inputs, vel, mass, dt, pairs = _constrained(arch, name)
    z, pos, batch, box, q = inputs
    dt = 5 * dt  # (the dt rule of the unconstrained tests keeps the atoms nearly still: the constraints would have nothing to do)
    md = model.capture_md_constrained(z, pos, vel, mass, dt, batch=batch, box=box, q=q, steps_per_replay=1, constraints=dict(pairs=pairs))
    con = md.constraints
    n = z.shape[0]
    bound = torch.tensor(sorted(set(pairs.reshape(-1).tolist())), dtype=torch.long, device="cuda")
    free = torch.tensor(sorted(set(range(n)) - set(bound.tolist())), dtype=torch.long, device="cuda")  # (none in the water box)
    assert md.ndof.tolist() == [3 * n - pairs.shape[0]]
    hk, dt_t = md.hk[:, None], torch.tensor(dt, dtype=torch.float32, device="cuda")
    worst_x = worst_v = oracle_x = oracle_v = 0.0
    for step in range(4):
        x0, v0, f0 = md.pos.clone(), md.vel.clone(), md.forces.clone()
        md()
        e, f = replay(md.pos)  # capture() at the device's positions
        assert _bits(md.forces, f) and _bits(md.epot[0], e.view(-1))
        v_half = torch.add(v0, torch.mul(hk, f0))
        x1 = torch.add(x0, torch.mul(dt_t, v_half))
        v1 = torch.add(v_half, torch.mul(hk, f))
        assert _bits(md.pos[free], x1[free]) and _bits(md.vel[free], v1[free]), step
        assert not _bits(md.pos[bound], x1[bound])  # the constraints did something
        a = M.advance(0, 1, con, x0.cpu().numpy(), v0.cpu().numpy(), f0.cpu().numpy(), md.hk.cpu().numpy(), mass.cpu().numpy(), dt)
        b = M.advance(1, 0, con, a["pos"], a["vel"], f.cpu().numpy(), md.hk.cpu().numpy(), mass.cpu().numpy(), dt, x_keep=a["x_keep"],
                      v_keep=a["v_keep"])
        assert a["fail"] == 0 and b["fail"] == 0
        scale = max(1.0, float(md.pos.abs().max()))
        worst_x = max(worst_x, float((md.pos.cpu() - torch.from_numpy(b["pos"])).abs().max()) / scale)
        worst_v = max(worst_v, float((md.vel.cpu() - torch.from_numpy(b["vel"])).abs().max()))
        # the Newton oracle, which shares nothing with the header, on every cluster with constraints
        at, xo, vo = _oracle_step(con, x0.cpu().numpy(), v0.cpu().numpy(), f0.cpu().numpy(), f.cpu().numpy(), md.hk.cpu().numpy(),
                                  mass.cpu().numpy(), dt)
        assert sorted(at.tolist()) == bound.tolist()
        oracle_x = max(oracle_x, float(np.abs(md.pos.cpu().numpy()[at] - xo).max()) / scale)
        oracle_v = max(oracle_v, float(np.abs(md.vel.cpu().numpy()[at] - vo).max()))
        assert _res_x(md.pos, con) <= 1 and _res_v(md.pos, md.vel, con, dt) <= 1
        ke = torch.zeros(1, dtype=torch.float64, device="cuda").index_add_(0, batch, 0.5 * mass.double() * (md.vel.double() ** 2).sum(1))
        assert ((md.ekin[0].double() - ke).abs() / ke).max().item() < 1e-5
    print(arch, name, "largest |device - host mirror|: x", worst_x, "v", worst_v, "|device - Newton oracle|: x", oracle_x, "v", oracle_v)
    assert worst_x <= M.ORACLE_X and worst_v <= M.ORACLE_V
    assert oracle_x <= M.ORACLE_X and oracle_v <= M.ORACLE_V
    assert md.check() == 4 and (md.pos - pos).abs().max().item() > 4 * dt * 0.002


# ------------------------------------------------------------------------------------------------ 3. K-independence
def _run(model, inputs, vel, mass, dt, K, replays, pairs, **kw):
    z, pos, batch, box, q = inputs
    md = model.capture_md_constrained(z, pos, vel, mass, dt, batch=batch, box=box, q=q, steps_per_replay=K,
                                      constraints=dict(pairs=pairs), **kw)
    epot, ekin = [], []
    for _ in range(replays):
        md()
        epot.append(md.epot.clone())
        ekin.append(md.ekin.clone())
    assert md.check() == K * replays == md.steps_done
    return md, torch.cat(epot), torch.cat(ekin)


@pytest.mark.parametrize("thermostat", [None, dict(friction=0.5, kT=0.01, seed=2 ** 40 + 5)])
def test_the_same_bits_whatever_k_and_from_run_to_run(hip_lib, thermostat):
    model, replay, inputs, vel, mass, dt, pairs = _constrained("tensornet", "water192")
    dt = 5 * dt
    runs = [_run(model, inputs, vel, mass, dt, K, r, pairs, thermostat=thermostat) for K, r in ((1, 16), (8, 2), (16, 1), (16, 1))]
    a = runs[0]
    assert (a[0].pos - inputs[1]).abs().max().item() > 16 * dt * 0.002
    for b in runs[1:]:
        assert _bits(a[0].pos, b[0].pos) and _bits(a[0].vel, b[0].vel) and _bits(a[0].forces, b[0].forces)
        assert _bits(a[1], b[1]) and _bits(a[2], b[2])
    # reset: back to the start (velocities projected again), the same trajectory again
    md = runs[-1][0]
    md.reset(pos=inputs[1], vel=vel)
    md()
    assert _bits(md.pos, a[0].pos) and _bits(md.vel, a[0].vel) and md.check() == 16


# ------------------------------------------------------------------------------------------------ 4. a trajectory
@pytest.mark.parametrize("thermostat", [None, dict(friction=0.01, kT=0.025, seed=7)])
def test_rigid_water_stays_rigid_over_64_steps_at_2_fs(hip_lib, thermostat):
    model = _model("tensornet", max_num_neighbors=128)  # (about 52 neighbours per atom at the start: room for the atoms to travel)
    z, pos, batch, box = (t.cuda() for t in _system("water192"))
    q = torch.zeros(1, device="cuda")
    mass = torch.where(z == 1, 1.008, 12.0).float()
    vel = 0.005 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    pairs = MD.hydrogen_pairs(z, pos, rigid_water=True)
    _, f0 = model.capture(z, pos, batch, box, q=q)(pos)
    fs = FS * 0.2 / float(f0.abs().max())  # the random model is no force field: its largest force counts as 0.2 eV / A
    md = model.capture_md_constrained(z, pos, vel, mass, 2.0, batch=batch, box=box, q=q, steps_per_replay=8, force_scale=fs,
                                      thermostat=thermostat, constraints=dict(pairs=pairs))
    assert md.ndof.tolist() == [3 * 192 - 192]
    tot = []
    for _ in range(8):
        md()
        assert _res_x(md.pos, md.constraints) <= 1 and _res_v(md.pos, md.vel, md.constraints, 2.0) <= 1
        tot.append(md.epot.double().sum(1) + md.ekin.double().sum(1) / fs)
    assert md.check() == 64 and (md.pos - pos).abs().max().item() > 0.1
    if thermostat is None:
        tot = torch.cat(tot).cpu()
        free = model.capture_md(z, pos, vel, mass, 1.0, batch=batch, box=box, q=q, steps_per_replay=8, force_scale=fs)
        tot1 = []
        for _ in range(8):
            free()
            tot1.append(free.epot.double().sum(1) + free.ekin.double().sum(1) / fs)
        tot1 = torch.cat(tot1).cpu()
        print("NVE drift of epot + ekin / force_scale over 64 steps: constrained, 2 fs:", float(tot[-8:].mean() - tot[:8].mean()),
              "(fluctuation", float(tot.std()), ") unconstrained, 1 fs:", float(tot1[-8:].mean() - tot1[:8].mean()), "(fluctuation",
              float(tot1.std()), ")")


# ------------------------------------------------------------------------------------------------ 5. projection
def test_velocities_are_projected_at_capture_and_at_reset(hip_lib):
    model, replay, inputs, vel, mass, dt, pairs = _constrained("tensornet", "water192")
    z, pos, batch, box, q = inputs
    md = model.capture_md_constrained(z, pos, vel, mass, dt, batch=batch, box=box, q=q, steps_per_replay=2, constraints=dict(pairs=pairs))
    assert _res_v(pos, vel, md.constraints, dt) > 100  # as drawn
    assert _res_v(md.pos, md.vel, md.constraints, dt) <= 1 and _bits(md.pos, pos) and not _bits(md.vel, vel) and md.check() == 0
    # atoms in no constraint keep their velocities: the O-H pairs of 20 waters only
    some = pairs[:40]
    md2 = model.capture_md_constrained(z, pos, vel, mass, dt, batch=batch, box=box, q=q, steps_per_replay=2, constraints=dict(pairs=some))
    free = torch.tensor(sorted(set(range(192)) - set(some.reshape(-1).tolist())), dtype=torch.long, device="cuda")
    assert _bits(md2.vel[free], vel[free]) and _res_v(md2.pos, md2.vel, md2.constraints, dt) <= 1
    vel2 = 0.03 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(2)).cuda()
    md2.reset(vel=vel2)
    assert _bits(md2.vel[free], vel2[free]) and not _bits(md2.vel, vel2) and _res_v(md2.pos, md2.vel, md2.constraints, dt) <= 1
    with pytest.raises(ValueError, match="worst is pair"):
        md2.reset(pos=pos * 1.01)
    md2()
    assert md2.check() == 2


# ------------------------------------------------------------------------------------------------ 6. status 3
def test_status_3_freezes_a_finite_state_until_reset(hip_lib):
    model, replay, inputs, vel, mass, dt, pairs = _constrained("tensornet", "water192")
    z, pos, batch, box, q = inputs
    big = 0.2 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(3)).cuda()
    md = model.capture_md_constrained(z, pos, torch.zeros_like(pos), mass, 2.0, batch=batch, box=box, q=q, steps_per_replay=4,
                                      constraints=dict(pairs=pairs, max_iter=1))  # (zero velocities: the projection has nothing to do)
    md.vel.copy_(big)  # 0.4 A per step, not projected: one sweep cannot converge
    md()
    with pytest.raises(RuntimeError, match="constraints: .*did not converge"):
        md.check()
    host = (C.c_uint64 * 2)()
    assert hip_lib.tmdnet_md_status(None, C.c_void_p(md._ws.data_ptr()), host) == 5 and int(host[1]) == 3
    assert torch.isfinite(md.pos).all() and torch.isfinite(md.vel).all()
    keep = [t.clone() for t in (md.pos, md.vel, md.forces, md.epot, md.ekin)]
    md(2)
    with pytest.raises(RuntimeError, match="reset"):
        md.check()
    for t, k in zip((md.pos, md.vel, md.forces, md.epot, md.ekin), keep):
        assert _bits(t, k)
    assert hip_lib.tmdnet_md_status(None, C.c_void_p(md._ws.data_ptr()), host) == 5 and int(host[1]) == 3
    # max_iter is a capture-time value: a second loop with sane settings runs from the same start
    sane = model.capture_md_constrained(z, pos, 0.1 * big, mass, dt, batch=batch, box=box, q=q, steps_per_replay=4,
                                        constraints=dict(pairs=pairs))
    sane()
    assert sane.check() == 4 and _res_x(sane.pos, sane.constraints) <= 1
    # the frozen state is not a point of the trajectory: a reset that keeps its positions or its velocities is refused, unchanged
    for kw in (dict(), dict(vel=torch.zeros_like(pos)), dict(pos=pos)):
        with pytest.raises(RuntimeError, match="needs both pos and vel"):
            md.reset(**kw)
    for t, k in zip((md.pos, md.vel, md.forces, md.epot, md.ekin), keep):
        assert _bits(t, k)
    assert hip_lib.tmdnet_md_status(None, C.c_void_p(md._ws.data_ptr()), host) == 5 and int(host[1]) == 3
    md.reset(pos=pos, vel=torch.zeros_like(pos))  # clears the status of the first
    assert md.check() == 0


# ------------------------------------------------------------------------------------------------ 7. overflow
def test_overflow_with_constraints_freezes_the_last_valid_step(hip_lib):
    """the max_num_neighbors = 72 water case of tests/test_gpu_md_loop.py, with rigid water"""
    model = _model("tensornet", max_num_neighbors=72)
    z, pos, batch, box = (t.cuda() for t in _system("water192"))
    box = box.clone()
    q = torch.zeros(1, device="cuda")
    vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    mass = torch.where(z == 1, 1.008, 12.0).float()
    pairs = MD.hydrogen_pairs(z, pos, rigid_water=True)
    md = model.capture_md_constrained(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, steps_per_replay=4, constraints=dict(pairs=pairs))
    md()
    assert md.check() == 4
    keep = [t.clone() for t in (md.pos, md.vel, md.forces, md.epot, md.ekin)]
    box.mul_(0.85)  # the box alone: the molecules stay rigid, but the periodic images come closer and the evaluation overflows
    md()
    with pytest.raises(RuntimeError, match="max_num_pairs"):
        md.check()
    host = (C.c_uint64 * 2)()
    assert hip_lib.tmdnet_md_status(None, C.c_void_p(md._ws.data_ptr()), host) == 3 and (int(host[0]), int(host[1])) == (4, 1)
    for t, k in zip((md.pos, md.vel, md.forces, md.epot, md.ekin), keep):
        assert _bits(t, k)
    assert _res_x(md.pos, md.constraints) <= 1 and _res_v(md.pos, md.vel, md.constraints, 0.01) <= 1


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_model_as_it_was(hip_lib):
    model = _model("tensornet")
    z, pos, batch, _ = (None if t is None else t.cuda() for t in _system("ragged"))  # molecules of 7, 12 and 20 atoms
    vel, mass = torch.zeros_like(pos), torch.full((z.shape[0],), 12.0, device="cuda")
    replay = model.capture(z, pos, batch)
    e0, f0 = (t.clone() for t in replay(pos))
    y0, g0 = model(z, pos, batch)
    heavy = mass.clone()
    heavy[:2] = float("inf")
    star = [[7, k] for k in range(8, 16)]  # 9 atoms
    for bad, m, err in (([[6, 7]], mass, ValueError), ([[0, 39]], mass, ValueError), ([[2, 2]], mass, ValueError),
                        ([[0, 1], [1, 0]], mass, ValueError), ([[0, 1]], heavy, ValueError), (star, mass, ValueError)):
        with pytest.raises(err, match="constraints"):
            model.capture_md_constrained(z, pos, vel, m, 0.01, batch=batch, constraints=dict(pairs=torch.tensor(bad)))
    with pytest.raises(ValueError, match="worst is pair"):
        model.capture_md_constrained(z, pos, vel, mass, 0.01, batch=batch, constraints=dict(pairs=torch.tensor([[0, 1]]), lengths=[9.0]))
    box = 30 * torch.eye(3, device="cuda").repeat(3, 1, 1)
    with pytest.raises(NotImplementedError, match="barostat"):
        model.capture_md_constrained(z, pos, vel, mass, 0.01, batch=batch, box=box, constraints=dict(pairs=torch.tensor([[0, 1]])),
                                     barostat=dict(pressure=0.0, tau=100.0, compressibility=1.0, kT=0.01))
    e1, f1 = replay(pos)
    y1, g1 = model(z, pos, batch)
    assert _bits(e1, e0) and _bits(f1, f0) and _bits(y1, y0) and _bits(g1, g0)
