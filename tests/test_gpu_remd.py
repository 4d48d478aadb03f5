"""-m gpu: temperature replica exchange in the device-resident MD loop (csrc/tn_remd.hip: k_remd_decide, k_remd_atoms;
TorchMD_Net.capture_remd).

1. the raw entries, no model: tmdnet_md_exchange on synthetic energies and velocities against the host mirror
2. forced outcomes: D >= 0, NaN energies, a frozen state
3. canonical sampling of a harmonic well through the raw entries (the protocol and the bounds of tests/remd_oracle.py)
4. through the model: equal temperatures are capture_md bit for bit, decisions equal the mirror on the device's own energies,
   continuing after a swap, overflow, refusals
5. Equivariant Transformer and TensorNet2"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import remd_host_mirror as HR
from tests import remd_oracle as O
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

OPEN, MIDDLE, CLOSE = 0, 1, 2
FS = 9.648533e-3


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _np(t):
    return t.detach().cpu().numpy()


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the raw entries
class _Raw:
    """The C entries on tensors of the test's own, graph_ws = NULL (no model): G ladders of R replicas of n atoms."""

    def __init__(self, lib, G, R, vel, mass1, kT, every, seed, force_scale=1.0, dt=0.1, friction=1.0, pos=None):
        self.L, self.G, self.R, self.n, self.every, self.seed, self.dt = lib, G, R, len(mass1), every, seed, dt
        self.B, self.N = G * R, G * R * len(mass1)
        beta, table, up, down = HR.tables(kT, mass1, force_scale)
        self.tables_np = (beta, table, up, down)
        self.beta, self.table, self.up, self.down = _cu(beta), _cu(table), _cu(up), _cu(down)
        self.vel = vel.clone().contiguous()
        self.pos = torch.zeros_like(self.vel) if pos is None else pos.clone().contiguous()
        self.slot = torch.arange(R, dtype=torch.int32).repeat(G).cuda()
        self.holder = torch.arange(R, dtype=torch.int32).repeat(G, 1).cuda()
        self.sigma = self.table[self.slot.long()].reshape(-1).contiguous()
        mass_all = np.tile(np.asarray(mass1, np.float64), self.B)
        self.mass = _cu(mass_all.astype(np.float32))
        self.hk = _cu((0.5 * dt * force_scale / mass_all).astype(np.float32))
        self.c1 = math.exp(-friction * dt)
        self.c2 = math.sqrt(1.0 - self.c1 * self.c1)
        self.batch = torch.repeat_interleave(torch.arange(self.B), self.n).cuda()
        self.counters = torch.zeros((2, G, R - 1), dtype=torch.int64, device="cuda")
        nb = C.c_size_t(0)
        assert lib.tmdnet_md_workspace_bytes(self.N, self.B, C.byref(nb)) == 0
        self.ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        assert lib.tmdnet_md_exchange_workspace_bytes(self.B, R, C.byref(nb)) == 0
        self.ex_ws = torch.full((nb.value,), 255, dtype=torch.uint8, device="cuda")  # scratch: need not be cleared
        self.ekin = torch.full((self.B,), float("nan"), device="cuda")
        self.reset(0)

    @staticmethod
    def _s():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def reset(self, step):
        assert self.L.tmdnet_md_reset(self._s(), self._p(self.ws), step) == 0

    def advance(self, phase, forces, ekin=None):
        p = self._p
        rc = self.L.tmdnet_md_advance(None, self._s(), None, p(self.ws), self.N, self.B, phase, p(self.pos), p(self.vel), p(forces), None,
                                      p(self.hk), p(self.mass), p(self.sigma), self.dt, self.c1, self.c2, self.seed, p(self.batch), None, None,
                                      p(self.ekin if ekin is None else ekin))
        assert rc == 0, rc

    def exchange(self, epot, slot_log=None, accept_log=None, expect=0, **over):
        p = self._p
        a = dict(vel=self.vel, sigma=self.sigma, epot=epot, beta=self.beta, table=self.table, up=self.up, down=self.down, slot=self.slot,
                 holder=self.holder, counters=self.counters, ws=self.ws, ex_ws=self.ex_ws, N=self.N, B=self.B, R=self.R, every=self.every)
        a.update(over)
        rc = self.L.tmdnet_md_exchange(None, self._s(), None, p(a["ws"]), p(a["ex_ws"]), a["N"], a["B"], a["R"], a["every"], p(a["vel"]),
                                       p(a["sigma"]), p(a["epot"]), p(a["beta"]), p(a["table"]), p(a["up"]), p(a["down"]), self.seed,
                                       p(a["slot"]), p(a["holder"]), p(slot_log), p(accept_log), p(a["counters"]))
        assert rc == expect, rc

    def status(self):
        host = (C.c_uint64 * 2)()
        rc = self.L.tmdnet_md_status(self._s(), self._p(self.ws), host)
        return rc, int(host[0]), int(host[1])

    def mirror(self):
        m = HR.Ladders(self.G, self.R, self.tables_np[0], self.every, self.seed)
        m.slot[:], m.holder[:], m.counters[:] = _np(self.slot), _np(self.holder), _np(self.counters)
        return m


def _expect_atoms(raw, vel0, sigma0, slot0):
    """velocities and sigma after an attempt, from the slots before and after: one torch.mul per moved replica, table rows"""
    v, s = vel0.clone().view(raw.B, raw.n, 3), sigma0.clone().view(raw.B, raw.n)
    new, old = _np(raw.slot), _np(slot0)
    for b in range(raw.B):
        if new[b] != old[b]:
            f = raw.up[old[b]] if new[b] == old[b] + 1 else raw.down[new[b]]
            v[b] = torch.mul(v[b], f)
            s[b] = raw.table[new[b]]
    return v.view(-1, 3), s.view(-1)


@pytest.mark.parametrize("shape", [(2, 3, 5), (2, 2, 300)])
def test_raw_attempts_equal_the_host_mirror(hip_lib, shape):
    G, R, n = shape
    g = torch.Generator().manual_seed(5)
    mass1 = 1.0 + 15.0 * torch.rand(n, generator=g).double().numpy()
    mass1[2] = np.inf  # one atom of infinite mass: sigma 0, velocity 0
    kT = np.array([0.025, 0.04, 0.07])[:R]
    vel = 0.05 * torch.randn(G * R * n, 3, generator=g)
    vel.view(G * R, n, 3)[:, 2] = 0.0
    every = 4
    raw = _Raw(hip_lib, G, R, vel.cuda(), mass1, kT, every, 2 ** 40 + 3, force_scale=FS)
    assert (raw.table[:, 2] == 0).all()
    seen = set()
    # energies of a few kT: both outcomes occur; each parity, on the permutations left behind (R = 2: odd attempts have no pair)
    for a in ((1, 2, 3, 4) if R == 3 else (1, 2, 4, 6, 8)):
        epot = (0.3 * torch.rand(G * R, generator=g)).cuda()
        raw.reset(a * every)
        mir = raw.mirror()
        slot_m, acc_m = mir.attempt(a * every, _np(epot))
        ora = O.Ladders(G, R, raw.tables_np[0], every, raw.seed)  # (only to know that no decision is within 4 ulp of u)
        ora.holder = [list(h) for h in _np(raw.holder)]
        ora.slot = [list(h) for h in _np(raw.slot).reshape(G, R)]
        ora.attempt(a * every, _np(epot))
        assert ora.undecidable == []
        vel0, sigma0, slot0 = raw.vel.clone(), raw.sigma.clone(), raw.slot.clone()
        slot_log = torch.full((G * R,), -7, dtype=torch.int32, device="cuda")
        acc_log = torch.full((G, R - 1), 9, dtype=torch.uint8, device="cuda")
        raw.exchange(epot, slot_log, acc_log)
        assert raw.status() == (0, a * every, 0)
        print("attempt", a, "accepted", _np(acc_log).tolist(), "slots", _np(raw.slot).tolist())
        assert (_np(acc_log) == acc_m).all() and (_np(slot_log) == slot_m).all()
        assert (_np(raw.slot) == mir.slot).all() and (_np(raw.holder) == mir.holder).all() and (_np(raw.counters) == mir.counters).all()
        O.check_inverse(_np(raw.slot), _np(raw.holder), G, R)
        v_ref, s_ref = _expect_atoms(raw, vel0, sigma0, slot0)
        assert _bits(raw.vel, v_ref) and _bits(raw.sigma, s_ref)
        v_m, s_m = mir.atoms(a * every, _np(vel0), _np(sigma0), raw.tables_np[1], raw.tables_np[2], raw.tables_np[3])
        assert _bits(raw.vel, _cu(v_m)) and _bits(raw.sigma, _cu(s_m))
        assert (raw.vel.view(G * R, n, 3)[:, 2] == 0).all() and (raw.sigma.view(G * R, n)[:, 2] == 0).all()
        seen.update(_np(acc_log).reshape(-1)[[p + gg * (R - 1) for gg in range(G) for p in O.pairs(a, R)]].tolist())
    assert seen == {0, 1}  # accepted and rejected pairs both occurred


# ------------------------------------------------------------------------------------------------ 2. forced outcomes
def _small(hip_lib, seed=1):
    g = torch.Generator().manual_seed(9)
    mass1 = np.array([1.0, 12.0, np.inf, 16.0, 1.008])
    vel = 0.05 * torch.randn(30, 3, generator=g)
    vel.view(6, 5, 3)[:, 2] = 0.0
    return _Raw(hip_lib, 2, 3, vel.cuda(), mass1, np.array([0.025, 0.04, 0.07]), 4, seed, force_scale=FS)


@pytest.mark.parametrize("seed", [1, 2, 3, 2 ** 63 + 5])
def test_cold_slot_with_the_higher_energy_always_swaps(hip_lib, seed):
    raw = _small(hip_lib, seed)
    raw.reset(8)  # attempt 2: pairs (0, 1)
    epot = torch.tensor([2.0, 1.0, 0.0, 7.0, 7.0, -1.0], device="cuda")  # ladder 0: D > 0; ladder 1: equal energies, D = 0
    v0 = raw.vel.clone()
    acc = torch.full((2, 2), 9, dtype=torch.uint8, device="cuda")
    raw.exchange(epot, None, acc)
    assert _np(acc).tolist() == [[1, 0], [1, 0]] and _np(raw.slot).tolist() == [1, 0, 2, 1, 0, 2]
    assert _np(raw.holder).tolist() == [[1, 0, 2], [1, 0, 2]] and _np(raw.counters).tolist() == [[[1, 0], [1, 0]], [[1, 0], [1, 0]]]
    assert _bits(raw.vel.view(6, 5, 3)[0], torch.mul(v0.view(6, 5, 3)[0], raw.up[0]))
    assert _bits(raw.vel.view(6, 5, 3)[1], torch.mul(v0.view(6, 5, 3)[1], raw.down[0]))
    assert _bits(raw.vel.view(6, 5, 3)[2], v0.view(6, 5, 3)[2])


def test_nan_energies_reject_and_the_status_stays_zero(hip_lib):
    raw = _small(hip_lib)
    keep = [t.clone() for t in (raw.vel, raw.sigma, raw.slot, raw.holder)]
    for step, epot in ((8, [float("nan"), 1.0, 0.0, 5.0, float("nan"), 0.0]), (4, [0.0, float("nan"), 1.0, 0.0, float("inf"), float("inf")])):
        raw.reset(step)
        acc = torch.full((2, 2), 9, dtype=torch.uint8, device="cuda")
        raw.exchange(torch.tensor(epot, device="cuda"), None, acc)
        assert (acc == 0).all() and raw.status() == (0, step, 0)
    for t, k in zip((raw.vel, raw.sigma, raw.slot, raw.holder), keep):
        assert _bits(t, k) if t.dtype == torch.float32 else torch.equal(t, k)
    assert _np(raw.counters).tolist() == [[[1, 1], [1, 1]], [[0, 0], [0, 0]]]  # tried, never accepted


def test_a_frozen_state_exchanges_nothing(hip_lib):
    """The status word is set the way tests/test_gpu_md_barostat.py sets it without a fault - a NaN in the virial makes the barostat's
    move unusable, status 2 -; the overflow (status 1) needs a model: test_overflow_freezes_the_exchange.  Every output is poisoned
    beforehand and compared afterwards."""
    raw = _small(hip_lib)
    nb = C.c_size_t(0)
    assert hip_lib.tmdnet_md_barostat_workspace_bytes(raw.B, C.byref(nb)) == 0
    baro_ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    box = torch.eye(3, device="cuda").repeat(raw.B, 1, 1) * 10.0
    vir = torch.full((raw.B, 3, 3), float("nan"), device="cuda")
    zero = torch.zeros(raw.N, 3, device="cuda")
    raw.reset(7)
    raw.advance(CLOSE, zero)  # step 8 completes: attempt 2 would try the pairs (0, 1)
    p = raw._p
    rc = hip_lib.tmdnet_md_barostat(None, raw._s(), None, p(raw.ws), p(baro_ws), raw.N, raw.B, 0, p(raw.pos), p(raw.vel), None, None, raw.dt,
                                    p(raw.batch), p(box), 2, p(vir), p(raw.ekin), 0.0, 0.025, 1.0, 1.0, FS, 0, None, None, None)
    assert rc == 0 and raw.status() == (5, 8, 2)
    epot = torch.tensor([2.0, 1.0, 0.0, 7.0, 6.0, -1.0], device="cuda")  # would swap in both ladders
    slot_log = torch.full((6,), -7, dtype=torch.int32, device="cuda")
    acc_log = torch.full((2, 2), 9, dtype=torch.uint8, device="cuda")
    raw.counters.fill_(-3)
    keep = [t.clone() for t in (raw.vel, raw.sigma, raw.slot, raw.holder, raw.counters, slot_log, acc_log, raw.ex_ws)]
    raw.exchange(epot, slot_log, acc_log)
    for t, k in zip((raw.vel, raw.sigma, raw.slot, raw.holder, raw.counters, slot_log, acc_log, raw.ex_ws), keep):
        assert torch.equal(t.view(torch.uint8), k.view(torch.uint8))
    assert raw.status() == (5, 8, 2)
    raw.reset(8)  # cleared: the same call now swaps
    raw.counters.zero_()
    raw.exchange(epot, slot_log, acc_log)
    assert _np(acc_log).tolist() == [[1, 0], [1, 0]] and _np(slot_log).tolist() == [1, 0, 2, 1, 0, 2]


def test_raw_refusals(hip_lib):
    raw = _small(hip_lib)
    raw.reset(8)
    epot = torch.tensor([2.0, 1.0, 0.0, 7.0, 6.0, -1.0], device="cuda")
    keep = [t.clone() for t in (raw.vel, raw.sigma, raw.slot, raw.holder, raw.counters)]
    raw.exchange(epot, expect=1, R=1)
    raw.exchange(epot, expect=1, R=4)  # 6 replicas are no whole number of ladders of 4
    raw.exchange(epot, expect=1, N=31)
    raw.exchange(epot, expect=1, every=0)
    raw.exchange(None, expect=1)
    for name in ("vel", "sigma", "beta", "table", "up", "down", "slot", "holder", "ws", "ex_ws"):
        raw.exchange(epot, expect=1, **{name: None})
    torch.cuda.synchronize()
    for t, k in zip((raw.vel, raw.sigma, raw.slot, raw.holder, raw.counters), keep):
        assert torch.equal(t, k)
    raw.exchange(epot, counters=None)  # logs and counters are optional
    assert _np(raw.slot).tolist() == [1, 0, 2, 1, 0, 2] and raw.status() == (0, 8, 0)


# ------------------------------------------------------------------------------------------------ 3. canonical sampling
def run_sampling(hip_lib):
    """The protocol of tests/remd_oracle.py (SAMPLING) through the C entries, forces and energies by torch between the launches, ten
    attempts per captured graph.  -> raw, epot, ekin [attempts, R], slot_log [attempts, R], acc_log [attempts, R-1] (numpy)"""
    e = O.SAMPLING
    R, n, X, k = e["R"], e["n"], e["every"], e["k"]
    x0, v0 = O.sampling_state()
    raw = _Raw(hip_lib, 1, R, _cu(v0), np.ones(n), np.asarray(e["kT"]), X, e["seed"], dt=e["dt"], friction=e["friction"], pos=_cu(x0))
    P = 10
    assert e["attempts"] % P == 0
    f = torch.empty_like(raw.pos)
    rows = dict(epot=torch.zeros(P, R, device="cuda"), ekin=torch.zeros(P, R, device="cuda"),
                slot=torch.zeros(P, R, dtype=torch.int32, device="cuda"), acc=torch.zeros(P, R - 1, dtype=torch.uint8, device="cuda"))
    logs = {name: [] for name in rows}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.mul(raw.pos, -k, out=f)
        raw.advance(OPEN, f)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for p in range(P):
            for t in range(X):
                torch.mul(raw.pos, -k, out=f)
                if t + 1 < X:
                    raw.advance(CLOSE, f)
                else:
                    rows["epot"][p].copy_((0.5 * k) * torch.mul(raw.pos, raw.pos).view(R, -1).sum(1))
                    raw.advance(CLOSE, f, rows["ekin"][p])
                    raw.exchange(rows["epot"][p], rows["slot"][p], rows["acc"][p])
                raw.advance(OPEN, f)
    for _ in range(e["attempts"] // P):
        graph.replay()
        for name in rows:
            logs[name].append(rows[name].clone())
    assert raw.status() == (0, e["attempts"] * X, 0)
    return (raw,) + tuple(_np(torch.cat(logs[name])) for name in ("epot", "ekin", "slot", "acc"))


def test_harmonic_well_is_sampled_canonically_at_every_slot(hip_lib):
    """The protocol, the statistics and the bounds of tests/remd_oracle.py (SAMPLING: one ladder of 4 replicas of 10 atoms in an
    isotropic harmonic well, omega dt = 0.1, 2 000 attempts 60 steps apart), which tests/test_remd_host.py runs on the host mirror."""
    e = O.SAMPLING
    R, n, X = e["R"], e["n"], e["every"]
    raw, epot, ekin, slot_log, acc_log = run_sampling(hip_lib)
    stats = O.sampling_statistics(epot, ekin, slot_log, acc_log.reshape(-1, 1, R - 1), e["kT"], n)
    for name in ("epot", "ekin", "acceptance"):
        for row in stats[name]:
            print(name, row)
    O.assert_sampling(stats)
    O.check_inverse(_np(raw.slot), _np(raw.holder), 1, R)
    assert _np(raw.counters)[0, 0].tolist() == [e["attempts"] // 2] * (R - 1)
    assert (_np(raw.counters)[1, 0] == acc_log.sum(0)).all()
    # the first 200 decisions are the mirror's on the device's own energies
    mir = HR.Ladders(1, R, 1.0 / np.asarray(e["kT"]), X, e["seed"])
    ora = O.Ladders(1, R, 1.0 / np.asarray(e["kT"]), X, e["seed"])
    for a in range(200):
        slot_m, acc_m = mir.attempt((a + 1) * X, epot[a])
        ora.attempt((a + 1) * X, epot[a])
        assert (slot_m == slot_log[a]).all() and (acc_m.reshape(-1) == acc_log[a]).all(), a
    assert ora.undecidable == []


# ------------------------------------------------------------------------------------------------ 4. through the model
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


G_, R_, DT = 2, 3, 0.05


def _system(arch):
    """one 20-atom molecule, G = 2 ladders of R = 3 replicas: the same molecule displaced a little, replica by replica"""
    z, pos, _ = W.synthetic_batch(n_mol=1, n_atoms=20)
    g = torch.Generator().manual_seed(12)
    pos = pos[None, None] + 0.05 * torch.randn(G_, R_, 20, 3, generator=g)
    vel = 0.01 * torch.randn(G_, R_, 20, 3, generator=g)
    mass = torch.where(z == 1, 1.008, 12.0).float()
    q = None if arch == "equivariant-transformer" else torch.zeros(G_, device="cuda")
    return z.cuda(), pos.cuda(), vel.cuda(), mass.cuda(), q


def _ladder_for(model, z, pos, q, spread):
    """kT[s] = T0 * 1.5^s with T0 = spread * the largest energy difference between two replicas at the start: `spread` large makes
    every D tiny (swaps all but certain), `spread` of order one gives both outcomes.  force_scale keeps sigma at 0.01 for kT = T0."""
    n = z.shape[0]
    B = G_ * R_
    batch = torch.repeat_interleave(torch.arange(B, device="cuda"), n)
    qq = None if q is None else torch.repeat_interleave(q, R_)
    E = model(z.repeat(B), pos.reshape(-1, 3), batch, q=qq)[0].reshape(-1)
    dE = float((E.max() - E.min()).abs().detach())
    T0 = spread * max(dE, 1e-6)
    return [T0, 1.5 * T0, 2.25 * T0], 1e-4 / T0


def _mirror_check(md, K, X, replays, seed, logs):
    """the logged decisions equal the host mirror's on the device's own logged epot; -> number of accepted swaps"""
    mir = HR.Ladders(G_, R_, 1.0 / _np(md.temperatures), X, seed)
    ora = O.Ladders(G_, R_, 1.0 / _np(md.temperatures), X, seed)
    accepted, step = 0, 0
    for r in range(replays):
        epot, slot_log, acc_log = logs[r]
        for a in range(K // X):
            step += X
            row = _np(epot[(a + 1) * X - 1])
            slot_m, acc_m = mir.attempt(step, row)
            before = len(ora.undecidable)
            ora.attempt(step, row)
            assert len(ora.undecidable) == before  # (a decision within 4 ulp of u: not seen with these seeds)
            assert (slot_m == _np(slot_log[a])).all() and (acc_m == _np(acc_log[a])).all(), (r, a)
            accepted += int(acc_m.sum())
    assert (mir.counters == _np(md._counters)).all()
    return accepted


def test_equal_temperatures_are_capture_md_bit_for_bit(hip_lib):
    model = _model("tensornet")
    z, pos, vel, mass, q = _system("tensornet")
    n, B, K = z.shape[0], G_ * R_, 4
    kT, seed = 0.02, 2 ** 40 + 5
    batch = torch.repeat_interleave(torch.arange(B, device="cuda"), n)
    ref = model.capture_md(z.repeat(B), pos.reshape(-1, 3), vel.reshape(-1, 3), mass.repeat(B), DT, batch=batch,
                           q=torch.repeat_interleave(q, R_), steps_per_replay=K, thermostat=dict(friction=2.0, kT=kT, seed=seed))
    ref(2)
    assert ref.check() == 8
    for X in (2, 0):
        md = model.capture_remd(z, pos, vel, mass, DT, temperatures=[kT] * R_, exchange_every=X, q=q, steps_per_replay=K,
                                thermostat=dict(friction=2.0, seed=seed))
        assert _bits(md.sigma, ref.sigma)
        md(2)
        assert md.check() == 8 == md.steps_done
        for name in ("pos", "vel", "forces", "epot", "ekin", "sigma"):
            assert _bits(getattr(md, name), getattr(ref, name)), (X, name)
        if X:  # D = 0: every attempt is accepted; only the slots differ
            assert md.slot_log.shape == (2, B) and md.accepted.shape == (2, G_, R_ - 1)
            assert _np(md.accepted).tolist() == [[[0, 1], [0, 1]], [[1, 0], [1, 0]]]  # attempts 3 (pairs (1,2)) and 4 (pairs (0,1))
            assert _np(md.attempts).tolist() == [[2, 2], [2, 2]] == _np(md.accepts).tolist() and (md.acceptance() == 1).all()
            assert not torch.equal(md.slot, torch.arange(R_, dtype=torch.int32, device="cuda").repeat(G_))
            O.check_inverse(_np(md.slot), _np(md.holder), G_, R_)
            assert _bits(md.by_slot(md.pos)[:, 0], md.pos.view(B, n, 3)[(torch.arange(G_, device="cuda") * R_ + md.holder[:, 0].long())])
            assert md.by_slot(md.epot[-1]).shape == (G_, R_)
        else:
            assert md.slot_log.shape == (0, B) and _np(md.attempts).sum() == 0
            assert torch.equal(md.slot, torch.arange(R_, dtype=torch.int32, device="cuda").repeat(G_))


def test_a_real_ladder_decides_as_the_mirror_and_continues_as_plain_md(hip_lib):
    model = _model("tensornet")
    z, pos, vel, mass, q = _system("tensornet")
    n, B = z.shape[0], G_ * R_
    seed = 2 ** 40 + 7
    th = dict(friction=2.0, seed=seed)
    # (a) temperatures of the order of the energy differences: decisions against the mirror, over six replays
    kT, fs = _ladder_for(model, z, pos, q, spread=1.0)
    md = model.capture_remd(z, pos, vel, mass, DT, temperatures=kT, exchange_every=2, q=q, steps_per_replay=4, force_scale=fs, thermostat=th)
    assert _bits(md.sigma.view(B, n), md.sigma_table[md.slot.long()])
    logs = []
    for _ in range(6):
        md()
        logs.append((md.epot.clone(), md.slot_log.clone(), md.accepted.clone()))
    assert md.check() == 24
    accepted = _mirror_check(md, 4, 2, 6, seed, logs)
    print("accepted", accepted, "of", int(_np(md.attempts).sum()), "acceptance", md.acceptance().tolist())
    assert _bits(md.sigma.view(B, n), md.sigma_table[md.slot.long()])
    O.check_inverse(_np(md.slot), _np(md.holder), G_, R_)
    # (b) a wide ladder (every D tiny: the swap of attempt 1 is all but certain), K = X = 2: after the first replay the pairs (1, 2)
    # have swapped; the second replay is bit for bit plain multi-temperature MD from that state
    kT, fs = _ladder_for(model, z, pos, q, spread=1000.0)
    a = model.capture_remd(z, pos, vel, mass, DT, temperatures=kT, exchange_every=2, q=q, steps_per_replay=2, force_scale=fs, thermostat=th)
    a()
    assert _np(a.accepted).tolist() == [[[0, 1], [0, 1]]] and _np(a.slot).tolist() == [0, 2, 1, 0, 2, 1]
    pos1, vel1, slot1 = a.pos.clone(), a.vel.clone(), a.slot.clone()
    v_in = vel.reshape(B, n, 3)
    assert not _bits(vel1.view(B, n, 3)[1], v_in[1])
    a()
    assert a.check() == 4
    b = model.capture_remd(z, pos, vel, mass, DT, temperatures=kT, exchange_every=0, q=q, steps_per_replay=2, force_scale=fs, thermostat=th)
    b.reset(pos=pos1, vel=vel1, step=2, slots=slot1)
    assert torch.equal(b.slot, slot1) and _bits(b.sigma, b.sigma_table[slot1.long()].reshape(-1))
    b()
    assert b.check() == 4
    assert _bits(a.pos, b.pos) and _bits(a.epot, b.epot) and _bits(a.ekin, b.ekin) and _bits(a.forces, b.forces)
    # a's second attempt (attempt 2, pairs (0, 1)) scaled the velocities of the replicas it moved, after the step
    v_ref = b.vel.clone().view(B, n, 3)
    new, old = _np(a.slot), _np(slot1)
    for r in range(B):
        if new[r] != old[r]:
            v_ref[r] = torch.mul(v_ref[r], a._up[old[r]] if new[r] == old[r] + 1 else a._down[new[r]])
    assert _bits(a.vel, v_ref.view(-1, 3))
    # repeats are bit-identical
    a.reset(pos=pos, vel=vel, step=0, slots=torch.arange(R_).repeat(G_))
    assert _np(a.attempts).sum() == 0
    a()
    assert _bits(a.pos, pos1) and _bits(a.vel, vel1) and torch.equal(a.slot, slot1)


def test_overflow_freezes_the_exchange(hip_lib):
    """The case of tests/test_gpu_md_loop.py::test_overflow_freezes_the_state_at_the_last_valid_step with two replicas of the
    192-atom water box in one ladder, an attempt after every step: box and positions scaled by 0.85 between two replays."""
    model = _model("tensornet", max_num_neighbors=72)
    z, pos, box = (t.cuda() for t in W.water_box(n_side=4))
    mass = torch.where(z == 1, 1.008, 12.0).float()
    pos2 = torch.stack([pos, pos])
    md = model.capture_remd(z, pos2, None, mass, 0.01, temperatures=[0.02, 0.03], exchange_every=1, box=box, q=torch.zeros(1, device="cuda"),
                            steps_per_replay=2, thermostat=dict(friction=1.0, seed=3))
    assert md.vel.shape == (384, 3) and float(md.vel.abs().max()) > 0
    md()
    assert md.check() == 2 and _np(md.attempts).tolist() == [[1]]  # attempt 1 has no pair with R = 2, attempt 2 has one
    md.box.mul_(0.85)
    md.pos.mul_(0.85)
    md.slot_log.fill_(-7)
    md.accepted.fill_(9)
    md._counters.fill_(-3)
    state = (md.pos, md.vel, md.forces, md.sigma, md.slot, md.holder, md.slot_log, md.accepted, md._counters, md.epot, md.ekin)
    keep = [t.clone() for t in state]
    for _ in range(2):  # the overflowing replay and one more
        md()
        with pytest.raises(RuntimeError, match="max_num_pairs"):
            md.check()
        for t, k in zip(state, keep):
            assert torch.equal(t.view(torch.uint8), k.view(torch.uint8))
    md.box.mul_(1.0 / 0.85)
    md.reset(pos=pos2, vel=None)
    md()
    assert md.check() == 2 and _np(md.attempts).tolist() == [[1]]


def test_refusals(hip_lib):
    model = _model("tensornet")
    z, pos, vel, mass, q = _system("tensornet")
    th = dict(friction=2.0, seed=1)
    ok = dict(temperatures=[0.02, 0.03, 0.04], exchange_every=2, q=q, steps_per_replay=4, thermostat=th)
    for over in (dict(steps_per_replay=5), dict(thermostat=dict(th, kT=0.02)), dict(barostat=dict(pressure=0.0, tau=1.0, compressibility=1.0)),
                 dict(constraints=dict(pairs=torch.tensor([[0, 1]]))), dict(thermostat=None), dict(temperatures=[0.02, 0.03]),
                 dict(atom_weights=torch.ones(20)), dict(halo_exchange=object())):
        with pytest.raises(ValueError):
            model.capture_remd(z, pos, vel, mass, DT, **dict(ok, **over))
    with pytest.raises(ValueError, match="temperatures"):
        model.capture_remd(z, pos, vel, mass, DT, **dict(ok, thermostat=dict(th, kT=0.02)))
    for bad in (pos.reshape(-1, 3), pos[:, :2], pos[0, 0]):
        with pytest.raises(ValueError):
            model.capture_remd(z, bad, None, mass, DT, **ok)
    md = model.capture_remd(z, pos, vel, mass, DT, **ok)
    slot0 = md.slot.clone()
    for bad in ([0, 1, 1, 0, 1, 2], [0, 1, 3, 0, 1, 2], [0, 1, 2], [[0, 1, 2], [2, 2, 0]]):
        with pytest.raises(ValueError):
            md.reset(slots=torch.tensor(bad))
    assert torch.equal(md.slot, slot0)
    md.reset(slots=torch.tensor([[2, 0, 1], [0, 2, 1]]))
    assert _np(md.holder).tolist() == [[1, 2, 0], [0, 2, 1]] and _bits(md.sigma, md.sigma_table[md.slot.long()].reshape(-1))
    md()
    assert md.check() == 4


# ------------------------------------------------------------------------------------------------ 5. the other architectures
@pytest.mark.parametrize("arch", ["equivariant-transformer", "tensornet2"])
def test_other_architectures_decide_as_the_mirror(hip_lib, arch):
    model = _model(arch)
    z, pos, vel, mass, q = _system(arch)
    seed = 2 ** 40 + 9
    kT, fs = _ladder_for(model, z, pos, q, spread=1.0)
    md = model.capture_remd(z, pos, vel, mass, DT, temperatures=kT, exchange_every=2, q=q, steps_per_replay=4, force_scale=fs,
                            thermostat=dict(friction=2.0, seed=seed))
    logs = []
    for _ in range(3):
        md()
        logs.append((md.epot.clone(), md.slot_log.clone(), md.accepted.clone()))
    assert md.check() == 12 == md.steps_done
    _mirror_check(md, 4, 2, 3, seed, logs)
    O.check_inverse(_np(md.slot), _np(md.holder), G_, R_)
    assert torch.isfinite(md.pos).all() and torch.isfinite(md.epot).all()
