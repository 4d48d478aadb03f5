"""-m gpu: collective-variable restraints and metadynamics in the device-resident MD loop (csrc/tn_bias.hip: k_md_bias;
TorchMD_Net.capture_md_biased).

1. the raw entries on a synthetic force buffer, no model: tmdnet_md_bias against the host mirror (tests/md_bias_host_mirror.py) - slots,
   untouched atoms, values within the recorded fp64 bound, bit-identical repeats, the frozen state, status 4, the capacity edge
2. through the model (TensorNet, Equivariant Transformer, TensorNet2 on the ragged batch of tests/test_gpu_md_loop.py): bit-identical to
   capture() plus a torch mirror that adds the device's own fp32 bias forces, for every K; zero bias is capture_md; NVE conservation
   with a restraint; reset(hills=); overflow; status 4; refusals
Recorded figures: profiles/md_bias.json, section "gpu" (the device may contract fp64 products, so it differs from the host mirror in
the last places; a bound is ten times the recorded deviation)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import md_bias_host_mirror as HM
from tests import md_bias_oracle as O
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

OPEN, MIDDLE, CLOSE = 0, 1, 2
REC = O.recorded().get("gpu", {})


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _np(t):
    return t.detach().cpu().numpy()


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the raw entries
RAW_CVS = [("distance", 0, 1), ("angle", 1, 2, 3), ("torsion", 3, 4, 5, 6), ("distance", 9, 6)]  # atoms 1, 3 and 6 are shared
RAW_METAD = dict(cvs=[2, 0], sigma=[0.4, 0.15], height=0.6, pace=4, kT=0.8, bias_factor=5.0)


def _raw_positions(rng, B, n1=12):
    """B walkers of n1 atoms along a jittered helix: no CV of RAW_CVS comes near a degenerate geometry"""
    k = np.arange(n1)
    base = np.stack([1.2 * np.cos(1.1 * k), 1.2 * np.sin(1.1 * k), 0.6 * k], 1)
    return (base[None] + 0.12 * rng.standard_normal((B, n1, 3)) + 4.0 * rng.standard_normal((B, 1, 3))).astype(np.float32).reshape(-1, 3)


class _Raw:
    """tmdnet_md_bias on tensors of the test's own, graph_ws = NULL (no model), next to the host mirror on the same tables."""

    def __init__(self, lib, B=6, n1=12, cvs=RAW_CVS, restraints=((0, "harmonic"), (1, "upper"), (2, "lower")), metad=RAW_METAD, Wg=3, H=40,
                 step0=0, base=0, seed=1):
        rng = np.random.default_rng(seed)
        self.L, self.B, self.n1, self.N, self.H, self.Wg = lib, B, n1, B * n1, H, Wg
        D = len(cvs)
        kappa, center = rng.uniform(2.0, 6.0, (B, D)), np.zeros((B, D))
        center[:, 0], center[:, 1], center[:, 2] = 1.2, 1.0, rng.uniform(-3.0, 3.0, B)  # the one-sided kinds are active for some walkers
        self.mir = HM.Walkers(B, n1, cvs, restraints, kappa, center, metad, W=Wg, H=H, step0=step0, base=base)
        m = self.mir
        self.tab = [_cu(a) for a in (m.kinds, m.atoms, m.start, m.distinct, m.offsets, m.entries, m.res_kind, m.kappa, m.center)]
        nb = C.c_size_t(0)
        assert lib.tmdnet_md_workspace_bytes(self.N, B, C.byref(nb)) == 0
        self.ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        assert lib.tmdnet_md_bias_workspace_bytes(B, D, m.dm, Wg, H, C.byref(nb)) == 0
        self.bias_ws = torch.full((nb.value,), 255, dtype=torch.uint8, device="cuda")  # all-ones doubles are NaN: unwritten slots show
        self.step0, self.base = step0, base
        self.zero = torch.zeros(self.N, 3, device="cuda")
        self.vel = torch.zeros(self.N, 3, device="cuda")
        self.x = torch.zeros(self.N, 3, device="cuda")
        self.mass = torch.ones(self.N, device="cuda")
        self.hk = torch.zeros(self.N, device="cuda")
        self.batch = torch.repeat_interleave(torch.arange(B), n1).cuda()
        self.reset(step0)

    @staticmethod
    def _s():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def reset(self, step):
        assert self.L.tmdnet_md_reset(self._s(), self._p(self.ws), step) == 0
        assert self.L.tmdnet_md_bias_reset(self._s(), self._p(self.bias_ws), self.step0, self.base) == 0

    def store(self):
        """[G, dm + 1, H] float64 view of the hills"""
        m = self.mir
        off = (-self.bias_ws.data_ptr()) % 256 + 256
        n = (self.B // self.Wg) * (m.dm + 1) * self.H
        return self.bias_ws[off:off + 8 * n].view(torch.float64).view(self.B // self.Wg, m.dm + 1, self.H)

    def launch(self, pos, forces, deposit=1, expect=0, **over):
        """-> dict like the mirror's launch, from the device; `forces` is updated in place"""
        m, p = self.mir, self._p
        cv = torch.full((self.B, m.D), float("nan"), dtype=torch.float64, device="cuda")
        er, eb = (torch.full((self.B,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
        fl = torch.full((self.B, m.A, 3), float("nan"), device="cuda")
        mc = m.mcv + [0, 0]
        a = dict(ws=self.ws, bias_ws=self.bias_ws, N=self.N, B=self.B, D=m.D, A=m.A, dm=m.dm, W=self.Wg, H=self.H, pace=m.pace, pos=pos,
                 forces=forces, sigma0=m.sigma[0], gamma=m.gamma)
        a.update(over)
        t = self.tab
        rc = self.L.tmdnet_md_bias(None, self._s(), None, p(a["ws"]), p(a["bias_ws"]), a["N"], a["B"], deposit, p(a["pos"]), p(a["forces"]),
                                   a["D"], p(t[0]), p(t[1]), p(t[2]), a["A"], p(t[3]), p(t[4]), p(t[5]), p(t[6]), p(t[7]), p(t[8]), a["dm"],
                                   mc[0], mc[1], a["sigma0"], m.sigma[1], m.h0, m.kT, a["gamma"], a["pace"], a["W"], a["H"], p(cv), p(er), p(eb),
                                   p(fl))
        assert rc == expect, rc
        return dict(forces=forces, cv=cv, restraint=er, bias=eb, bias_forces=fl)

    def close_step(self):
        """the closing launch on zero forces and velocities: only the step counter moves"""
        p = self._p
        rc = self.L.tmdnet_md_advance(None, self._s(), None, p(self.ws), self.N, self.B, CLOSE, p(self.x), p(self.vel), p(self.zero), None,
                                      p(self.hk), p(self.mass), None, 0.1, 1.0, 0.0, 0, p(self.batch), None, None, None)
        assert rc == 0, rc

    def status(self):
        host = (C.c_uint64 * 2)()
        rc = self.L.tmdnet_md_status(self._s(), self._p(self.ws), host)
        return rc, int(host[0]), int(host[1])


def run_raw(lib, steps=40, seed=1):
    """40 steps, pace 4, W = 3, dm = 2 on the device and on the mirror -> (raw, per-step device outputs, per-step mirror outputs)"""
    raw = _Raw(lib, seed=seed)
    rng = np.random.default_rng(100 + seed)
    dev, mir = [], []
    for n in range(steps):
        pos = _raw_positions(rng, raw.B)
        f0 = rng.standard_normal((raw.N, 3)).astype(np.float32)
        out = raw.launch(_cu(pos), _cu(f0))
        dev.append({k: _np(v) for k, v in out.items()})
        mir.append(dict(raw.mir.launch(n, pos, f0), f0=f0))
        raw.close_step()
    assert raw.status() == (0, steps, 0) and raw.mir.status[0] == 0
    return raw, dev, mir


def raw_deviations(raw, dev, mir):
    """largest relative deviations device - mirror: fp64 values (CVs, energies, hills) and the fp32 forces in units of their ulp"""
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))
    v = max(max(rel(d[k], m[k]) for k in ("cv", "restraint", "bias")) for d, m in zip(dev, mir))
    hills, want = _np(raw.store()), raw.mir.hills
    ok = ~np.isnan(want)
    v = max(v, rel(hills[ok], want[ok]))
    ulp = max(float(np.max(np.abs(d["bias_forces"].astype(np.float64) - m["bias_forces"]) / np.spacing(np.abs(m["bias_forces"])))) for d, m in zip(dev, mir))
    return v, ulp


def test_raw_launches_equal_the_host_mirror(hip_lib):
    raw, dev, mir = run_raw(hip_lib)
    hills, want = _np(raw.store()), raw.mir.hills
    assert (np.isnan(hills) == np.isnan(want)).all() and (~np.isnan(want)).sum() == 2 * 3 * 30  # the same slots: 10 deposits of 3 walkers
    named = np.zeros(raw.N, bool)
    named[_np(raw.tab[2])[:, None] + _np(raw.tab[3])[None, :]] = True
    for d, m in zip(dev, mir):
        assert (d["forces"][~named].view(np.uint32) == m["f0"][~named].view(np.uint32)).all()  # atoms in no CV keep their bits
        assert (d["forces"][named] != m["f0"][named]).any()
        # the force buffer is the logged fp32 bias force added once
        assert (d["forces"][named].reshape(raw.B, -1, 3) == m["f0"][named].reshape(raw.B, -1, 3) + d["bias_forces"]).all()
    v, ulp = raw_deviations(raw, dev, mir)
    print("fp64 values: largest relative deviation", v, "recorded", REC.get("raw_value_rel_dev"), "; fp32 forces: ulp", ulp)
    assert v <= 10.0 * max(REC["raw_value_rel_dev"], 2.0 ** -52)
    assert ulp <= 1.0  # fp64 sums that agree to 1e-13 round to the same fp32 value or to its neighbour
    assert max(float(np.abs(d["bias"]).max()) for d in dev) > 0.1  # the hills are felt


def test_repeat_launches_are_bit_identical(hip_lib):
    a = run_raw(hip_lib, seed=2)
    b = run_raw(hip_lib, seed=2)
    for da, db in zip(a[1], b[1]):
        for k in da:
            assert da[k].tobytes() == db[k].tobytes(), k
    assert _bits(a[0].store(), b[0].store())
    # the same launch again on the same state (deposit off: nothing is written but the outputs)
    raw = a[0]
    pos, f = _cu(_raw_positions(np.random.default_rng(0), raw.B)), torch.ones(raw.N, 3, device="cuda")
    outs = [raw.launch(pos, f.clone(), deposit=0) for _ in range(3)]
    for o in outs[1:]:
        assert all(_bits(o[k], outs[0][k]) for k in o)


def test_a_frozen_state_writes_nothing(hip_lib):
    """The status word is set the way tests/test_gpu_md_barostat.py sets it without a fault - a NaN in the virial makes the barostat's
    move unusable, status 2 -; the overflow flag counts[2] needs a model: test_overflow_freezes_the_bias."""
    raw = _Raw(hip_lib)
    nb = C.c_size_t(0)
    assert hip_lib.tmdnet_md_barostat_workspace_bytes(raw.B, C.byref(nb)) == 0
    baro_ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
    box = torch.eye(3, device="cuda").repeat(raw.B, 1, 1) * 10.0
    vir = torch.full((raw.B, 3, 3), float("nan"), device="cuda")
    ekin = torch.zeros(raw.B, device="cuda")
    for _ in range(3):
        raw.close_step()  # n = 3: the launch below would deposit
    p = raw._p
    rc = hip_lib.tmdnet_md_barostat(None, raw._s(), None, p(raw.ws), p(baro_ws), raw.N, raw.B, 0, p(raw.x), p(raw.vel), None, None, 0.1,
                                    p(raw.batch), p(box), 2, p(vir), p(ekin), 0.0, 0.025, 1.0, 1.0, 1.0, 0, None, None, None)
    assert rc == 0 and raw.status() == (5, 3, 2)
    pos = _cu(_raw_positions(np.random.default_rng(3), raw.B))
    f = torch.ones(raw.N, 3, device="cuda")
    keep = raw.bias_ws.clone()
    out = raw.launch(pos, f)
    assert (f == 1).all() and all(torch.isnan(out[k]).all() for k in ("cv", "restraint", "bias", "bias_forces")) and _bits(raw.bias_ws, keep)
    assert raw.status() == (5, 3, 2)
    raw.reset(3)  # cleared: the same call now works and deposits
    out = raw.launch(pos, f)
    assert not (f == 1).all() and not torch.isnan(out["cv"]).any() and not _bits(raw.bias_ws, keep)
    assert int((~torch.isnan(raw.store())).sum()) == 2 * 3 * 3


def test_a_non_finite_cv_gives_status_4(hip_lib):
    raw = _Raw(hip_lib)
    rng = np.random.default_rng(4)
    for _ in range(3):
        raw.close_step()
    pos = _raw_positions(rng, raw.B)
    pos[4 * 12 + 1] = pos[4 * 12 + 0]  # walker 4: the distance CV's atoms coincide
    pos[2 * 12 + 1:2 * 12 + 4] = np.array([[1, 0, 0], [2, 0, 0], [3, 0, 0]], np.float32) + pos[2 * 12]  # walker 2: a collinear angle
    f0 = rng.standard_normal((raw.N, 3)).astype(np.float32)
    f = _cu(f0)
    out = raw.launch(_cu(pos), f)
    assert raw.status() == (5, 3, 4)
    fd = _np(f)
    for b in (2, 4):
        rows = slice(b * 12, b * 12 + 12)
        assert (fd[rows].view(np.uint32) == f0[rows].view(np.uint32)).all()  # its forces keep their bits
        assert torch.isnan(out["cv"][b]).all() and torch.isnan(out["bias_forces"][b]).all()  # no log row
        assert torch.isnan(raw.store()[b // 3, :, b % 3]).all()  # and no hill in its slot
    assert np.isfinite(fd).all()
    keep, fk = raw.bias_ws.clone(), f.clone()
    raw.close_step()  # the closing launch returns at once: the counter stays
    raw.launch(_cu(_raw_positions(rng, raw.B)), f)  # and so does the next bias launch
    assert raw.status() == (5, 3, 4) and _bits(f, fk) and _bits(raw.bias_ws, keep)


def test_the_capacity_edge(hip_lib):
    """H = 7, hill_base = 2, W = 3, pace 2 from step0 = 4: the deposit after step 6 fills slots 2..4, the one after step 8 slots 5 and 6
    and drops walker 2's, later ones write nothing; no byte of the workspace outside the hills changes"""
    raw = _Raw(hip_lib, metad=dict(RAW_METAD, pace=2), H=7, step0=4, base=2, seed=5)
    raw.store()[:, :, :2] = 0.4
    raw.mir.hills[:, :, :2] = 0.4
    rng = np.random.default_rng(6)
    before = raw.bias_ws.clone()
    for n in range(4, 14):
        pos = _raw_positions(rng, raw.B)
        f0 = rng.standard_normal((raw.N, 3)).astype(np.float32)
        out = raw.launch(_cu(pos), _cu(f0))
        m = raw.mir.launch(n, pos, f0)
        assert np.abs(_np(out["bias"]) - m["bias"]).max() <= 1e-12 * max(1.0, np.abs(m["bias"]).max())
        raw.close_step()
    hills, want = _np(raw.store()), raw.mir.hills
    assert not np.isnan(want).any() and not np.isnan(hills).any() and np.abs(hills - want).max() < 1e-12
    off = (-raw.bias_ws.data_ptr()) % 256 + 256
    end = off + 8 * 2 * 3 * 7
    assert _bits(raw.bias_ws[:off], before[:off]) and _bits(raw.bias_ws[end:], before[end:])  # header and slack keep their bytes
    assert raw.status() == (0, 14, 0)


# ------------------------------------------------------------------------------------------------ 2. through the model
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


ARCHS = ["tensornet", "equivariant-transformer", "tensornet2"]
CVS = [("distance", 0, 3), ("angle", 1, 3, 5), ("torsion", 2, 3, 4, 6)]  # atom 3 is in every CV


def _setup(arch):
    """the ragged batch of tests/test_gpu_md_loop.py: molecules of 7, 12 and 20 atoms"""
    model = _model(arch)
    zs, ps, bs = [], [], []
    for m, n in enumerate([7, 12, 20]):
        z, p = W.synthetic_molecule(40 + m, n)
        zs.append(torch.from_numpy(z))
        ps.append(torch.from_numpy(p) + 3.0 * m)
        bs.append(torch.full((n,), m, dtype=torch.long))
    z, pos, batch = torch.cat(zs).cuda(), torch.cat(ps).cuda(), torch.cat(bs).cuda()
    q = torch.zeros(3, device="cuda") if arch != "equivariant-transformer" else None
    vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    mass = torch.where(z == 1, 1.008, 12.0).float().cuda()
    replay = model.capture(z, pos, batch, None, q=q)
    _, f0 = replay(pos)
    dt = min(0.05, 0.02 * (12.0 / max(float(f0.abs().max()), 1e-6)) ** 0.5)  # the dt rule of tests/test_gpu_md.py
    return model, replay, (z, pos, batch, None, q), vel, mass, dt


def _bias(model, inputs, scale=1.0, **over):
    """restraints of every kind around the start values and 2-D metadynamics shared by the three walkers; energies in units of the
    model's own force scale so that the bias matters and the step stays stable"""
    z, pos, batch, _, q = inputs
    f = float(model(z, pos, batch, q=q)[1].abs().max())
    x = _np(pos).reshape(-1, 3)
    start = [0, 7, 19]
    s0 = np.array([[O.cv(c[0], x[[st + i for i in c[1:]] + [0] * (5 - len(c))])[0] for c in CVS] for st in start])
    b = dict(cvs=CVS,
             restraints=[dict(cv=0, kind="harmonic", kappa=scale * f, center=(s0[:, 0] + 0.1).tolist()),
                         dict(cv=1, kind="upper", kappa=scale * 0.5 * f, center=(s0[:, 1] - 0.1).tolist()),
                         dict(cv=2, kind="lower", kappa=scale * 0.2 * f, center=(s0[:, 2] + 0.2).tolist())],
             metad=dict(cvs=[2, 0], sigma=[0.3, 0.1], height=scale * 0.05 * f, pace=4, kT=0.1 * f, bias_factor=6.0, walkers_per_group=3,
                        capacity=64),
             log_forces=True)
    b.update(over)
    return b


def _capture(model, inputs, vel, mass, dt, K, bias, **kw):
    z, pos, batch, box, q = inputs
    return model.capture_md_biased(z, pos, vel, mass, dt, batch=batch, box=box, q=q, steps_per_replay=K, bias=bias, **kw)


@pytest.mark.parametrize("arch", ARCHS)
def test_biased_nve_is_bit_identical_to_capture_plus_torch_mirror(hip_lib, arch):
    model, replay, inputs, vel, mass, dt = _setup(arch)
    pos = inputs[1]
    bias = _bias(model, inputs)
    md = _capture(model, inputs, vel, mass, dt, 16, bias)
    idx = md.bias_atoms.reshape(-1)
    _, fm = replay(pos)
    f = fm.clone()
    f[idx] = torch.add(fm[idx], md.start_bias_forces.reshape(-1, 3))
    assert _bits(md.forces, f) and float(md.start_bias_forces.abs().max()) > 0  # the start forces are the total forces
    md()
    assert md.check() == 16 == md.steps_done and md.n_hills == 12
    logs = [t.clone() for t in (md.bias_forces, md.cv, md.restraint_energy, md.bias_energy, md.epot, md.ekin)]
    assert float(md.bias_energy[-1].abs().max()) > 0 and float(md.restraint_energy.abs().max()) > 0
    # the mirror: capture() for the model's force, the device's fp32 bias force added with torch.add, torch.mul / torch.add steps
    hk = (0.5 * dt / mass.double()).float()[:, None]
    dt_t = torch.tensor(dt, dtype=torch.float32, device="cuda")
    p, v = pos.clone(), vel.clone()
    for k in range(16):
        v = torch.add(v, torch.mul(hk, f))
        p = torch.add(p, torch.mul(dt_t, v))
        e, fm = replay(p)
        assert _bits(e.view(-1), logs[4][k])
        f = fm.clone()
        f[idx] = torch.add(fm[idx], logs[0][k].reshape(-1, 3))
        v = torch.add(v, torch.mul(hk, f))
    assert (p - pos).abs().max().item() > 4 * dt * 0.02  # the atoms really moved
    assert _bits(md.pos, p) and _bits(md.vel, v) and _bits(md.forces, f)
    hills = md.hills()
    for K in (1, 8):
        md2 = _capture(model, inputs, vel, mass, dt, K, bias)
        got = [[] for _ in logs]
        for _ in range(16 // K):
            md2()
            for g, t in zip(got, (md2.bias_forces, md2.cv, md2.restraint_energy, md2.bias_energy, md2.epot, md2.ekin)):
                g.append(t.clone())
        assert md2.check() == 16 and _bits(md2.pos, p) and _bits(md2.vel, v) and _bits(md2.forces, f), K
        for g, want in zip(got, logs):
            assert _bits(torch.cat(g), want), K
        assert all(_bits(a, b) for a, b in zip(md2.hills(), hills))
    # the logged CVs are the oracle's on the positions of the last step; the hills' potential in torch agrees with the device's
    x = _np(p).astype(np.float64)
    for b, st in enumerate([0, 7, 19]):
        for c, cv in enumerate(CVS):
            so = O.cv(cv[0], x[[st + i for i in cv[1:]] + [0] * (5 - len(cv))])[0]
            assert abs(float(md.cv[-1, b, c]) - so) < 1e-12 * max(1.0, abs(so))
    V = md.bias_potential(md.cv[-1][:, [2, 0]])  # [1, 3]: the group's 12 hills; the last step saw the first 9
    assert V.shape == (1, 3) and torch.isfinite(V).all()
    md.reset(pos=p, vel=v, step=16)
    assert (md._start_row[2] - V[0]).abs().max().item() <= 1e-12 * float(V.abs().max())
    assert torch.allclose(md.free_energy(md.cv[-1][:, [2, 0]]), -(6.0 / 5.0) * V)


@pytest.mark.parametrize("arch", ARCHS)
def test_zero_bias_is_capture_md_bit_for_bit(hip_lib, arch):
    model, replay, inputs, vel, mass, dt = _setup(arch)
    z, pos, batch, box, q = inputs
    th = dict(friction=2.0, kT=0.01, seed=2 ** 40 + 5)
    ref = model.capture_md(z, pos, vel, mass, dt, batch=batch, q=q, steps_per_replay=8, thermostat=th)
    ref(2)
    md = _capture(model, inputs, vel, mass, dt, 8, _bias(model, inputs, scale=0.0), thermostat=th)
    md(2)
    assert md.check() == ref.check() == 16 and md.n_hills == 12
    for name in ("pos", "vel", "forces", "epot", "ekin"):
        assert _bits(getattr(md, name), getattr(ref, name)), name
    assert float(md.bias_energy.abs().max()) == 0 and float(md.restraint_energy.abs().max()) == 0 and float(md.hills()[1].abs().max()) == 0


def nve_drift(model, inputs, vel, mass, dt, bias):
    """64 NVE steps -> (|mean of the last 16 - mean of the first 16| of the conserved sum, its standard deviation), summed over the
    batch; with a bias the sum is epot + restraint + ekin / force_scale"""
    z, pos, batch, box, q = inputs
    if bias is None:
        md = model.capture_md(z, pos, vel, mass, dt, batch=batch, q=q, steps_per_replay=64)
    else:
        md = _capture(model, inputs, vel, mass, dt, 64, bias)
    md()
    assert md.check() == 64
    tot = md.epot.double() + md.ekin.double()
    if bias is not None:
        tot = tot + md.restraint_energy
    tot = tot.sum(1).cpu()
    return abs(float(tot[-16:].mean() - tot[:16].mean())), float(tot.std()), md


@pytest.mark.parametrize("arch", ARCHS)
def test_nve_with_a_distance_restraint_conserves_the_biased_energy(hip_lib, arch):
    """One harmonic distance restraint per walker, kappa of the size of the model's largest force per length, displaced by 0.1: the
    conserved quantity is epot + restraint + ekin.  The random-weight model is no force field, so the yardstick is the unbiased run
    of the same model, same dt, same 64 steps: drift and fluctuation of the biased sum against the unbiased ones, with the margin
    recorded in profiles/md_bias.json (ten times the measured ratio, never below 2)."""
    model, replay, inputs, vel, mass, dt = _setup(arch)
    bias = _bias(model, inputs)
    bias = dict(cvs=CVS[:1], restraints=bias["restraints"][:1])
    d0, s0, _ = nve_drift(model, inputs, vel, mass, dt, None)
    d1, s1, md = nve_drift(model, inputs, vel, mass, dt, bias)
    yard = max(d0, s0)
    print(arch, "unbiased drift", d0, "fluctuation", s0, "biased drift", d1, "fluctuation", s1, "ratio", max(d1, s1) / yard,
          "restraint energy", float(md.restraint_energy.sum(1).min()), float(md.restraint_energy.sum(1).max()))
    assert float(md.restraint_energy.sum(1).max() - md.restraint_energy.sum(1).min()) > 3 * yard  # left out, the sum would not be conserved
    assert max(d1, s1) <= max(10.0 * REC["nve_ratio"][arch], 2.0) * yard


def test_reset_keeps_clears_or_restores_the_hills(hip_lib):
    model, replay, inputs, vel, mass, dt = _setup("tensornet")
    bias = _bias(model, inputs)
    md = _capture(model, inputs, vel, mass, dt, 8, bias)
    md(2)
    p, v = md.pos.clone(), md.vel.clone()
    c, w = md.hills()
    assert c.shape == (1, 12, 2) and w.shape == (1, 12) and md.n_hills == 12 and float(w.min()) > 0

    def run(m, **kw):
        m.reset(pos=p, vel=v, step=16, **kw)
        n0 = m.n_hills
        m()
        assert m.check() == 24
        return n0, m.pos.clone(), m.vel.clone(), m.bias_energy.clone(), m.hills()

    keep = run(md)  # hills="keep"
    assert keep[0] == 12 and md.n_hills == 18 and _bits(keep[4][0][:, :12], c) and _bits(keep[4][1][:, :12], w)
    fresh = _capture(model, inputs, vel, mass, dt, 8, bias)
    restored = run(fresh, hills=(c, w))  # a new loop started from the saved hills: the same trajectory
    assert restored[0] == 12 and all(_bits(a, b) for a, b in zip(keep[1:4], restored[1:4]))
    assert all(_bits(a, b) for a, b in zip(keep[4], restored[4]))
    clear = run(md, hills="clear")
    assert clear[0] == 0 and md.n_hills == 6 and not _bits(clear[1], keep[1])
    z, pos, batch, box, q = inputs
    scratch = model.capture_md_biased(z, p, v, mass, dt, batch=batch, q=q, steps_per_replay=8, bias=bias)  # no hills, from (p, v)
    scratch()
    assert _bits(scratch.pos, clear[1]) and _bits(scratch.vel, clear[2]) and _bits(scratch.bias_energy, clear[3])
    assert float(keep[3][0].abs().min()) > 0 and float(clear[3][0].abs().max()) == 0  # 12 hills felt at once / none yet
    with pytest.raises(ValueError, match="hills"):
        md.reset(hills="drop")
    with pytest.raises(ValueError, match="capacity"):
        md.reset(hills=(torch.zeros(1, 65, 2), torch.zeros(1, 65)))
    with pytest.raises(ValueError, match="free_energy|well-tempered"):
        plain = dict(bias, metad=dict(bias["metad"], bias_factor=None))
        _capture(model, inputs, vel, mass, dt, 4, plain).free_energy(torch.zeros(2))


def test_a_replay_past_the_capacity_is_refused(hip_lib):
    model, replay, inputs, vel, mass, dt = _setup("tensornet")
    bias = _bias(model, inputs)
    bias["metad"] = dict(bias["metad"], capacity=15)
    md = _capture(model, inputs, vel, mass, dt, 8, bias)
    md(2)  # 12 hills
    assert md.n_hills == 12
    keep = md.pos.clone()
    with pytest.raises(ValueError, match="capacity"):
        md()  # would reach 18
    assert _bits(md.pos, keep) and md.steps_done == 16 and md.check() == 16
    md.reset(hills="clear", step=16)
    md()
    assert md.check() == 24 and md.n_hills == 6


def test_a_collinear_angle_freezes_the_loop_with_status_4(hip_lib):
    model, replay, inputs, vel, mass, dt = _setup("tensornet")
    bias = _bias(model, inputs)
    md = _capture(model, inputs, vel, mass, dt, 4, bias)
    md()
    assert md.check() == 4
    p, v = md.pos.clone(), md.vel.clone()
    # molecule 1 (atoms 7..18): the atoms of angle(1, 3, 5) on one line.  With zero velocities and zero start forces the opening
    # half leaves every atom where it is, so the first bias launch of the replay meets exactly this geometry.
    md.vel.zero_()
    md.forces.zero_()
    line = md.pos[7 + 3].clone()
    md.pos[7 + 1] = line + torch.tensor([1.0, 0.0, 0.0], device="cuda")
    md.pos[7 + 5] = line + torch.tensor([-1.5, 0.0, 0.0], device="cuda")
    store = md._hill_store().clone()
    md()
    with pytest.raises(RuntimeError, match="bias: a collective variable"):
        md.check()
    host = (C.c_uint64 * 2)()
    assert hip_lib.tmdnet_md_status(None, C.c_void_p(md._ws.data_ptr()), host) == 5 and (int(host[0]), int(host[1])) == (4, 4)
    assert torch.isfinite(md.pos).all() and torch.isfinite(md.vel).all()
    assert _bits(md._hill_store(), store)  # the first launch of the replay froze the loop: no deposit
    with pytest.raises(RuntimeError, match="both pos and vel"):
        md.reset()
    md.reset(pos=p, vel=v, step=4)
    md()
    assert md.check() == 8 and md.n_hills == 6


def test_overflow_freezes_the_bias(hip_lib):
    """The case of tests/test_gpu_md_loop.py::test_overflow_freezes_the_state_at_the_last_valid_step with a restraint and
    metadynamics on the 192-atom water box: box and positions scaled by 0.85 between two replays; the evaluation's counts[2] is what
    the bias launch reads"""
    model = _model("tensornet", max_num_neighbors=72)
    z, pos, box = (t.cuda() for t in W.water_box(n_side=4))
    box = box.clone()
    batch = torch.zeros_like(z)
    q = torch.zeros(1, device="cuda")
    vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    mass = torch.where(z == 1, 1.008, 12.0).float()
    bias = dict(cvs=[("distance", 0, 1), ("angle", 1, 0, 2)], restraints=[dict(cv=0, kappa=1.0, center=1.0)],
                metad=dict(cvs=[1], sigma=[0.2], height=0.01, pace=2, kT=0.05, bias_factor=4.0, capacity=16), log_forces=True)
    md = model.capture_md_biased(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, steps_per_replay=4, bias=bias)
    md()
    assert md.check() == 4 and md.n_hills == 2
    box.mul_(0.85)
    md.pos.mul_(0.85)
    state = (md.pos, md.vel, md.forces, md.epot, md.ekin, md.cv, md.restraint_energy, md.bias_energy, md.bias_forces, md._bias_ws)
    keep = [t.clone() for t in state]
    for _ in range(2):  # the overflowing replay and one more
        md()
        with pytest.raises(RuntimeError, match="max_num_pairs"):
            md.check()
        for t, k in zip(state, keep):
            assert _bits(t, k)
    box.mul_(1.0 / 0.85)
    md.reset(pos=pos, vel=vel, step=4)  # hills="keep": the device's counter says 4 steps, 2 hills
    assert md.n_hills == 2
    md()
    assert md.check() == 8 and md.n_hills == 4


def test_refusals(hip_lib):
    model, replay, inputs, vel, mass, dt = _setup("tensornet")
    z, pos, batch, box, q = inputs
    good = _bias(model, inputs)
    sd = {k: v.clone() for k, v in model.state_dict().items()}

    def refuse(exc, match, bias=good, **kw):
        with pytest.raises(exc, match=match):
            model.capture_md_biased(z, pos, vel, mass, dt, batch=batch, q=q, steps_per_replay=4, bias=bias, **kw)

    refuse(NotImplementedError, "barostat", barostat=dict(pressure=0.0, tau=1.0, compressibility=1.0, kT=0.01))
    refuse(NotImplementedError, "constraints", constraints=dict(pairs=torch.tensor([[0, 1]])))
    refuse(ValueError, "needs bias", bias=None)
    metad = good["metad"]
    for match, over in (("outside its molecule", dict(cvs=[("distance", 0, 7)])),  # the smallest molecule has 7 atoms
                        ("twice", dict(cvs=[("angle", 1, 2, 1)])),
                        ("at most 8", dict(cvs=[("distance", 0, 1)] * 9)),
                        ("1 or 2", dict(metad=dict(metad, cvs=[0, 1, 2], sigma=[0.1] * 3))),
                        ("1 or 2", dict(metad=dict(metad, cvs=[], sigma=[]))),
                        ("positive widths", dict(metad=dict(metad, sigma=[0.3, 0.0]))),
                        ("pace", dict(metad=dict(metad, pace=0))),
                        ("bias_factor", dict(metad=dict(metad, bias_factor=1.0))),
                        ("whole number of groups", dict(metad=dict(metad, walkers_per_group=2))),
                        ("capacity", dict(metad=dict(metad, capacity=2)))):
        b = dict(good, **over)
        if "cvs" in over:
            b = dict(cvs=over["cvs"])
        refuse(ValueError, match, bias=b)
    with pytest.raises(ValueError, match="sorted"):
        model.capture_md_biased(z, pos, vel, mass, dt, batch=batch.flip(0), q=q, steps_per_replay=4, bias=good)
    for k, v in model.state_dict().items():  # nothing was staged
        assert torch.equal(v, sd[k])
    md = _capture(model, inputs, vel, mass, dt, 4, good)  # and the model still captures
    md()
    assert md.check() == 4
