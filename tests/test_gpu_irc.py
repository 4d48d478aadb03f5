"""-m gpu: the device-resident IRC follower (csrc/tn_irc.hip, TorchMD_Net.capture_irc).

1.-4.   the C entries alone (no model, graph_ws = NULL) on the analytic surface of tests/irc_oracle.py, energies and forces from torch
        between the launches: every step against the host mirror (tests/irc_host_mirror.py: the header's statements on the CPU, the
        sums in the device's order) - one saddle of 3 atoms in both directions, two saddles, one path of 1 500 atoms (two slices),
        fixed atoms
5.-7.   repeatability, finished paths, a NaN force, a zero velocity and a NaN energy
8.-16.  through the model: bit-identity with capture() + a torch mirror, the constant speed, path(), run, overflow, status 2,
        refusals, the stale-graph guard, reset"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import irc_host_mirror as H
from tests import irc_oracle as O
from tests import min_oracle as MO
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

OPEN, MIDDLE, CLOSE = 0, 1, 2
DT, STEP = 0.05, 0.02
# the paper's v0 and error taken as numbers, as the issue's prototype did: about 250 steps from the saddle to a minimum
PRM = dict(fmax=1e-3, v0=0.04, error=0.003, dt_min=DT / 16, dt_max=DT * 16, every=1, capacity=400)


def _bits(a, b):
    if not a.is_floating_point():
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                                              b.contiguous().view(torch.int64 if b.dtype == torch.float64 else torch.int32))


def _np_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all()


# ------------------------------------------------------------------------------------------------ the C entries alone
class _Raw:
    """The C entries on tensors of the test's own, m = graph_ws = NULL (no model: energies and forces are what the test hands in)."""

    def __init__(self, lib, pos, vel, masses, prm=PRM, fixed=None, dt=DT):
        from torchmdnet_amd.irc import record_views

        self.L, self.prm, self.dt0 = lib, dict(prm), dt
        P, n = self.shape = tuple(pos.shape[:2])
        self.pos, self.vel = pos.clone().contiguous(), vel.clone().contiguous()
        self.masses = torch.as_tensor(np.asarray(masses, np.float32)).cuda()
        self.ca = torch.from_numpy(H.half_inv_mass(masses)).cuda()
        self.fixed = fixed
        nb = C.c_size_t(0)
        assert lib.tmdnet_irc_workspace_bytes(n, P, self.prm["capacity"], C.byref(nb)) == 0
        self.ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        self.n_rec_ws, self.frame_s, self.frame_e, self.frames = record_views(self.ws, n, P, self.prm["capacity"])
        nan = float("nan")
        f32, f64 = dict(device="cuda"), dict(dtype=torch.float64, device="cuda")
        self.fkeep = torch.full_like(pos, nan)
        self.epot, self.fmax = torch.full((P,), nan, **f32), torch.full((P,), nan, **f32)
        self.sums, self.coef = torch.full((P, 6), nan, **f64), torch.full((P, 2), nan, **f32)
        self.dt, self.arc, self.power = (torch.full((P,), nan, **f64) for _ in range(3))
        self.conv = torch.full((P,), -7, dtype=torch.int64, device="cuda")
        self.reason = torch.full((P,), -7, dtype=torch.int32, device="cuda")
        self.step_size, self.arc_length = torch.full((P,), nan, **f64), torch.full((P,), nan, **f64)
        self.n_rec = torch.full((P,), -7, dtype=torch.int32, device="cuda")
        self.reset()

    @staticmethod
    def _s():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def reset(self):
        assert self.L.tmdnet_irc_reset(self._s(), self._p(self.ws), 0, self.dt0) == 0

    def logs(self):
        return [self.epot, self.fmax, self.sums, self.coef, self.dt, self.arc, self.power, self.conv, self.reason, self.step_size,
                self.arc_length, self.n_rec]

    def tensors(self):
        return [self.pos, self.vel, self.fkeep, self.frames, self.frame_s, self.frame_e] + self.logs()

    def advance(self, phase, forces, energy):
        p, q = self._p, self.prm
        P, n = self.shape
        logs = [None] * 12 if phase == OPEN else [p(t) for t in self.logs()]
        rc = self.L.tmdnet_irc_advance(None, self._s(), None, p(self.ws), n, P, q["capacity"], q["every"], phase, p(self.pos), p(self.vel),
                                       p(forces), p(energy), p(self.ca), p(self.masses), p(self.fixed), None if phase == OPEN else p(self.fkeep),
                                       q["fmax"], q["v0"], q["error"], q["dt_min"], q["dt_max"], *logs)
        assert rc == 0, rc

    def status(self):
        host = (C.c_uint64 * 3)()
        rc = self.L.tmdnet_irc_status(self._s(), self._p(self.ws), host)
        return rc, int(host[0]), int(host[1]), int(host[2])


def _surface(pos, sites):
    """torch, fp64 at the fp32 positions, rounded once: pos [P,n,3] -> e [P] fp32, f [P,n,3] fp32"""
    x = pos.double()
    X, Y = x[:, 0, 0], x[:, 1, 1]
    u = X * X - 1.0
    w = Y + O.A * u
    d = x - sites
    d[:, 0, 0] = 0.0
    d[:, 1, 1] = 0.0
    e = u * u + O.KAPPA * w * w + 0.5 * O.KAPPA * (d * d).sum((-1, -2))
    f = -O.KAPPA * d
    f[:, 0, 0] = -(4.0 * X * u + 2.0 * O.KAPPA * w * (2.0 * O.A * X))
    f[:, 1, 1] = -(2.0 * O.KAPPA * w)
    return e.float().contiguous(), f.float().contiguous()


def _check_step(raw, mirror, e, f, where):
    """The launch just made (CLOSE or MIDDLE's accept on energies e and forces f) against the host mirror, which is fed the same e
    and f.  Sums, arc, damping, state, frames and the accepted x, v, F bit for bit; dt within one fp32 ulp (the cube root is
    another library's), after which the mirror takes the device's dt so that the next step starts from the same bits."""
    was = mirror.conv.copy()
    assert mirror.close(e.cpu().numpy(), f.cpu().numpy()) == 0, where
    sums, coef, dt, arc, power = (t.cpu().numpy() for t in (raw.sums, raw.coef, raw.dt, raw.arc, raw.power))
    assert _np_bits(sums, mirror.rec) and _np_bits(arc, mirror.arc) and _np_bits(power, np.ascontiguousarray(mirror.rec[:, H.S_P])), (where, sums, mirror.rec)
    # (c = v0 / sqrt(vv) is a correctly rounded square root and quotient on both sides: the allowance of one ulp is not needed)
    assert _np_bits(coef[:, 1], mirror.dt_used) and _np_bits(coef[:, 0], mirror.damp), (where, coef, mirror.damp, mirror.dt_used)
    assert MO.ulp_distance(dt.astype(np.float32), mirror.dt.astype(np.float32)).max() <= 1, (where, dt, mirror.dt)
    assert np.abs(dt - mirror.dt).max() <= 1e-15 * np.abs(dt).max(), (where, dt, mirror.dt)
    assert (raw.conv.cpu().numpy() == mirror.conv).all() and (raw.reason.cpu().numpy() == mirror.reason).all(), where
    assert (raw.n_rec.cpu().numpy() == mirror.n_rec).all() and (raw.n_rec_ws.cpu().numpy() == mirror.n_rec).all(), where
    assert _np_bits(raw.step_size.cpu().numpy(), dt) and _np_bits(raw.arc_length.cpu().numpy(), arc), where
    live = was < 0
    assert _np_bits(raw.epot.cpu().numpy()[live], e.cpu().numpy()[live]), where
    assert _np_bits(raw.fmax.cpu().numpy(), np.sqrt(mirror.rec[:, H.S_FMAX2]).astype(np.float32)), where
    assert _np_bits(raw.pos.cpu().numpy(), mirror.pos) and _np_bits(raw.vel.cpu().numpy(), mirror.vel), where
    assert _np_bits(raw.fkeep.cpu().numpy()[live], mirror.fkeep[live]), where
    k = int(mirror.n_rec.max())
    cap = raw.prm["capacity"]
    assert _np_bits(raw.frames.cpu().numpy()[:, :min(k, cap)], mirror.frames[:, :min(k, cap)]), where
    assert _np_bits(raw.frame_s.cpu().numpy(), mirror.frame_s) and _np_bits(raw.frame_e.cpu().numpy(), mirror.frame_e), where
    mirror.dt[:] = dt


def _drive(lib, pos, vel, masses, sites, prm=PRM, fixed=None, fused=False, checks=True, max_steps=1000, raw=None):
    """Follow the paths through the C entries: per step OPEN, energies and forces from torch, CLOSE (fused: one OPEN, then MIDDLE
    after every evaluation).  With `checks`, every step against the mirror.  -> the _Raw, the steps taken, the history."""
    sites_t = sites if torch.is_tensor(sites) else torch.from_numpy(np.asarray(sites)).cuda()
    if raw is None:
        raw = _Raw(lib, pos, vel, masses, prm, fixed)
    fx = None if raw.fixed is None else raw.fixed.cpu().numpy()
    assert not (fused and checks)
    mirror = H.Paths(raw.pos.cpu().numpy(), raw.vel.cpu().numpy(), masses, raw.prm, raw.dt0, fx) if checks else None
    e, f = _surface(raw.pos, sites_t)
    raw.advance(CLOSE, f, e)
    if checks:
        _check_step(raw, mirror, e, f, "start")
    assert raw.status() == (0, 0, 0, 0)
    hist = dict(pos=[raw.pos.clone()], vel=[raw.vel.clone()], conv=[raw.conv.clone()])
    step = 0
    while step < max_steps and not bool((raw.conv >= 0).all()):
        if not fused or step == 0:
            raw.advance(OPEN, raw.fkeep, None)  # (fused: the MIDDLE below has made this move already)
        if checks:
            mirror.open()
            assert _np_bits(raw.pos.cpu().numpy(), mirror.pos) and _np_bits(raw.vel.cpu().numpy(), mirror.vel), step
        step += 1
        e, f = _surface(raw.pos, sites_t)
        raw.advance(MIDDLE if fused else CLOSE, f, e)
        if checks:
            _check_step(raw, mirror, e, f, step)
        hist["pos"].append(raw.pos.clone())
        hist["vel"].append(raw.vel.clone())
        hist["conv"].append(raw.conv.clone())
    assert raw.status() == (0, step, 0, 0)
    return raw, step, hist, sites_t


def _starts(n, masses2=(1.0, 16.0), shifts=(0.0,), D=2, fixed=None):
    """G = len(shifts) start points on the surface (point g: the saddle with atom 1 moved by shifts[g] along Y, off the valley floor):
    pos, vel [G D, n, 3] (cuda), masses, sites"""
    x_ts, u, masses, sites = O.problem(n, *masses2)
    if fixed is not None:
        u = u * (np.asarray(fixed) == 0)[:, None]
    xs = np.stack([x_ts] * len(shifts))
    xs[:, 1, 1] += np.asarray(shifts, np.float32)
    pos, vel = H.start(xs, np.stack([u.astype(np.float32)] * len(shifts)), STEP, PRM["v0"], D=D)
    return torch.from_numpy(pos).cuda(), torch.from_numpy(vel).cuda(), masses, sites


_cache = {}


def _one_saddle(lib):
    if "one" not in _cache:
        pos, vel, masses, sites = _starts(3)
        _cache["one"] = _drive(lib, pos, vel, masses, sites) + ((pos, vel, masses),)
    return _cache["one"]


def _two_saddles(lib):
    if "two" not in _cache:
        pos, vel, masses, sites = _starts(3, shifts=(0.0, 0.3))
        _cache["two"] = _drive(lib, pos, vel, masses, sites) + ((pos, vel, masses),)
    return _cache["two"]


def test_one_saddle_every_step_equals_the_host_mirror(hip_lib):
    """1. one saddle of 3 atoms (masses 1, 16 and a spectator), both directions, to the end.  Per step (the assertions are in
    _check_step and _drive): positions, velocities, the kept forces, the six sums, the arc, the frames and their s and energy, the
    step counts and reasons bit for bit against the header on the host; dt and c within one fp32 ulp.  The whole path finishes at
    the step the host mirror finishes at when it runs alone, at the minimum, and the two directions are mirror images."""
    raw, steps, hist, sites, (pos, vel, masses) = _one_saddle(hip_lib)
    ref = H.run(pos.cpu().numpy(), vel.cpu().numpy(), masses, sites.cpu().numpy(), O.KAPPA, O.A, PRM, DT, 1000)
    print("finished at", raw.conv.tolist(), "reason", raw.reason.tolist(), "host mirror", ref["steps"], "arc", raw.arc.tolist())
    assert steps == ref["steps"] and raw.conv.tolist() == ref["conv"].tolist() == [steps] * 2 and raw.reason.tolist() == ref["reason"].tolist()
    assert 100 < steps < 1000
    x = raw.pos.double().cpu().numpy()
    assert abs(x[0, 0, 0] - 1.0) < 0.01 and abs(x[1, 0, 0] + 1.0) < 0.01 and np.abs(x[:, 1, 1]).max() < 0.03
    assert _bits(raw.pos[0, 0, 0], -raw.pos[1, 0, 0]) and _bits(raw.pos[0, 1:], raw.pos[1, 1:]) and _bits(raw.arc[0], raw.arc[1])
    assert raw.n_rec.tolist() == [steps + 1] * 2 and _bits(raw.frames[:, steps], raw.pos)
    assert float(raw.epot.max()) < 1e-3 and abs(float(raw.frame_e[0, 0]) - 1.0) < 0.01


def test_two_saddles_finish_and_freeze_on_their_own(hip_lib):
    """2. two saddles in one call, the second started 0.3 off the valley floor (the masses are per atom and shared), both
    directions, every step checked: one controller per path - the paths of the two saddles finish at their own steps, a finished path
    keeps its bits while the others still move, and each ends as it does when its saddle is followed alone."""
    raw, steps, hist, sites, (pos, vel, masses) = _two_saddles(hip_lib)
    conv = raw.conv.tolist()
    print("finished at", conv, "reason", raw.reason.tolist())
    assert min(conv) > 20 and conv[0] == conv[1] != conv[2] == conv[3] and steps == max(conv)
    first = int(np.argmin(conv))
    for s in range(conv[first], steps + 1):
        assert _bits(hist["pos"][s][first], hist["pos"][conv[first]][first]) and _bits(hist["vel"][s][first], hist["vel"][conv[first]][first]), s
        assert int(hist["conv"][s][first]) == conv[first]
    last = int(np.argmax(conv))
    assert not _bits(hist["pos"][steps][last], hist["pos"][conv[first]][last])
    for g in range(2):  # alone: the same bits
        alone, steps1, _, _ = _drive(hip_lib, pos[2 * g:2 * g + 2], vel[2 * g:2 * g + 2], masses, sites, checks=False)
        assert steps1 == max(conv[2 * g:2 * g + 2]) and _bits(alone.pos, raw.pos[2 * g:2 * g + 2]) and _bits(alone.arc, raw.arc[2 * g:2 * g + 2])
        assert alone.conv.tolist() == conv[2 * g:2 * g + 2]


def test_path_in_two_slices(hip_lib):
    """3. one path of 1 500 atoms: two slices of 750 atoms, added in slice order.  Most atoms are spectators on their sites.  Six
    steps, every one checked as above - the mirror adds in the device's order, so the sums are compared bit for bit."""
    pos, vel, masses, sites = _starts(1500, D=1)
    pos[0, 700:800] += 0.01  # some spectators off their sites, in both slices: they feel forces and move
    raw, steps, _, _ = _drive(hip_lib, pos, vel, masses, sites, max_steps=6)
    assert steps == 6 and int(raw.conv[0]) == -1 and float(raw.sums[0, 5]) == 1500.0 and not _bits(raw.pos, pos)
    assert raw.n_rec.tolist() == [7] and _bits(raw.frames[0, 6], raw.pos[0])


def test_fixed_atoms(hip_lib):
    """4. a spectator held off its site and fixed: it keeps its bits, has v = 0 and is left out of the sums - the others take the
    path they take with that spectator free on its site.  All atoms fixed: the paths are finished as they stand."""
    n = 5
    fixed_np = np.array([0, 0, 0, 1, 0], np.uint8)
    fixed = torch.from_numpy(fixed_np).cuda()
    pos, vel, masses, sites = _starts(n)
    ref, steps_ref, _, _ = _drive(hip_lib, pos, vel, masses, sites, checks=False, fused=True)
    off = pos.clone()
    off[:, 3] += 0.3
    vel_f = vel.clone()
    vel_f[:, 3] = 0.5  # whatever velocity a fixed atom is given, it ends as zero
    raw, steps, _, sites_t = _drive(hip_lib, off, vel_f, masses, sites, fixed=fixed)
    keep = [0, 1, 2, 4]
    assert steps == steps_ref and _bits(raw.pos[:, 3], off[:, 3]) and (raw.vel[:, 3] == 0).all() and float(raw.sums[0, 5]) == 4.0
    assert _bits(raw.pos[:, keep], ref.pos[:, keep]) and _bits(raw.arc, ref.arc) and (raw.fkeep[:, 3] != 0).any()
    every = torch.ones(n, dtype=torch.uint8, device="cuda")
    raw, steps, _, _ = _drive(hip_lib, pos, vel, masses, sites, fixed=every)
    assert steps == 0 and raw.conv.tolist() == [0, 0] and raw.reason.tolist() == [1, 1] and _bits(raw.pos, pos) and (raw.vel == 0).all()
    raw.advance(OPEN, raw.fkeep, None)
    assert _bits(raw.pos, pos) and (raw.vel == 0).all()


def test_two_runs_are_bit_identical(hip_lib):
    """5. fixed summation order, no floating-point atomics; and MIDDLE after every evaluation is the same path as OPEN / CLOSE"""
    pos, vel, masses, sites = _starts(3, shifts=(0.0, 0.3))
    a, sa, _, _ = _drive(hip_lib, pos, vel, masses, sites, fused=True, checks=False)
    b, sb, _, _ = _drive(hip_lib, pos, vel, masses, sites, fused=True, checks=False)
    assert sa == sb
    for s, t in zip(a.tensors(), b.tensors()):
        assert _bits(s, t)
    ref = _two_saddles(hip_lib)[0]
    assert _bits(a.pos, ref.pos) and _bits(a.vel, ref.vel) and torch.equal(a.conv, ref.conv) and _bits(a.frames, ref.frames)


def test_finished_path_changes_nothing_on_further_launches(hip_lib):
    """6. all paths finished: OPEN, MIDDLE and CLOSE launches leave x, v, the kept forces, dt, the arc, the record and the state
    as they are"""
    pos, vel, masses, sites = _starts(3, shifts=(0.0, 0.3))
    raw, steps, _, sites_t = _drive(hip_lib, pos, vel, masses, sites, fused=True, checks=False)
    watched = lambda: (raw.pos, raw.vel, raw.fkeep, raw.conv, raw.reason, raw.dt, raw.arc, raw.sums, raw.coef, raw.n_rec, raw.frames,
                       raw.frame_s, raw.frame_e)
    keep = [t.clone() for t in watched()]
    e, f = _surface(raw.pos, sites_t)
    for phase in (OPEN, MIDDLE, CLOSE, OPEN):
        raw.advance(phase, raw.fkeep if phase == OPEN else f, None if phase == OPEN else e)
    for t, k in zip(watched(), keep):
        assert _bits(t, k)
    assert raw.status() == (0, steps + 2, 0, 0)


def _three_steps(lib):
    pos, vel, masses, sites = _starts(3, shifts=(0.0, 0.3))
    raw = _Raw(lib, pos, vel, masses)
    sites_t = torch.from_numpy(sites).cuda()
    e, f = _surface(raw.pos, sites_t)
    raw.advance(CLOSE, f, e)
    for _ in range(3):
        raw.advance(OPEN, raw.fkeep, None)
        e, f = _surface(raw.pos, sites_t)
        raw.advance(CLOSE, f, e)
    assert raw.status() == (0, 3, 0, 0)
    return raw, sites_t


def _latched(raw, sites_t, e_bad, f_bad, cause, step, valid):
    """after the launch on (e_bad, f_bad): status 2 with `cause` (a status latch, not a fault); x and v are back at the last valid
    step (`valid`), nothing else is written, and every later launch changes nothing"""
    keep = [t.clone() for t in raw.tensors()[2:]]
    raw.advance(CLOSE, f_bad, e_bad)
    assert raw.status() == (5, step, 2, cause)
    assert _bits(raw.pos, valid[0]) and _bits(raw.vel, valid[1])
    e, f = _surface(raw.pos, sites_t)
    raw.advance(OPEN, raw.fkeep, None)
    raw.advance(MIDDLE, f, e)
    raw.advance(CLOSE, f, e)
    assert raw.status() == (5, step, 2, cause)
    assert _bits(raw.pos, valid[0]) and _bits(raw.vel, valid[1])
    for t, k in zip(raw.tensors()[2:], keep):
        assert _bits(t, k) or (torch.isnan(t).all() and torch.isnan(k).all())


def test_nan_force_zero_velocity_and_nan_energy_latch_status_2(hip_lib):
    """7. after three valid steps and the move of the fourth: a NaN force on an atom of the third path: cause 1; a path whose
    half-step velocity and new forces are zero: cause 2; a NaN energy: cause 3 (it outranks the others).  x and v are those of the
    last valid step.  A reset recovers."""
    raw, sites_t = _three_steps(hip_lib)
    valid = raw.pos.clone(), raw.vel.clone()
    raw.advance(OPEN, raw.fkeep, None)
    e, f = _surface(raw.pos, sites_t)
    bad = f.clone()
    bad[2, 1, 2] = float("nan")
    _latched(raw, sites_t, e, bad, 1, 3, valid)
    raw, sites_t = _three_steps(hip_lib)
    valid = raw.pos.clone(), raw.vel.clone()
    raw.advance(OPEN, raw.fkeep, None)
    e, f = _surface(raw.pos, sites_t)
    raw.vel[1] = 0
    still = f.clone()
    still[1] = 0
    _latched(raw, sites_t, e, still, 2, 3, valid)
    raw.reset()
    e, f = _surface(raw.pos, sites_t)
    raw.advance(CLOSE, f, e)
    assert raw.status() == (0, 0, 0, 0) and raw.n_rec.tolist() == [1] * 4 and (raw.arc == 0).all() and _bits(raw.dt, torch.full_like(raw.dt, DT))
    raw, sites_t = _three_steps(hip_lib)
    valid = raw.pos.clone(), raw.vel.clone()
    raw.advance(OPEN, raw.fkeep, None)
    e, f = _surface(raw.pos, sites_t)
    e_bad = e.clone()
    e_bad[3] = float("nan")
    _latched(raw, sites_t, e_bad, bad, 3, 3, valid)


# ------------------------------------------------------------------------------------------------ through the model
_models = {}
ARCHS = ["tensornet", "equivariant-transformer", "tensornet2"]
KW = dict(dt=0.5, fmax=1e-5, v0=0.02, error=1.5e-3, initial_step=0.05, force_scale=0.8)


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


def _molecule(n_atoms=40, n_saddles=2):
    """-> z [n], pos [G,n,3], masses [n]: a molecule and copies displaced smoothly by at most 0.1 per atom"""
    z, pos, _ = W.synthetic_batch(n_mol=1, n_atoms=n_atoms, first_seed=31)
    z, pos = (z % 8 + 1).cuda(), pos.cuda()
    out = []
    for g in range(n_saddles):
        gen = torch.Generator().manual_seed(50 + g)
        k, ph = torch.rand(3, 3, generator=gen).cuda(), (6.28 * torch.rand(3, generator=gen)).cuda()
        out.append(pos + g * (0.1 / math.sqrt(3)) * torch.sin(pos @ k + ph))
    return z, torch.stack(out), (1.0 + 2.0 * z.float()).cuda()


def _q(arch, G):
    return torch.zeros(G, device="cuda") if arch != "equivariant-transformer" else None


def _downhill(model, z, pos, q):
    """the direction of the force at every start point: the forward path goes downhill, the backward one has turned uphill at once"""
    G, n = pos.shape[:2]
    batch = torch.arange(G, device="cuda").repeat_interleave(n)
    _, f = model.energy_and_forces(z.repeat(G), pos.reshape(-1, 3), batch, None, q, G, want_forces=True)
    return f.detach().view(G, n, 3).clone()


def _record(irc, replays):
    keys = ("epot", "fmax", "coef", "dt", "arc", "power", "sums")
    logs = {k: [] for k in keys + ("conv", "speed")}
    for _ in range(replays):
        irc()
        for key in keys:
            logs[key].append(getattr(irc, key).clone())
        logs["conv"].append(irc.converged_at.clone())
    assert irc.check() == irc.steps_per_replay * replays == irc.steps_done
    return {k: (torch.cat(v) if k in keys else v) for k, v in logs.items()}


def _mirror_kick(v, dtf, ca, f):
    return torch.add(v, torch.mul(torch.mul(dtf[..., None, None], ca[:, None]), f))


@pytest.mark.parametrize("arch", ARCHS)
def test_irc_is_bit_identical_to_capture_plus_torch_mirror(hip_lib, arch):
    """8. two start points of 40 atoms, both directions, K = 4, three replays, against capture() on the stacked paths and a torch
    mirror that takes the device's c and dt and issues torch.mul and torch.add separately: positions, velocities, forces and
    energies equal bit for bit; the frames equal the positions at the recorded steps; one replay of 12 steps gives the same bits."""
    model = _model(arch)
    z, pos, masses = _molecule()
    G, n = pos.shape[:2]
    q = _q(arch, G)
    fixed = torch.zeros(n, dtype=torch.bool, device="cuda")
    fixed[::11] = True
    mode = _downhill(model, z, pos, q)
    kw = dict(KW, q=q, fixed=fixed, record=dict(every=2, capacity=16))
    batch = torch.arange(2 * G, device="cuda").repeat_interleave(n)
    replay = model.capture(z.repeat(2 * G), pos.repeat_interleave(2, 0).reshape(-1, 3), batch, q=None if q is None else q.repeat_interleave(2))
    from torchmdnet_amd.irc import unit_direction

    irc = model.capture_irc(z, pos, mode, masses, steps_per_replay=4, **kw)
    u = unit_direction(mode, G, n, fixed).cuda()
    ca = (0.8 / (2.0 * masses.double())).float()
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")
    sg = torch.tensor([1.0, -1.0], device="cuda")[None, :, None, None]
    x = torch.add(pos[:, None], torch.mul(torch.mul(sg, f32(KW["initial_step"])), u[:, None]))
    v = torch.mul(torch.mul(sg, f32(KW["v0"])), u[:, None])
    still = fixed[None, None, :, None]
    e, f = (t.clone() for t in replay(x.reshape(-1, 3)))
    f = f.view(G, 2, n, 3)
    assert _bits(irc.epot0, e.view(G, 2)) and _bits(irc.coef0[..., 1], torch.zeros(G, 2, device="cuda"))
    v = torch.where(still, torch.zeros_like(v), torch.mul(irc.coef0[..., 0, None, None], _mirror_kick(v, irc.coef0[..., 1], ca, f)))
    conv = torch.where(irc.sums0[..., 1] <= 0, 0, -1)  # forward: downhill; backward: uphill at once
    assert conv[:, 0].tolist() == [-1] * G and conv[:, 1].tolist() == [0] * G
    frames = [[[x[g, d].clone()] for d in range(2)] for g in range(G)]
    dt_next = torch.full((G, 2), KW["dt"], dtype=torch.float64, device="cuda")
    logs = _record(irc, 3)
    for s in range(12):
        live = (conv < 0)[..., None, None]
        dtf = dt_next.float()
        vh = _mirror_kick(v, dtf, ca, f)
        x_new = torch.add(x, torch.mul(dtf[..., None, None], vh))
        x = torch.where(live & ~still, x_new, x)
        e, f_new = (t.clone() for t in replay(x.reshape(-1, 3)))
        f_new = f_new.view(G, 2, n, 3)
        c, du = logs["coef"][s, ..., 0], logs["coef"][s, ..., 1]
        assert _bits(du[conv < 0], dtf[conv < 0]), s
        v_new = torch.mul(c[..., None, None], _mirror_kick(vh, dtf, ca, f_new))
        v = torch.where(live, torch.where(still, torch.zeros_like(v), v_new), v)
        f = torch.where(live, f_new, f)
        assert _bits(logs["epot"][s][conv < 0], e.view(G, 2)[conv < 0]), s
        ff = torch.where(fixed[None, None, :], 0.0, (f * f)[..., 0] + (f * f)[..., 1] + (f * f)[..., 2])
        assert _bits(logs["fmax"][s][conv < 0], ff.amax(-1).double().sqrt().float()[conv < 0]), s
        now = logs["conv"][s // 4] if s % 4 == 3 else None
        fin = (logs["sums"][s, ..., 1] <= 0) | (logs["sums"][s, ..., 2].sqrt() < KW["fmax"])
        for g in range(G):
            for d in range(2):
                if conv[g, d] < 0 and ((s + 1) % 2 == 0 or bool(fin[g, d])):
                    frames[g][d].append(x[g, d].clone())
        conv = torch.where((conv < 0) & fin, s + 1, conv)
        if now is not None:
            assert torch.equal(now, conv), s
        dt_next = logs["dt"][s]
    assert _bits(irc.pos, x) and _bits(irc.vel, v) and _bits(irc.forces, f)
    assert (x[:, 0] - pos).abs().max().item() > 1e-3 and _bits(x[:, :, fixed], pos[:, None, fixed].expand(G, 2, -1, 3))
    for g in range(G):
        for d in range(2):
            k = len(frames[g][d])
            assert int(irc.n_recorded[g, d]) == k and _bits(irc.frames[g, d, :k], torch.stack(frames[g][d])), (g, d, k)
    assert not irc.truncated
    irc12 = model.capture_irc(z, pos, mode, masses, steps_per_replay=12, **kw)
    logs12 = _record(irc12, 1)
    for a, b in ((irc12.pos, irc.pos), (irc12.vel, irc.vel), (irc12.forces, irc.forces), (irc12.frames, irc.frames), (irc12.frame_s, irc.frame_s)):
        assert _bits(a, b)
    for key in ("epot", "fmax", "coef", "dt", "arc", "power"):
        assert _bits(logs12[key], logs[key]), key
    # one start point as [n,3], forward only (a batch of another size may take other kernels in the evaluation: no bits are compared)
    one = model.capture_irc(z, pos[0], mode[0], masses, direction="forward", steps_per_replay=4, **dict(kw, q=None if q is None else q[:1]))
    one()
    assert one.check() == 4 and one.pos.shape == (1, 1, n, 3) and one.epot.shape == (4, 1, 1) and not _bits(one.pos[0, 0], pos[0])


@pytest.mark.parametrize("arch", ARCHS)
def test_speed_arc_power_and_the_joined_path(hip_lib, arch):
    """9., 10. after every step the speed is v0 to a relative 1e-6; for every path the arc grows and the power is positive on every
    step before the finishing one; the forward and backward ends lie on opposite sides of the start; path(g) joins the two halves
    with s strictly increasing and the start point at s = 0; a backward-only run is the backward half."""
    model = _model(arch)
    z, pos, masses = _molecule()
    G, n = pos.shape[:2]
    q = _q(arch, G)
    mode = _downhill(model, z, pos, q)
    irc = model.capture_irc(z, pos, mode, masses, steps_per_replay=4, q=q, **KW)
    arcs, powers = [], []
    for _ in range(3):
        irc()
        speed = irc.vel.double().pow(2).sum((-1, -2)).sqrt()
        assert ((speed - KW["v0"]).abs() <= 1e-6 * KW["v0"]).all(), speed
        for k in range(4):
            sp = (irc.coef[k, ..., 0].double() * irc.sums[k, ..., 0].sqrt() - KW["v0"]).abs()
            assert (sp <= 1e-6 * KW["v0"]).all(), sp
        arcs.append(irc.arc.clone())
        powers.append(irc.power.clone())
    assert irc.check() == 12
    arcs, powers = torch.cat(arcs), torch.cat(powers)
    conv = irc.converged_at
    for g in range(G):
        for d in range(2):
            last = 12 if conv[g, d] < 0 else int(conv[g, d])
            a = torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), arcs[:last, g, d]])
            assert (a[1:] > a[:-1]).all() and (powers[:max(last - 1, 0), g, d] > 0).all(), (g, d)
    assert (conv[:, 0] < 0).all() and (conv[:, 1] == 0).all() and (irc.reason[:, 1] == 2).all() and (irc.sums0[:, 0, 1] > 0).all()
    u = irc.direction.double()
    along = ((irc.pos.double() - pos[:, None].double()) * u[:, None]).sum((-1, -2))
    assert (along[:, 0] > 0).all() and (along[:, 1] < 0).all()
    for g in range(G):
        path = irc.path(g)
        s, k = path["s"], int(irc.n_recorded[g].sum()) + 1
        assert s.shape == (k,) and path["pos"].shape == (k, n, 3) and path["energy"].shape == (k,)
        assert (s[1:] > s[:-1]).all() and int((s == 0).sum()) == 1
        mid = int((s < 0).sum())
        assert mid == int(irc.n_recorded[g, 1]) and torch.equal(path["pos"][mid], pos[g].cpu()) and torch.equal(path["pos"][-1], irc.pos[g, 0].cpu())
        assert torch.equal(path["pos"][0], irc.pos[g, 1].cpu()) and (path["energy"][mid + 1:][1:] < path["energy"][mid + 1:][:-1]).all()
        m = masses.double().cpu()
        want = (m[:, None] * (path["pos"][mid + 1].double() - pos[g].cpu().double()) ** 2).sum().sqrt()
        assert abs(float(s[mid + 1]) - float(want)) <= 1e-12 and abs(float(s[mid - 1]) + float(want)) <= 1e-6 * float(want)
    back = model.capture_irc(z, pos, mode, masses, direction="backward", steps_per_replay=4, q=q, **KW)
    back()
    assert back.check() == 4 and (back.converged_at == 0).all() and back.pos.shape == (G, 1, n, 3)
    assert (back.path(0)["s"][:-1] < 0).all() and float(back.path(0)["s"][-1]) == 0.0


def test_run_stops_at_convergence_or_at_max_steps(hip_lib):
    """11."""
    model = _model("tensornet")
    z, pos, masses = _molecule(n_saddles=1)
    q = _q("tensornet", 1)
    mode = _downhill(model, z, pos, q)
    irc = model.capture_irc(z, pos, mode, masses, direction="forward", steps_per_replay=4, q=q, **KW)
    assert irc.run(20, check_every=2) == 20 and irc.check() == 20 and (irc.converged_at == -1).all()
    assert irc.run(7) == 4 and irc.check() == 24  # whole replays only, never beyond max_steps
    assert not _bits(irc.pos[0, 0], pos[0]) and irc.arc.shape == (4, 1, 1) and int(irc.n_recorded) == 25
    done = model.capture_irc(z, pos, mode, masses, direction="backward", steps_per_replay=4, q=q, **KW)
    assert done.run(100) == 0 and done.check() == 0  # finished at the start: nothing is replayed
    small = model.capture_irc(z, pos, mode, masses, direction="forward", steps_per_replay=4, q=q, record=dict(every=1, capacity=3), **KW)
    small(2)
    assert small.check() == 8 and small.truncated and int(small.n_recorded) == 9


def test_overflow_freezes_the_state_at_the_last_valid_step(hip_lib):
    """12. a path of the 192-atom periodic box with max_num_neighbors = 72, box and positions scaled by 0.85 between two replays:
    the first evaluation of the second replay overflows; status 1 latches and the point the last move began from comes back."""
    model = _model("tensornet", max_num_neighbors=72)
    z, pos, box = (t.cuda() for t in W.water_box(n_side=4))
    box0 = box.clone()
    q = torch.zeros(1, device="cuda")
    batch = torch.zeros(pos.shape[0], dtype=torch.long, device="cuda")
    _, f = model.energy_and_forces(z, pos, batch, box, q, 1, want_forces=True)
    irc = model.capture_irc(z, pos, f.detach().clone(), torch.ones(pos.shape[0]), direction="forward", box=box, q=q, steps_per_replay=4, **KW)
    irc()
    assert irc.check() == 4
    staged_box = irc.inputs[2]
    staged_box.mul_(0.85)
    irc.pos.mul_(0.85)
    watched = lambda: (irc.pos, irc.vel, irc.forces, irc.epot, irc.fmax, irc.coef, irc.sums, irc.dt, irc.arc, irc.power, irc.step_size,
                       irc.arc_length, irc.converged_at, irc.n_recorded)
    keep = [t.clone() for t in watched()]
    host = (C.c_uint64 * 3)()
    for _ in range(2):  # the replay that overflows, and one more: frozen, nothing moves
        irc()
        with pytest.raises(RuntimeError, match="max_num_pairs"):
            irc.check()
        assert hip_lib.tmdnet_irc_status(None, C.c_void_p(irc._ws.data_ptr()), host) == 3 and (int(host[0]), int(host[1])) == (4, 1)
        for t, k in zip(watched(), keep):
            assert _bits(t, k)
    staged_box.copy_(box0)
    irc.reset(pos=pos)
    irc()
    assert irc.check() == 4 and not _bits(irc.pos, keep[0])


def test_check_names_each_cause_of_status_2(hip_lib):
    """13. the status word and the cause written into the workspace's header, as the controller writes them (the latches themselves
    are test 7): check() names each cause, replays change nothing, reset recovers and refuses tensors of another layout"""
    model = _model("tensornet")
    z, pos, masses = _molecule(n_saddles=1)
    q = _q("tensornet", 1)
    mode = _downhill(model, z, pos, q)
    irc = model.capture_irc(z, pos, mode, masses, steps_per_replay=4, q=q, **KW)
    irc()
    assert irc.check() == 4
    head = irc._ws[(-irc._ws.data_ptr()) % 256:][:32].view(torch.int32)
    watched = lambda: (irc.pos, irc.vel, irc.forces, irc.epot, irc.arc, irc.frames)
    for cause, text in ((1, "forces are not finite"), (2, "velocity of a path has no length"), (3, "energy is not finite")):
        head[4], head[2] = cause, 2
        irc()  # (a latched step is taken back: x and v return to where the last move began)
        with pytest.raises(RuntimeError, match=rf"step 4 .*{text}.*frozen"):
            irc.check()
        keep = [t.clone() for t in watched()]
        irc()
        with pytest.raises(RuntimeError, match=rf"step 4 .*{text}.*frozen"):
            irc.check()
        for t, k in zip(watched(), keep):
            assert _bits(t, k)
    for wrong in (dict(pos=pos.transpose(1, 2)), dict(pos=pos[:, :39]), dict(mode=mode[:, :39]), dict(mode=mode.reshape(-1, 3)[:39])):
        with pytest.raises(ValueError):
            irc.reset(**wrong)
    with pytest.raises(ValueError):
        irc.reset(mode=torch.zeros_like(mode))
    head[4], head[2] = 2, 2
    irc.reset(pos=pos[0], mode=mode)  # one saddle: [n,3] is accepted
    assert irc.check() == 0 and (irc.n_recorded == 1).all()
    irc()
    assert irc.check() == 4
    two = model.capture_irc(z, torch.cat([pos, pos]), mode[0], masses, steps_per_replay=1, q=_q("tensornet", 2), **KW)
    with pytest.raises(ValueError):
        two.reset(pos=pos[0])  # [n,3] stands for one saddle only


def test_refusals_leave_the_model_as_it_was(hip_lib):
    """14. everything capture_dimer refuses, masses that are not positive, v0 / error / initial_step / dt <= 0, dt_min > dt_max,
    capacity < 1, shapes that disagree with z, a box per path - raised before anything is staged"""
    from torchmdnet_amd.models.model import create_model

    model = _model("tensornet")
    z, pos, masses = _molecule(n_saddles=1)
    q = _q("tensornet", 1)
    mode = torch.ones(40, 3, device="cuda")
    batch = torch.arange(2, device="cuda").repeat_interleave(40)
    stacked = pos.repeat_interleave(2, 0).reshape(-1, 3)
    replay = model.capture(z.repeat(2), stacked, batch, q=q.repeat_interleave(2))
    e0, f0 = (t.clone() for t in replay(stacked))
    only_fixed = torch.zeros(40, 3, device="cuda")
    only_fixed[3, 1] = 1.0
    three = torch.zeros(40, device="cuda")
    three[3] = 1
    bad_mass = masses.clone()
    bad_mass[5] = 0.0
    base = dict(q=q, mode=mode, masses=masses, dt=0.5)
    for bad in (dict(steps_per_replay=0), dict(fmax=0.0), dict(v0=0.0), dict(v0=-0.02), dict(error=0.0), dict(initial_step=0.0), dict(dt=0.0),
                dict(dt=float("inf")), dict(dt_min=1.0, dt_max=0.5), dict(dt_min=0.0), dict(record=dict(every=1, capacity=0)),
                dict(record=dict(every=0, capacity=4)), dict(record=dict(stride=2)), dict(direction="up"), dict(masses=bad_mass),
                dict(masses=-masses), dict(masses=masses[:39]), dict(fixed=torch.zeros(3, device="cuda")), dict(q=torch.zeros(2, device="cuda")),
                dict(box=torch.eye(3).repeat(2, 1, 1).cuda()), dict(mode=torch.zeros(40, 3, device="cuda")), dict(mode=only_fixed, fixed=three),
                dict(mode=torch.ones(39, 3, device="cuda")), dict(mode=torch.ones(2, 40, 3, device="cuda"))):
        kw = dict(base, **bad)
        with pytest.raises(ValueError):
            model.capture_irc(z, pos, kw.pop("mode"), kw.pop("masses"), kw.pop("dt"), **kw)
    for bad_pos in (pos[:, :39], pos[0, 0], pos[..., :2], pos[:0]):
        with pytest.raises(ValueError):
            model.capture_irc(z, bad_pos, mode, masses, 0.5, q=q)
    with pytest.raises(NotImplementedError):
        model.capture_irc(z, pos.double(), mode, masses, 0.5, q=q)
    model.parameter_gradients = True
    try:
        with pytest.raises(NotImplementedError):
            model.capture_irc(z, pos, mode, masses, 0.5, q=q)
    finally:
        model.parameter_gradients = False
    torch.manual_seed(0)
    with pytest.raises(NotImplementedError):
        create_model(dict(W.TINY_ARGS, static_shapes=True, output_model="DipoleMoment")).to("cuda").capture_irc(z, pos, mode, masses, 0.5)
    with pytest.raises(RuntimeError, match="static_shapes"):
        create_model(dict(W.TINY_ARGS)).to("cuda").capture_irc(z, pos, mode, masses, 0.5)
    e1, f1 = replay(stacked)  # the graph captured before the refusals is still valid, and gives the same bits
    assert _bits(e1, e0) and _bits(f1, f0)


class _NeverReplayed:
    """stands in for the graph once the engine has changed: the guard has to raise before it gets here"""

    def replay(self):
        raise AssertionError("a stale graph was replayed")


def test_a_stale_irc_raises_and_replays_nothing(hip_lib):
    """15. once the engine's workspaces are re-created, a replay, a reset and a run raise instead of touching freed memory"""
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(4)
    model = create_model(dict(W.TINY_ARGS, static_shapes=True)).to("cuda")  # (its own model: the test re-creates its workspaces)
    z, pos, masses = _molecule(n_saddles=1)
    q = _q("tensornet", 1)
    irc = model.capture_irc(z, pos, _downhill(model, z, pos, q), masses, direction="forward", steps_per_replay=2, q=q, warmup=1, **KW)
    irc()
    assert irc.check() == 2 == irc.steps_done
    zb, pb, bb = W.synthetic_batch(n_mol=40, n_atoms=60)
    model(zb.cuda() % 19 + 1, pb.cuda(), bb.cuda())  # a larger system: the workspaces grow
    graph, irc.graph = irc.graph, _NeverReplayed()  # (the real graph stays alive, unreplayed, until the test ends)
    stale = r"stale HIP graph.*capture_irc\(\)"
    with pytest.raises(RuntimeError, match=stale):
        irc()
    with pytest.raises(RuntimeError, match=stale):
        irc.reset()
    with pytest.raises(RuntimeError, match=stale):
        irc.run(2)
    assert irc.steps_done == 2
    del graph


def test_reset_restarts_and_clears_the_record(hip_lib):
    """16. reset(pos=, mode=) writes the start images again, forgets both generations and the record: the run that follows has the
    bits of a fresh capture from the same start"""
    model = _model("tensornet")
    z, pos, masses = _molecule()
    q = _q("tensornet", 2)
    mode = _downhill(model, z, pos, q)
    irc = model.capture_irc(z, pos, mode, masses, steps_per_replay=4, q=q, **KW)
    irc(2)
    assert irc.check() == 8 and (irc.n_recorded[:, 0] == 9).all()
    first = [t.clone() for t in (irc.pos, irc.vel, irc.arc, irc.dt, irc.frames[:, :, :9], irc.frame_s[:, :, :9])]
    other = pos.flip(0).contiguous()
    irc.reset(pos=other, mode=mode.flip(0))
    assert irc.check() == 0 and (irc.n_recorded == 1).all() and irc.steps_done == 0 and (irc.converged_at[:, 0] == -1).all()
    assert _bits(irc.frames[:, 0, 0], irc.pos[:, 0]) and (irc.frame_s[:, :, 0] == 0).all() and (irc.step_size == KW["dt"]).all()
    irc()
    assert irc.check() == 4 and (irc.n_recorded[:, 0] == 5).all()
    irc.reset(pos=pos, mode=mode)
    irc(2)
    assert irc.check() == 8
    for t, k in zip((irc.pos, irc.vel, irc.arc, irc.dt, irc.frames[:, :, :9], irc.frame_s[:, :, :9]), first):
        assert _bits(t, k)
