"""-m gpu: the device-resident FIRE minimiser (csrc/tn_min.hip, TorchMD_Net.capture_minimize).

1.-5. the C entries alone (no model, graph_ws = NULL) on harmonic wells whose forces torch computes between the calls: every step
      against a torch mirror and tests/min_oracle.py, the end state, an interleaved batch, frozen molecules, repeatability,
      and a molecule large enough for two slices
6.    through the model: K steps per graph launch are bit-identical to capture() + a torch mirror that takes the device's
      coefficients and evaluates the update one rounded operation at a time (torch.mul, then torch.add)
7.    overflow: the state freezes at the last valid step;  8. a NaN force: status 2;  9. refusals;  10. opt.run"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import min_oracle as O
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

OPEN, MIDDLE, CLOSE = 0, 1, 2
P = dict(O.FIRE, fmax=1e-3)  # ASE's defaults, the bound of the wells


def _bits(a, b):
    if a.dtype == torch.float64:
        return a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ the C entries alone
class _Raw:
    """The C entries on tensors of the test's own, m = graph_ws = NULL (no model: the forces are whatever `forces` holds)."""

    def __init__(self, lib, pos, batch, n_mol, p, fixed=None):
        self.L, self.n, self.n_mol, self.p = lib, pos.shape[0], n_mol, p
        self.pos, self.vel = pos.clone().contiguous(), torch.zeros_like(pos)
        self.batch, self.fixed = batch, fixed
        nb = C.c_size_t(0)
        assert lib.tmdnet_min_workspace_bytes(self.n, n_mol, C.byref(nb)) == 0
        self.ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        nan = float("nan")
        self.forces = torch.full_like(pos, nan)  # forces_keep
        self.fmax = torch.full((n_mol,), nan, device="cuda")
        self.sums = torch.full((n_mol, 4), nan, dtype=torch.float64, device="cuda")
        self.coef = torch.full((n_mol, 3), nan, device="cuda")
        self.dt, self.alpha = (torch.full((n_mol,), nan, dtype=torch.float64, device="cuda") for _ in range(2))
        self.conv = torch.full((n_mol,), -7, dtype=torch.int64, device="cuda")
        assert lib.tmdnet_min_reset(self._s(), self._p(self.ws), 0, p["dt"], p["alpha"]) == 0

    @staticmethod
    def _s():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def advance(self, phase, forces):
        p, f = self._p, self.p
        logs = [None] * 7 if phase == OPEN else [None] + [p(t) for t in (self.fmax, self.sums, self.coef, self.dt, self.alpha, self.conv)]
        rc = self.L.tmdnet_min_advance(None, self._s(), None, p(self.ws), self.n, self.n_mol, phase, p(self.pos), p(self.vel), p(forces),
                                       None, p(self.fixed), p(self.batch), None if phase == OPEN else p(self.forces), f["dt_max"],
                                       f["n_min"], f["f_inc"], f["f_dec"], f["alpha"], f["f_alpha"], f["max_step"], f["fmax"], *logs)
        assert rc == 0, rc

    def status(self):
        host = (C.c_uint64 * 2)()
        rc = self.L.tmdnet_min_status(self._s(), self._p(self.ws), host)
        return rc, int(host[0]), int(host[1])

    def logs(self):
        return [t.clone() for t in (self.fmax, self.sums, self.coef, self.dt, self.alpha, self.conv)]


def _dot(a, b):
    """(ax bx + ay by) + az bz, every product and every sum its own rounded fp32 kernel"""
    return torch.add(torch.add(torch.mul(a[:, 0], b[:, 0]), torch.mul(a[:, 1], b[:, 1])), torch.mul(a[:, 2], b[:, 2]))


def _terms(v, f, fixed):
    """the mirror's fp32 terms [N,3]: v.f, f.f, v.v; a fixed atom contributes nothing"""
    t = torch.stack([_dot(f, v), _dot(f, f), _dot(v, v)], 1)
    return t if fixed is None else torch.where(fixed.bool()[:, None], torch.zeros_like(t), t)


def _move(x, v, f, coef, conv, batch, fixed):
    """the per-atom update with the device's coefficients, torch.mul then torch.add; frozen molecule or fixed atom: v = 0"""
    c = coef[batch]
    still = conv[batch] >= 0
    if fixed is not None:
        still = still | fixed.bool()
    v_new = torch.add(torch.mul(c[:, 0:1], v), torch.mul(c[:, 1:2], f))
    x_new = torch.add(x, torch.mul(c[:, 2:3], v_new))
    return torch.where(still[:, None], x, x_new), torch.where(still[:, None], torch.zeros_like(v), v_new)


def _check_sums(dev_sums, terms, batch, n_mol, where):
    """Each device sum within n 2^-52 sum|t| of the exact sum (math.fsum) of the mirror's fp32 terms - the worst case of any fp64
    summation order over n terms is (n - 1) 2^-53 sum|t| -, and fmax2 equal to their maximum."""
    t, b, d = terms.double().cpu().numpy(), batch.cpu().numpy(), dev_sums.cpu().numpy()
    for m in range(n_mol):
        tm = t[b == m]
        for k in range(3):
            exact, bound = math.fsum(tm[:, k]), len(tm) * 2.0 ** -52 * math.fsum(np.abs(tm[:, k]))
            assert abs(d[m, k] - exact) <= bound, (where, m, k, d[m, k], exact, bound)
        assert d[m, 3] == (tm[:, 1].max() if len(tm) else 0.0), (where, m)


def _check_control(state, p, dev, step, where):
    """the oracle fed with the device's sums: dt, alpha, converged_at equal (single IEEE operations), the coefficients within 1 ulp
    (the device compiler may contract an fp64 product into the sum that consumes it)"""
    fmax, sums, coef, dt, alpha, conv = (t.cpu().numpy() for t in dev)
    for m, s in enumerate(state):
        ret, c = O.control(s, p, *sums[m], step)
        assert ret != O.UNUSABLE
        assert dt[m] == s["dt"] and alpha[m] == s["alpha"] and conv[m] == s["converged_at"], (where, m, dt[m], alpha[m], conv[m], s)
        assert O.ulp_distance(coef[m], np.array(c, np.float32)).max() <= 1, (where, m, coef[m], c)
        assert fmax[m] == np.float32(math.sqrt(sums[m, 3])), (where, m)


def _problem(interleave=False):
    """the five wells of tests/min_oracle.py plus a sixth molecule index without atoms, and a few fixed atoms"""
    batch, kspring, x0, x = O.wells_problem(interleave=interleave)
    fixed = np.zeros(len(batch), np.uint8)
    fixed[[2, 50, 51, 700, 1607]] = 1
    return batch, kspring, x0, x, fixed


_runs = {}


def _drive(lib, interleave=False, fused=False, checks=True, cache=True):
    """Minimise the wells through the C entries, the forces from torch between the calls: per step OPEN, forces, CLOSE (fused: one
    OPEN, then forces, MIDDLE).  With `checks`, every step against the mirror and the oracle.  -> dict of the end state and (not
    fused) the positions, velocities and converged_at of every step."""
    key = (interleave, fused)
    if cache and key in _runs:
        return _runs[key]
    batch_np, kspring, x0, x, fixed_np = _problem(interleave)
    batch, fixed = torch.from_numpy(batch_np).cuda(), torch.from_numpy(fixed_np).cuda()
    k_t, x0_t, x_t = (torch.from_numpy(a).cuda() for a in (kspring[:, None], x0, x))
    force = lambda pos: -(k_t * (pos - x0_t))
    n_mol = 6
    steps_ref, conv_ref, _ = O.wells(batch_np, n_mol, kspring, x0, x, P, 1000, fixed_np)  # the oracle's own count
    limit = int(1.25 * steps_ref + 5)
    raw = _Raw(lib, x_t, batch, n_mol, P, fixed)
    state = O.new_state(P, n_mol)
    f = force(raw.pos)
    raw.advance(CLOSE, f)  # the start geometry: counts no step
    xm, vm = x_t.clone(), torch.zeros_like(x_t)
    if checks:
        _check_sums(raw.sums, _terms(vm, f, fixed), batch, n_mol, "start")
        _check_control(state, P, raw.logs(), 0, "start")
    assert raw.status() == (0, 0, 0) and _bits(raw.forces, f)
    hist = dict(pos=[raw.pos.clone()], vel=[raw.vel.clone()], conv=[raw.conv.clone()])  # (unfused only) the state at every step
    step = 0
    while step < limit and not bool((raw.conv >= 0).all()):
        xm, vm = _move(xm, vm, f, raw.coef, raw.conv, batch, fixed)  # the logs of the control of `step`, and the forces it saw
        if not fused or step == 0:
            raw.advance(OPEN, raw.forces)  # (fused: the MIDDLE below has made this move already)
        if checks:
            assert _bits(raw.pos, xm) and _bits(raw.vel, vm), step
        step += 1
        f = force(raw.pos)
        raw.advance(MIDDLE if fused else CLOSE, f)
        if checks:
            _check_sums(raw.sums, _terms(vm, f, fixed), batch, n_mol, step)
            _check_control(state, P, raw.logs(), step, step)
        if not fused:
            assert _bits(raw.forces, f)
            hist["pos"].append(raw.pos.clone())
            hist["vel"].append(raw.vel.clone())
            hist["conv"].append(raw.conv.clone())
    assert raw.status() == (0, step, 0)
    out = dict(raw=raw, steps=step, limit=limit, conv_ref=conv_ref, batch=batch, fixed=fixed, x_start=x_t, x0=x0_t, k=k_t, hist=hist)
    if cache:
        _runs[key] = out
    return out


def test_every_step_equals_the_mirror_and_the_oracle(hip_lib):
    """1. OPEN / CLOSE per step: x and v bit-identical to the torch mirror fed with the device's coefficients, the sums within the
    fp64 summation bound of the mirror's terms, dt / alpha / converged_at equal to the oracle fed with the device's sums, the
    coefficients within 1 ulp.  (The assertions are in _drive.)"""
    r = _drive(hip_lib)
    assert r["steps"] > 30 and not _bits(r["raw"].pos, r["x_start"])


def _check_end_state(r):
    raw = r["raw"]
    conv = raw.conv.cpu().numpy()
    print("converged at", conv.tolist(), "oracle", r["conv_ref"].tolist())
    assert (conv >= 0).all()
    assert (conv <= 1.25 * r["conv_ref"] + 5).all() and r["steps"] == conv.max()
    assert conv[5] == 0 and r["conv_ref"][5] == 0  # no atoms: converged as it stands
    for t in (raw.pos, raw.vel, raw.forces, raw.fmax, raw.sums, raw.coef, raw.dt, raw.alpha):
        assert torch.isfinite(t).all()
    free = ~r["fixed"].bool()
    assert (r["k"] * (raw.pos - r["x0"])).abs()[free].max().item() < 1e-3  # at the minimum
    assert _bits(raw.pos[~free], r["x_start"][~free]) and (raw.vel[~free] == 0).all()  # fixed atoms never moved
    assert (raw.fmax < 1e-3).all() and len(set(raw.dt.tolist())) > 2  # every molecule its own controller


def test_end_state(hip_lib):
    """2. every molecule converged within 1.25 n_ref + 5 steps (n_ref: the fp64 oracle's own count for that molecule; the margin
    covers a controller branch decided differently near vf = 0), the empty molecule at step 0, no NaN anywhere."""
    _check_end_state(_drive(hip_lib))
    fused = _drive(hip_lib, fused=True)  # one OPEN, then MIDDLE after every evaluation: the same minimisation
    _check_end_state(fused)
    assert _bits(fused["raw"].pos, _drive(hip_lib)["raw"].pos) and torch.equal(fused["raw"].conv, _drive(hip_lib)["raw"].conv)
    assert (fused["raw"].vel == 0).all()  # the MIDDLE that found everything converged froze it


def test_interleaved_batch(hip_lib):
    """3. the same with the atoms of the molecules interleaved: no molecule is a contiguous range"""
    r = _drive(hip_lib, interleave=True)
    b = r["batch"].cpu().numpy()
    assert (np.diff(b) < 0).sum() > 100
    _check_end_state(r)


def test_frozen_after_convergence(hip_lib):
    """4. once converged_at[m] >= 0 the molecule's x keeps its bits and v = 0 while the others still move; converged_at never changes"""
    r = _drive(hip_lib)
    h, batch = r["hist"], r["batch"]
    final = h["conv"][-1]
    order = torch.argsort(final[:5])
    first, last = int(order[0]), int(order[-1])
    assert int(final[first]) + 10 < int(final[last])
    for m in range(5):
        at = int(final[m])
        mine = batch == m
        for s in range(at, len(h["pos"])):
            assert int(h["conv"][s][m]) == at
            assert _bits(h["pos"][s][mine], h["pos"][at][mine]), (m, s)
            if s > at:
                assert (h["vel"][s][mine] == 0).all(), (m, s)
        assert all(int(c[m]) == -1 for c in h["conv"][:at])
    others = batch == last
    assert not _bits(h["pos"][int(final[first]) + 5][others], h["pos"][int(final[first])][others])  # the others still moved


def test_two_runs_are_bit_identical(hip_lib):
    """5. fixed summation order, no floating-point atomics"""
    a = _drive(hip_lib, fused=True, checks=False, cache=False)["raw"]
    b = _drive(hip_lib, fused=True, checks=False, cache=False)["raw"]
    for s, t in zip([a.pos, a.vel, a.forces] + a.logs()[:5], [b.pos, b.vel, b.forces] + b.logs()[:5]):
        assert _bits(s, t)
    assert torch.equal(a.conv, b.conv)


def test_one_large_molecule_in_two_slices(hip_lib):
    """1 500 atoms in ONE molecule without a batch vector: two slices of 750, added in slice order by the controller"""
    g = torch.Generator().manual_seed(12)
    x0 = (4 * torch.randn(1500, 3, generator=g)).cuda()
    x = x0 + (0.3 * torch.randn(1500, 3, generator=g)).cuda()
    raw = _Raw(hip_lib, x, None, 1, P)
    batch = torch.zeros(1500, dtype=torch.long, device="cuda")
    state = O.new_state(P, 1)
    v = torch.zeros_like(x)
    f = -4.0 * (raw.pos - x0)
    raw.advance(CLOSE, f)
    for step in range(1, 9):
        _check_sums(raw.sums, _terms(v, f, None), batch, 1, step)
        _check_control(state, P, raw.logs(), step - 1, step)
        xm, v = _move(raw.pos.clone(), v, f, raw.coef, raw.conv, batch, None)
        raw.advance(OPEN, raw.forces)
        assert _bits(raw.pos, xm) and _bits(raw.vel, v)
        f = -4.0 * (raw.pos - x0)
        raw.advance(CLOSE, f)
    assert raw.status() == (0, 8, 0)


def test_nan_force_latches_status_2(hip_lib):
    """8. a NaN force through the C entry: status 2, nothing of that step is written, every later launch returns at once"""
    batch_np, kspring, x0, x, _ = _problem()
    batch = torch.from_numpy(batch_np).cuda()
    k_t, x0_t, x_t = (torch.from_numpy(a).cuda() for a in (kspring[:, None], x0, x))
    raw = _Raw(hip_lib, x_t, batch, 6, P)
    f = -(k_t * (raw.pos - x0_t))
    raw.advance(CLOSE, f)
    for _ in range(3):
        raw.advance(OPEN, raw.forces)
        f = -(k_t * (raw.pos - x0_t))
        raw.advance(CLOSE, f)
    assert raw.status() == (0, 3, 0)
    raw.advance(OPEN, raw.forces)
    keep = [t.clone() for t in [raw.pos, raw.vel, raw.forces] + raw.logs()]
    bad = -(k_t * (raw.pos - x0_t))
    bad[1234, 1] = float("nan")
    raw.advance(CLOSE, bad)
    assert raw.status() == (5, 3, 2)
    raw.advance(OPEN, raw.forces)
    raw.advance(MIDDLE, f)
    raw.advance(CLOSE, f)
    assert raw.status() == (5, 3, 2)
    for t, k in zip([raw.pos, raw.vel, raw.forces] + raw.logs(), keep):
        assert _bits(t, k) if t.is_floating_point() else torch.equal(t, k)
    # an infinite force in a molecule that has converged is not looked at; in one that moves it is
    raw2 = _Raw(hip_lib, x_t, batch, 6, dict(P, fmax=1e6))
    raw2.advance(CLOSE, f)
    assert (raw2.conv == 0).all()
    raw2.advance(OPEN, raw2.forces)
    raw2.advance(CLOSE, bad)
    assert raw2.status() == (0, 1, 0) and _bits(raw2.pos, x_t)


def test_more_molecules_than_controller_threads(hip_lib):
    """257 molecules of 2 atoms: the one-block controller (256 threads) takes a second trip over its units, in both passes.  Every
    step against the host mirror (tests/min_host.hip), for every molecule: the sums equal - a slice of two atoms is
    (0 + t_0) + (0 + t_1), one rounding, whatever the reduction's order -, dt / alpha / converged_at and fmax equal to the mirror's
    controller, which carries its own state from step to step; the coefficients within 1 ulp (fp32 roundings of fp64 results into
    which the device compiler may contract a product, as in _check_control); x and v bit-identical to the mirror's update.  Then
    the same shape with a force that is not finite in molecule 256 only - the last unit of the second trip: status 2, and no row,
    state or counter is written."""
    from tests import min_host_mirror as MH

    B, n = 257, 2
    rng = np.random.default_rng(257)
    batch_np = np.repeat(np.arange(B), n)
    k = (0.5 + 4.0 * rng.random(B)).astype(np.float32)[batch_np][:, None]
    x0 = rng.standard_normal((B * n, 3)).astype(np.float32)
    x = (x0 + 0.3 * rng.standard_normal((B * n, 3))).astype(np.float32)
    for m in (5, 200):  # one molecule of each trip starts at its minimum: converged as it stands
        x[batch_np == m] = x0[batch_np == m]
    fixed_np = np.zeros(B * n, np.uint8)
    fixed_np[[3, 2 * 256 + 1]] = 1  # an atom of molecule 1 and one of molecule 256
    batch, fixed = torch.from_numpy(batch_np).cuda(), torch.from_numpy(fixed_np).cuda()
    k_t, x0_t, x_t = (torch.from_numpy(a).cuda() for a in (k, x0, x))
    force = lambda pos: -(k_t * (pos - x0_t))

    def controlled(raw, state, xm, vm, f, step):
        """the control of `step` on the mirror; the device's logs against it -> the mirror's new state"""
        t = MH.terms(vm, f.cpu().numpy(), fixed_np).astype(np.float64).reshape(B, n, 3)
        sums = np.concatenate([(0.0 + t[:, 0]) + (0.0 + t[:, 1]), np.maximum(t[:, :, 1].max(1), 0.0)[:, None]], 1)
        state, coef, ret = MH.control(state, sums, P, step)
        assert (ret != 2).all()
        fmax, dsums, dcoef, dt, alpha, conv = (a.cpu().numpy() for a in raw.logs())
        assert np.array_equal(dsums, sums), step
        assert np.array_equal(dt, state[0]) and np.array_equal(alpha, state[1]) and np.array_equal(conv, state[3]), step
        assert np.array_equal(fmax, np.sqrt(sums[:, 3]).astype(np.float32)), step
        assert O.ulp_distance(dcoef, coef).max() <= 1, step
        return state

    raw = _Raw(hip_lib, x_t, batch, B, P, fixed)
    state = (np.full(B, P["dt"]), np.full(B, P["alpha"]), np.zeros(B, np.int32), np.full(B, -1, np.int64))
    xm, vm = x.copy(), np.zeros_like(x)
    f = force(raw.pos)
    raw.advance(CLOSE, f)
    state = controlled(raw, state, xm, vm, f, 0)
    assert raw.status() == (0, 0, 0) and state[3][5] == 0 and state[3][200] == 0 and (state[3] >= 0).sum() == 2
    steps = 12
    for step in range(1, steps + 1):
        xm, vm = MH.update(batch_np, state[3], fixed_np, raw.coef.cpu().numpy(), xm, vm, raw.forces.cpu().numpy())
        raw.advance(OPEN, raw.forces)
        assert np.array_equal(raw.pos.cpu().numpy().view(np.int32), xm.view(np.int32)), step
        assert np.array_equal(raw.vel.cpu().numpy().view(np.int32), vm.view(np.int32)), step
        f = force(raw.pos)
        raw.advance(CLOSE, f)
        state = controlled(raw, state, xm, vm, f, step)
        assert _bits(raw.forces, f)
    assert raw.status() == (0, steps, 0)
    assert len(set(raw.dt.tolist())) > 1 and (raw.conv[[0, 255, 256]] < 0).all()  # molecules of both trips still move
    # a NaN in molecule 256 only
    raw.advance(OPEN, raw.forces)
    keep = [t.clone() for t in [raw.pos, raw.vel, raw.forces] + raw.logs()]
    good = force(raw.pos)
    bad = good.clone()
    bad[2 * 256, 2] = float("nan")
    raw.advance(CLOSE, bad)
    assert raw.status() == (5, steps, 2)
    raw.advance(OPEN, raw.forces)
    raw.advance(MIDDLE, good)
    raw.advance(CLOSE, good)
    assert raw.status() == (5, steps, 2)
    for t, kept in zip([raw.pos, raw.vel, raw.forces] + raw.logs(), keep):
        assert _bits(t, kept) if t.is_floating_point() else torch.equal(t, kept)


# ------------------------------------------------------------------------------------------------ through the model
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
    """-> z, pos, batch, box (CPU): the systems of tests/test_gpu_md_loop.py, and a ragged batch of 1 000 atoms"""
    if name == "mol40":
        z, pos, batch = W.synthetic_batch(n_mol=1, n_atoms=40, first_seed=31)
        return z % 8 + 1, pos, batch, None
    if name in ("ragged", "ragged1000"):
        sizes, density = ([7, 12, 20], 0.1) if name == "ragged" else ([300, 333, 367], 0.05)
        zs, ps, bs = [], [], []
        for m, n in enumerate(sizes):
            z, p = W.synthetic_molecule(40 + m, n, density=density)
            zs.append(torch.from_numpy(z))
            ps.append(torch.from_numpy(p) + 3.0 * m)
            bs.append(torch.full((n,), m, dtype=torch.long))
        return torch.cat(zs), torch.cat(ps), torch.cat(bs), None
    z, pos, box = W.water_box(n_side=4)  # 192 atoms, periodic
    return z, pos, torch.zeros_like(z), box


def _inputs(arch, name):
    z, pos, batch, box = (None if t is None else t.cuda() for t in _system(name))
    n_mol = int(batch.max()) + 1
    q = torch.zeros(n_mol, device="cuda") if arch != "equivariant-transformer" else None
    return z, pos, batch, box, q


def _minimise(model, inputs, K, replays, **kw):
    z, pos, batch, box, q = inputs
    opt = model.capture_minimize(z, pos, batch=batch, box=box, q=q, steps_per_replay=K, **kw)
    start = [t.clone() for t in (opt.coef0, opt.converged_at, opt.epot0, opt.fmax0)]
    logs = dict(epot=[], fmax=[], coef=[], sums=[], conv=[], dt=[])
    for _ in range(replays):
        opt()
        for key, t in (("epot", opt.epot), ("fmax", opt.fmax), ("coef", opt.coef), ("sums", opt.sums)):
            logs[key].append(t.clone())
        logs["conv"].append(opt.converged_at.clone())
        logs["dt"].append(opt.step_size.clone())
    assert opt.check() == K * replays == opt.steps_done
    return opt, start, {k: (torch.cat(v) if k in ("epot", "fmax", "coef", "sums") else v) for k, v in logs.items()}


@pytest.mark.parametrize("arch,name", [("tensornet", "mol40"), ("equivariant-transformer", "mol40"), ("tensornet2", "mol40"),
                                       ("tensornet", "ragged"), ("tensornet", "ragged1000"), ("tensornet", "water192")])
def test_minimisation_is_bit_identical_to_capture_plus_torch_mirror(hip_lib, arch, name):
    """6. 16 steps, one per replay, against capture() and the torch mirror fed with the device's coefficients: positions, forces,
    energies equal bit for bit, the sums (mstart..mend ranges of the graph workspace) within the summation bound; then 8 x 2 and
    16 x 1 replays give the same bits."""
    model, inputs = _model(arch), _inputs(arch, name)
    z, pos, batch, box, q = inputs
    n_mol = int(batch.max()) + 1
    fixed = torch.zeros(z.shape[0], dtype=torch.bool, device="cuda")
    fixed[::11] = True
    kw = dict(fmax=1e-4, fixed=fixed)
    replay = model.capture(z, pos, batch, box, q=q)
    opt, start, logs = _minimise(model, inputs, 1, 16, **kw)
    x, v = pos.clone(), torch.zeros_like(pos)
    e, f = (t.clone() for t in replay(x))
    assert _bits(start[2], e.view(-1)) and (start[1] == -1).all()
    _check_sums(opt._sums0, _terms(v, f, fixed), batch, n_mol, "start")
    coef, conv = start[0], start[1]
    for s in range(16):
        x, v = _move(x, v, f, coef, conv, batch, fixed)
        e, f = (t.clone() for t in replay(x))
        assert _bits(logs["epot"][s], e.view(-1)), s
        _check_sums(logs["sums"][s], _terms(v, f, fixed), batch, n_mol, s)
        ff = torch.where(fixed, 0.0, _dot(f, f))
        fmax = torch.stack([ff[batch == m].max() for m in range(n_mol)]).double().sqrt().float()
        assert _bits(logs["fmax"][s], fmax), s
        coef, conv = logs["coef"][s], logs["conv"][s]
    assert _bits(opt.pos, x) and _bits(opt.forces, f)
    assert (x - pos).abs().max().item() > 1e-3 and _bits(x[fixed], pos[fixed])  # the atoms really moved, the fixed ones did not
    for K, replays in ((8, 2), (16, 1)):
        opt2, start2, logs2 = _minimise(model, inputs, K, replays, **kw)
        assert _bits(opt2.pos, opt.pos) and _bits(opt2.forces, opt.forces) and _bits(opt2.vel, opt.vel), (K, replays)
        for key in ("epot", "fmax", "coef", "sums"):
            assert _bits(logs2[key], logs[key]), (K, replays, key)
        assert torch.equal(logs2["conv"][-1], logs["conv"][-1]) and _bits(logs2["dt"][-1], logs["dt"][-1])
    # reset: back to the start, the same minimisation again
    opt2.reset(pos=pos)
    assert _bits(opt2.coef0, start[0]) and (opt2.vel == 0).all() and opt2.check() == 0
    opt2()
    assert _bits(opt2.pos, opt.pos) and _bits(opt2.forces, opt.forces) and opt2.check() == 16


def test_overflow_freezes_the_state_at_the_last_valid_step(hip_lib):
    """7. the 192-atom periodic box with max_num_neighbors = 72, scaled by 0.85 between two replays (box and positions in place): the
    first evaluation of the second replay overflows."""
    model = _model("tensornet", max_num_neighbors=72)
    z, pos, batch, box = (t.cuda() for t in _system("water192"))
    box = box.clone()
    box0 = box.clone()
    q = torch.zeros(1, device="cuda")
    opt = model.capture_minimize(z, pos, batch=batch, box=box, q=q, steps_per_replay=4, fmax=1e-4)
    opt()
    assert opt.check() == 4
    box.mul_(0.85)
    opt.pos.mul_(0.85)
    watched = lambda: (opt.pos, opt.vel, opt.forces, opt.epot, opt.fmax, opt.coef, opt.sums, opt.step_size, opt.alpha, opt.converged_at)
    keep = [t.clone() for t in watched()]
    host = (C.c_uint64 * 2)()
    for _ in range(2):  # the replay that overflows, and one more: frozen, nothing moves
        opt()
        with pytest.raises(RuntimeError, match="max_num_pairs"):
            opt.check()
        assert hip_lib.tmdnet_min_status(None, C.c_void_p(opt._ws.data_ptr()), host) == 3 and (int(host[0]), int(host[1])) == (4, 1)
        for t, k in zip(watched(), keep):
            assert torch.equal(t, k) if not t.is_floating_point() else _bits(t, k)
    # the model evaluates eagerly afterwards, and the loop runs again after a reset at a geometry that fits
    box.copy_(box0)
    E, F = model(z, pos, batch, box=box, q=q)
    assert torch.isfinite(E).all() and torch.isfinite(F).all()
    opt.reset(pos=pos)
    opt()
    assert opt.check() == 4 and not _bits(opt.pos, keep[0])


def test_check_names_the_forces_after_status_2(hip_lib):
    """8. (through the object) a NaN force handed to the C entry on the minimiser's own workspace: check() names the forces, replays
    change nothing, reset recovers"""
    from torchmdnet_amd.minimize import MIN_CLOSE

    model, inputs = _model("tensornet"), _inputs("tensornet", "ragged")
    z, pos, batch, box, q = inputs
    opt = model.capture_minimize(z, pos, batch=batch, q=q, steps_per_replay=2, fmax=1e-4)
    opt()
    assert opt.check() == 2
    keep = [t.clone() for t in (opt.pos, opt.vel, opt.forces, opt.epot, opt.fmax)]
    bad = opt.forces.clone()
    bad[5, 0] = float("nan")
    opt._advance(MIN_CLOSE, bad, None, 0)
    with pytest.raises(RuntimeError, match="forces"):
        opt.check()
    opt()
    with pytest.raises(RuntimeError, match="not finite"):
        opt.check()
    for t, k in zip((opt.pos, opt.vel, opt.forces, opt.epot, opt.fmax), keep):
        assert _bits(t, k)
    opt.reset()
    opt()
    assert opt.check() == 2 and not _bits(opt.pos, keep[0])


def test_refusals_leave_the_model_as_it_was(hip_lib):
    """9."""
    from torchmdnet_amd.models.model import create_model

    model = _model("tensornet")
    z, pos, batch, _, q = _inputs("tensornet", "ragged")
    replay = model.capture(z, pos, batch, q=q)
    e0, f0 = (t.clone() for t in replay(pos))
    with pytest.raises(ValueError):
        model.capture_minimize(z, pos, batch=batch, q=q, steps_per_replay=0)
    with pytest.raises(ValueError):
        model.capture_minimize(z, pos, batch=batch, q=q, fire=dict(timestep=0.1))
    with pytest.raises(ValueError):
        model.capture_minimize(z, pos, batch=batch, q=q, fmax=0.0)
    with pytest.raises(ValueError):
        model.capture_minimize(z, pos, batch=batch, q=q, fixed=torch.zeros(3, device="cuda"))
    with pytest.raises(NotImplementedError):
        model.capture_minimize(z, pos, batch=batch, q=q, atom_weights=torch.ones(z.shape[0], device="cuda"))
    with pytest.raises(NotImplementedError):
        model.capture_minimize(z, pos, batch=batch, q=q, halo_exchange=lambda *a: None)
    model.parameter_gradients = True
    try:
        with pytest.raises(NotImplementedError):
            model.capture_minimize(z, pos, batch=batch, q=q)
    finally:
        model.parameter_gradients = False
    torch.manual_seed(0)
    with pytest.raises(NotImplementedError):
        create_model(dict(W.TINY_ARGS, static_shapes=True, output_model="DipoleMoment")).to("cuda").capture_minimize(z, pos, batch=batch)
    with pytest.raises(RuntimeError, match="static_shapes"):
        create_model(dict(W.TINY_ARGS)).to("cuda").capture_minimize(z, pos, batch=batch)
    e1, f1 = replay(pos)  # the graph captured before the refusals is still valid, and gives the same bits
    assert _bits(e1, e0) and _bits(f1, f0)


def test_run_stops_at_convergence_or_at_max_steps(hip_lib):
    """10."""
    model, inputs = _model("tensornet"), _inputs("tensornet", "ragged")
    z, pos, batch, box, q = inputs
    opt = model.capture_minimize(z, pos, batch=batch, q=q, steps_per_replay=4, fmax=1e6)  # above every force: converged as it stands
    assert opt.run(100) == 0 and _bits(opt.pos, pos) and (opt.converged_at == 0).all() and opt.check() == 0
    assert (opt.fmax0 > 0).all() and (opt.fmax0 < 1e6).all()
    opt = model.capture_minimize(z, pos, batch=batch, q=q, steps_per_replay=4, fmax=1e-7)  # below what 20 steps reach
    assert opt.run(20, check_every=2) == 20 and opt.check() == 20 and (opt.converged_at == -1).all()
    assert opt.run(7) == 4 and opt.check() == 24  # whole replays only, never beyond max_steps
    assert not _bits(opt.pos, pos)
