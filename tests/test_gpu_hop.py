"""Minima hopping on the GPU (csrc/tn_hop.hip).  Part 1 drives the C entries alone (m = graph_ws = NULL), with energies and forces of
closed-form surfaces computed on the host in fp64 at the device's fp32 positions and rounded once, and checks every step against the
host mirror of the header (tests/hop_host_mirror.py).  Part 2 goes through ``TorchMD_Net.capture_minima_hopping`` for TensorNet, the
Equivariant Transformer and TensorNet2.

What is compared how.  Everything is compared bit for bit - positions, velocities, every sum, coefficient, counter, kT, ediff, the
ring - with ONE exception: the velocities a launch draws go through logf, sqrtf and cosf / sinf (tn_md::normals3), which the device
does not round as the host does.  Each of the three is allowed one fp32 ulp at the place it enters: a drawn velocity must lie in the
interval the host's statements span when the results of logf, sqrtf and cosf / sinf each move by at most one ulp (``_draw_bounds``).
The mirror then goes on from the device's velocities, so that every other quantity stays bit for bit.  That interval is what is
asserted.  The distance of a drawn velocity from the host's own, in ulp of the product, is only printed: on an MI355X up to 3 for
the chains, 4 for the ragged batch and 5 for the 1 100 atoms - the ulp of a factor is up to twice the ulp of the product."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import hop_host_mirror as H
from tests import hop_oracle as O
from torchmdnet_amd import _C
from torchmdnet_amd import hop as HP
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
_models = {}


def _bits(a, b):
    if not a.is_floating_point():
        return a.shape == b.shape and torch.equal(a, b)
    view = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _np_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def _ulps(a, b):
    """the largest distance of a from b in units of the spacing of fp32 at the larger of the two"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    gap = np.maximum(np.spacing(np.abs(a)), np.spacing(np.abs(b))).astype(np.float64)
    return float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / gap).max())


def _draw_bounds(seed, hops, atoms, vscale, sig):
    """[lo, hi] per component of the velocities tn_hop::atom_apply draws for the caller's atoms `atoms` of walkers with hop counts
    `hops`: the statements of tn_md::normals3 in fp32 numpy with the result of logf, of sqrtf and of cosf / sinf each moved by -1, 0
    or +1 ulp - one ulp where a device transcendental enters, nothing anywhere else"""
    from tests import md_oracle as M

    f32 = np.float32
    w = np.array([M.philox4x32_10((int(h) & M.MASK, int(h) >> 32, int(i), 2), (seed & M.MASK, seed >> 32)) for h, i in zip(hops, atoms)],
                 dtype=np.uint64)
    u = ((w >> np.uint64(8)).astype(f32) + f32(0.5)) * f32(2.0 ** -24)
    s = f32(vscale) * f32(sig)

    def nudge(x, k):
        return x if k == 0 else np.nextafter(x, f32(np.inf) * f32(k), dtype=f32)

    out = []
    for kl in (-1, 0, 1):
        for ks in (-1, 0, 1):
            for kc in (-1, 0, 1):
                r = [nudge(np.sqrt(f32(-2.0) * nudge(np.log(u[:, c]), kl)), ks) for c in (0, 2)]
                a = [f32(6.283185307179586) * u[:, c] for c in (1, 3)]
                xi = np.stack([r[0] * nudge(np.cos(a[0]), kc), r[0] * nudge(np.sin(a[0]), kc), r[1] * nudge(np.cos(a[1]), kc)], 1)
                assert xi.dtype == f32
                out.append(s[:, None] * xi)
    out = np.stack(out)
    return out.min(0), out.max(0)


# ------------------------------------------------------------------------------------------------ the C entries alone
STATE = ("pos", "vel", "forces", "minimum_pos", "best_pos", "ring_pos", "ring_energy", "ring_found", "ring_visits", "kT", "ediff",
         "minimum_energy", "best_energy", "phase", "counters")
LOGS = ("epot", "fmax", "ekin", "phase_log", "outcome", "sums", "coef")


class _Raw:
    """The C entries on tensors of the test's own: the buffers of ``HostHop`` under the same names, on the device."""

    def __init__(self, lib, host):
        self.L, self.host = lib, host
        self.N, self.B, self.params = host.n_atoms, host.n_mol, host.params
        for name in STATE + LOGS + ("hk", "masses", "sig", "batch"):
            setattr(self, name, torch.from_numpy(getattr(host, name).copy()).cuda())
        self.fixed = None if host.fixed is None else torch.from_numpy(host.fixed.copy()).cuda()
        self.energy, self.f_in = torch.zeros(self.B, device="cuda"), torch.zeros((self.N, 3), device="cuda")
        nb = C.c_size_t(0)
        assert lib.tmdnet_hop_workspace_bytes(self.N, self.B, self.params["capacity"], C.byref(nb)) == 0
        self.ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        a = HP.fill_args(_C.HopArgs(), self.params)
        for name, t in (("pos", self.pos), ("vel", self.vel), ("forces", self.f_in), ("energy", self.energy), ("hk", self.hk),
                        ("mass", self.masses), ("sig", self.sig), ("fixed", self.fixed), ("batch", self.batch),
                        ("forces_keep", self.forces), ("cur_pos", self.minimum_pos), ("best_pos", self.best_pos),
                        ("ring_pos", self.ring_pos), ("ring_energy", self.ring_energy), ("ring_found", self.ring_found),
                        ("ring_visits", self.ring_visits), ("kT", self.kT), ("ediff", self.ediff), ("cur_energy", self.minimum_energy),
                        ("best_energy", self.best_energy), ("phase", self.phase), ("counters", self.counters), ("epot_row", self.epot),
                        ("fmax_row", self.fmax), ("ekin_row", self.ekin), ("phase_row", self.phase_log), ("outcome_row", self.outcome),
                        ("sums_row", self.sums), ("coef_row", self.coef)):
            setattr(a, name, None if t is None else t.data_ptr())
        self.args = a
        f64 = dict(dtype=torch.float64, device="cuda")
        self.kT0, self.ediff0 = torch.full((self.B,), self.params["kT0"], **f64), torch.full((self.B,), self.params["ediff0"], **f64)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.tmdnet_hop_reset(s, C.c_void_p(self.ws.data_ptr()), self.N, self.B, C.byref(a), 0, C.c_void_p(self.kT0.data_ptr()),
                                    C.c_void_p(self.ediff0.data_ptr()), 0) == 0

    def step(self, energy, forces):
        self.energy.copy_(torch.from_numpy(np.asarray(energy, np.float32)))
        self.f_in.copy_(torch.from_numpy(np.asarray(forces, np.float32)))
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert self.L.tmdnet_hop_advance(None, s, None, C.c_void_p(self.ws.data_ptr()), self.N, self.B, C.byref(self.args)) == 0

    def status(self):
        host = (C.c_uint64 * 2)()
        rc = self.L.tmdnet_hop_status(None, C.c_void_p(self.ws.data_ptr()), host)
        return rc, int(host[0]), int(host[1])


def _chains(n):
    """n chains side by side (the surface of tests/hop_oracle.py per chain)"""
    def surface(x):
        E, F = zip(*(O.chain_surface(x[4 * b:4 * b + 4]) for b in range(n)))
        return np.array(E), np.concatenate(F)

    pos = np.concatenate([O.CHAIN_START + 7.0 * b for b in range(n)])
    return surface, pos, np.repeat(np.arange(n), 4)


def _wells(sizes, seed=0):
    """harmonic sites E = 1/2 sum k_i |x_i - s_i|^2 per molecule, k_i in 2..5; the start is 0.3 off the sites"""
    rng = np.random.default_rng(seed)
    N = sum(sizes)
    batch = np.repeat(np.arange(len(sizes)), sizes)
    sites = rng.uniform(-4, 4, (N, 3)) + 10.0 * batch[:, None]
    k = rng.uniform(2.0, 5.0, N)

    def surface(x):
        d = x - sites
        e = 0.5 * k * (d * d).sum(1)
        return np.bincount(batch, weights=e, minlength=len(sizes)), -k[:, None] * d

    return surface, sites + 0.3 * rng.standard_normal((N, 3)), batch, sites


def _lockstep(lib, surface, pos, batch, masses, hops, max_steps, fixed=None, seeds=None, **kw):
    """device and mirror step by step from the same energies and forces until every walker has `hops` hops; -> (raw, host, phases)"""
    params = HP.parse_hop(**dict(O.CHAIN_PARAMS, **kw))
    host = H.HostHop(params, pos, masses, batch, fixed)
    raw = _Raw(lib, host)
    phases, worst_draw = set(), 0.0
    for step in range(max_steps):
        x = raw.pos.cpu().numpy()
        assert _np_bits(x, host.pos), f"positions differ before step {step + 1}"
        E, F = surface(x.astype(np.float64))
        E, F = np.asarray(E, np.float32), np.asarray(F, np.float32)
        raw.step(E, F)
        host.step(E, F)
        drew = np.isin(host.outcome, (HP.OUT_START, HP.OUT_SAME, HP.OUT_KNOWN, HP.OUT_ACCEPTED, HP.OUT_REJECTED, HP.OUT_UNCONVERGED))
        if drew.any():  # the one place a device transcendental enters: logf, sqrtf, cosf / sinf of the draw
            v = raw.vel.cpu().numpy()
            rows = drew[host.batch]
            worst_draw = max(worst_draw, _ulps(v[rows], host.vel[rows]))
            idx = np.nonzero(rows)[0]
            lo, hi = _draw_bounds(params["seed"], host.counters[host.batch[idx], 0], idx, host.coef[host.batch[idx], 9], host.sig[idx])
            assert ((v[rows] >= lo) & (v[rows] <= hi)).all(), f"a drawn velocity leaves its interval at step {step + 1}"
            assert _np_bits(v[~rows], host.vel[~rows])
            host.vel[:] = v
        for name in STATE + LOGS:
            assert _np_bits(getattr(raw, name).cpu().numpy(), getattr(host, name)), f"{name} differs after step {step + 1}"
        phases.add(tuple(host.phase_log.tolist()))
        if (host.n_hops >= hops).all():
            break
    print(f"{step + 1} steps, drawn velocities within {worst_draw:.2f} ulp of the mirror's")
    assert (host.n_hops >= hops).all() and raw.status() == (0, step + 1, 0) == (0,) + host.status()
    return raw, host, phases


def test_chain_every_step_of_three_hops_equals_the_mirror(hip_lib):
    surface, pos, batch = _chains(1)
    raw, host, _ = _lockstep(hip_lib, surface, pos, batch, np.ones(4), 3, 1500, seed=0)
    n = host.counters[0]
    assert n[0] == n[1] + n[2] + n[3] + n[5] and n[4] <= n[3]


def test_two_chains_in_different_phases_share_a_step(hip_lib):
    """Two chains in different phases at the same step.  A capture has ONE seed - the key of the Philox stream; the walkers' draws
    differ through the atom index and the hop count in the counter - so 'different seeds' cannot be had within one call: the walkers
    get different start geometries instead, so that their quenches end at different steps, and draw different velocities as atoms
    0..3 and 4..7 of the stream."""
    surface, pos, batch = _chains(2)
    pos[4:] += 0.15 * np.random.default_rng(1).standard_normal((4, 3))
    _, _, phases = _lockstep(hip_lib, surface, pos, batch, np.ones(8), 3, 1500, seed=3)
    assert any(a != b for a, b in phases)


def test_ragged_batch_across_a_wave_equals_the_mirror(hip_lib):
    surface, pos, batch, _ = _wells((3, 40, 65))
    m = np.random.default_rng(2).uniform(1.0, 16.0, len(batch))
    fixed = np.zeros(len(batch), np.uint8)
    fixed[[5, 50]] = 1
    _lockstep(hip_lib, surface, pos, batch, m, 3, 1500, fixed=fixed, seed=4, kT0=0.5, fmax=1e-2, align="translation")


def test_one_walker_in_two_slices_equals_the_mirror(hip_lib):
    surface, pos, batch, _ = _wells((1100,), seed=5)
    _lockstep(hip_lib, surface, pos, batch, np.full(1100, 4.0), 3, 1500, seed=6, kT0=0.5, fmax=1e-2)  # 1100 > 1024: S = 2


def test_a_launch_leaves_no_momentum_and_no_angular_momentum(hip_lib):
    """Walkers that start on their minimum (zero force): step 1 converges, step 2 records and draws, step 3 launches.  A chain-like
    walker of 5 atoms, one of 2 atoms (the translation path) and a collinear one of 3 atoms (singular inertia tensor: flagged, no NaN)."""
    sizes = (5, 2, 3)
    surface, _, batch, sites = _wells(sizes, seed=8)
    sites[7:10] = sites[7] + np.outer(np.arange(3.0), [1.0, 0.5, -0.25])
    m = np.random.default_rng(9).uniform(1.0, 16.0, len(batch))
    params = HP.parse_hop(**dict(O.CHAIN_PARAMS, seed=12))
    host = H.HostHop(params, sites, m, batch)
    raw = _Raw(hip_lib, host)
    zeroE, zeroF = np.zeros(3, np.float32), np.zeros((10, 3), np.float32)
    for _ in range(2):
        raw.step(zeroE, zeroF)
    x0, v0 = raw.pos.cpu().numpy().astype(np.float64), raw.vel.cpu().numpy().astype(np.float64)
    assert raw.phase.tolist() == [HP.LAUNCH] * 3 and np.abs(v0).min() > 0
    raw.step(zeroE, zeroF)
    v = raw.vel.cpu().numpy().astype(np.float64)
    assert raw.outcome.tolist() == [0, 0, HP.OUT_SINGULAR] and np.isfinite(v).all() and raw.status() == (0, 3, 0)
    assert _np_bits(raw.pos.cpu().numpy(), (x0.astype(np.float32) + np.float32(params["dt"]) * v.astype(np.float32)))
    coef = raw.coef.cpu().numpy()
    assert not coef[1, 6:9].any() and not coef[2, 6:9].any() and coef[0, 6:9].any()  # omega only where it is defined
    for b in range(3):
        rows = batch == b
        mb, xb, vb, vb0 = m[rows, None].astype(np.float32).astype(np.float64), x0[rows], v[rows], v0[rows]
        scale = (mb * (np.abs(vb0) + np.abs(vb))).sum()  # the terms: each carries a few fp32 roundings
        assert np.abs((mb * vb).sum(0)).max() < 8 * EPS32 * scale
        if b == 0:
            d = xb - (mb * xb).sum(0) / mb.sum()
            assert np.abs((mb * np.cross(d, vb)).sum(0)).max() < 8 * EPS32 * scale * np.abs(xb - xb.mean(0)).max() * 3
            assert np.abs((mb * np.cross(d, vb0)).sum(0)).max() > 1e-3  # (the draw had angular momentum)


def test_nan_and_invalid_arguments(hip_lib):
    surface, pos, batch = _chains(1)
    host = H.HostHop(HP.parse_hop(**O.CHAIN_PARAMS), pos, np.ones(4), batch)
    raw = _Raw(hip_lib, host)
    E, F = surface(pos)
    raw.step(E, F)
    keep = [getattr(raw, n).clone() for n in STATE + LOGS]
    F = np.array(F)
    F[1, 2] = np.nan
    for _ in range(2):
        raw.step(E, F)
        assert raw.status() == (5, 1, 2)
        for n, k in zip(STATE + LOGS, keep):
            assert _bits(getattr(raw, n), k)
    nb = C.c_size_t(0)
    assert hip_lib.tmdnet_hop_workspace_bytes(4, 1, 0, C.byref(nb)) == 1 and hip_lib.tmdnet_hop_workspace_bytes(4, 1, 65, C.byref(nb)) == 1
    raw.args.mdmin = 0
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip_lib.tmdnet_hop_advance(None, s, None, C.c_void_p(raw.ws.data_ptr()), 4, 1, C.byref(raw.args)) == 1


# ------------------------------------------------------------------------------------------------ through the model
ARCHS = ("tensornet", "equivariant-transformer", "tensornet2")
MODEL_KW = dict(steps_per_replay=8, kT0=0.05, ediff0=0.05, fmax=0.05, md_steps=24, opt_steps=80, capacity=8)
FS = 9.648533e-3


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


def _walkers(n_atoms=40, n_mol=2):
    z, pos, batch = W.synthetic_batch(n_mol=n_mol, n_atoms=n_atoms, first_seed=31)
    return (z % 8 + 1).cuda(), pos.cuda(), batch.cuda(), torch.full((n_mol * n_atoms,), 12.0, device="cuda")


def _q(arch, B):
    return torch.zeros(B, device="cuda") if arch != "equivariant-transformer" else None


def _capture(model, arch, seed=7, pos=None, **kw):
    z, pos0, batch, m = _walkers()
    return model.capture_minima_hopping(z, pos0 if pos is None else pos, m, 0.5, batch=batch, q=_q(arch, 2), seed=seed,
                                        **dict(MODEL_KW, **kw))


def _relaxed(model, arch):
    """-> (pos, fmax): the walkers after 400 FIRE steps and twice the largest atomic force left there.  A random-weight surface has
    no scale of its own; this gives the search a bound that its quenches can reach, before any of its code runs."""
    z, pos, batch, _ = _walkers()
    opt = model.capture_minimize(z, pos, batch=batch, q=_q(arch, 2), steps_per_replay=8, fmax=1e-9)
    opt(50)
    assert opt.check() == 400
    return opt.pos.clone(), 2.0 * float(opt.fmax[-1].max())


def _state(hop):
    return [getattr(hop, n) for n in STATE + LOGS]


@pytest.mark.parametrize("arch", ARCHS)
def test_model_search_graph_equals_eager_and_is_reproducible(hip_lib, arch):
    model = _model(arch)
    start, bound = _relaxed(model, arch)
    kw = dict(pos=start, fmax=bound)
    hop = _capture(model, arch, **kw)
    taken = hop.run(2, 2400)
    assert hop.check() == taken == hop.steps_done and taken % 8 == 0
    n = hop.counters.cpu()
    print(arch, taken, "steps", n.tolist())
    assert bool((n[:, 0] == n[:, 1] + n[:, 2] + n[:, 3] + n[:, 5]).all()) and bool((n[:, 4] <= n[:, 3]).all())
    assert bool((n[:, 0] >= 2).all()), "two hops per walker within 2400 steps"
    # a second capture with the same seed gives the same bits; another seed another search
    again = _capture(model, arch, **kw)
    again(taken // 8)
    for a, b in zip(_state(hop), _state(again)):
        assert _bits(a, b)
    other = _capture(model, arch, seed=8, **kw)
    other(taken // 8)
    assert not _bits(other.pos, hop.pos)
    # the same steps issued one by one from the host: the same bits; its per-step logs are kept for what follows
    eager = _capture(model, arch, **kw)
    rows = []
    for s in range(taken):
        before = (eager.pos.clone(), eager.vel.clone()) if int(eager.phase[0]) == HP.LAUNCH else None
        eager.step_eager(s % 8)
        k = s % 8
        rows.append((int(eager.phase_log[k, 0]), float(eager.epot[k, 0]), float(eager.ekin[k, 0]), before))
    assert eager.check() == taken
    for a, b in zip(_state(hop), _state(eager)):
        assert _bits(a, b)
    # every ring entry is a minimum to the bound, with the logged energy
    z, _, batch, m = _walkers()
    for slot in range(hop.params["capacity"]):
        live = (hop.counters[:, 6].clamp(max=hop.params["capacity"]) > slot)
        if not bool(live.any()):
            continue
        e, f = (t.detach() for t in model(z, hop.ring_pos[slot].clone(), batch, q=_q(arch, 2)))
        fm = torch.zeros(2, device="cuda").scatter_reduce(0, batch, f.norm(dim=1), "amax")
        for b in torch.nonzero(live).reshape(-1).tolist():
            assert float(fm[b]) < bound * (1 + 1e-5)
            assert abs(float(e[b]) - float(hop.ring_energy[b, slot])) <= 4 * EPS32 * abs(float(e[b]))
    # NVE: the drift of E + ekin / force_scale over walker 0's first escape against capture_md from the same minimum with the drawn
    # velocities, over as many steps
    start = next(i for i, r in enumerate(rows) if r[0] == HP.LAUNCH)
    stop = next(i for i in range(start + 1, taken) if rows[i][0] != HP.MD)
    tot = np.array([r[1] + r[2] / FS for r in rows[start + 1:stop]])
    assert len(tot) >= 3
    x0, v0 = rows[start][3]
    md = model.capture_md(z, x0, v0, m, 0.5, batch=batch, q=_q(arch, 2), steps_per_replay=len(tot), force_scale=FS)
    md()
    ref = (md.epot[:, 0] + md.ekin[:, 0] / FS).cpu().numpy().astype(np.float64)
    drift, drift_md = float(tot.max() - tot.min()), float(ref.max() - ref.min())
    print(f"{arch}: NVE drift over {len(tot)} steps {drift:.3e}, capture_md {drift_md:.3e}")
    assert drift <= 2.0 * drift_md


def test_overflow_freezes_the_state_at_the_last_valid_step(hip_lib):
    model = _model("tensornet", max_num_neighbors=72)
    z, pos, box = (t.cuda() for t in W.water_box(n_side=4))
    m = torch.full((z.shape[0],), 12.0, device="cuda")
    hop = model.capture_minima_hopping(z, pos, m, 0.5, box=box, q=torch.zeros(1, device="cuda"), steps_per_replay=4, kT0=0.05, ediff0=0.05)
    assert hop.params["align"] == HP.ALIGN["translation"]
    hop()
    assert hop.check() == 4
    box0 = hop.inputs[2].clone()
    hop.inputs[2].mul_(0.85)
    hop.pos.mul_(0.85)
    keep = [t.clone() for t in _state(hop)[2:]]
    hop()
    x_keep = hop.pos.clone()
    for _ in range(2):
        with pytest.raises(RuntimeError, match="max_num_pairs"):
            hop.check()
        for t, k in zip(_state(hop)[2:], keep):
            assert _bits(t, k)
        assert _bits(hop.pos, x_keep)
        hop()
    hop.inputs[2].copy_(box0)
    hop.reset(pos=pos)
    hop()
    assert hop.check() == 4 and not _bits(hop.pos, x_keep)


def test_check_names_forces_that_are_not_finite(hip_lib):
    tn2 = _model("tensornet2")
    hop = _capture(tn2, "tensornet2", steps_per_replay=4)
    hop()
    assert hop.check() == 4
    hop.inputs[3].fill_(float("nan"))
    hop()
    keep = [t.clone() for t in _state(hop)]
    hop()
    with pytest.raises(RuntimeError, match=r"step 4 an energy or a sum.*not finite.*frozen"):
        hop.check()
    for t, k in zip(_state(hop), keep):
        assert _bits(t, k)
    hop.inputs[3].zero_()
    hop.reset(kT=0.1, history="keep")
    assert hop.check() == 0 and float(hop.kT[0]) == 0.1
    hop()
    assert hop.check() == 4


class _NeverReplayed:
    def replay(self):
        raise AssertionError("a stale graph was replayed")


def test_a_stale_search_raises_and_replays_nothing(hip_lib):
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(4)
    model = create_model(dict(W.TINY_ARGS, static_shapes=True)).to("cuda")  # (its own model: the test re-creates its workspaces)
    hop = _capture(model, "tensornet", steps_per_replay=2, warmup=1)
    hop()
    assert hop.check() == 2 == hop.steps_done
    zb, pb, bb = W.synthetic_batch(n_mol=40, n_atoms=60)
    model(zb.cuda() % 19 + 1, pb.cuda(), bb.cuda())  # a larger system: the workspaces grow
    graph, hop.graph = hop.graph, _NeverReplayed()
    stale = r"stale HIP graph.*capture_minima_hopping\(\)"
    for call in (hop, hop.reset, lambda: hop.run(1, 100), hop.step_eager):
        with pytest.raises(RuntimeError, match=stale):
            call()
    assert hop.steps_done == 2


def test_refusals_leave_the_model_as_it_was(hip_lib):
    from torchmdnet_amd.models.model import create_model

    model = _model("tensornet")
    z, pos, batch, m = _walkers()
    q = _q("tensornet", 2)
    replay = model.capture(z, pos, batch, q=q)
    e0, f0 = (t.clone() for t in replay(pos))
    for bad in (dict(capacity=0), dict(capacity=65), dict(mdmin=0), dict(dt=0.0), dict(dt=-0.5), dict(kT0=0.0), dict(fmax=0.0),
                dict(rmsd_tol=0.0), dict(energy_tol=-1e-3), dict(align="mirror"), dict(steps_per_replay=0), dict(fire=dict(timestep=0.1)),
                dict(fixed=torch.zeros(3, device="cuda")), dict(masses=m[:5])):
        kw = dict(dict(masses=m, dt=0.5, kT0=0.05, ediff0=0.05), **bad)
        with pytest.raises(ValueError):
            model.capture_minima_hopping(z, pos, kw.pop("masses"), kw.pop("dt"), batch=batch, q=q, **kw)
    with pytest.raises(NotImplementedError, match="atom weights"):
        model.capture_minima_hopping(z, pos, m, 0.5, batch=batch, q=q, atom_weights=torch.ones(80, device="cuda"))
    with pytest.raises(NotImplementedError):
        model.capture_minima_hopping(z, pos.double(), m, 0.5, batch=batch, q=q)
    torch.manual_seed(0)
    with pytest.raises(NotImplementedError, match="output_model"):
        create_model(dict(W.TINY_ARGS, static_shapes=True, output_model="DipoleMoment")).to("cuda").capture_minima_hopping(
            z, pos, m, 0.5, batch=batch)
    e1, f1 = replay(pos)
    assert _bits(e1, e0) and _bits(f1, f0)
