"""-m gpu: the device-resident nudged elastic band (csrc/tn_neb.hip, TorchMD_Net.capture_neb).

1.-4.   the C entries alone (no model, graph_ws = NULL) on the analytic surface of tests/neb_oracle.py, energies and forces from torch
        between the launches: every step against the host mirror (tests/neb_host_mirror.py: the header's statements on the CPU) and
        the oracle - one band of 5 x 3, two bands of 7 x 3, one band of 3 x 1 100 (two slices per image), a band with fixed atoms.
        That endpoint images keep their bits is asserted in 1, 2, 3 and 10.
5.-9.   repeatability, frozen bands, coincident images, a NaN force and a NaN energy, reset(climb = 1) on a converged band
10.-15. through the model: bit-identity with capture() + a torch mirror, bands that cannot move, overflow, status 2 with barrier()
        and reset(images=), refusals, run"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import min_oracle as MO
from tests import neb_host_mirror as H
from tests import neb_oracle as O
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

OPEN, MIDDLE, CLOSE = 0, 1, 2
P = dict(MO.FIRE, fmax=1e-3)  # ASE's defaults, the bound of the surface runs


def _bits(a, b):
    if not a.is_floating_point():
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                                              b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))


def _np_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all()


# ------------------------------------------------------------------------------------------------ the C entries alone
class _Raw:
    """The C entries on tensors of the test's own, m = graph_ws = NULL (no model: energies and forces are what the test hands in)."""

    def __init__(self, lib, images, p, spring, climb=0, fixed=None):
        self.L, self.p, self.spring = lib, p, spring
        G, M, n = self.shape = tuple(images.shape[:3])
        self.pos = images.reshape(-1, 3).clone().contiguous()
        self.vel = torch.zeros_like(self.pos)
        self.fixed = fixed
        nb = C.c_size_t(0)
        assert lib.tmdnet_neb_workspace_bytes(n, M, G, C.byref(nb)) == 0
        self.ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        nan = float("nan")
        f32, f64 = dict(device="cuda"), dict(dtype=torch.float64, device="cuda")
        self.forces = torch.full_like(self.pos, nan)  # forces_keep: F_neb
        self.epot, self.fmax = torch.full((G, M), nan, **f32), torch.full((G,), nan, **f32)
        self.sums, self.coef = torch.full((G, 4), nan, **f64), torch.full((G, 3), nan, **f32)
        self.dt, self.alpha = torch.full((G,), nan, **f64), torch.full((G,), nan, **f64)
        self.conv = torch.full((G,), -7, dtype=torch.int64, device="cuda")
        self.path, self.w = torch.full((G, M, 5), nan, **f64), torch.full((G, M, 2), nan, **f64)
        self.s = torch.full((G, M, 2), nan, **f32)
        self.top = torch.full((G,), -7, dtype=torch.int32, device="cuda")
        self.reset(climb)

    @staticmethod
    def _s():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def reset(self, climb):
        self.climb = int(climb)
        assert self.L.tmdnet_neb_reset(self._s(), self._p(self.ws), 0, self.p["dt"], self.p["alpha"], self.climb) == 0

    def tensors(self):
        return [self.pos, self.vel, self.forces] + self.logs()

    def logs(self):
        return [self.epot, self.fmax, self.sums, self.coef, self.dt, self.alpha, self.conv, self.path, self.w, self.s, self.top]

    def advance(self, phase, forces, energy):
        p, f = self._p, self.p
        G, M, n = self.shape
        logs = [None] * 11 if phase == OPEN else [p(t) for t in self.logs()]
        rc = self.L.tmdnet_neb_advance(None, self._s(), None, p(self.ws), n, M, G, phase, p(self.pos), p(self.vel), p(forces), p(energy),
                                       p(self.fixed), None if phase == OPEN else p(self.forces), f["dt_max"], f["n_min"], f["f_inc"],
                                       f["f_dec"], f["alpha"], f["f_alpha"], f["max_step"], f["fmax"], self.spring, *logs)
        assert rc == 0, rc

    def status(self):
        host = (C.c_uint64 * 3)()
        rc = self.L.tmdnet_neb_status(self._s(), self._p(self.ws), host)
        return rc, int(host[0]), int(host[1]), int(host[2])


def _surface(pos, shape, sites):
    """torch, fp64 at the fp32 positions, rounded once -> e [G,M] fp32, f [N,3] fp32"""
    G, M, n = shape
    x = pos.double().view(G, M, n, 3)
    X, Y, Z = x[..., 0, 0], x[..., 0, 1], x[..., 0, 2]
    u = X * X - 1.0
    w = Y + O.A * u
    dr = x[..., 1:, :] - sites[1:]
    e = u * u + O.KAPPA * w * w + O.KAPPA * Z * Z + 0.5 * O.KAPPA * (dr * dr).sum((-1, -2))
    f = torch.empty_like(x)
    f[..., 0, 0] = -(4.0 * X * u + 2.0 * O.KAPPA * w * (2.0 * O.A * X))
    f[..., 0, 1] = -(2.0 * O.KAPPA * w)
    f[..., 0, 2] = -(2.0 * O.KAPPA * Z)
    f[..., 1:, :] = -O.KAPPA * dr
    return e.float().contiguous(), f.float().reshape(-1, 3).contiguous()


def _sum_bound_ok(dev, terms, where):
    """a device sum within n 2^-52 sum|t| of the exact sum (math.fsum) of the mirror's fp32 terms: the worst case of any fp64
    summation order over n terms is (n - 1) 2^-53 sum|t|"""
    t = np.asarray(terms, np.float64).ravel()
    exact, bound = math.fsum(t), len(t) * 2.0 ** -52 * math.fsum(np.abs(t))
    assert abs(dev - exact) <= bound, (where, dev, exact, bound)


def _check_step(raw, x, v, f, e, state, step, where):
    """The launch just made (CLOSE / MIDDLE on energies e and forces f at positions x with velocities v, numpy) against the host mirror
    and the oracle.  -> F_neb (numpy): the device's, equal to the mirror's bit for bit."""
    G, M, n = raw.shape
    fixed = None if raw.fixed is None else raw.fixed.cpu().numpy()
    has_free = fixed is None or bool((fixed == 0).any())
    x4, f4, v4 = x.reshape(G, M, n, 3), f.reshape(G, M, n, 3), v.reshape(G, M, n, 3)
    epot, fmax, sums, coef, dt, alpha, conv, path, w, s, top = (t.cpu().numpy() for t in raw.logs())
    assert _np_bits(epot, e), where
    # the path sums: fp32 terms of the header, any fp64 order
    t = H.path_terms(x4, f4, fixed)
    for b in range(G):
        for i in range(M):
            for k in range(5):
                _sum_bound_ok(path[b, i, k], t[b, i, :, k], (where, "path", b, i, k))
    # weights, coefficients, climber: the header on the host and the oracle, both fed with the device's sums
    wh, sh, why, toph = H.image_control(e, path, raw.spring, raw.climb, has_free)
    assert (why == 0).all() and (top == toph).all() and _np_bits(w, wh), where
    assert MO.ulp_distance(s, sh).max() <= 1, (where, s, sh)  # (the device compiler may contract an fp64 product into a sum)
    for b in range(G):
        assert top[b] == O.climber(e[b])
        for i in range(1, M - 1):
            cause, wo, so = O.image_control(e[b], i, path[b, i], raw.spring, raw.climb, has_free)
            assert cause == 0 and tuple(w[b, i]) == wo, (where, b, i)
            assert MO.ulp_distance(s[b, i], np.array(so, np.float32)).max() <= 1, (where, b, i, s[b, i], so)
    # the projection with the device's coefficients: bit for bit
    fneb = raw.forces.cpu().numpy().reshape(G, M, n, 3)
    assert _np_bits(fneb, H.project(x4, f4, s, fixed)), where
    assert (fneb[:, [0, -1]] == 0).all()
    # the FIRE sums of the band on F_neb, the controller
    still = np.zeros(n, np.uint8) if fixed is None else fixed
    rows_fixed = np.broadcast_to(still[None, None, :], (G, M, n)).copy()
    rows_fixed[:, [0, -1]] = 1  # endpoints contribute nothing
    tt = _fire_terms(v4.reshape(-1, 3), fneb.reshape(-1, 3), rows_fixed.reshape(-1)).reshape(G, M * n, 3)
    for b in range(G):
        for k in range(3):
            _sum_bound_ok(sums[b, k], tt[b, :, k], (where, "fire", b, k))
        assert sums[b, 3] == tt[b, :, 1].max(), where
        ret, c = MO.control(state[b], raw.p, *sums[b], step)
        assert ret != MO.UNUSABLE
        assert dt[b] == state[b]["dt"] and alpha[b] == state[b]["alpha"] and conv[b] == state[b]["converged_at"], (where, b)
        assert MO.ulp_distance(coef[b], np.array(c, np.float32)).max() <= 1, (where, b, coef[b], c)
        assert fmax[b] == np.float32(math.sqrt(sums[b, 3])), where
    return fneb


def _fire_terms(v, f, fixed):
    from tests import min_host_mirror as MH

    return MH.terms(v, f, fixed)


def _drive(lib, images, sites, spring, climb, fixed=None, fused=False, checks=True, max_steps=400, raw=None):
    """Optimise through the C entries: per step OPEN, energies and forces from torch, CLOSE (fused: one OPEN, then MIDDLE after every
    evaluation).  With `checks`, every step against the mirror and the oracle.  -> the _Raw, the steps taken, the history."""
    sites_t = sites if torch.is_tensor(sites) else torch.from_numpy(np.asarray(sites)).cuda()
    if raw is None:
        raw = _Raw(lib, images, P, spring, climb, fixed)
    G, M, n = raw.shape
    fx = None if raw.fixed is None else raw.fixed.cpu().numpy()
    state = MO.new_state(P, G)
    e, f = _surface(raw.pos, raw.shape, sites_t)
    raw.advance(CLOSE, f, e)
    x, v = raw.pos.cpu().numpy(), raw.vel.cpu().numpy()
    assert (v == 0).all()
    if checks:
        _check_step(raw, x, v, f.cpu().numpy(), e.cpu().numpy(), state, 0, "start")
    assert raw.status() == (0, 0, 0, 0)
    hist = dict(pos=[raw.pos.clone()], conv=[raw.conv.clone()])
    step = 0
    while step < max_steps and not bool((raw.conv >= 0).all()):
        if checks:
            xm, vm = H.move(raw.conv.cpu().numpy(), raw.coef.cpu().numpy(), x.reshape(G, M, n, 3), v.reshape(G, M, n, 3),
                            raw.forces.cpu().numpy().reshape(G, M, n, 3), fx)
        if not fused or step == 0:
            raw.advance(OPEN, raw.forces, None)  # (fused: the MIDDLE below has made this move already)
        x, v = raw.pos.cpu().numpy(), raw.vel.cpu().numpy()
        if checks:
            assert _np_bits(x, xm.reshape(-1, 3)) and _np_bits(v, vm.reshape(-1, 3)), step
        step += 1
        e, f = _surface(raw.pos, raw.shape, sites_t)
        raw.advance(MIDDLE if fused else CLOSE, f, e)
        if checks:
            _check_step(raw, x, v, f.cpu().numpy(), e.cpu().numpy(), state, step, step)
        hist["pos"].append(raw.pos.clone())
        hist["conv"].append(raw.conv.clone())
    assert raw.status() == (0, step, 0, 0)
    return raw, step, hist, sites_t


def _images(M, n, seeds=(0,)):
    xs, sites = [], None
    for seed in seeds:
        x, s = O.problem(M, n, seed=seed)
        if sites is None:
            sites = s
        else:
            x[0, :, 1:] = xs[0][0, :, 1:]  # the same sites for every band; atom 0 perturbed by its own seed
        xs.append(x)
    return torch.from_numpy(np.concatenate(xs)).cuda(), sites


def _saddle_distance(raw):
    G, M, n = raw.shape
    top = raw.top.cpu().numpy()
    x = raw.pos.view(G, M, n, 3).double().cpu().numpy()
    e = raw.epot.double().cpu().numpy()
    return (np.array([np.abs(x[b, top[b], 0] - O.SADDLE).max() for b in range(G)]),
            np.array([e[b, top[b]] - e[b, 0] - 1.0 for b in range(G)]))


_cache = {}


def _band_5x3(lib):
    if "5x3" not in _cache:
        images, sites = _images(5, 3)
        _cache["5x3"] = _drive(lib, images, sites, 0.1, 1) + (images,)
    return _cache["5x3"]


def _bands_7x3(lib):
    if "7x3" not in _cache:
        images, sites = _images(7, 3, seeds=(0, 2))
        _cache["7x3"] = _drive(lib, images, sites, 1.0, 1) + (images,)
    return _cache["7x3"]


def test_one_band_every_step_equals_the_mirror_and_the_oracle(hip_lib):
    """1. 5 images x 3 atoms, climbing, k = 0.1, to convergence.  Per step (the assertions are in _check_step and _drive): the path
    sums and the FIRE sums within the fp64 summation bound of the header's fp32 terms, the weights and the climber equal, s+ / s-
    and the controller's coefficients within 1 ulp of the header on the host and of the oracle fed with the device's sums, dt / alpha
    / converged_at equal, F_neb and the moved x, v bit-identical to the header on the host fed with the device's coefficients.  At
    the end the climber sits on the saddle within the bounds of tests/neb_oracle.py, and the endpoints kept their bits."""
    raw, steps, hist, sites, images = _band_5x3(hip_lib)
    ref = H.run(images.cpu().numpy(), sites.cpu().numpy(), O.KAPPA, O.A, P, 0.1, 1, 400)[0]
    print("converged at", raw.conv.tolist(), "host mirror", ref)
    assert 30 < steps < 400 and steps == int(raw.conv[0]) and steps <= 1.25 * ref + 5
    d, b = _saddle_distance(raw)
    print("distance", d, "barrier - 1", b)
    assert d[0] < O.position_bound(3, P["fmax"]) and abs(b[0]) < O.barrier_bound(3, P["fmax"])
    x = raw.pos.view(5, 3, 3)
    assert _bits(x[[0, 4]], images[0][[0, 4]]) and not _bits(x[1:4], images[0][1:4])
    assert (raw.vel.view(5, 3, 3)[[0, 4]] == 0).all() and float(raw.fmax[0]) < P["fmax"]


def test_two_bands_converge_and_freeze_on_their_own(hip_lib):
    """2. two bands of 7 x 3 with different seeds in one call, k = 1.0, climbing, every step checked: one controller per band - they
    converge at different steps, the first one to converge keeps its bits from then on while the other still moves, and each ends as
    it does when it is optimised alone."""
    raw, steps, hist, sites, images = _bands_7x3(hip_lib)
    conv = raw.conv.tolist()
    print("converged at", conv)
    assert min(conv) > 30 and conv[0] != conv[1] and steps == max(conv)
    first, last = (0, 1) if conv[0] < conv[1] else (1, 0)
    x = lambda s: hist["pos"][s].view(2, 7, 3, 3)
    for s in range(conv[first], steps + 1):
        assert _bits(x(s)[first], x(conv[first])[first]) and int(hist["conv"][s][first]) == conv[first], s
    assert not _bits(x(steps)[last], x(conv[first])[last])
    assert len(set(raw.dt.tolist())) == 2
    d, b = _saddle_distance(raw)
    assert (d < O.position_bound(3, P["fmax"])).all() and (np.abs(b) < O.barrier_bound(3, P["fmax"])).all()
    assert _bits(raw.pos.view(2, 7, 3, 3)[:, [0, 6]], images[:, [0, 6]])
    for b_ in range(2):  # alone: the same bits
        alone, steps1, _, _ = _drive(hip_lib, images[b_:b_ + 1], sites, 1.0, 1, checks=False)
        assert steps1 == conv[b_] and _bits(alone.pos, raw.pos.view(2, -1, 3)[b_])


def test_image_in_two_slices(hip_lib):
    """3. one band of 3 x 1 100 atoms: the one interior image spans two slices of 550 atoms, added in slice order.  Eight steps,
    every one checked as above."""
    images, sites = _images(3, 1100)
    raw, steps, _, _ = _drive(hip_lib, images, sites, 0.1, 1, max_steps=8)
    assert steps == 8 and int(raw.conv[0]) == -1 and int(raw.top[0]) == 1
    assert _bits(raw.pos.view(3, 1100, 3)[[0, 2]], images[0][[0, 2]]) and not _bits(raw.pos.view(3, 1100, 3)[1], images[0][1])


def test_fixed_atoms(hip_lib):
    """4. atom 1 fixed: it keeps its bits in every image, contributes to no sum, keeps the evaluation's force in `forces`, and the
    band still converges onto the saddle.  All atoms fixed: no tangent is needed, the band converges as it stands."""
    images, sites = _images(5, 3)
    fixed = torch.tensor([0, 1, 0], dtype=torch.uint8, device="cuda")
    raw, steps, _, sites_t = _drive(hip_lib, images, sites, 1.0, 1, fixed=fixed)
    assert 30 < steps < 400 and steps == int(raw.conv[0])
    x = raw.pos.view(5, 3, 3)
    assert _bits(x[:, 1], images[0][:, 1]) and not _bits(x[1:4, 2], images[0][1:4, 2]) and (raw.vel.view(5, 3, 3)[:, 1] == 0).all()
    e, f = _surface(raw.pos, raw.shape, sites_t)
    assert _bits(raw.forces.view(5, 3, 3)[1:4, 1], f.view(5, 3, 3)[1:4, 1]) and (f.view(5, 3, 3)[1:4, 1].abs() > P["fmax"]).any()
    assert _saddle_distance(raw)[0][0] < O.position_bound(3, P["fmax"])
    every = torch.ones(3, dtype=torch.uint8, device="cuda")
    raw, steps, _, _ = _drive(hip_lib, images, sites, 1.0, 1, fixed=every)
    assert steps == 0 and int(raw.conv[0]) == 0 and _bits(raw.pos.view(5, 3, 3), images[0]) and (raw.s == 0).all()
    raw.advance(OPEN, raw.forces, None)
    assert _bits(raw.pos.view(5, 3, 3), images[0]) and (raw.vel == 0).all()


def test_two_runs_are_bit_identical(hip_lib):
    """5. fixed summation order, no floating-point atomics; and MIDDLE after every evaluation is the same optimisation as OPEN / CLOSE"""
    images, sites = _images(7, 3, seeds=(0, 2))
    a, sa, _, _ = _drive(hip_lib, images, sites, 1.0, 1, fused=True, checks=False)
    b, sb, _, _ = _drive(hip_lib, images, sites, 1.0, 1, fused=True, checks=False)
    assert sa == sb
    for s, t in zip(a.tensors(), b.tensors()):
        assert _bits(s, t)
    ref = _bands_7x3(hip_lib)[0]
    assert _bits(a.pos, ref.pos) and torch.equal(a.conv, ref.conv) and (a.vel == 0).all()


def test_frozen_band_changes_nothing_on_further_launches(hip_lib):
    """6. both bands converged: OPEN, MIDDLE and CLOSE launches leave x, converged_at, dt and F_neb as they are, v = 0"""
    images, sites = _images(7, 3, seeds=(0, 2))
    raw, steps, _, sites_t = _drive(hip_lib, images, sites, 1.0, 1, fused=True, checks=False)
    keep = [t.clone() for t in (raw.pos, raw.forces, raw.conv, raw.dt, raw.alpha, raw.epot, raw.s)]
    e, f = _surface(raw.pos, raw.shape, sites_t)
    for phase in (OPEN, MIDDLE, CLOSE, OPEN):
        raw.advance(phase, raw.forces if phase == OPEN else f, None if phase == OPEN else e)
    for t, k in zip((raw.pos, raw.forces, raw.conv, raw.dt, raw.alpha, raw.epot, raw.s), keep):
        assert _bits(t, k)
    assert (raw.vel == 0).all() and (raw.coef == 0).all() and raw.status() == (0, steps + 2, 0, 0)


def _latched(raw, sites_t, e_bad, f_bad, cause, step):
    """after the launch on (e_bad, f_bad): status 2 with `cause`, nothing written, every later launch returns at once"""
    keep = [t.clone() for t in raw.tensors()]
    raw.advance(CLOSE, f_bad, e_bad)
    assert raw.status() == (5, step, 2, cause)
    e, f = _surface(raw.pos, raw.shape, sites_t)
    raw.advance(OPEN, raw.forces, None)
    raw.advance(MIDDLE, f, e)
    raw.advance(CLOSE, f, e)
    assert raw.status() == (5, step, 2, cause)
    for t, k in zip(raw.tensors(), keep):
        assert _bits(t, k)


def _three_steps(lib, images, sites):
    raw = _Raw(lib, images, P, 0.1, 0)
    sites_t = torch.from_numpy(sites).cuda()
    e, f = _surface(raw.pos, raw.shape, sites_t)
    raw.advance(CLOSE, f, e)
    for _ in range(3):
        raw.advance(OPEN, raw.forces, None)
        e, f = _surface(raw.pos, raw.shape, sites_t)
        raw.advance(CLOSE, f, e)
    assert raw.status() == (0, 3, 0, 0)
    raw.advance(OPEN, raw.forces, None)
    return raw, sites_t


def test_coincident_images_latch_status_2_with_cause_2(hip_lib):
    """7. images 1, 2, 3 of a band made equal after three steps: the tangent of image 2 has no length"""
    images, sites = _images(5, 3, seeds=(0, 2))
    raw, sites_t = _three_steps(hip_lib, images, sites)
    x = raw.pos.view(2, 5, 3, 3)
    x[1, 1] = x[1, 3]
    x[1, 2] = x[1, 3]
    e, f = _surface(raw.pos, raw.shape, sites_t)
    _latched(raw, sites_t, e, f, 2, 3)
    # on the start path: the same, at step 0, and a reset with usable images recovers
    bad = images.clone()
    bad[0, 1] = bad[0, 2] = bad[0, 3]
    raw = _Raw(hip_lib, bad, P, 0.1, 0)
    e, f = _surface(raw.pos, raw.shape, sites_t)
    raw.advance(CLOSE, f, e)
    assert raw.status() == (5, 0, 2, 2) and _bits(raw.pos.view(2, 5, 3, 3), bad)
    raw.pos.copy_(images.reshape(-1, 3))
    raw.reset(0)
    e, f = _surface(raw.pos, raw.shape, sites_t)
    raw.advance(CLOSE, f, e)
    assert raw.status() == (0, 0, 0, 0)


def test_nan_force_and_nan_energy_latch_status_2(hip_lib):
    """8. a NaN force in an interior image: cause 1; a NaN energy: cause 3 (it outranks the others); a force that is not finite on an
    endpoint image is not looked at"""
    images, sites = _images(5, 3, seeds=(0, 2))
    raw, sites_t = _three_steps(hip_lib, images, sites)
    e, f = _surface(raw.pos, raw.shape, sites_t)
    bad = f.clone()
    bad.view(2, 5, 3, 3)[1, 2, 1, 0] = float("nan")
    _latched(raw, sites_t, e, bad, 1, 3)
    raw, sites_t = _three_steps(hip_lib, images, sites)
    e, f = _surface(raw.pos, raw.shape, sites_t)
    e_bad = e.clone()
    e_bad[0, 4] = float("nan")
    _latched(raw, sites_t, e_bad, bad, 3, 3)
    raw, sites_t = _three_steps(hip_lib, images, sites)
    e, f = _surface(raw.pos, raw.shape, sites_t)
    ends = f.clone()
    ends.view(2, 5, 3, 3)[0, 0, 1, 2] = float("inf")
    ends.view(2, 5, 3, 3)[1, 4, 0, 0] = float("nan")
    raw.advance(CLOSE, ends, e)
    assert raw.status() == (0, 4, 0, 0) and torch.isfinite(raw.forces).all()


def test_reset_with_climb_moves_the_climber_onto_the_saddle(hip_lib):
    """9. the plain band converges with its highest image off the saddle (further than the bound); tmdnet_neb_reset(climb = 1) on the
    same workspace and positions, and the same launches, bring it within the bound"""
    images, sites = _images(7, 3)
    raw, steps, _, _ = _drive(hip_lib, images, sites, 0.1, 0, fused=True, checks=False)
    d0, b0 = _saddle_distance(raw)
    bound = O.position_bound(3, P["fmax"])
    assert 30 < steps < 400 and d0[0] > bound
    raw.reset(1)
    raw.vel.zero_()
    raw, steps2, _, _ = _drive(hip_lib, None, sites, 0.1, 1, fused=True, checks=False, raw=raw)
    d1, b1 = _saddle_distance(raw)
    print("plain", steps, d0, b0, "climbing", steps2, d1, b1)
    assert 0 < steps2 < 400 and d1[0] < bound and abs(b1[0]) < O.barrier_bound(3, P["fmax"])


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


def _path(n_bands=1, M=5):
    """-> z [40], images [G,M,40,3]: from a 40-atom molecule to a copy displaced smoothly by at most 0.3 per atom"""
    from torchmdnet_amd.neb import interpolate

    z, pos, _ = W.synthetic_batch(n_mol=1, n_atoms=40, first_seed=31)
    z, pos = (z % 8 + 1).cuda(), pos.cuda()
    bands = []
    for b in range(n_bands):
        g = torch.Generator().manual_seed(50 + b)
        k, ph = torch.rand(3, 3, generator=g).cuda(), (6.28 * torch.rand(3, generator=g)).cuda()
        disp = (0.3 / math.sqrt(3)) * torch.sin(pos @ k + ph)
        assert float(disp.norm(dim=1).max()) <= 0.3
        bands.append(interpolate(pos, pos + disp, M))
    return z, torch.stack(bands)


def _q(arch, G):
    return torch.zeros(G, device="cuda") if arch != "equivariant-transformer" else None


def _dot(a, b):
    return torch.add(torch.add(torch.mul(a[..., 0], b[..., 0]), torch.mul(a[..., 1], b[..., 1])), torch.mul(a[..., 2], b[..., 2]))


def _mirror_fneb(x, f, s, fixed):
    """F_neb with the device's coefficients, torch.sub / torch.mul / torch.add one rounded operation at a time; x, f [G,M,n,3]"""
    out = torch.zeros_like(f)
    dp, dm = torch.sub(x[:, 2:], x[:, 1:-1]), torch.sub(x[:, 1:-1], x[:, :-2])
    sp, sm = s[:, 1:-1, 0, None, None], s[:, 1:-1, 1, None, None]
    proj = torch.add(torch.add(f[:, 1:-1], torch.mul(sp, dp)), torch.mul(sm, dm))
    out[:, 1:-1] = torch.where(fixed[None, None, :, None], f[:, 1:-1], proj)
    return out


def _mirror_move(x, v, fneb, coef, conv, fixed):
    c = coef[:, None, None, :]
    still = (conv >= 0)[:, None, None] | fixed[None, None, :]
    still = still.expand(x.shape[:3]).clone()
    still[:, [0, -1]] = True
    v_new = torch.add(torch.mul(c[..., 0:1], v), torch.mul(c[..., 1:2], fneb))
    x_new = torch.add(x, torch.mul(c[..., 2:3], v_new))
    return torch.where(still[..., None], x, x_new), torch.where(still[..., None], torch.zeros_like(v), v_new)


def _record(neb, replays):
    logs = dict(epot=[], fmax=[], coef=[], s=[], conv=[], top=[])
    for _ in range(replays):
        neb()
        for key, t in (("epot", neb.epot), ("fmax", neb.fmax), ("coef", neb.coef), ("s", neb.tangent_coef), ("top", neb.climber)):
            logs[key].append(t.clone())
        logs["conv"].append(neb.converged_at.clone())
    assert neb.check() == neb.steps_per_replay * replays == neb.steps_done
    return {k: (torch.cat(v) if k != "conv" else v) for k, v in logs.items()}


@pytest.mark.parametrize("arch", ["tensornet", "equivariant-transformer", "tensornet2"])
def test_band_is_bit_identical_to_capture_plus_torch_mirror(hip_lib, arch):
    """10. two bands of 5 x 40, climbing, 8 steps, one per replay, against capture() on the stacked batch and a torch mirror that takes
    the device's coefficients and issues torch.mul and torch.add separately: positions, F_neb and energies equal bit for bit; then
    one replay of 8 steps gives the same bits; reset restores the start; one band given as [M,n,3]."""
    model = _model(arch)
    z, images = _path(n_bands=2)
    G, M, n = images.shape[:3]
    q = _q(arch, G)
    fixed = torch.zeros(n, dtype=torch.bool, device="cuda")
    fixed[::11] = True
    kw = dict(q=q, fmax=1e-5, spring=0.5, climb=True, fixed=fixed)
    batch = torch.arange(G * M, device="cuda").repeat_interleave(n)
    replay = model.capture(z.repeat(G * M), images.reshape(-1, 3), batch, q=None if q is None else q.repeat_interleave(M))
    neb = model.capture_neb(z, images, steps_per_replay=1, **kw)
    start = [t.clone() for t in (neb.coef0, neb.converged_at, neb.epot0, neb.tangent_coef0, neb.forces)]
    logs = _record(neb, 8)
    x, v = images.clone(), torch.zeros_like(images)
    e, f = (t.clone() for t in replay(x.reshape(-1, 3)))
    assert _bits(start[2], e.view(G, M)) and (start[1] == -1).all()
    fneb = _mirror_fneb(x, f.view(G, M, n, 3), start[3], fixed)
    assert _bits(start[4], fneb)
    coef, conv = start[0], start[1]
    for s in range(8):
        x, v = _mirror_move(x, v, fneb, coef, conv, fixed)
        e, f = (t.clone() for t in replay(x.reshape(-1, 3)))
        assert _bits(logs["epot"][s], e.view(G, M)), s
        fneb = _mirror_fneb(x, f.view(G, M, n, 3), logs["s"][s], fixed)
        ff = torch.where(fixed[None, None, :], 0.0, _dot(fneb, fneb))[:, 1:-1]
        assert _bits(logs["fmax"][s], ff.amax((1, 2)).double().sqrt().float()), s
        assert torch.equal(logs["top"][s].long(), e.view(G, M)[:, 1:-1].argmax(1) + 1), s
        coef, conv = logs["coef"][s], logs["conv"][s]
    assert _bits(neb.images, x) and _bits(neb.forces, fneb)
    moved = (x - images).abs()
    assert moved[:, 1:-1].max().item() > 1e-4 and _bits(x[:, [0, -1]], images[:, [0, -1]]) and _bits(x[:, :, fixed], images[:, :, fixed])
    neb8 = model.capture_neb(z, images, steps_per_replay=8, **kw)
    logs8 = _record(neb8, 1)
    assert _bits(neb8.images, neb.images) and _bits(neb8.forces, neb.forces) and _bits(neb8.vel, neb.vel)
    for key in ("epot", "fmax", "coef", "s", "top"):
        assert _bits(logs8[key], logs[key]), key
    assert float(neb8.barrier()[0]) == float((neb8.epot[-1, 0].max() - neb8.epot[-1, 0, 0]).cpu())
    neb8.reset(images=images)
    assert _bits(neb8.coef0, start[0]) and (neb8.vel == 0).all() and neb8.check() == 0 and _bits(neb8.images, images)
    neb8()
    assert _bits(neb8.images, neb.images) and neb8.check() == 8
    # one band as [M,n,3] (a batch of another size may take other kernels in the evaluation: no bits are compared across the two)
    one = model.capture_neb(z, images[0], steps_per_replay=8, **dict(kw, q=None if q is None else q[:1]))
    one()
    assert one.check() == 8 and one.images.shape == (1, M, n, 3) and one.epot.shape == (8, 1, M)
    assert _bits(one.images[0, [0, -1]], images[0, [0, -1]]) and not _bits(one.images[0, 1:-1], images[0, 1:-1])


def test_bands_that_cannot_move_stay_where_they_are(hip_lib):
    """11. every atom fixed, or fmax above every force: the band converges at step 0 and replays move nothing, as capture_minimize"""
    model = _model("tensornet")
    z, images = _path()
    q = _q("tensornet", 1)
    for kw in (dict(fixed=torch.ones(40, device="cuda")), dict(fmax=1e6)):
        neb = model.capture_neb(z, images, q=q, steps_per_replay=3, **kw)
        assert (neb.converged_at == 0).all()
        neb(2)
        assert neb.check() == 6 and _bits(neb.images, images) and (neb.vel == 0).all() and (neb.converged_at == 0).all()
        assert neb.run(100) == 0


def test_overflow_freezes_the_state_at_the_last_valid_step(hip_lib):
    """12. five images of the 192-atom periodic box with max_num_neighbors = 72, box and positions scaled by 0.85 between two
    replays: the first evaluation of the second replay overflows."""
    from torchmdnet_amd.neb import interpolate

    model = _model("tensornet", max_num_neighbors=72)
    z, pos, box = (t.cuda() for t in W.water_box(n_side=4))
    g = torch.Generator().manual_seed(3)
    images = interpolate(pos, pos + 0.1 * torch.randn(pos.shape, generator=g).cuda(), 5)
    box0 = box.clone()
    neb = model.capture_neb(z, images, box=box, q=torch.zeros(1, device="cuda"), steps_per_replay=4, fmax=1e-4)
    neb()
    assert neb.check() == 4
    staged_box = neb.inputs[2]
    staged_box.mul_(0.85)
    neb.pos.mul_(0.85)
    watched = lambda: (neb.pos, neb.vel, neb.forces, neb.epot, neb.fmax, neb.coef, neb.sums, neb.step_size, neb.alpha, neb.converged_at,
                       neb.tangent_coef, neb.climber)
    keep = [t.clone() for t in watched()]
    host = (C.c_uint64 * 3)()
    for _ in range(2):  # the replay that overflows, and one more: frozen, nothing moves
        neb()
        with pytest.raises(RuntimeError, match="max_num_pairs"):
            neb.check()
        assert hip_lib.tmdnet_neb_status(None, C.c_void_p(neb._ws.data_ptr()), host) == 3 and (int(host[0]), int(host[1])) == (4, 1)
        for t, k in zip(watched(), keep):
            assert _bits(t, k)
    staged_box.copy_(box0)
    neb.reset(images=images)
    neb()
    assert neb.check() == 4 and not _bits(neb.pos, keep[0])


def test_check_names_the_cause_of_status_2(hip_lib):
    """13. coincident images handed to the C entry on the band's own workspace, part-way through a replay made by hand (OPEN, one
    MIDDLE, then the CLOSE that latches): check() names them, barrier() reads the row of the step the state is frozen at, replays
    change nothing, reset recovers and refuses images of another layout"""
    from torchmdnet_amd.minimize import MIN_CLOSE, MIN_MIDDLE, MIN_OPEN

    model = _model("tensornet")
    z, images = _path()
    q = _q("tensornet", 1)
    neb = model.capture_neb(z, images, q=q, steps_per_replay=4, fmax=1e-5)
    neb()
    assert neb.check() == 4
    row = lambda e: float((e[0].max() - e[0, 0]).cpu())
    assert float(neb.barrier()[0]) == row(neb.epot[3])
    neb._advance(MIN_OPEN, neb._forces, None, None)
    e, f = neb._evaluate()
    neb._advance(MIN_MIDDLE, f, e, 0)  # step 5, logged in row 0
    neb.epot[3, 0, 2] += 100.0  # mark the last row, which is stale from here on (the endpoints alone set this path's barrier)
    good = neb.images.clone()
    neb.images[0, 1] = neb.images[0, 2]
    neb.images[0, 3] = neb.images[0, 2]
    keep = [t.clone() for t in (neb.pos, neb.vel, neb.forces, neb.epot, neb.fmax)]
    e, f = neb._evaluate()
    neb._advance(MIN_CLOSE, f, e, 1)
    with pytest.raises(RuntimeError, match="coincident images"):
        neb.check()
    assert float(neb.barrier()[0]) == row(neb.epot[0]) != row(neb.epot[3])  # the device's step 5, not the last row of the log
    neb()
    with pytest.raises(RuntimeError, match="step 5 .* frozen"):
        neb.check()
    for t, k in zip((neb.pos, neb.vel, neb.forces, neb.epot, neb.fmax), keep):
        assert _bits(t, k)
    for wrong in (good.transpose(2, 3), good.reshape(5, 1, 40, 3), good[0, :, :39], good[0, 0]):
        with pytest.raises(ValueError):
            neb.reset(images=wrong)
    neb.reset(images=good[0])  # one band: [M,n,3] is accepted
    assert _bits(neb.images, good) and neb.check() == 0 and float(neb.barrier()[0]) == row(neb.epot0)
    neb()
    assert neb.check() == 4 and not _bits(neb.images, good)
    with pytest.raises(RuntimeError, match="coincident images"):
        neb.reset(images=good[:, :1].expand(1, 5, 40, 3)).check()
    two = model.capture_neb(z, torch.cat([images, images]), q=_q("tensornet", 2), steps_per_replay=1, fmax=1e-5)
    with pytest.raises(ValueError):
        two.reset(images=images[0])  # [M,n,3] stands for one band only


def test_refusals_leave_the_model_as_it_was(hip_lib):
    """14."""
    from torchmdnet_amd.models.model import create_model

    model = _model("tensornet")
    z, images = _path()
    q = _q("tensornet", 1)
    batch = torch.arange(5, device="cuda").repeat_interleave(40)
    replay = model.capture(z.repeat(5), images.reshape(-1, 3), batch, q=q.repeat_interleave(5))
    e0, f0 = (t.clone() for t in replay(images.reshape(-1, 3)))
    for bad in (dict(steps_per_replay=0), dict(fire=dict(timestep=0.1)), dict(fmax=0.0), dict(spring=0.0), dict(spring=-0.1),
                dict(fixed=torch.zeros(3, device="cuda")), dict(q=torch.zeros(2, device="cuda")), dict(box=torch.eye(3).repeat(5, 1, 1).cuda())):
        with pytest.raises(ValueError):
            model.capture_neb(z, images, **dict(dict(q=q), **bad))
    for bad_images in (images[:, :2], images[:, :, :39], images[0, 0], images[..., :2]):
        with pytest.raises(ValueError):
            model.capture_neb(z, bad_images, q=q)
    with pytest.raises(NotImplementedError):
        model.capture_neb(z, images.double(), q=q)
    model.parameter_gradients = True
    try:
        with pytest.raises(NotImplementedError):
            model.capture_neb(z, images, q=q)
    finally:
        model.parameter_gradients = False
    torch.manual_seed(0)
    with pytest.raises(NotImplementedError):
        create_model(dict(W.TINY_ARGS, static_shapes=True, output_model="DipoleMoment")).to("cuda").capture_neb(z, images)
    with pytest.raises(RuntimeError, match="static_shapes"):
        create_model(dict(W.TINY_ARGS)).to("cuda").capture_neb(z, images)
    e1, f1 = replay(images.reshape(-1, 3))  # the graph captured before the refusals is still valid, and gives the same bits
    assert _bits(e1, e0) and _bits(f1, f0)


def test_run_stops_at_convergence_or_at_max_steps(hip_lib):
    """15."""
    model = _model("tensornet")
    z, images = _path()
    q = _q("tensornet", 1)
    neb = model.capture_neb(z, images, q=q, steps_per_replay=4, fmax=1e-7)  # below what 20 steps reach
    assert neb.run(20, check_every=2) == 20 and neb.check() == 20 and (neb.converged_at == -1).all()
    assert neb.run(7) == 4 and neb.check() == 24  # whole replays only, never beyond max_steps
    assert not _bits(neb.images, images) and _bits(neb.images[:, [0, -1]], images[:, [0, -1]])
    assert float(neb.barrier()[0]) >= 0.0
    neb = model.capture_neb(z, images, q=q, steps_per_replay=4, fmax=1e6)  # above every force: converged as it stands
    assert neb.run(100) == 0 and _bits(neb.images, images) and (neb.converged_at == 0).all() and neb.check() == 0
    assert (neb.fmax0 > 0).all() and (neb.fmax0 < 1e6).all()
