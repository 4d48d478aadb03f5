"""-m gpu: the device-resident L-BFGS minimiser (csrc/tn_lbfgs.hip, TorchMD_Net.capture_minimize(lbfgs=...)).

1.-8. the C entries alone (no model, graph_ws = NULL) on spring wells whose forces torch computes between the calls: every step against
      a torch mirror and tests/lbfgs_oracle.py (memory 3, 1 and 100), an interleaved batch, a molecule in two slices, the non-convex
      well, fused against unfused, repeatability, freezing, a NaN force
9.    through the model: K steps per graph launch are bit-identical to capture() + the torch mirror x + c p with the device's c and p
10.   overflow: the state freezes at the last valid step;  11. refusals;  12. the stale-graph guard;  13. opt.run"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import lbfgs_oracle as O
from tests import min_oracle as MO
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

OPEN, MIDDLE, CLOSE = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = dict(O.LBFGS, fmax=1e-3, memory=3)  # ASE's parameters, the bound of the wells, a ring that wraps


def _tol():
    """64 x the error of the coefficient-space recursion measured on the CPU (tests/test_lbfgs_host.py, profiles/minimize_lbfgs.json)"""
    with open(os.path.join(ROOT, "profiles", "minimize_lbfgs.json")) as fh:
        return 64 * json.load(fh)["gram_vs_two_loop"]["max"]


def _bits(a, b):
    if a.dtype == torch.float64:
        return a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ the C entries alone
class _Raw:
    """The C entries on tensors of the test's own, m = graph_ws = NULL (no model: the forces are whatever `forces` holds)."""

    def __init__(self, lib, pos, batch, n_mol, p, fixed=None):
        self.L, self.n, self.n_mol, self.p, self.M1 = lib, pos.shape[0], n_mol, p, p["memory"] + 1
        self.pos = pos.clone().contiguous()
        self.batch, self.fixed = batch, fixed
        nb = C.c_size_t(0)
        assert lib.tmdnet_lbfgs_workspace_bytes(self.n, n_mol, p["memory"], C.byref(nb)) == 0
        self.ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        assert self.ws.data_ptr() % 256 == 0
        off = (C.c_int64 * 17)()
        assert lib.tmdnet_lbfgs_layout(self.n, n_mol, p["memory"], off) == 0
        self.off = list(off)
        nan = float("nan")
        self.forces = torch.full_like(pos, nan)  # forces_keep
        self.direction = torch.full_like(pos, nan)
        self.fmax, self.scale = torch.full((n_mol,), nan, device="cuda"), torch.full((n_mol,), nan, device="cuda")
        self.sums = torch.full((n_mol, 4), nan, dtype=torch.float64, device="cuda")
        self.pairs, self.accepted = (torch.full((n_mol,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
        self.conv = torch.full((n_mol,), -7, dtype=torch.int64, device="cuda")
        assert lib.tmdnet_lbfgs_reset(self._s(), self._p(self.ws), 0) == 0

    @staticmethod
    def _s():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def advance(self, phase, forces):
        p, f = self._p, self.p
        logs = [None] * 7 if phase == OPEN else [None] + [p(t) for t in (self.fmax, self.sums, self.pairs, self.accepted, self.scale, self.conv)]
        rc = self.L.tmdnet_lbfgs_advance(None, self._s(), None, p(self.ws), self.n, self.n_mol, phase, p(self.pos), p(forces), None,
                                         p(self.fixed), p(self.batch), None if phase == OPEN else p(self.forces), p(self.direction),
                                         f["memory"], f["alpha"], f["max_step"], f["damping"], f["fmax"], *logs)
        assert rc == 0, rc

    def status(self):
        host = (C.c_uint64 * 3)()
        rc = self.L.tmdnet_lbfgs_status(self._s(), self._p(self.ws), host)
        return rc, int(host[0]), int(host[1])

    def _view(self, k, dtype, shape):
        return self.ws[self.off[k]:self.off[k] + int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()].view(dtype).view(shape)

    def state(self):
        """the workspace's own arrays (views): pairs held, ring order, converged_at, Gram blocks, x_prev, F_prev, the rings"""
        B, M1, n = self.n_mol, self.M1, self.n
        return dict(h=self._view(1, torch.int32, (B,)), conv=self._view(2, torch.int64, (B,)), order=self._view(3, torch.int32, (B, M1)),
                    SS=self._view(4, torch.float64, (B, M1, M1)), SY=self._view(5, torch.float64, (B, M1, M1)),
                    YY=self._view(6, torch.float64, (B, M1, M1)), x_prev=self._view(11, torch.float32, (n, 3)),
                    f_prev=self._view(12, torch.float32, (n, 3)), S=self._view(13, torch.float32, (M1, n, 3)),
                    Y=self._view(14, torch.float32, (M1, n, 3)), cmove=self._view(15, torch.float32, (B,)))

    def logs(self):
        return [t.clone() for t in (self.fmax, self.sums, self.pairs, self.accepted, self.conv, self.direction)]


def _sum_bound(t):
    """any fp64 summation order over n terms is within (n - 1) 2^-53 sum |t| of the exact sum; the bound asked is n 2^-52 sum |t|"""
    return math.fsum(t), len(t) * 2.0 ** -52 * math.fsum(np.abs(t))


def _check_step(raw, st_before, x_before, f_before, f, mols, idx, fixed_np, step, fresh, tol, stats):
    """everything the launches after one evaluation wrote, against torch and the oracle.  st_before: the pairs held and the ring
    order before the launch; mols: one oracle molecule per molecule, stepped along."""
    s = {k: v.cpu().numpy() for k, v in raw.state().items()}
    fmax, sums, pairs, accepted, conv, direction = (t.cpu().numpy() for t in raw.logs())
    x, f_np = raw.pos.cpu().numpy(), f.cpu().numpy()
    assert np.array_equal(raw.scale.cpu().numpy(), np.zeros(raw.n_mol, np.float32) if fresh else s["cmove"]), step
    free_all = np.ones(raw.n, bool) if fixed_np is None else fixed_np == 0
    if not fresh:  # the state the move saved, and the candidate: one rounded subtraction each, bit-equal to torch.sub
        assert np.array_equal(s["x_prev"], x_before) and np.array_equal(s["f_prev"], f_before)
        s_t = torch.sub(raw.pos, torch.from_numpy(x_before).cuda()).cpu().numpy()
        y_t = torch.sub(torch.from_numpy(f_before).cuda(), f).cpu().numpy()
    for m, mol in enumerate(mols):
        i = idx[m]
        free = free_all[i]
        was_frozen = mol.converged_at >= 0
        g = -np.where(free[:, None], f_np[i], 0.0).astype(np.float64)
        # ff and fmax2: sums of exact fp64 products
        exact, bound = _sum_bound((g * g).ravel())
        assert abs(sums[m, 0] - exact) <= bound, (step, m, sums[m, 0], exact, bound)
        assert sums[m, 1] == ((g * g).sum(1).max() if len(i) else 0.0) or abs(sums[m, 1] - (g * g).sum(1).max()) <= 2.0 ** -51 * sums[m, 1]
        assert fmax[m] == np.float32(math.sqrt(sums[m, 1])), (step, m)
        pair = None
        if not fresh and not was_frozen:
            h0, order0 = st_before[0][m], st_before[1][m]
            spare = order0[h0]
            sc, yc = s["S"][spare][i], s["Y"][spare][i]
            assert np.array_equal(sc.view(np.int32), np.where(free[:, None], s_t[i], 0).astype(np.float32).view(np.int32)), (step, m)
            assert np.array_equal(yc.view(np.int32), np.where(free[:, None], y_t[i], 0).astype(np.float32).view(np.int32)), (step, m)
            exact, bound = _sum_bound((sc.astype(np.float64) * yc.astype(np.float64)).ravel())
            assert abs(sums[m, 2] - exact) <= bound, (step, m, sums[m, 2], exact, bound)
            pair = (sc, yc)
        ret, p_ref, c_ref = mol.control(x[i], f_np[i], step, pair=pair)
        assert ret != O.UNUSABLE
        assert mol.converged_at == conv[m] == s["conv"][m], (step, m, mol.converged_at, conv[m])
        if was_frozen:
            continue
        assert mol.accepted == accepted[m] and mol.h == pairs[m] == s["h"][m], (step, m, mol.accepted, accepted[m], mol.h, pairs[m])
        assert sorted(s["order"][m]) == list(range(raw.M1))
        held = s["order"][m][:mol.h]
        S = [s["S"][a][i].astype(np.float64).ravel() for a in held]
        Y = [s["Y"][a][i].astype(np.float64).ravel() for a in held]
        for k in range(mol.h):  # the same pairs, oldest first
            assert np.array_equal(S[k], mol.s[k].ravel()) and np.array_equal(Y[k], mol.y[k].ravel()), (step, m, k)
        if pair is not None and not mol.accepted and ret == O.MOVING:  # a rejected candidate leaves the history untouched
            stats["rejected"] += 1
            assert np.array_equal(s["order"][m][:mol.h], st_before[1][m][:mol.h]) and mol.h == st_before[0][m]
            for key in ("SS", "SY", "YY"):
                blk, was = s[key][m][np.ix_(held, held)], st_before[2][key][m][np.ix_(held, held)]
                assert np.array_equal(blk, was), (step, m, key)
        stats["h_max"] = max(stats["h_max"], mol.h)
        if ret == O.MOVING and len(i):
            ref = O.two_loop(S, Y, g.ravel(), raw.p["alpha"]).reshape(-1, 3)  # from the device's stored s, y and F
            half_ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) / 2
            err = np.abs(direction[i].astype(np.float64) - ref)
            assert (err <= half_ulp + tol * np.abs(ref).max()).all(), (step, m, err.max())
            gp = float((g * direction[i].astype(np.float64)).sum())
            assert abs(sums[m, 3] - gp) <= (2.0 ** -23 + tol) * float(np.abs(g * ref).sum()) + 1e-300, (step, m, sums[m, 3], gp)
            assert sums[m, 3] < 0  # a descent direction
            assert (direction[i][~free] == 0).all()


def _problem(interleave=False):
    """the five wells of tests/min_oracle.py plus a sixth molecule index without atoms, and a few fixed atoms"""
    batch, kspring, x0, x = MO.wells_problem(interleave=interleave)
    fixed = np.zeros(len(batch), np.uint8)
    fixed[[2, 50, 51, 700, 1607]] = 1
    return batch, kspring, x0, x, fixed


def _force_fn(k_t, x0_t, anharmonic):
    def force(pos):
        d = pos - x0_t
        if anharmonic == 0.0:
            return -(k_t * d)
        u = (d * d).sum(1, keepdim=True)
        return -(k_t * d * (1.0 - 1.8 * anharmonic * u + (anharmonic * anharmonic) * (u * u)))

    return force


_runs = {}


def _drive(lib, memory=3, anharmonic=0.0, interleave=False, fused=False, checks=True, cache=True, max_steps=1000):
    """Minimise the wells through the C entries, the forces from torch between the calls: per step OPEN, forces, CLOSE (fused: one
    OPEN, then forces, MIDDLE).  With `checks`, every step against the mirror and the oracle.  -> dict of the end state and (not
    fused) the positions and converged_at of every step."""
    key = (memory, anharmonic, interleave, fused, max_steps)
    if cache and key in _runs:
        return _runs[key]
    p = dict(P, memory=memory)
    batch_np, kspring, x0, x, fixed_np = _problem(interleave)
    batch, fixed = torch.from_numpy(batch_np).cuda(), torch.from_numpy(fixed_np).cuda()
    k_t, x0_t, x_t = (torch.from_numpy(a).cuda() for a in (kspring[:, None], x0, x))
    force = _force_fn(k_t, x0_t, anharmonic)
    n_mol = 6
    idx = [np.nonzero(batch_np == m)[0] for m in range(n_mol)]
    mols = [O.Molecule(p, fixed_np[idx[m]] == 0) for m in range(n_mol)]
    tol = _tol()
    stats = dict(rejected=0, h_max=0)
    raw = _Raw(lib, x_t, batch, n_mol, p, fixed)
    f = force(raw.pos)
    raw.advance(CLOSE, f)  # the start geometry: counts no step
    if checks:
        _check_step(raw, None, None, None, f, mols, idx, fixed_np, 0, True, tol, stats)
    assert raw.status() == (0, 0, 0) and _bits(raw.forces, f)
    hist = dict(pos=[raw.pos.clone()], conv=[raw.conv.clone()], pairs=[raw.pairs.clone()])
    step = 0
    still_fixed = fixed.bool()
    while step < max_steps and not bool((raw.conv >= 0).all()):
        x_before, f_before = raw.pos.clone(), f.clone()
        p_dev, conv_dev = raw.direction.clone(), raw.conv.clone()
        if not fused or step == 0:
            raw.advance(OPEN, raw.forces)  # (fused: the MIDDLE below has made this move already)
        if checks:  # x is bit-identical to torch.add(x, torch.mul(c, p)) with the device's c and p
            c = raw.state()["cmove"].clone()  # (the next controller copies it to the scale log row: _check_step)
            still = (conv_dev[batch] >= 0) | still_fixed
            xm = torch.where(still[:, None], x_before, torch.add(x_before, torch.mul(c[batch][:, None], p_dev)))
            assert _bits(raw.pos, xm), step
            c_np, p_np = c.cpu().numpy(), p_dev.cpu().numpy()
            for m in range(n_mol):
                if int(conv_dev[m]) >= 0:
                    assert c_np[m] == 0
                elif len(idx[m]):
                    assert MO.ulp_distance(c_np[m], np.float32(O.clamp(p_np[idx[m]].astype(np.float64), p))) <= 1, (step, m)
        for m, mol in enumerate(mols):
            mol.moved(x_before.cpu().numpy()[idx[m]], f_before.cpu().numpy()[idx[m]])
        st_before = None
        if checks:
            s = raw.state()
            st_before = (s["h"].cpu().numpy().copy(), s["order"].cpu().numpy().copy(), {k: s[k].cpu().numpy().copy() for k in ("SS", "SY", "YY")})
        step += 1
        f = force(raw.pos)
        raw.advance(MIDDLE if fused else CLOSE, f)
        if checks:
            _check_step(raw, st_before, x_before.cpu().numpy(), f_before.cpu().numpy(), f, mols, idx, fixed_np, step, False, tol, stats)
        if not fused:
            assert _bits(raw.forces, f)
            hist["pos"].append(raw.pos.clone())
            hist["conv"].append(raw.conv.clone())
            hist["pairs"].append(raw.pairs.clone())
    assert raw.status() == (0, step, 0)
    out = dict(raw=raw, steps=step, batch=batch, fixed=fixed, x_start=x_t, x0=x0_t, k=k_t, hist=hist, stats=stats, idx=idx)
    if cache:
        _runs[key] = out
    return out


@pytest.mark.parametrize("memory,anharmonic,max_steps", [(3, 0.0, 1000), (3, 2.0, 40), (1, 2.0, 24), (100, 2.0, 30)])
def test_every_step_equals_the_mirror_and_the_oracle(hip_lib, memory, anharmonic, max_steps):
    """1. OPEN / CLOSE per step on the five wells plus an empty molecule index, with fixed atoms (the assertions are in _drive and
    _check_step): the stored candidate bit-equal to torch.sub; ff and s.y within n 2^-52 sum |t| of math.fsum of the float64
    products, fmax2 their maximum; pairs held, accepted, converged_at and the stored pairs equal to the oracle fed with the device's
    candidate; the direction within half an fp32 ulp + tol max |p| of the oracle's two loops on the device's stored s, y and F; x
    bit-identical to torch.add(x, torch.mul(c, p)) with the device's c and p, c within 1 ulp of the oracle's clamp.  g.p, which the
    controller takes from the coefficients, is compared with sum g_i p_i of the rounded direction within (2^-23 + tol) sum |g_i p_i|:
    each p_i is within half an fp32 ulp + tol of the fp64 direction.  memory 3 and 1: the ring wraps; memory 100: it never fills."""
    r = _drive(hip_lib, memory=memory, anharmonic=anharmonic, max_steps=max_steps)
    print("steps", r["steps"], r["stats"])
    assert not _bits(r["raw"].pos, r["x_start"])
    if memory <= 3:
        assert r["stats"]["h_max"] == memory and r["steps"] >= memory + 3  # the ring filled and wrapped at least three times
    else:
        assert r["stats"]["h_max"] < memory
    if anharmonic:
        assert r["stats"]["rejected"] >= 1  # 4. the non-convex well: a rejected candidate left the history untouched


def _check_end_state(r, anharmonic):
    raw = r["raw"]
    conv = raw.conv.cpu().numpy()
    batch_np, kspring, x0, x, fixed_np = _problem()
    _, conv_ref, _, _ = O.wells(batch_np, 6, kspring, x0, x, dict(P), 1000, fixed_np, anharmonic=anharmonic)
    print("converged at", conv.tolist(), "oracle", conv_ref.tolist())
    assert (conv >= 0).all() and (conv <= 2 * np.maximum(conv_ref, 1)).all() and r["steps"] == conv.max()
    assert conv[5] == 0 and conv_ref[5] == 0  # no atoms: converged as it stands
    for t in (raw.pos, raw.forces, raw.fmax, raw.sums, raw.scale):
        assert torch.isfinite(t).all()
    free = ~r["fixed"].bool()
    assert (r["k"] * (raw.pos - r["x0"])).abs()[free].max().item() < 2e-3  # at the minimum
    assert _bits(raw.pos[~free], r["x_start"][~free])  # fixed atoms never moved
    assert (raw.fmax < 1e-3).all()


@pytest.mark.parametrize("anharmonic", [0.0, 2.0])
def test_end_state_and_fused_launches(hip_lib, anharmonic):
    """2. every molecule converged within twice the fp64 oracle's own count, the empty molecule at step 0, no NaN anywhere; 5. one
    OPEN, then MIDDLE after every evaluation, is the same minimisation bit for bit"""
    plain = _drive(hip_lib, anharmonic=anharmonic, checks=False)
    _check_end_state(plain, anharmonic)
    fused = _drive(hip_lib, anharmonic=anharmonic, fused=True, checks=False)
    _check_end_state(fused, anharmonic)
    a, b = plain["raw"], fused["raw"]
    for s, t in zip([a.pos, a.forces] + a.logs(), [b.pos, b.forces] + b.logs()):
        assert _bits(s, t) if s.is_floating_point() else torch.equal(s, t)
    for key in a.state():  # (the fused run's last launch also moved - nothing - and so saved x_prev, F_prev and c once more)
        if key not in ("x_prev", "f_prev", "cmove"):
            assert torch.equal(a.state()[key], b.state()[key]), key


def test_interleaved_batch(hip_lib):
    """3. the same with the atoms of the molecules interleaved: no molecule is a contiguous range"""
    r = _drive(hip_lib, anharmonic=2.0, interleave=True, max_steps=20)
    b = r["batch"].cpu().numpy()
    assert (np.diff(b) < 0).sum() > 100 and r["steps"] == 20 and r["stats"]["h_max"] == 3


def test_one_large_molecule_in_two_slices(hip_lib):
    """3. 1 100 atoms in ONE molecule without a batch vector: two slices of 550, added in slice order by the controller"""
    g = torch.Generator().manual_seed(12)
    n = 1100
    x0 = (4 * torch.randn(n, 3, generator=g)).cuda()
    x = x0 + (0.3 * torch.randn(n, 3, generator=g)).cuda()
    k_t = torch.full((n, 1), 4.0, device="cuda")
    force = _force_fn(k_t, x0, 2.0)
    p = dict(P)
    raw = _Raw(hip_lib, x, None, 1, p)
    idx, mols = [np.arange(n)], [O.Molecule(p, np.ones(n, bool))]
    tol, stats = _tol(), dict(rejected=0, h_max=0)
    f = force(raw.pos)
    raw.advance(CLOSE, f)
    _check_step(raw, None, None, None, f, mols, idx, None, 0, True, tol, stats)
    for step in range(1, 11):
        x_before, f_before, p_dev = raw.pos.clone(), f.clone(), raw.direction.clone()
        raw.advance(OPEN, raw.forces)
        assert _bits(raw.pos, torch.add(x_before, torch.mul(raw.state()["cmove"][0], p_dev)))
        mols[0].moved(x_before.cpu().numpy(), f_before.cpu().numpy())
        s = raw.state()
        st_before = (s["h"].cpu().numpy().copy(), s["order"].cpu().numpy().copy(), {k: s[k].cpu().numpy().copy() for k in ("SS", "SY", "YY")})
        f = force(raw.pos)
        raw.advance(CLOSE, f)
        _check_step(raw, st_before, x_before.cpu().numpy(), f_before.cpu().numpy(), f, mols, idx, None, step, False, tol, stats)
    assert raw.status() == (0, 10, 0) and stats["h_max"] == 3


def test_two_runs_are_bit_identical(hip_lib):
    """6. fixed summation order, no floating-point atomics"""
    a = _drive(hip_lib, anharmonic=2.0, fused=True, checks=False, cache=False, max_steps=60)["raw"]
    b = _drive(hip_lib, anharmonic=2.0, fused=True, checks=False, cache=False, max_steps=60)["raw"]
    for s, t in zip([a.pos, a.forces] + a.logs(), [b.pos, b.forces] + b.logs()):
        assert _bits(s, t) if s.is_floating_point() else torch.equal(s, t)
    for s, t in zip(a.state().values(), b.state().values()):
        assert torch.equal(s, t)


def test_frozen_molecules(hip_lib):
    """7. once converged_at[m] >= 0 the molecule's x keeps its bits while the others still move, converged_at never changes and
    its history no longer grows; a molecule that starts at its minimum converges at step 0, never moves and never holds a pair"""
    r = _drive(hip_lib, anharmonic=2.0, checks=False)
    h, batch = r["hist"], r["batch"]
    final = h["conv"][-1]
    assert int(final[:5].max()) > int(final[:5].min()) + 10
    for m in range(5):
        at = int(final[m])
        mine = batch == m
        for s in range(at, len(h["pos"])):
            assert int(h["conv"][s][m]) == at and int(h["pairs"][s][m]) == int(h["pairs"][at][m])
            assert _bits(h["pos"][s][mine], h["pos"][at][mine]), (m, s)
        assert all(int(c[m]) == -1 for c in h["conv"][:at])
    # molecule 0 of a second problem starts AT its minimum
    batch_np, kspring, x0, x, fixed_np = _problem()
    x = x.copy()
    x[batch_np == 3] = x0[batch_np == 3]
    batch_t = torch.from_numpy(batch_np).cuda()
    k_t, x0_t, x_t = (torch.from_numpy(a).cuda() for a in (kspring[:, None], x0, x))
    force = _force_fn(k_t, x0_t, 0.0)
    raw = _Raw(hip_lib, x_t, batch_t, 6, dict(P))
    f = force(raw.pos)
    raw.advance(CLOSE, f)
    assert int(raw.conv[3]) == 0 and int(raw.conv[4]) == -1
    for _ in range(5):
        raw.advance(OPEN, raw.forces)
        f = force(raw.pos)
        raw.advance(CLOSE, f)
    mine = batch_t == 3
    assert _bits(raw.pos[mine], x_t[mine]) and int(raw.conv[3]) == 0 and int(raw.pairs[3]) == 0 and int(raw.state()["h"][3]) == 0
    assert int(raw.pairs[4]) == 3 and not _bits(raw.pos[batch_t == 4], x_t[batch_t == 4])


def test_nan_force_latches_status_2(hip_lib):
    """8. a NaN force through the C entry: status 2, nothing of that step is written, every later launch returns at once"""
    batch_np, kspring, x0, x, _ = _problem()
    batch = torch.from_numpy(batch_np).cuda()
    k_t, x0_t, x_t = (torch.from_numpy(a).cuda() for a in (kspring[:, None], x0, x))
    force = _force_fn(k_t, x0_t, 2.0)
    raw = _Raw(hip_lib, x_t, batch, 6, dict(P))
    f = force(raw.pos)
    raw.advance(CLOSE, f)
    for _ in range(5):
        raw.advance(OPEN, raw.forces)
        f = force(raw.pos)
        raw.advance(CLOSE, f)
    assert raw.status() == (0, 5, 0)
    raw.advance(OPEN, raw.forces)
    watched = lambda: [raw.pos, raw.forces, raw.scale] + raw.logs() + [v for k, v in raw.state().items() if k in ("h", "conv", "order", "SS", "SY", "YY")]
    keep = [t.clone() for t in watched()]
    h4 = int(raw.state()["h"][4])
    assert h4 >= 2
    held = raw.state()["order"][4][:h4].tolist()
    mine = batch == 4  # (a slot index means something per molecule: the rows of molecule 4's atoms)
    rings = [raw.state()[k][held][:, mine].clone() for k in ("S", "Y")]
    bad = force(raw.pos)
    bad[1234, 1] = float("nan")
    raw.advance(CLOSE, bad)
    assert raw.status() == (5, 5, 2)
    raw.advance(OPEN, raw.forces)
    raw.advance(MIDDLE, f)
    raw.advance(CLOSE, f)
    assert raw.status() == (5, 5, 2)
    for t, k in zip(watched(), keep):
        assert _bits(t, k) if t.is_floating_point() else torch.equal(t, k)
    for k, ring in zip(("S", "Y"), rings):  # the pairs held are what they were (the candidate went to the spare slot)
        assert _bits(raw.state()[k][held][:, mine], ring)
    # an infinite force in a molecule that has converged is not looked at
    raw2 = _Raw(hip_lib, x_t, batch, 6, dict(P, fmax=1e6))
    raw2.advance(CLOSE, f)
    assert (raw2.conv == 0).all()
    raw2.advance(OPEN, raw2.forces)
    raw2.advance(CLOSE, bad)
    assert raw2.status() == (0, 1, 0) and _bits(raw2.pos, x_t)


# ------------------------------------------------------------------------------------------------ through the model
_models = {}
LB = dict(memory=4)


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


def _ragged(sizes, density=0.1):
    zs, ps, bs = [], [], []
    for m, n in enumerate(sizes):
        z, p = W.synthetic_molecule(40 + m, n, density=density)
        zs.append(torch.from_numpy(z))
        ps.append(torch.from_numpy(p) + 3.0 * m)
        bs.append(torch.full((n,), m, dtype=torch.long))
    return torch.cat(zs), torch.cat(ps), torch.cat(bs), None


def _system(name):
    if name == "mol40":
        z, pos, batch = W.synthetic_batch(n_mol=1, n_atoms=40, first_seed=31)
        return z % 8 + 1, pos, batch, None
    if name == "ragged":
        return _ragged([7, 12, 20])
    if name == "ragged2":
        return _ragged([7, 12])
    z, pos, box = W.water_box(n_side=4)  # 192 atoms, periodic
    return z, pos, torch.zeros_like(z), box


def _inputs(arch, name):
    z, pos, batch, box = (None if t is None else t.cuda() for t in _system(name))
    n_mol = int(batch.max()) + 1
    q = torch.zeros(n_mol, device="cuda") if arch != "equivariant-transformer" else None
    return z, pos, batch, box, q


def _minimise(model, inputs, K, replays, **kw):
    z, pos, batch, box, q = inputs
    opt = model.capture_minimize(z, pos, batch=batch, box=box, q=q, steps_per_replay=K, lbfgs=LB, **kw)
    logs = dict(epot=[], fmax=[], scale=[], accepted=[], sums=[])
    for _ in range(replays):
        opt()
        for key in logs:
            logs[key].append(getattr(opt, key).clone())
    assert opt.check() == K * replays == opt.steps_done
    return opt, {k: torch.cat(v) for k, v in logs.items()}


@pytest.mark.parametrize("arch", ["tensornet", "equivariant-transformer", "tensornet2"])
def test_minimisation_is_bit_identical_to_capture_plus_torch_mirror(hip_lib, arch):
    """9. mol40, memory 4, 16 steps with K = 1 against capture() and the torch mirror x + c p fed with the device's c and p:
    positions, forces and energies equal bit for bit, the direction of every step within the bound of the two loops on the device's
    own stored pairs; then K = 8 gives the same bits; then reset gives the same minimisation again."""
    from torchmdnet_amd.lbfgs import DeviceLBFGS

    model, inputs = _model(arch), _inputs(arch, "mol40")
    z, pos, batch, box, q = inputs
    fixed = torch.zeros(z.shape[0], dtype=torch.bool, device="cuda")
    fixed[::11] = True
    kw = dict(fmax=1e-4, fixed=fixed)
    replay = model.capture(z, pos, batch, box, q=q)
    opt = model.capture_minimize(z, pos, batch=batch, box=box, q=q, steps_per_replay=1, lbfgs=LB, **kw)
    assert isinstance(opt, DeviceLBFGS) and opt.lbfgs == dict(memory=4, alpha=70.0, max_step=0.2, damping=1.0)
    x = pos.clone()
    e, f = (t.clone() for t in replay(x))
    assert _bits(opt.epot0, e.view(-1)) and _bits(opt.forces, f) and (opt.converged_at == -1).all() and int(opt.pairs[0]) == 0
    want = (f.double() / 70.0).float()
    want[fixed] = 0
    assert _bits(opt.direction, want)  # h = 0: p = F / alpha
    tol = _tol()
    off = (C.c_int64 * 17)()
    assert hip_lib.tmdnet_lbfgs_layout(z.shape[0], 1, 4, off) == 0
    ring = lambda k: opt._ws[off[k]:off[k] + 5 * z.shape[0] * 12].view(torch.float32).view(5, -1, 3)
    logs = dict(epot=[], fmax=[], scale=[], accepted=[], pos=[], forces=[])
    for s in range(16):
        p_dev = opt.direction.clone()
        opt()
        c = opt.scale[0].clone()  # the clamp factor of the move that led to this step
        x = torch.where(fixed[:, None], x, torch.add(x, torch.mul(c[batch][:, None], p_dev)))
        assert _bits(opt.pos, x), s
        e, f = (t.clone() for t in replay(x))
        assert _bits(opt.epot[0], e.view(-1)) and _bits(opt.forces, f), s
        ff = torch.where(fixed, 0.0, (f.double() ** 2).sum(1))
        assert _bits(opt.fmax[0], ff.max().sqrt().float().view(1)), s
        # the direction prepared, from the device's own stored pairs
        h = int(opt.pairs[0])
        order = opt._ws[off[3]:off[3] + 20].view(torch.int32).tolist()[:h]
        g = -torch.where(fixed[:, None], 0.0, f.double()).cpu().numpy().ravel()
        S = [ring(13)[a].double().cpu().numpy().ravel() for a in order]
        Y = [ring(14)[a].double().cpu().numpy().ravel() for a in order]
        ref = O.two_loop(S, Y, g, 70.0).reshape(-1, 3)
        err = np.abs(opt.direction.double().cpu().numpy() - ref)
        assert (err <= np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) / 2 + tol * np.abs(ref).max()).all(), (s, err.max())
        for key in ("epot", "fmax", "scale", "accepted"):
            logs[key].append(getattr(opt, key).clone())
    assert opt.check() == 16 and (x - pos).abs().max().item() > 1e-3 and _bits(x[fixed], pos[fixed])
    assert int(opt.pairs[0]) == 4 or int(torch.cat(logs["accepted"]).sum()) < 4
    logs = {k: torch.cat(v) for k, v in logs.items() if v}
    opt8, logs8 = _minimise(model, inputs, 8, 2, **kw)
    assert _bits(opt8.pos, opt.pos) and _bits(opt8.forces, opt.forces) and _bits(opt8.direction, opt.direction)
    assert torch.equal(opt8.pairs, opt.pairs) and torch.equal(opt8.converged_at, opt.converged_at)
    for key in ("epot", "fmax", "scale"):
        assert _bits(logs8[key], logs[key]), key
    assert torch.equal(logs8["accepted"], logs["accepted"])
    opt8.reset(pos=pos)  # back to the start, the same minimisation again
    assert opt8.check() == 0 and int(opt8.pairs[0]) == 0 and _bits(opt8.direction, want)
    opt8(2)
    assert _bits(opt8.pos, opt.pos) and _bits(opt8.forces, opt.forces) and opt8.check() == 16


def test_overflow_freezes_the_state_at_the_last_valid_step(hip_lib):
    """10. the 192-atom periodic box with max_num_neighbors = 72, scaled by 0.85 between two replays (box and positions in place): the
    first evaluation of the second replay overflows.  pos, the history and the logs stay at the last valid step; check() raises the
    reference's error and reset() clears it."""
    model = _model("tensornet", max_num_neighbors=72)
    z, pos, batch, box = (t.cuda() for t in _system("water192"))
    box = box.clone()
    box0 = box.clone()
    q = torch.zeros(1, device="cuda")
    opt = model.capture_minimize(z, pos, batch=batch, box=box, q=q, steps_per_replay=4, fmax=1e-4, lbfgs=LB)
    opt()
    assert opt.check() == 4
    box.mul_(0.85)
    opt.pos.mul_(0.85)
    off = (C.c_int64 * 17)()
    assert hip_lib.tmdnet_lbfgs_layout(192, 1, 4, off) == 0
    history = lambda: (opt._ws[off[1]:off[8]].clone(), opt._ws[off[13]:off[15]].clone())  # pairs held ... coefficients; the rings
    watched = lambda: (opt.pos, opt.forces, opt.direction, opt.epot, opt.fmax, opt.scale, opt.accepted, opt.sums, opt.pairs, opt.converged_at)
    keep, keep_ws = [t.clone() for t in watched()], history()
    host = (C.c_uint64 * 3)()
    for _ in range(2):  # the replay that overflows, and one more: frozen, nothing moves
        opt()
        with pytest.raises(RuntimeError, match="max_num_pairs"):
            opt.check()
        assert hip_lib.tmdnet_lbfgs_status(None, C.c_void_p(opt._ws.data_ptr()), host) == 3 and (int(host[0]), int(host[1])) == (4, 1)
        for t, k in zip(watched(), keep):
            assert torch.equal(t, k) if not t.is_floating_point() else _bits(t, k)
        head, rings = history()
        # the spare slot took no candidate (the scalar products did not run), so the rings are untouched as a whole
        assert torch.equal(head, keep_ws[0]) and torch.equal(rings, keep_ws[1])
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
    opt = model.capture_minimize(z, pos, batch=batch, q=q, steps_per_replay=2, fmax=1e-4, lbfgs=LB)
    opt()
    assert opt.check() == 2
    keep = [t.clone() for t in (opt.pos, opt.forces, opt.direction, opt.epot, opt.fmax)]
    bad = opt.forces.clone()
    bad[5, 0] = float("nan")
    opt._advance(MIN_CLOSE, bad, None, 0)
    with pytest.raises(RuntimeError, match="forces"):
        opt.check()
    opt()
    with pytest.raises(RuntimeError, match="not finite"):
        opt.check()
    for t, k in zip((opt.pos, opt.forces, opt.direction, opt.epot, opt.fmax), keep):
        assert _bits(t, k)
    opt.reset()
    opt()
    assert opt.check() == 2 and not _bits(opt.pos, keep[0])


def test_refusals_leave_the_model_as_it_was(hip_lib):
    """11."""
    model = _model("tensornet")
    z, pos, batch, _, q = _inputs("tensornet", "ragged")
    box = (30.0 * torch.eye(3, device="cuda")).repeat(3, 1, 1)
    replay = model.capture(z, pos, batch, q=q)
    e0, f0 = (t.clone() for t in replay(pos))
    for bad in (dict(history=3), dict(memory=0), dict(memory=513), dict(alpha=0.0), dict(max_step=-0.1), dict(damping=0.0),
                dict(alpha=float("nan")), dict(memory=2.5)):
        with pytest.raises(ValueError, match="lbfgs"):
            model.capture_minimize(z, pos, batch=batch, q=q, lbfgs=bad)
    with pytest.raises(ValueError, match="exclude"):
        model.capture_minimize(z, pos, batch=batch, q=q, lbfgs={}, fire=dict(dt=0.1))
    with pytest.raises(NotImplementedError, match="cell"):
        model.capture_minimize(z, pos, batch=batch, q=q, box=box, lbfgs={}, cell={})
    with pytest.raises(ValueError):
        model.capture_minimize(z, pos, batch=batch, q=q, lbfgs={}, steps_per_replay=0)
    with pytest.raises(ValueError):
        model.capture_minimize(z, pos, batch=batch, q=q, lbfgs={}, fmax=0.0)
    with pytest.raises(ValueError):
        model.capture_minimize(z, pos, batch=batch, q=q, lbfgs={}, fixed=torch.zeros(3, device="cuda"))
    with pytest.raises(NotImplementedError):
        model.capture_minimize(z, pos, batch=batch, q=q, lbfgs={}, atom_weights=torch.ones(z.shape[0], device="cuda"))
    with pytest.raises(NotImplementedError):
        model.capture_minimize(z, pos, batch=batch, q=q, lbfgs={}, halo_exchange=lambda *a: None)
    e1, f1 = replay(pos)  # the graph captured before the refusals is still valid, and gives the same bits
    assert _bits(e1, e0) and _bits(f1, f0)


class _NeverReplayed:
    """stands in for the graph once the engine has changed: the guard has to raise before it gets here"""

    def replay(self):
        raise AssertionError("a stale graph was replayed")


def test_a_stale_loop_raises_and_replays_nothing(hip_lib):
    """12. once the engine's workspaces are re-created, a replay, a reset and a run raise instead of touching freed memory"""
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(4)
    model = create_model(dict(W.TINY_ARGS, static_shapes=True)).to("cuda")  # (its own model: the test re-creates its workspaces)
    z, pos, batch, _, q = _inputs("tensornet", "ragged")
    opt = model.capture_minimize(z, pos, batch=batch, q=q, steps_per_replay=2, fmax=1e-6, lbfgs=LB, warmup=1)
    opt()
    assert opt.check() == 2 == opt.steps_done
    zb, pb, bb = W.synthetic_batch(n_mol=40, n_atoms=60)
    model(zb.cuda() % 19 + 1, pb.cuda(), bb.cuda())  # a larger system: the workspaces grow
    graph, opt.graph = opt.graph, _NeverReplayed()  # (the real graph stays alive, unreplayed, until the test ends)
    stale = r"stale HIP graph.*capture_minimize\(\)"
    with pytest.raises(RuntimeError, match=stale):
        opt()
    with pytest.raises(RuntimeError, match=stale):
        opt.reset()
    assert not bool((opt.converged_at >= 0).all())
    with pytest.raises(RuntimeError, match=stale):
        opt.run(2)
    assert opt.steps_done == 2
    del graph


#: the steps the fp64 CPU oracle (oracle/tensornet_torch.py forces of this model + tests/lbfgs_oracle.py, ASE's defaults, fmax 0.05)
#: takes on the molecules of 7 and 12 atoms of _system("ragged2"), recorded once on the CPU
ORACLE_STEPS = (46, 115)


def test_run_stops_at_convergence_or_at_max_steps(hip_lib):
    """13. fmax above every force: converged as it stands.  The convergence leg: ragged2 with ASE's defaults, on which the fp64 CPU
    oracle converges in ORACLE_STEPS; the device may take twice that.  Then the max_steps stop."""
    model, inputs = _model("tensornet"), _inputs("tensornet", "ragged2")
    z, pos, batch, box, q = inputs
    opt = model.capture_minimize(z, pos, batch=batch, q=q, steps_per_replay=4, fmax=1e6, lbfgs={})
    assert opt.run(100) == 0 and _bits(opt.pos, pos) and (opt.converged_at == 0).all() and opt.check() == 0
    assert (opt.fmax0 > 0).all() and (opt.fmax0 < 1e6).all() and (opt.pairs == 0).all()
    opt = model.capture_minimize(z, pos, batch=batch, q=q, steps_per_replay=5, fmax=0.05, lbfgs={})
    taken = opt.run(2 * max(ORACLE_STEPS), check_every=2)
    conv = opt.converged_at.tolist()
    print("converged at", conv, "oracle", ORACLE_STEPS, "steps taken", taken)
    assert opt.check() == taken
    assert all(0 <= c <= 2 * r for c, r in zip(conv, ORACLE_STEPS)) and taken <= 2 * max(ORACLE_STEPS)
    assert (opt.fmax[-1] < 0.05).all()
    opt = model.capture_minimize(z, pos, batch=batch, q=q, steps_per_replay=4, fmax=1e-7, lbfgs=LB)  # below what 20 steps reach
    assert opt.run(20, check_every=2) == 20 and opt.check() == 20 and (opt.converged_at == -1).all()
    assert opt.run(7) == 4 and opt.check() == 24  # whole replays only, never beyond max_steps
    assert not _bits(opt.pos, pos)
