"""-m gpu: cell relaxation in the device-resident FIRE minimiser (csrc/tn_min.hip, TorchMD_Net.capture_minimize(cell=...)).

1. the C entries alone (no model, graph_ws = NULL) on the spring crystal of tests/min_cell_oracle.py, whose forces and virial torch
   computes between single launches: every step against the host mirror and the oracle, the end state, repeatability, two slices
2. through the model: K steps per graph launch are bit-identical to capture(virial=True) + a torch mirror that takes the device's
   coefficients and D32 and issues torch.mul / torch.add separately
3. a fully masked cell equals cell=None bit for bit;  4. the enthalpy falls and the stress log is the evaluation's
5. overflow and a NaN virial freeze the state, the box included;  6. refusals"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import min_cell_host_mirror as H
from tests import min_cell_oracle as CO
from tests import min_oracle as O
from tests.test_gpu_minimize import _bits, _check_sums, _model, _system

pytestmark = pytest.mark.gpu

OPEN, MIDDLE, CLOSE = 0, 1, 2
P = dict(O.FIRE, fmax=1e-4)
ONES = [[1.0] * 3] * 3


def _cp(pressure=0.0, **kw):
    return dict(CO.CELL, pressure=pressure, **kw)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ the C entries alone
class _Crystals:
    """Several spring crystals as one batch, the atoms interleaved: positions, boxes, and forces / virials by torch in fp64 from the
    fp32 positions and boxes, rounded to fp32 as an engine's would be."""

    def __init__(self, reps_list, interleave=True, seed=3):
        rng = np.random.default_rng(seed)
        xs, Hs, bi, bj, bn, bm, batch, off = [], [], [], [], [], [], [], 0
        self.parts = []
        for m, reps in enumerate(reps_list):
            x, Hm, bonds = CO.crystal(reps)
            x = 0.95 * (x + 0.03 * rng.normal(size=x.shape))  # compressed by 5 %, in its sheared box, atoms displaced
            xs.append(x); Hs.append(0.95 * Hm)
            bi.append(bonds[0] + off); bj.append(bonds[1] + off); bn.append(bonds[2]); bm.append(np.full(len(bonds[0]), m))
            batch.append(np.full(len(x), m))
            self.parts.append((off, len(x), bonds))
            off += len(x)
        x, batch = np.concatenate(xs), np.concatenate(batch)
        perm = rng.permutation(off) if interleave else np.arange(off)
        inv = np.empty(off, np.int64)
        inv[perm] = np.arange(off)
        self.perm, self.n_mol = perm, len(reps_list)
        self.x = torch.from_numpy(x[perm].astype(np.float32)).cuda()
        self.batch = torch.from_numpy(batch[perm]).cuda()
        self.box = torch.from_numpy(np.stack(Hs).astype(np.float32)).cuda()
        self.bi, self.bj = (torch.from_numpy(inv[np.concatenate(a)]).cuda() for a in (bi, bj))
        self.bn, self.bm = torch.from_numpy(np.concatenate(bn)).cuda(), torch.from_numpy(np.concatenate(bm)).cuda()
        self.cfac = torch.tensor([float(n) for _, n, _ in self.parts], dtype=torch.float64, device="cuda")

    def efw(self, x, box):
        x, Hb = x.double(), box.double()[self.bm]
        r = x[self.bj] - x[self.bi] + torch.einsum("bk,bkc->bc", self.bn, Hb)
        L = r.norm(dim=1)
        f = -(CO.KSPRING * (L - CO.R0) / L)[:, None] * r
        F = torch.zeros_like(x).index_add_(0, self.bj, f).index_add_(0, self.bi, -f)
        W = torch.zeros(self.n_mol, 3, 3, dtype=torch.float64, device="cuda").index_add_(0, self.bm, r[:, :, None] * f[:, None, :])
        return F.float(), W.float()

    def molecule(self, m, x):
        """the atoms of molecule m in the crystal's own order (fp64 numpy), and its bonds"""
        off, n, bonds = self.parts[m]
        inv = np.empty(len(self.perm), np.int64)
        inv[self.perm] = np.arange(len(self.perm))
        return _np(x).astype(np.float64)[inv[off:off + n]], bonds


class _RawCell:
    """The cell C entries on tensors of the test's own, m = graph_ws = NULL."""

    def __init__(self, lib, sys, p, cp, fixed=None):
        self.L, self.sys, self.p, self.cp = lib, sys, p, cp
        self.n, self.n_mol = sys.x.shape[0], sys.n_mol
        self.pos, self.xt, self.vel = sys.x.clone(), torch.full_like(sys.x, float("nan")), torch.zeros_like(sys.x)
        self.box, self.fixed = sys.box.clone(), fixed
        nb = C.c_size_t(0)
        assert lib.tmdnet_min_workspace_bytes_cell(self.n, self.n_mol, C.byref(nb)) == 0
        self.ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        nan, B = float("nan"), self.n_mol
        f64 = dict(dtype=torch.float64, device="cuda")
        self.deform, self.cell_vel = torch.full((B, 3, 3), nan, **f64), torch.full((B, 3, 3), nan, **f64)
        self.forces = torch.full_like(sys.x, nan)
        self.fmax, self.coef = torch.full((B,), nan, device="cuda"), torch.full((B, 3), nan, device="cuda")
        self.sums, self.dt, self.alpha = torch.full((B, 4), nan, **f64), torch.full((B,), nan, **f64), torch.full((B,), nan, **f64)
        self.conv = torch.full((B,), -7, dtype=torch.int64, device="cuda")
        self.stress, self.volume, self.cell_force = torch.full((B, 3, 3), nan, **f64), torch.full((B,), nan, **f64), torch.full((B, 3, 3), nan, **f64)
        self.mask = (C.c_double * 9)(*[float(v) for row in cp["mask"] for v in row])
        pp = self._p
        assert lib.tmdnet_min_reset_cell(self._s(), pp(self.ws), self.n, B, 0, p["dt"], p["alpha"], pp(self.box), pp(self.deform),
                                         pp(self.cell_vel), pp(self.pos), pp(self.xt)) == 0

    @staticmethod
    def _s():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def advance(self, phase, forces, virial=None):
        p, f = self._p, self.p
        logs = [None] * 7 if phase == OPEN else [None] + [p(t) for t in (self.fmax, self.sums, self.coef, self.dt, self.alpha, self.conv)]
        cell_logs = [None] * 3 if phase == OPEN else [p(t) for t in (self.stress, self.volume, self.cell_force)]
        rc = self.L.tmdnet_min_advance_cell(None, self._s(), None, p(self.ws), self.n, self.n_mol, phase, p(self.pos), p(self.vel), p(forces),
                                            None, p(self.fixed), p(self.sys.batch), None if phase == OPEN else p(self.forces), f["dt_max"],
                                            f["n_min"], f["f_inc"], f["f_dec"], f["alpha"], f["f_alpha"], f["max_step"], f["fmax"], *logs,
                                            p(self.xt), p(self.box), p(self.deform), p(self.cell_vel), p(virial), p(self.sys.cfac), self.mask,
                                            H.flags(self.cp), self.cp["pressure"], *cell_logs)
        assert rc == 0, rc

    def status(self):
        host = (C.c_uint64 * 3)()
        rc = self.L.tmdnet_min_status_cell(self._s(), self._p(self.ws), host)
        return rc, int(host[0]), int(host[1]), int(host[2])

    def state(self):
        return [t.clone() for t in (self.pos, self.xt, self.vel, self.box, self.deform, self.cell_vel, self.forces, self.fmax, self.sums,
                                    self.coef, self.dt, self.alpha, self.conv, self.stress, self.volume, self.cell_force)]


def _same(a, b):
    return all(torch.equal(s, t) if not s.is_floating_point() else _bits(s, t) for s, t in zip(a, b))


def _close64(a, b):
    """fp64 results of the same statements, up to the contraction of a product into a sum: 1e-13 of the largest entry (a sum of three
    products that cancel keeps the absolute error of its terms, not the relative one)"""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return bool(np.abs(a - b).max() <= 1e-13 * np.abs(b).max())


def _check_step(raw, state, vt, F, Wv, d32, step, where):
    """After a CLOSE on (F, Wv): the device's atoms' sums against the mirror's terms, and the controller against the host mirror and the
    oracle fed with the device's sums, D and V_D.  dt, alpha, converged_at are equal; the fp32 outputs (coefficients, next D32, next
    box) are within 1 ulp and the fp64 ones within 1e-13 of their scale (the device compiler may contract an fp64 product into the sum
    that consumes it).  -> the mirror's output (the next D32 and box the OPEN that follows must install)."""
    sys, B = raw.sys, raw.n_mol
    batch = _np(sys.batch)
    fixed = None if raw.fixed is None else _np(raw.fixed)
    ft, t = H.terms(batch, d32.reshape(B, 9), _np(vt), _np(F), fixed)
    _check_sums(raw.sums, torch.from_numpy(t), sys.batch, B, where)
    sums, D, VD, box = _np(raw.sums), _np(raw.deform), _np(raw.cell_vel), _np(raw.box)
    new_state, o = H.control(state, sums, _np(Wv), box, d32, raw.H0, D, VD, _np(sys.cfac), raw.p, raw.cp, step)
    assert (o["ret"] != O.UNUSABLE).all(), (where, o["why"])
    assert (_np(raw.dt) == new_state[0]).all() and (_np(raw.alpha) == new_state[1]).all() and (_np(raw.conv) == new_state[3]).all(), where
    assert O.ulp_distance(_np(raw.coef), o["coef"]).max() <= 1, (where, _np(raw.coef), o["coef"])
    assert _close64(_np(raw.cell_force), o["Gc"]) and _close64(_np(raw.stress), o["stress"]) and _close64(_np(raw.volume), o["V"]), where
    assert O.ulp_distance(_np(raw.fmax), np.sqrt(o["sums"][:, 3]).astype(np.float32)).max() <= 1, where  # with the cell rows
    for m in range(B):  # the oracle, molecule by molecule, from the same inputs: the mirror's bits
        s = dict(dt=float(state[0][m]), alpha=float(state[1][m]), n_pos=int(state[2][m]), converged_at=int(state[3][m]))
        r = CO.control(s, raw.p, raw.cp, float(_np(sys.cfac)[m]), sums[m], _np(Wv)[m], box[m], d32[m], raw.H0[m], D[m], VD[m], step)
        assert (np.asarray(r["coef"]).view(np.uint32) == o["coef"][m].view(np.uint32)).all() and (r["d32"].view(np.uint32) == o["d32"][m].view(np.uint32)).all(), where
        assert (r["box"].view(np.uint32) == o["box"][m].view(np.uint32)).all() and s["dt"] == new_state[0][m], where
    return new_state, o


_runs = {}


def _drive(lib, reps_list, cp, fused=False, checks=True, max_steps=600, fixed_every=0, cache_key=None):
    """Relax the crystals through the C entries: per step OPEN, forces, CLOSE (fused: one OPEN, then forces, MIDDLE)."""
    if cache_key is not None and cache_key in _runs:
        return _runs[cache_key]
    sys = _Crystals(reps_list)
    fixed = None
    if fixed_every:
        fixed = torch.zeros(sys.x.shape[0], dtype=torch.uint8, device="cuda")
        fixed[::fixed_every] = 1
    raw = _RawCell(lib, sys, P, cp, fixed)
    raw.H0 = _np(sys.box).astype(np.float64).reshape(sys.n_mol, 9)
    B = sys.n_mol
    assert _bits(raw.xt, sys.x) and (raw.deform == torch.eye(3, device="cuda", dtype=torch.float64)).all() and (raw.cell_vel == 0).all()
    state = (np.full(B, P["dt"]), np.full(B, P["alpha"]), np.zeros(B, np.int32), np.full(B, -1, np.int64))
    d32 = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (B, 1))
    F, Wv = sys.efw(raw.pos, raw.box)
    raw.advance(CLOSE, F, Wv)
    xt, vt, x = raw.xt.clone(), raw.vel.clone(), raw.pos.clone()
    o = None
    if checks:
        state, o = _check_step(raw, state, vt, F, Wv, d32, 0, "start")
    assert raw.status() == (0, 0, 0, 0) and _bits(raw.forces, F)
    step = 0
    while step < max_steps and not bool((raw.conv >= 0).all()):
        if not fused or step == 0:
            raw.advance(OPEN, raw.forces)
        if checks:  # the move: D32 and box from the mirror's control (within 1 ulp), then xt, vt, x bit for bit with the device's D32
            d32_new = _np(raw.deform).astype(np.float32).reshape(B, 9)
            assert O.ulp_distance(d32_new, o["d32"]).max() <= 1 and O.ulp_distance(_np(raw.box).reshape(B, 9), o["box"]).max() <= 1, step
            assert _close64(_np(raw.deform), o["D"]), step
            xt_m, vt_m, x_m = H.update(_np(sys.batch), state[3], None if fixed is None else _np(fixed), _np(raw.coef), d32, d32_new, _np(xt),
                                       _np(vt), _np(F), _np(x))
            xt, vt, x = (torch.from_numpy(a).cuda() for a in (xt_m, vt_m, x_m))
            assert _bits(raw.xt, xt) and _bits(raw.vel, vt) and _bits(raw.pos, x), step
            d32 = d32_new
        step += 1
        F, Wv = sys.efw(raw.pos, raw.box)
        raw.advance(MIDDLE if fused else CLOSE, F, Wv)
        if checks:
            state, o = _check_step(raw, state, vt, F, Wv, d32, step, step)
    assert raw.status() == (0, step, 0, 0)
    out = dict(raw=raw, sys=sys, steps=step, fixed=fixed)
    if cache_key is not None:
        _runs[cache_key] = out
    return out


def test_every_step_equals_the_host_mirror_and_the_oracle(hip_lib):
    """1. Two crystals of 4 and 32 atoms with interleaved `batch`, OPEN / CLOSE per step until both have converged (assertions in
    _drive and _check_step), then the end state: every bond at R0 within tests/min_cell_oracle.py's length_bound (measured: converged
    at steps 143 and 322; max |L - R0| 2.7e-5 and 4.0e-5 against bounds of 2.7e-4 and 1.7e-3)."""
    r = _drive(hip_lib, [(1, 1, 1), (2, 2, 2)], _cp(), cache_key="pair")
    raw, sys = r["raw"], r["sys"]
    conv = _np(raw.conv)
    print("converged at", conv.tolist())
    assert (conv > 20).all() and r["steps"] == conv.max() and len(set(conv.tolist())) == 2  # every molecule its own controller
    assert (np.diff(_np(sys.batch)) < 0).sum() > 3
    for m in range(2):
        xt, bonds = sys.molecule(m, raw.xt)
        x, _ = sys.molecule(m, raw.pos)
        D, c = _np(raw.deform)[m], float(_np(sys.cfac)[m])
        bound = CO.length_bound(xt, D, raw.H0[m].reshape(3, 3), bonds, c, P["fmax"])
        L = CO.bond_lengths(x, _np(raw.box)[m].astype(np.float64), bonds)
        print("molecule", m, "max |L - R0|", np.abs(L - CO.R0).max(), "bound", bound)
        assert np.abs(L - CO.R0).max() < bound < 1e-2
    assert (raw.fmax < P["fmax"]).all()


def test_fused_launches_and_pressure(hip_lib):
    """1. One OPEN, then MIDDLE after every evaluation is the same minimisation bit for bit; it repeats bit for bit; and at pressure
    0.4 the converged state, evaluated again in fp64, satisfies the criterion it stopped on within criterion_slack."""
    a = _drive(hip_lib, [(1, 1, 1), (2, 2, 2)], _cp(), cache_key="pair")
    b = _drive(hip_lib, [(1, 1, 1), (2, 2, 2)], _cp(), fused=True, checks=False)
    c = _drive(hip_lib, [(1, 1, 1), (2, 2, 2)], _cp(), fused=True, checks=False)
    sa, sb, sc = a["raw"].state(), b["raw"].state(), c["raw"].state()
    assert _same(sb, sc)  # fixed summation order, no floating-point atomics
    # (the velocities: the MIDDLE that found everything converged has frozen them, the last CLOSE has not)
    assert _same(sa[:2] + sa[3:5] + sa[6:], sb[:2] + sb[3:5] + sb[6:]) and (b["raw"].vel == 0).all() and b["steps"] == a["steps"]
    p = 0.4
    r = _drive(hip_lib, [(1, 1, 1), (2, 2, 2)], _cp(p), fused=True, checks=False)
    raw, sys = r["raw"], r["sys"]
    assert (raw.conv > 0).all()
    for m in range(2):
        xt, bonds = sys.molecule(m, raw.xt)
        x, _ = sys.molecule(m, raw.pos)
        D, c = _np(raw.deform)[m], float(_np(sys.cfac)[m])
        Ft, Gc, _ = CO.generalised_forces(xt, raw.H0[m].reshape(3, 3), D, bonds, _cp(p), c)
        fmax64 = math.sqrt(max((Ft * Ft).sum(1).max(), (Gc * Gc).sum(1).max()))
        slack = CO.criterion_slack(x, _np(raw.box)[m], bonds, c, P["fmax"])
        V = abs(np.linalg.det(_np(raw.box)[m].astype(np.float64)))
        print("molecule", m, "fmax", float(raw.fmax[m]), "in fp64", fmax64, "slack", slack, "V / V_rest", V / abs(np.linalg.det(CO.crystal(((1, 1, 1), (2, 2, 2))[m])[1])))
        assert float(raw.fmax[m]) < P["fmax"] and fmax64 < P["fmax"] + slack
        assert V < 0.99 * abs(np.linalg.det(CO.crystal(((1, 1, 1), (2, 2, 2))[m])[1]))


def test_one_molecule_in_two_reduction_slices(hip_lib):
    """1. 1 100 atoms in ONE molecule (5 x 5 x 11 cells): two slices of 550, added in slice order by the controller; a few fixed
    atoms; 8 steps, each against the host mirror and the oracle."""
    r = _drive(hip_lib, [(5, 5, 11)], _cp(0.1), max_steps=8, fixed_every=97)
    raw, sys = r["raw"], r["sys"]
    assert raw.n == 1100 and r["steps"] == 8 and not _bits(raw.box, sys.box) and not _bits(raw.pos, sys.x)
    fixed = r["fixed"].bool()
    assert _bits(raw.xt[fixed], sys.x[fixed]) and not _bits(raw.pos[fixed], sys.x[fixed])  # a fixed atom follows the cell


def test_nan_virial_and_flat_box_latch_status_2(hip_lib):
    """5. a NaN in the virial buffer: status 2, detail 2, nothing of that step is written - the box keeps its bits - and every later
    launch returns at once; a box without volume: detail 3."""
    sys = _Crystals([(1, 1, 1), (2, 2, 2)])
    raw = _RawCell(hip_lib, sys, P, _cp())
    F, Wv = sys.efw(raw.pos, raw.box)
    raw.advance(CLOSE, F, Wv)
    for _ in range(3):
        raw.advance(OPEN, raw.forces)
        F, Wv = sys.efw(raw.pos, raw.box)
        raw.advance(CLOSE, F, Wv)
    assert raw.status() == (0, 3, 0, 0)
    raw.advance(OPEN, raw.forces)
    F, Wv = sys.efw(raw.pos, raw.box)
    keep = raw.state()
    bad = Wv.clone()
    bad[1, 0, 2] = float("nan")
    raw.advance(CLOSE, F, bad)
    assert raw.status() == (5, 3, 2, 2)
    raw.advance(OPEN, raw.forces)
    raw.advance(MIDDLE, F, Wv)
    raw.advance(CLOSE, F, Wv)
    assert raw.status() == (5, 3, 2, 2) and _same(raw.state(), keep)
    raw2 = _RawCell(hip_lib, sys, P, _cp())
    raw2.box[0, 2] = raw2.box[0, 1]
    raw2.advance(CLOSE, F, Wv)
    assert raw2.status() == (5, 0, 2, 3)


# ------------------------------------------------------------------------------------------------ through the model
def _inputs(arch, name):
    if name == "tiny_pbc":
        f = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_pbc_ref.pt"))
        z, pos, batch, box = f["z"], f["pos"].float(), f["batch"], f["box"].float().reshape(3, 3)
    else:
        z, pos, batch, box = _system("water192")
    q = torch.zeros(1, device="cuda") if arch != "equivariant-transformer" else None
    return z.cuda(), pos.cuda(), batch.cuda(), box.cuda().clone(), q


def _mul_rows(a, M):
    """out[:, k] = (a_0 M[k][0] + a_1 M[k][1]) + a_2 M[k][2], every product and sum its own rounded fp32 kernel"""
    col = lambda k, j: M[k, j].expand_as(a[:, j])
    return torch.stack([torch.add(torch.add(torch.mul(a[:, 0], col(k, 0)), torch.mul(a[:, 1], col(k, 1))), torch.mul(a[:, 2], col(k, 2)))
                        for k in range(3)], 1)


def _run(model, inputs, K, replays, cell, **kw):
    z, pos, batch, box, q = inputs
    opt = model.capture_minimize(z, pos, batch=batch, box=box.clone(), q=q, steps_per_replay=K, cell=cell, **kw)
    logs = {k: [] for k in ("epot", "fmax", "coef", "sums", "stress", "volume", "cell_force")}
    for _ in range(replays):
        opt()
        for k in logs:
            logs[k].append(getattr(opt, k).clone())
    assert opt.check() == K * replays
    return opt, {k: torch.cat(v) for k, v in logs.items()}


@pytest.mark.parametrize("arch,name", [("tensornet", "tiny_pbc"), ("equivariant-transformer", "tiny_pbc"), ("tensornet", "water192"),
                                       ("equivariant-transformer", "water192")])
def test_cell_relaxation_is_bit_identical_to_capture_plus_torch_mirror(hip_lib, arch, name):
    """2. 16 steps, one per replay, against capture(virial=True) and the torch mirror: with each step's c_v, c_f, d and D32 taken from
    the device, positions, box, forces and energies are equal bit for bit; the coefficients and the next D32 are within 1 fp32 ulp of
    the oracle fed with the device's sums, D and V_D.  Then 8 x 2 and 16 x 1 replays give the same bits."""
    model, inputs = _model(arch), _inputs(arch, name)
    z, pos, batch, box, q = inputs
    n = z.shape[0]
    fixed = torch.zeros(n, dtype=torch.bool, device="cuda")
    fixed[::11] = True
    cell = dict(pressure=0.002)
    kw = dict(fmax=1e-5, fixed=fixed)
    box_m = box.clone()
    replay = model.capture(z, pos, batch, box_m, q=q, virial=True)
    opt = model.capture_minimize(z, pos, batch=batch, box=box.clone(), q=q, steps_per_replay=1, cell=cell, **kw)
    H0 = _np(box).astype(np.float64).reshape(-1)
    cp = dict(_cp(0.002), mask=[[1.0 if a <= b else 0.0 for b in range(3)] for a in range(3)])  # the rotation gauge of the model path
    p = dict(O.FIRE, fmax=1e-5)
    e, f, w = (t.clone() for t in replay(pos))
    assert _bits(opt.epot0, e.view(-1)) and (opt.converged_at == -1).all()
    xt, vt, x = pos.clone(), torch.zeros_like(pos), pos.clone()
    d32 = torch.eye(3, device="cuda")
    s = O.new_state(p, 1)[0]
    rows = dict(sums=opt._sums0.clone(), coef=opt.coef0.clone())
    logs = {k: [] for k in ("epot", "fmax", "coef", "sums", "stress", "volume", "cell_force")}
    for step in range(17):
        # the oracle on what the device's control of this step saw
        D, VD = _np(opt.deform)[0].reshape(-1), _np(opt._cell_vel)[0].reshape(-1)
        ft = torch.where(fixed[:, None], torch.zeros_like(f), _mul_rows(f, d32.T.contiguous()))
        terms = torch.stack([(ft * vt).sum(1), (ft * ft).sum(1), (vt * vt).sum(1)], 1)  # (rounded differently: the summation bound covers it)
        r = CO.control(s, p, cp, float(n), _np(rows["sums"])[0], _np(w)[0], _np(box_m), _np(d32), H0, D, VD, step)
        assert r["ret"] == O.MOVING and O.ulp_distance(_np(rows["coef"])[0], r["coef"]).max() <= 1, step
        assert abs(float(rows["sums"][0, 1]) - float(terms[:, 1].double().sum())) <= 1e-5 * float(rows["sums"][0, 1]), step
        if step == 16:
            break
        opt()
        d32_new = opt.deform[0].float()
        assert O.ulp_distance(_np(d32_new).reshape(-1), r["d32"]).max() <= 1 and O.ulp_distance(_np(opt.box).reshape(-1), r["box"]).max() <= 1, step
        assert (_np(opt.deform)[0][np.tril_indices(3, -1)] == 0).all() and (_np(opt.box).reshape(3, 3)[np.triu_indices(3, 1)] == 0).all()
        # the torch mirror: the device's coefficients and D32, torch.mul and torch.add separately
        cv, cf, d = (t.expand_as(vt) for t in rows["coef"][0])
        v_new = torch.add(torch.mul(cv, vt), torch.mul(cf, ft))
        vt = torch.where(fixed[:, None], torch.zeros_like(vt), v_new)
        xt = torch.where(fixed[:, None], xt, torch.add(xt, torch.mul(d, v_new)))
        x = _mul_rows(xt, d32_new)
        d32 = d32_new
        box_m.copy_(opt.box.reshape(3, 3))
        e, f, w = (t.clone() for t in replay(x))
        assert _bits(opt.pos, x) and _bits(opt.vel, vt) and _bits(opt._xt, xt), step
        assert _bits(opt.forces, f) and _bits(opt.epot[0], e.view(-1)), step
        Ws = 0.5 * (w[0].double() + w[0].double().T)
        V = float(opt.volume[0, 0])
        assert abs(V - abs(np.linalg.det(_np(box_m).astype(np.float64)))) <= 1e-12 * V
        assert torch.allclose(opt.stress[0, 0], -Ws / V, rtol=1e-12, atol=0)
        rows = dict(sums=opt.sums[0].clone(), coef=opt.coef[0].clone())
        for k in logs:
            logs[k].append(getattr(opt, k).clone())
    assert opt.check() == 16
    assert (x - pos).abs().max().item() > 1e-4 and not _bits(opt.box.reshape(3, 3), box)  # the atoms and the box really moved
    assert _bits(xt[fixed], pos[fixed]) and not _bits(x[fixed], pos[fixed])  # a fixed atom keeps xt and follows the cell
    logs = {k: torch.cat(v) for k, v in logs.items()}
    for K, replays in ((8, 2), (16, 1)):
        opt2, logs2 = _run(model, inputs, K, replays, cell, **kw)
        assert _bits(opt2.pos, opt.pos) and _bits(opt2.forces, opt.forces) and _bits(opt2.vel, opt.vel), (K, replays)
        assert _bits(opt2.box, opt.box) and _bits(opt2.deform, opt.deform) and torch.equal(opt2.converged_at, opt.converged_at), (K, replays)
        for k in logs:
            assert _bits(logs2[k], logs[k]), (K, replays, k)
    # reset: the current box becomes the reference, D = I; with the start geometry the same minimisation again
    opt2.reset(pos=pos, box=box)
    assert (opt2.deform == torch.eye(3, device="cuda", dtype=torch.float64)).all() and _bits(opt2.box.reshape(3, 3), box) and opt2.check() == 0
    opt2()
    assert _bits(opt2.pos, opt.pos) and _bits(opt2.box, opt.box) and opt2.check() == 16


def test_a_fully_masked_cell_equals_the_fixed_box_run(hip_lib):
    """3. mask = zeros: D stays I, every product with D32 is a product with 1 or an exact zero - positions, forces, epot, fmax and
    converged_at equal the cell=None run bit for bit (K = 4, three replays, fixed atoms, the 192-atom periodic box)."""
    model, inputs = _model("tensornet"), _inputs("tensornet", "water192")
    z, pos, batch, box, q = inputs
    fixed = torch.zeros(z.shape[0], dtype=torch.bool, device="cuda")
    fixed[::7] = True
    kw = dict(steps_per_replay=4, fmax=1e-4, fixed=fixed)
    a = model.capture_minimize(z, pos, batch=batch, box=box.clone(), q=q, **kw)
    b = model.capture_minimize(z, pos, batch=batch, box=box.clone(), q=q, cell=dict(mask=torch.zeros(3, 3), pressure=0.3), **kw)
    assert _bits(a.epot0, b.epot0) and _bits(a.fmax0, b.fmax0) and _bits(a.coef0, b.coef0)
    for _ in range(3):
        a()
        b()
        for name in ("pos", "vel", "forces", "epot", "fmax", "coef", "sums", "step_size", "alpha"):
            assert _bits(getattr(a, name), getattr(b, name)), name
        assert torch.equal(a.converged_at, b.converged_at)
    assert a.check() == b.check() == 12 and _bits(b.box, box) and (b.deform == torch.eye(3, device="cuda", dtype=torch.float64)).all()
    assert not _bits(a.pos, pos)


@pytest.mark.parametrize("seed,grows", [(2, True), (4, False)])
def test_enthalpy_falls_and_the_box_follows_the_stress(hip_lib, seed, grows):
    """4. the water box compressed by 3 %, pressure 0, 40 steps: E + p V from energy_forces_virial at opt.pos / opt.box is below the
    start value, the box has grown, and opt.stress[k] is -W_s / V of a separate evaluation at step k's state.  The weights are
    random, so whether this box resists compression depends on the seed: with seed 2 it does (the fp64 oracle gives E = 54.8 -> 61.1
    under the compression and tr stress = -0.115 at the start), and the box grows (measured: V 1740.1 -> 1764.2, E 61.09 -> 41.64).  With seed 4, the model of the other tests here,
    the same box is under tension (tr stress = +0.075) and shrinks (measured: V 1740.1 -> 1716.8, E -56.95 -> -64.96): the second
    case, the same assertions in the other direction."""
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(seed)
    model = create_model(dict(W.TINY_ARGS, static_shapes=True)).to("cuda")
    z, pos, batch, box, q = _inputs("tensornet", "water192")
    pos, box = pos * 0.97, box * 0.97
    with torch.no_grad():
        E0, _, W0 = model.energy_forces_virial(z, pos, batch, box=box, q=q)
    opt = model.capture_minimize(z, pos, batch=batch, box=box.clone(), q=q, steps_per_replay=10, cell=dict(pressure=0.0))
    V0 = float(torch.linalg.det(box.double()).abs())
    ref = -0.5 * (W0[0].double() + W0[0].double().T) / V0
    assert torch.allclose(opt.stress0[0], ref, rtol=1e-5, atol=1e-6 * float(ref.abs().max())) and float(opt.volume0[0]) == pytest.approx(V0, rel=1e-12)
    opt(4)
    assert opt.check() == 40
    with torch.no_grad():
        E1, F1, W1 = model.energy_forces_virial(z, opt.pos, batch, box=opt.box, q=q)
    V1 = float(torch.linalg.det(opt.box.double().reshape(3, 3)).abs())
    print("E", float(E0), "->", float(E1), "V", V0, "->", V1, "tr stress", float(opt.stress0[0].trace()), "->", float(opt.stress[9, 0].trace()))
    assert (float(opt.stress0[0].trace()) < 0) == grows  # the premise: compressive stress at the start
    assert float(E1) < float(E0) and (V1 > V0) == grows and V1 != V0
    # (an eager evaluation against the graph's: the same kernels, compared to fp32 rounding rather than bit for bit)
    assert torch.allclose(F1, opt.forces, rtol=1e-5, atol=1e-6) and torch.allclose(E1.view(-1), opt.epot[9], rtol=1e-6)
    assert float(opt.volume[9, 0]) == pytest.approx(V1, rel=1e-12)
    ref = -0.5 * (W1[0].double() + W1[0].double().T) / V1
    assert torch.allclose(opt.stress[9, 0], ref, rtol=1e-5, atol=1e-6 * float(ref.abs().max()))
    assert (opt.fmax[:, 0] >= torch.linalg.norm(opt.cell_force[:, 0], dim=2).max(1).values.float() * (1 - 1e-6)).all()  # fmax sees the cell rows


def _shrinking(model, inputs, K):
    z, pos, batch, box, q = inputs
    return model.capture_minimize(z, pos, batch=batch, box=box.clone(), q=q, steps_per_replay=K, fmax=1e-4,
                                  cell=dict(hydrostatic=True, pressure=5.0, cell_factor=10.0))


def test_overflow_freezes_atoms_and_box_at_the_last_valid_step(hip_lib):
    """5. max_num_neighbors = 72 and a pressure that shrinks the 192-atom box by about 1 % per step until an evaluation overflows:
    status 1, and opt.pos, opt.box, opt.deform and the logs hold the last valid step bit for bit - the one a run with K = 1 recorded
    before its own overflow.  reset(pos=, box=) recovers; a NaN written into the virial gives status 2 and a box with its bits
    unchanged."""
    from torchmdnet_amd.minimize import MIN_CLOSE

    model, inputs = _model("tensornet", max_num_neighbors=72), _inputs("tensornet", "water192")
    z, pos, batch, box, q = inputs
    watched = lambda o: (o.pos, o.vel, o._xt, o.box, o.deform, o._cell_vel, o.forces, o.step_size, o.alpha, o.converged_at)
    one = _shrinking(model, inputs, 1)
    good, last = 0, None
    for _ in range(40):
        keep = [t.clone() for t in watched(one)] + [one.epot.clone(), one.fmax.clone(), one.stress.clone(), one.volume.clone()]
        one()
        try:
            good = one.check()
        except RuntimeError as e:
            assert "max_num_pairs" in str(e)
            last = keep
            break
    assert last is not None and good >= 3, good
    now = [t.clone() for t in watched(one)] + [one.epot.clone(), one.fmax.clone(), one.stress.clone(), one.volume.clone()]
    assert _same(now, last)
    host = (C.c_uint64 * 3)()
    assert hip_lib.tmdnet_min_status_cell(None, C.c_void_p(one._ws.data_ptr()), host) == 3 and (int(host[0]), int(host[1])) == (good, 1)
    V = float(torch.linalg.det(one.box.double().reshape(3, 3)).abs()) / float(torch.linalg.det(box.double()).abs())
    print("valid steps", good, "volume ratio at the last valid step", V)
    assert V < 1.0
    four = _shrinking(model, inputs, 4)
    for _ in range(good // 4 + 2):  # the replay that overflows, and one more: frozen, nothing moves
        four()
    with pytest.raises(RuntimeError, match="max_num_pairs"):
        four.check()
    assert _same([t.clone() for t in watched(four)], last[:10])
    # the model evaluates eagerly afterwards, and the loop runs again after a reset at a geometry that fits
    four.reset(pos=pos, box=box)
    assert four.check() == 0 and _bits(four.box.reshape(3, 3), box) and (four.deform == torch.eye(3, device="cuda", dtype=torch.float64)).all()
    four()
    assert four.check() == 4 and not _bits(four.box.reshape(3, 3), box)
    # a NaN in the virial: status 2, the box keeps its bits, check() names the virial
    keep = [t.clone() for t in watched(four)]
    bad = torch.zeros(1, 3, 3, device="cuda")
    bad[0, 1, 1] = float("nan")
    four._advance(MIN_CLOSE, four.forces, None, 0, bad)
    with pytest.raises(RuntimeError, match="virial"):
        four.check()
    four()
    assert _same([t.clone() for t in watched(four)], keep)
    four.reset()
    four()
    assert four.check() == 4


def test_refusals_leave_the_model_as_it_was(hip_lib):
    """6. every refusal, each before anything is staged: a graph captured before them still replays the same bits."""
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    model = _model("tensornet")
    z, pos, batch, box, q = _inputs("tensornet", "tiny_pbc")
    replay = model.capture(z, pos, batch, box, q=q, virial=True)
    e0, f0, w0 = (t.clone() for t in replay(pos))
    for bad in (dict(scalar_pressure=1.0), dict(mask=[[1, 1, 0], [0, 1, 0], [0, 0, 1]]), dict(hydrostatic=True, constant_volume=True),
                dict(cell_factor=0.0), dict(cell_factor=-2.0)):
        with pytest.raises(ValueError):
            model.capture_minimize(z, pos, batch=batch, box=box, q=q, cell=bad)
    open_model = create_model(dict(W.TINY_ARGS, static_shapes=True)).to("cuda")
    with pytest.raises(ValueError, match="box"):
        open_model.capture_minimize(z, pos, batch=batch, q=q, cell={})
    with pytest.raises(ValueError, match="volume"):
        flat = box.clone()
        flat[2] = flat[1]
        model.capture_minimize(z, pos, batch=batch, box=flat, q=q, cell={})
    two = torch.cat([batch, batch + 1])
    with pytest.raises(NotImplementedError, match="per molecule"):
        model.capture_minimize(torch.cat([z, z]), torch.cat([pos, pos]), batch=two, box=box, q=torch.zeros(2, device="cuda"), cell={})
    with pytest.raises(NotImplementedError):
        model.capture_minimize(z, pos, batch=batch, box=box, q=q, cell={}, atom_weights=torch.ones(z.shape[0], device="cuda"))
    with pytest.raises(NotImplementedError):
        model.capture_minimize(z, pos, batch=batch, box=box, q=q, cell={}, halo_exchange=lambda *a: None)
    model.parameter_gradients = True
    try:
        with pytest.raises(NotImplementedError):
            model.capture_minimize(z, pos, batch=batch, box=box, q=q, cell={})
    finally:
        model.parameter_gradients = False
    with pytest.raises(NotImplementedError, match="TensorNet2"):
        _model("tensornet2").capture_minimize(z, pos, batch=batch, box=box, q=torch.zeros(1, device="cuda"), cell={})
    torch.manual_seed(0)
    with pytest.raises(NotImplementedError):
        create_model(dict(W.TINY_ARGS, static_shapes=True, output_model="DipoleMoment")).to("cuda").capture_minimize(
            z, pos, batch=batch, box=box, cell={})
    with pytest.raises(ValueError, match="cell"):
        model.capture_minimize(z, pos, batch=batch, box=box, q=q, steps_per_replay=2).reset(box=box)
    e1, f1, w1 = replay(pos)
    assert _bits(e1, e0) and _bits(f1, f0) and _bits(w1, w0)
