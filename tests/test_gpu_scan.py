"""The relaxed coordinate scan on the GPU (csrc/tn_scan.hip).  Part 1 drives the C entries alone, with energies and forces of the
analytic surface of tests/test_scan_host.py written in torch (fp64 with autograd at the fp32 positions, rounded once), and checks every
step against the host mirror of the header (tests/scan_host_mirror.py) and the fp64 oracle (tests/scan_oracle.py).  Part 2 goes through
``TorchMD_Net.capture_scan`` for TensorNet, the Equivariant Transformer and TensorNet2.

What is compared how.  Per atom everything is fp32 with single-rounded operations and is compared bit for bit.  Per point the device
works in fp64 through sqrt, division and atan2; the device's atan2 is not the host's to the last bit, so what a point hands on after its
one fp32 rounding - the multipliers, the corrections of the CV atoms, their constrained positions - is compared within ONE fp32 ulp with
the mirror and the mirror then goes on from the device's values, so that every other quantity stays bit for bit."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import min_oracle as MO
from tests import scan_host_mirror as H
from tests import scan_oracle as O
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPEN, MIDDLE, CLOSE = 0, 1, 2
P = dict(MO.FIRE, fmax=1e-3)  # ASE's defaults, the bound of the surface runs
TOL, MAX_ITER = 1e-10, 16
TORSION = [("torsion", 0, 1, 2, 3)]
_models = {}


def _bits(a, b):
    if not a.is_floating_point():
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                                              b.contiguous().view(torch.int64 if b.dtype == torch.float64 else torch.int32))


def _np_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all()


def _within_one_ulp(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.maximum(np.spacing(np.abs(a)), np.spacing(np.abs(b)))).all())


def _gap(cvs, cv, target):
    """|cv - target| per CV, a torsion the short way round; the last axis runs over the CVs"""
    d = np.asarray(cv, np.float64) - np.asarray(target, np.float64)
    turn = np.array([cv_[0] == "torsion" for cv_ in cvs])
    return np.abs(np.where(turn, (d + math.pi) % (2 * math.pi) - math.pi, d))


def _drives(cvs):
    return [0.05 if cv[0] == "distance" else 0.1 for cv in cvs]


# ------------------------------------------------------------------------------------------------ the C entries alone
def _surface(x, sites, kappa):
    """torch, fp64 at the fp32 positions x [G,n,3] with autograd, rounded once -> e [G] fp32, f [G n,3] fp32"""
    X = x.detach().double().requires_grad_(True)
    c = [X[:, a] for a in range(4)]
    E = torch.zeros(X.shape[0], dtype=torch.float64, device=X.device)
    for b in range(3):
        E = E + 15.0 * ((c[b] - c[b + 1]).norm(dim=1) - 1.5) ** 2
    th = []
    for b in range(2):
        r1, r2 = c[b] - c[b + 1], c[b + 2] - c[b + 1]
        th.append(torch.atan2(torch.linalg.cross(r1, r2).norm(dim=1), (r1 * r2).sum(1)))
        E = E + 4.0 * (th[b] - 1.9) ** 2
    b1, b2, b3 = c[1] - c[0], c[2] - c[1], c[3] - c[2]
    n1, n2 = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
    phi = torch.atan2(b2.norm(dim=1) * (b1 * n2).sum(1), (n1 * n2).sum(1))
    E = E + 0.6 * (1 + torch.cos(3 * phi)) + 0.3 * (1 - torch.cos(phi)) + 1.5 * (th[0] - 1.9) * torch.cos(phi)
    if X.shape[1] > 4:
        E = E + 0.5 * kappa * ((X[:, 4:] - sites[4:]) ** 2).sum((1, 2))
    (g,) = torch.autograd.grad(E.sum(), X)
    return E.detach().float().contiguous(), (-g).float().reshape(-1, 3).contiguous()


class _Raw:
    """The C entries on tensors of the test's own, m = graph_ws = NULL (no model: energies and forces are what the test hands in)."""

    def __init__(self, lib, cvs, x0, t_fin, p=P, fixed=None, tol=TOL, max_iter=MAX_ITER, drive=None):
        self.L, self.p, self.cvs = lib, p, cvs
        G, n = self.shape = tuple(x0.shape[:2])
        D = self.D = len(cvs)
        kind, atoms = H.cv_arrays(cvs)
        self.kind, self.atoms = (C.c_int32 * D)(*kind.tolist()), (C.c_int32 * (4 * D))(*atoms.reshape(-1).tolist())
        self.distinct = sorted({i for cv in cvs for i in cv[1:]})
        A = self.A = len(self.distinct)
        self.drive_list = _drives(cvs) if drive is None else drive
        self.drive = (C.c_double * D)(*self.drive_list)
        self.tol, self.max_iter = tol, max_iter
        self.x = x0.clone().contiguous()
        self.pos = self.x.view(-1, 3)
        self.vel = torch.zeros_like(self.x)
        self.fixed = fixed
        self.t_fin = torch.as_tensor(t_fin, dtype=torch.float64).reshape(G, D).cuda().contiguous()
        nb = C.c_size_t(0)
        assert lib.tmdnet_scan_workspace_bytes(n, G, C.byref(nb)) == 0
        self.ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
        nan = float("nan")
        f32, f64 = dict(device="cuda"), dict(dtype=torch.float64, device="cuda")
        self.fkeep, self.fperp = torch.full_like(self.x, nan), torch.full_like(self.x, nan)
        self.epot, self.fmax = torch.full((G,), nan, **f32), torch.full((G,), nan, **f32)
        self.sums, self.coef = torch.full((G, 4), nan, **f64), torch.full((G, 3), nan, **f32)
        self.dt, self.alpha = torch.full((G,), nan, **f64), torch.full((G,), nan, **f64)
        self.conv = torch.full((G,), -7, dtype=torch.int64, device="cuda")
        self.cv, self.target = torch.full((G, D), nan, **f64), torch.full((G, D), nan, **f64)
        self.mult, self.corr = torch.full((G, 2, D), nan, **f32), torch.full((G, A, 2, 3), nan, **f32)
        self.cons, self.iters = torch.full((G, A, 3), nan, **f32), torch.full((G,), -7, dtype=torch.int32, device="cuda")
        self.reset()

    @staticmethod
    def _s():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(0 if t is None else t.data_ptr())

    def reset(self):
        G, n = self.shape
        assert self.L.tmdnet_scan_reset(self._s(), self._p(self.ws), n, G, 0, self.p["dt"], self.p["alpha"]) == 0

    def logs(self):
        return [self.epot, self.fmax, self.sums, self.coef, self.dt, self.alpha, self.conv, self.cv, self.target, self.mult, self.corr]

    def tensors(self):
        return [self.x, self.vel, self.fkeep, self.fperp] + self.logs()

    def advance(self, phase, forces, energy):
        p, f = self._p, self.p
        G, n = self.shape
        logs = [None] * 11 if phase == OPEN else [p(t) for t in self.logs()]
        cons = [None, None] if phase == CLOSE else [p(self.cons), p(self.iters)]
        rc = self.L.tmdnet_scan_advance(None, self._s(), None, p(self.ws), n, G, phase, p(self.pos), p(self.vel), p(forces), p(energy),
                                        p(self.fixed), None if phase == OPEN else p(self.fkeep), p(self.fperp), self.D, self.kind,
                                        self.atoms, p(self.t_fin), self.drive, self.tol, self.max_iter, f["dt_max"], f["n_min"], f["f_inc"],
                                        f["f_dec"], f["alpha"], f["f_alpha"], f["max_step"], f["fmax"], *logs, *cons)
        assert rc == 0, rc

    def status(self):
        host = (C.c_uint64 * 3)()
        rc = self.L.tmdnet_scan_status(self._s(), self._p(self.ws), host)
        return rc, int(host[0]), int(host[1]), int(host[2])


def _apply(raw, u, corr, h):
    """u [G,n,3] with the corrections [G,A,2,3] added on the distinct CV atoms (one fp32 sum each); other atoms keep their bits"""
    out = u.copy()
    out[:, raw.distinct] = u[:, raw.distinct] + corr[:, :, h]
    return out


def _drive(lib, cvs, x0, t_fin, sites=None, kappa=2.0, fixed=None, fused=False, max_steps=400, raw=None, **kw):
    """A whole scan through the C entries, every step checked against the mirror.  fused: MIDDLE launches; otherwise CLOSE + OPEN.
    -> (raw, steps, the mirror's state)"""
    G, n = x0.shape[:2]
    D = len(cvs)
    sites_t = None if sites is None else torch.as_tensor(sites, dtype=torch.float64).cuda()
    fx = None if fixed is None else torch.as_tensor(fixed, dtype=torch.uint8).cuda()
    raw = raw or _Raw(lib, cvs, x0, t_fin, fixed=fx, **kw)
    t_fin = raw.t_fin.cpu().numpy()
    state = (np.full(G, P["dt"]), np.full(G, P["alpha"]), np.zeros(G, np.int32), np.full(G, -1, np.int64))
    t_cur = np.zeros((G, 4))
    step = 0
    while True:
        pos, vel = raw.x.cpu().numpy(), raw.vel.cpu().numpy()
        was = state[3].copy()
        e, f = _surface(raw.x, sites_t, kappa)
        raw.advance(MIDDLE if fused else CLOSE, f, e)
        assert raw.status() == (0, step, 0, 0), (raw.status(), step)
        live = was < 0
        m = H.project(cvs, pos, vel, f.cpu().numpy().reshape(G, n, 3), fixed)
        assert (m["why"][live] == 0).all()
        dmult, dcorr = raw.mult.cpu().numpy(), raw.corr.cpu().numpy()
        assert _within_one_ulp(dmult[live], m["mult"][live][:, :, :D]), step
        assert _within_one_ulp(dcorr[live], m["corr"][live][:, :raw.A]), step
        assert np.abs(raw.cv.cpu().numpy()[live] - m["cv"][live][:, :D]).max() <= 1e-14 * max(1.0, np.abs(pos).max()), step
        if step == 0:
            t_cur[:, :D] = raw.target.cpu().numpy()  # the CVs of the start geometry, as the device found them
            assert _np_bits(raw.target.cpu().numpy(), raw.cv.cpu().numpy())
        assert _np_bits(raw.target.cpu().numpy()[live], t_cur[live][:, :D]), step
        # from the device's corrections on: bit for bit
        fperp = _apply(raw, f.cpu().numpy().reshape(G, n, 3), dcorr, 0)
        vperp = _apply(raw, vel, dcorr, 1)
        assert _np_bits(raw.fperp.cpu().numpy()[live], fperp[live]) and _np_bits(raw.fkeep.cpu().numpy()[live], f.cpu().numpy().reshape(G, n, 3)[live])
        free = np.ones(n, bool) if fixed is None else np.asarray(fixed) == 0
        dsums = raw.sums.cpu().numpy()
        want = np.stack([(vperp.astype(np.float64) * fperp)[:, free].sum((1, 2)), (fperp.astype(np.float64) ** 2)[:, free].sum((1, 2)),
                         (vperp.astype(np.float64) ** 2)[:, free].sum((1, 2)), (fperp.astype(np.float64) ** 2).sum(-1)[:, free].max(1)], 1)
        assert np.allclose(dsums[live], want[live], rtol=1e-5, atol=1e-12), (step, dsums, want)
        assert _np_bits(dsums[live], H.tree_sums(fperp, vperp, fixed)[live]), step  # the device's order of addition, restated on the host
        state, coef, ret = H.control(state, dsums, t_cur, t_fin, step, P)
        assert _np_bits(raw.coef.cpu().numpy(), coef) and np.array_equal(raw.conv.cpu().numpy(), state[3]), step
        assert _np_bits(raw.dt.cpu().numpy(), state[0]) and _np_bits(raw.alpha.cpu().numpy(), state[1])
        if (state[3] >= 0).all() or step >= max_steps:
            return raw, step, dict(state=state, t_cur=t_cur, fperp=fperp)
        if not fused:
            raw.advance(OPEN, raw.fperp, None)
        # the move, bit for bit; the constraint step within one ulp, then on from the device's positions
        vel_in = np.where(live[:, None, None], vperp, vel)
        x_m, v_m = H.move(state[3], coef, pos, vel_in, np.where(live[:, None, None], fperp, 0.0).astype(np.float32), fixed)
        x_c, t_cur, why2, iters = H.constrain(cvs, x_m, state[3], t_cur, t_fin, raw.drive_list, raw.tol, raw.max_iter, fixed)
        moving = state[3] < 0
        assert (why2[moving] == 0).all()
        x_d, v_d = raw.x.cpu().numpy(), raw.vel.cpu().numpy()
        assert _np_bits(v_d, v_m), step
        others = np.setdiff1d(np.arange(n), raw.distinct)
        assert _np_bits(x_d[:, others], x_m[:, others]), step
        assert _within_one_ulp(x_d[:, raw.distinct], x_c[:, raw.distinct]), step
        assert _np_bits(x_d[~moving], pos[~moving])
        assert _np_bits(raw.cons.cpu().numpy()[moving], x_d[moving][:, raw.distinct])
        assert np.array_equal(raw.iters.cpu().numpy()[moving], iters[moving]), step
        step += 1


def _chains(G, n=4, sites=None, offsets=None):
    off = [0.0] * G if offsets is None else offsets
    return torch.tensor(np.stack([O.chain(1.0, n, sites, off[g]) for g in range(G)]), dtype=torch.float32).cuda()


def test_one_point_every_step_equals_the_mirror_and_the_closed_form(hip_lib):
    """1. n = 4, one point, to phi = 2.1241: every step against the mirror; the end against E*(phi) and -dE*/dphi with the bounds of
    tests/test_scan_host.py; the step count is the oracle's"""
    t = 2.1241
    raw, steps, _ = _drive(hip_lib, TORSION, _chains(1), [[t]])
    o = O.run(TORSION, O.chain(1.0), [t], [0.1], TOL, MAX_ITER, P, 2000, store32=True)
    E_star, dE_star = O.relaxed_energy(t)
    assert steps == o["converged_at"] == int(raw.conv[0])
    assert abs(float(raw.epot[0]) - E_star) <= 1e-6 and abs(float(raw.mult[0, 0, 0]) + dE_star) <= 3e-3 + 1e-4
    assert float(raw.target[0, 0]) == t and abs(float(raw.cv[0, 0]) - t) <= 4 * 2.0 ** -23


def _forty(hip_lib, fused=False, raw=None):
    rng = np.random.default_rng(7)
    sites = rng.uniform(4.0, 12.0, size=(40, 3))
    fixed = np.zeros(40, np.uint8)
    fixed[[0, 9, 17]] = 1  # a CV atom and two atoms in wells
    cvs = [("torsion", 0, 1, 2, 3), ("distance", 1, 2)]
    x0 = _chains(2, 40, sites, [0.02, 0.5])
    return _drive(hip_lib, cvs, x0, [[1.3, 1.52], [2.4, 1.45]], sites, fixed=fixed, fused=fused, raw=raw), (cvs, x0, sites, fixed)


def test_two_points_of_forty_atoms_freeze_on_their_own_with_fixed_atoms(hip_lib):
    """2. two points x 40 atoms, a torsion and a distance, three fixed atoms (one of them a CV atom): they converge at different steps;
    the point that has converged keeps its bits while the other goes on; fixed atoms never move; a second run gives the same bits;
    further launches on the converged scan change nothing"""
    (raw, steps, _), (cvs, x0, sites, fixed) = _forty(hip_lib)
    conv = raw.conv.cpu().numpy()
    assert (conv > 0).all() and conv[0] != conv[1] and steps == conv.max()
    assert _bits(raw.x[:, [0, 9, 17]], x0[:, [0, 9, 17]])
    assert _gap(cvs, raw.cv.cpu().numpy(), raw.t_fin.cpu().numpy()).max() <= 16 * 2.0 ** -23
    keep = [t.clone() for t in raw.tensors()]
    (again, steps2, _), _ = _forty(hip_lib)
    assert steps2 == steps and all(_bits(a, b) for a, b in zip(again.tensors(), keep))
    e, f = _surface(raw.x, torch.as_tensor(sites).cuda(), 2.0)
    for phase in (OPEN, MIDDLE, CLOSE, OPEN):
        raw.advance(phase, raw.fperp if phase == OPEN else f, None if phase == OPEN else e)
    rc, step, status, _ = raw.status()
    assert (rc, status) == (0, 0) and step == steps + 2
    for a, b in zip(raw.tensors(), keep):
        if a is not raw.vel:
            assert _bits(a, b)
    assert (raw.vel == 0).all()


def test_fused_launches_give_the_bits_of_separate_ones(hip_lib):
    """3. MIDDLE = CLOSE + OPEN"""
    (raw, steps, _), _ = _forty(hip_lib)
    (fused, steps_f, _), _ = _forty(hip_lib, fused=True)
    assert steps == steps_f and _bits(raw.conv, fused.conv) and _bits(raw.x, fused.x) and _bits(raw.epot, fused.epot)


def test_two_slices_with_cv_atoms_across_the_boundary(hip_lib):
    """4. 1 100 atoms are two slices of 550: one torsion on atoms 548...551 straddles that boundary, a second on atoms 1022...1025;
    twelve steps, every one against the mirror"""
    n = 1100
    rng = np.random.default_rng(11)
    turn = np.where((np.arange(n) // 40) % 2 == 0, 1.0, -1.0)[:, None]  # a serpentine: the coordinates stay below 64
    walk = np.cumsum(turn * np.array([1.2, 0.0, 0.0]) + np.array([0.0, 0.03, 0.0]) + 0.4 * rng.normal(size=(n, 3)), 0)
    sites = walk.copy()
    x0 = np.stack([walk + 0.05 * rng.normal(size=(n, 3)) for _ in range(2)])
    x0[:, :4] = O.chain(1.0)
    cvs = [("torsion", 548, 549, 550, 551), ("torsion", 1022, 1023, 1024, 1025)]
    x0_t = torch.tensor(x0, dtype=torch.float32).cuda()
    s0 = np.array([O.cv_all(cvs, x.astype(np.float64))[0] for x in x0_t.cpu().numpy()])
    raw, steps, _ = _drive(hip_lib, cvs, x0_t, s0 + np.array([[0.35, -0.25], [-0.15, 0.3]]), sites, max_steps=12)
    assert steps == 12 and raw.status()[1] == 12
    assert _gap(cvs, raw.cv.cpu().numpy(), raw.target.cpu().numpy()).max() <= 64 * np.spacing(np.float32(np.abs(x0).max()))


def test_four_coupled_cvs(hip_lib):
    """5. D = 4 on five atoms of the chain and a neighbour in a well: twenty steps, every one against the mirror"""
    sites = np.zeros((9, 3))
    sites[4:] = O.chain(1.0)[3] + np.array([[1.2, 0.7, 0.4], [2.5, -0.3, 0.9], [3.6, 0.8, 0.1], [4.9, -0.2, 0.6], [6.0, 0.5, 1.1]])
    cvs = [("torsion", 0, 1, 2, 3), ("angle", 1, 2, 3), ("distance", 0, 3), ("torsion", 1, 2, 3, 4)]
    x0 = _chains(1, 9, sites, [0.05])
    s0 = O.cv_all(cvs, x0[0].cpu().numpy().astype(np.float64))[0]
    raw, steps, _ = _drive(hip_lib, cvs, x0, [s0 + np.array([0.3, -0.1, 0.12, -0.25])], sites, max_steps=20)
    assert steps == 20 and _gap(cvs, raw.cv.cpu().numpy(), raw.target.cpu().numpy()).max() <= 32 * 2.0 ** -23


def test_every_cause_latches_status_2(hip_lib):
    """6. a NaN force (1), a NaN position of a CV atom (2), two identical CVs (3), a constraint step with one correction (4): the
    status, the cause, the step counter of the last valid step, and nothing written afterwards"""
    x0 = _chains(1)
    # cause 3 at the start: nothing is ever accepted
    raw = _Raw(hip_lib, TORSION * 2, x0, [[2.0, 2.0]])
    e, f = _surface(raw.x, None, 0.0)
    raw.advance(CLOSE, f, e)
    assert raw.status() == (5, 0, 2, 3) and torch.isnan(raw.coef).all()
    # causes 1 and 2 after three good steps
    for cause in (1, 2):
        raw, steps, _ = _drive(hip_lib, TORSION, x0, [[2.0]], max_steps=3)
        raw.advance(OPEN, raw.fperp, None)
        keep = [t.clone() for t in [raw.vel, raw.fkeep, raw.fperp] + raw.logs()]
        x_before = raw.x.clone()
        e, f = _surface(raw.x, None, 0.0)
        if cause == 1:
            f[2, 1] = float("nan")
        else:
            raw.x[0, 1, 0] = float("nan")
        for _ in range(2):
            raw.advance(MIDDLE, f, e)
            assert raw.status() == (5, 3, 2, cause)
            assert all(_bits(a, b) for a, b in zip([raw.vel, raw.fkeep, raw.fperp] + raw.logs(), keep))
        if cause == 1:
            assert _bits(raw.x, x_before)
    # cause 4: the constraint step of the move after step 0 fails; the next control latches it and x, v come back
    raw = _Raw(hip_lib, TORSION, x0, [[2.0]], max_iter=1)
    e, f = _surface(raw.x, None, 0.0)
    raw.advance(MIDDLE, f, e)
    assert raw.status() == (0, 0, 0, 0) and not _bits(raw.x, x0) and int(raw.iters[0]) == 1
    e, f = _surface(raw.x, None, 0.0)
    raw.advance(MIDDLE, f, e)
    assert raw.status() == (5, 0, 2, 4) and _bits(raw.x, x0) and (raw.vel == 0).all()


def test_reset_with_new_targets(hip_lib):
    """7. the same workspace, new final targets: the points start again from the CVs of where they stand"""
    raw, steps, _ = _drive(hip_lib, TORSION, _chains(1), [[1.6]])
    assert abs(float(raw.cv[0, 0]) - 1.6) <= 4 * 2.0 ** -23
    raw.t_fin.copy_(torch.tensor([[0.4]], dtype=torch.float64))
    raw.vel.zero_()
    raw.reset()
    raw, steps2, _ = _drive(hip_lib, TORSION, raw.x, [[0.4]], raw=raw)
    assert steps2 > 5 and abs(float(raw.cv[0, 0]) - 0.4) <= 4 * 2.0 ** -23 and abs(float(raw.epot[0]) - O.relaxed_energy(0.4)[0]) <= 1e-6


# ------------------------------------------------------------------------------------------------ through the model
ARCHS = ["tensornet", "equivariant-transformer", "tensornet2"]
CVS = [("torsion", 3, 8, 15, 21), ("distance", 8, 30)]


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


def _molecule(n_atoms=40, n_points=2):
    """-> z [n], pos [G,n,3]: a molecule and copies displaced smoothly by at most 0.1 per atom"""
    z, pos, _ = W.synthetic_batch(n_mol=1, n_atoms=n_atoms, first_seed=31)
    z, pos = (z % 8 + 1).cuda(), pos.cuda()
    out = []
    for g in range(n_points):
        gen = torch.Generator().manual_seed(50 + g)
        k, ph = torch.rand(3, 3, generator=gen).cuda(), (6.28 * torch.rand(3, generator=gen)).cuda()
        out.append(pos + g * (0.1 / math.sqrt(3)) * torch.sin(pos @ k + ph))
    return z, torch.stack(out)


def _q(arch, G):
    return torch.zeros(G, device="cuda") if arch != "equivariant-transformer" else None


def _targets(pos, cvs=CVS, offsets=((0.25, 0.08), (-0.18, -0.06))):
    s0 = np.array([O.cv_all(cvs, x.astype(np.float64))[0] for x in pos.cpu().numpy()])
    return torch.tensor(s0 + np.array(offsets)[:len(s0)], dtype=torch.float64)


def _field(scan, u, corr, h):
    """u [G,n,3] with the corrections [G,A,2,3] added on the CV atoms (one torch.add); other atoms keep their bits"""
    idx = scan.cv_atoms.to(u.device)
    out = u.clone()
    out[:, idx] = torch.add(u[:, idx], corr[:, :, h])
    return out


def _mirror_move(x, v, f, coef, conv, fixed):
    c = coef[:, None, :]
    still = (conv >= 0)[:, None] | fixed[None, :]
    v_new = torch.add(torch.mul(c[..., 0:1], v), torch.mul(c[..., 1:2], f))
    x_new = torch.add(x, torch.mul(c[..., 2:3], v_new))
    return torch.where(still[..., None], x, x_new), torch.where(still[..., None], torch.zeros_like(v), v_new)


def _record(scan, replays):
    keys = ("epot", "fmax", "coef", "corrections", "constrained", "multipliers", "cv", "target")
    logs = {k: [] for k in keys + ("conv",)}
    for _ in range(replays):
        scan()
        for k in keys:
            logs[k].append(getattr(scan, k).clone())
        logs["conv"].append(scan.converged_at.clone())
    assert scan.check() == scan.steps_per_replay * replays == scan.steps_done
    return {k: (torch.cat(v) if k != "conv" else v) for k, v in logs.items()}


@pytest.mark.parametrize("arch", ARCHS)
def test_scan_is_bit_identical_to_capture_plus_torch_mirror(hip_lib, arch):
    """8. two points of 40 atoms, a torsion and a distance, 8 steps one per replay, against capture() on the stacked molecules and a
    torch mirror that takes the device's FIRE coefficients, corrections and constrained CV atoms and issues torch.mul and torch.add
    separately: positions, velocities, F, F_perp, energies and fmax equal bit for bit; then one replay of 8 steps gives the same bits;
    reset restores the start; one start geometry given as [n,3]."""
    model = _model(arch)
    z, pos = _molecule()
    G, n = pos.shape[:2]
    q = _q(arch, G)
    fixed = torch.zeros(n, dtype=torch.bool, device="cuda")
    fixed[::11] = True
    targets = _targets(pos)
    kw = dict(q=q, fmax=1e-5, tol=1e-9, fixed=fixed)
    batch = torch.arange(G, device="cuda").repeat_interleave(n)
    replay = model.capture(z.repeat(G), pos.reshape(-1, 3), batch, q=q)
    scan = model.capture_scan(z, pos, CVS, targets, steps_per_replay=1, **kw)
    idx = scan.cv_atoms.cuda()
    assert _bits(scan.pos, pos) and scan.cv_atoms.tolist() == [3, 8, 15, 21, 30]
    e, f = (t.clone() for t in replay(pos.reshape(-1, 3)))
    assert _bits(scan.epot0, e.view(G)) and (scan.converged_at == -1).all() and _bits(scan.forces, f.view(G, n, 3))
    fp = _field(scan, f.view(G, n, 3), scan.corrections0, 0)
    assert _bits(scan.projected_forces, fp) and _bits(scan.target0, scan.cv0)
    coef, conv = scan.coef0.clone(), scan.converged_at.clone()
    logs = _record(scan, 8)
    x, v = pos.clone(), torch.zeros_like(pos)
    for s in range(8):
        x, v = _mirror_move(x, v, fp, coef, conv, fixed)
        x[:, idx] = logs["constrained"][s]
        e, f = (t.clone() for t in replay(x.reshape(-1, 3)))
        assert _bits(logs["epot"][s], e.view(G)), s
        fp = _field(scan, f.view(G, n, 3), logs["corrections"][s], 0)
        v = _field(scan, v, logs["corrections"][s], 1)
        ff = torch.where(fixed[None, :], 0.0, (fp * fp).sum(-1))  # (the device's terms are single-rounded fp32 sums: a loose look only)
        assert torch.allclose(logs["fmax"][s], ff.amax(1).sqrt(), rtol=1e-5), s
        coef, conv = logs["coef"][s], logs["conv"][s]
        assert (conv == -1).all()
    assert _bits(scan.pos, x) and _bits(scan.vel, v) and _bits(scan.projected_forces, fp) and _bits(scan.forces, f.view(G, n, 3))
    assert (x - pos).abs().max().item() > 1e-4 and _bits(x[:, fixed], pos[:, fixed])
    # the CVs follow the driven targets: |cv - target| within the fp32 rounding of the CV atoms' coordinates
    _, grad = O.cv_all(CVS, x[0].cpu().numpy().astype(np.float64))
    assert _gap(CVS, logs["cv"].cpu().numpy(), logs["target"].cpu().numpy()).max() <= float(np.abs(grad).sum((1, 2)).max()) * 2 * float(np.spacing(np.float32(pos.abs().max().item())))
    scan8 = model.capture_scan(z, pos, CVS, targets, steps_per_replay=8, **kw)
    logs8 = _record(scan8, 1)
    for a, b in ((scan8.pos, scan.pos), (scan8.vel, scan.vel), (scan8.projected_forces, scan.projected_forces), (scan8.forces, scan.forces)):
        assert _bits(a, b)
    for key in ("epot", "fmax", "coef", "corrections", "constrained", "multipliers", "cv", "target"):
        assert _bits(logs8[key].reshape(logs[key].shape), logs[key]), key
    scan8.reset(pos=pos)
    assert (scan8.vel == 0).all() and scan8.check() == 0 and _bits(scan8.pos, pos) and _bits(scan8.epot0, scan.epot0)
    scan8()
    assert scan8.check() == 8 and _bits(scan8.pos, scan.pos)
    one = model.capture_scan(z, pos[0], CVS, targets, steps_per_replay=8, **kw)  # one start geometry for both points
    one()
    assert one.check() == 8 and one.pos.shape == (G, n, 3) and one.epot.shape == (8, G) and not _bits(one.pos[1], pos[0])


def _slope_run(arch, n_free=8, h=0.02, fmax=0.002, max_steps=4000):
    """The figures of test 9.  Stage 1 relaxes three copies of the start geometry at the torsion t; stage 2 is ``reset`` from that relaxed
    geometry to the neighbouring targets t - h, t, t + h and a second run to convergence, so that the three points stay in one basin.
    (Driven independently from the unrelaxed start, the points end 4 length units apart on the random-weight test models, which are
    no force field, and a difference of their energies says nothing.)  For the same reason only the n_free atoms nearest to the
    torsion's bond move, the four torsion atoms among them, and FIRE's whole-molecule step is clamped to the length the branch needs,
    max_step = 0.02: with ASE's 0.2 a point can leave the basin it was relaxed in."""
    model = _model(arch)
    z, pos = _molecule(n_points=1)
    n = pos.shape[1]
    cvs = CVS[:1]
    idx = list(cvs[0][1:])
    centre = pos[0, idx[1:3]].mean(0)
    order = (pos[0] - centre).norm(dim=1)
    order[idx] = -1.0  # the torsion's own atoms first
    fixed = torch.ones(n, dtype=torch.bool, device="cuda")
    fixed[order.argsort()[:n_free]] = False
    s0 = float(O.cv_all(cvs, pos[0].cpu().numpy().astype(np.float64))[0][0])
    # t lies 0.2 rad below the start's torsion.  (Above it, at s0 + 0.2, TensorNet2's random-weight surface falls off a cliff between t
    # and t + h: measured E(t + h) - E(t) = -6.79 against E(t) - E(t - h) = +0.0147, whose quotient 0.735 does agree with -lambda = 0.729.)
    t = s0 - 0.2
    scan = model.capture_scan(z, pos[0], cvs, torch.full((3, 1), t, dtype=torch.float64), q=_q(arch, 3), steps_per_replay=10, fmax=fmax,
                              fixed=fixed, fire=dict(max_step=0.02))
    first = scan.run(max_steps)
    assert scan.check() == first and bool((scan.converged_at >= 0).all()), (first, scan.fmax[-1])
    targets = torch.tensor([[t - h], [t], [t + h]], dtype=torch.float64)
    scan.reset(pos=scan.pos[1].clone(), targets=targets)
    taken = scan.run(max_steps)
    assert scan.check() == taken
    prof = scan.profile()
    fperp = scan.projected_forces[:, ~fixed].pow(2).sum(-1).sqrt().amax(1)
    _, grad = O.cv_all(cvs, scan.pos[1].cpu().numpy().astype(np.float64), fixed.cpu().numpy())
    cv_bound = float(np.abs(grad).sum()) * 2 * float(np.spacing(np.float32(scan.pos.abs().max().item()))) + 1e-8
    E, lam = prof["energy"].double(), prof["multiplier"][:, 0].double()
    slope = float(E[2] - E[0]) / (2 * h)
    tangent = float((scan.pos[2] - scan.pos[0]).double().pow(2).sum().sqrt()) / (2 * h)
    terms = dict(h2_energy=abs(float(E[2] - 2 * E[1] + E[0])), h2_multiplier=abs(float(lam[2] - 2 * lam[1] + lam[0])) / 3,
                 fmax=fmax * math.sqrt(n_free) * tangent, resolution=2 * float(np.spacing(np.float32(E.abs().max().item()))) / (2 * h))
    return dict(arch=arch, n_free=n_free, h=h, fmax=fmax, steps_to_relax=first, steps=taken, converged=prof["converged"].tolist(), fperp_max=fperp.tolist(),
                cv_gap=float(_gap(cvs, prof["cv"].numpy(), targets.numpy()).max()), cv_bound=cv_bound,
                target_exact=bool(torch.equal(prof["target"], targets)), slope=slope, minus_lambda=-float(lam[1]),
                deviation=abs(slope + float(lam[1])), bound=sum(terms.values()), terms=terms, converged_at=scan.converged_at.tolist())


@pytest.mark.parametrize("arch", ARCHS)
def test_converged_scan_holds_its_targets_and_its_multiplier_is_the_slope(hip_lib, arch):
    """9. three neighbouring torsion targets t - h, t, t + h, branched by ``reset`` from the geometry relaxed at t and run to
    convergence (``_slope_run``): every point converged, max |F_perp| < fmax, |cv - target| within the fp32 rounding of the coordinates, and the central difference of the converged energies
    against -lambda at t.

    Along a relaxed path dE/dt = -F.dx/dt = -lambda - F_perp.dx/dt (g.dx/dt = 1), so the bound is the sum of
      the h^2 term of the central difference: |E+ - 2 E0 + E-|, that is h^2 |E2| with E2 the second derivative, which bounds the
        h^2 |E3| / 6 of the third for a profile of period >= 2 pi / 6, plus |lambda+ - 2 lambda0 + lambda-| / 3, the same h^2 |E3| / 3
        from the multipliers themselves,
      the fmax term: fmax sqrt(n_free) |x+ - x-| / (2 h), the residual force along the measured tangent,
      and the energies' fp32 resolution: 2 ulp(E) / (2 h).
    Measured, central difference against -lambda: TensorNet 0.02851 / 0.02644 (bound 1.9e-2), ET 0.06293 / 0.06208 (2.2e-2), TensorNet2
    1.33104 / 1.33042 (2.8e-2)."""
    r = _slope_run(arch)
    print(json.dumps(r))
    out = os.environ.get("TMDNET_RECORD_DIR", os.path.join(ROOT, "test_records"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"scan_slope_{arch}.json"), "w") as fh:
        json.dump(r, fh)
    assert all(r["converged"]), (r["steps"], r["fperp_max"])
    assert max(r["fperp_max"]) < r["fmax"]
    assert r["cv_gap"] <= r["cv_bound"] and r["target_exact"]
    assert r["deviation"] <= r["bound"], r


@pytest.mark.parametrize("arch", ARCHS)
def test_run_converges_two_points_with_a_torsion_and_a_distance(hip_lib, arch):
    """9b. the shape of test 8 - two points x 40 atoms, every atom free, a torsion and a distance held together - run to convergence with
    the defaults of capture_scan (fmax = 0.05, drive, tol): every point converged with its targets arrived, max |F_perp| < fmax, and
    |cv - target| within the fp32 rounding of the coordinates (twice the L1 norm of a CV's gradient times an ulp of the largest one)."""
    model = _model(arch)
    z, pos = _molecule()
    targets = _targets(pos)
    scan = model.capture_scan(z, pos, CVS, targets, q=_q(arch, 2), steps_per_replay=10)
    taken = scan.run(6000, check_every=5)
    assert scan.check() == taken
    prof = scan.profile()
    fperp = scan.projected_forces.pow(2).sum(-1).sqrt().amax(1)
    gap = _gap(CVS, prof["cv"].numpy(), targets.numpy())
    bound = np.array([np.abs(O.cv_all(CVS, x.astype(np.float64))[1]).sum((1, 2)) for x in scan.pos.cpu().numpy()])
    bound = bound * 2 * float(np.spacing(np.float32(scan.pos.abs().max().item()))) + 1e-8
    print(json.dumps(dict(arch=arch, steps=taken, converged_at=scan.converged_at.tolist(), fperp_max=fperp.tolist(), gap=gap.tolist(),
                          gap_bound=bound.tolist())))
    assert bool(prof["converged"].all()), (taken, fperp.tolist())
    assert torch.equal(prof["target"], targets) and (gap <= bound).all()
    assert (fperp < 0.05).all() and (scan.converged_at <= taken).all()


def test_overflow_freezes_the_state_at_the_last_valid_step(hip_lib):
    """10. a scan of the 192-atom periodic box with max_num_neighbors = 72, box and positions scaled by 0.85 between two replays: the
    first evaluation of the second replay overflows; status 1 latches and the positions the last move saved come back."""
    model = _model("tensornet", max_num_neighbors=72)
    z, pos, box = (t.cuda() for t in W.water_box(n_side=4))
    box0 = box.clone()
    cvs = [("distance", 0, 1)]
    targets = _targets(pos[None], cvs, ((0.05,),))
    scan = model.capture_scan(z, pos, cvs, targets, box=box, q=torch.zeros(1, device="cuda"), steps_per_replay=4, fmax=1e-4)
    scan()
    assert scan.check() == 4
    staged_box = scan.inputs[2]
    staged_box.mul_(0.85)
    scan.pos.mul_(0.85)
    watched = lambda: (scan.forces, scan.projected_forces, scan.epot, scan.fmax, scan.coef, scan.sums, scan.step_size, scan.alpha,
                       scan.converged_at, scan.cv, scan.target, scan.multipliers)
    keep = [t.clone() for t in watched()]
    host = (C.c_uint64 * 3)()
    scan()  # OPEN moves the scaled positions once more; the evaluation overflows; x and v of before that move come back
    x_keep = scan.pos.clone()
    for _ in range(2):
        with pytest.raises(RuntimeError, match="max_num_pairs"):
            scan.check()
        assert hip_lib.tmdnet_scan_status(None, C.c_void_p(scan._ws.data_ptr()), host) == 3 and (int(host[0]), int(host[1])) == (4, 1)
        for t, k in zip(watched(), keep):
            assert _bits(t, k)
        assert _bits(scan.pos, x_keep)
        scan()
    staged_box.copy_(box0)
    scan.reset(pos=pos)
    scan()
    assert scan.check() == 4 and not _bits(scan.pos, x_keep)


def test_check_names_the_cause_of_status_2(hip_lib):
    """11. a constraint step with one correction (cause 4), two identical CVs (3), a collinear torsion (2) and forces that are not
    finite (1) through the model: check() names each, replays change nothing, reset recovers and refuses tensors of another layout"""
    model = _model("tensornet")
    z, pos = _molecule(n_points=1)
    q = _q("tensornet", 1)
    scan = model.capture_scan(z, pos, CVS, _targets(pos), q=q, steps_per_replay=4, max_iter=1, tol=1e-12)
    scan()
    with pytest.raises(RuntimeError, match=r"step 0 the constraint step did not converge.*frozen"):
        scan.check()
    assert _bits(scan.pos, pos)
    keep = [t.clone() for t in (scan.pos, scan.vel, scan.forces, scan.projected_forces, scan.epot, scan.cv)]
    scan()
    for t, k in zip((scan.pos, scan.vel, scan.forces, scan.projected_forces, scan.epot, scan.cv), keep):
        assert _bits(t, k)
    twice = model.capture_scan(z, pos, [CVS[0], CVS[0]], _targets(pos, [CVS[0], CVS[0]], ((0.1, 0.1),)), q=q, steps_per_replay=2)
    twice()
    with pytest.raises(RuntimeError, match=r"step 0 the Gram matrix.*not positive definite.*frozen"):
        twice.check()
    line = pos.clone()
    line[0, [3, 8, 15]] = torch.tensor([[0.0, 0.0, 0.0], [1.1, 0.0, 0.0], [2.2, 0.0, 0.0]], device="cuda") + line[0, 3]
    good = model.capture_scan(z, pos, CVS, _targets(pos), q=q, steps_per_replay=2)
    good()
    assert good.check() == 2
    for wrong in (dict(pos=pos[:, :39]), dict(pos=pos.transpose(1, 2)), dict(targets=torch.zeros(2, 2)), dict(targets=torch.zeros(1, 3)),
                  dict(targets=torch.full((1, 2), float("nan")))):
        with pytest.raises(ValueError):
            good.reset(**wrong)
    good.reset(pos=line)
    good()
    with pytest.raises(RuntimeError, match=r"step 0 a collective variable or its gradient is not finite.*frozen"):
        good.check()
    good.reset(pos=pos[0], targets=_targets(pos, offsets=((-0.1, 0.05),)))
    assert good.check() == 0 and _bits(good.pos, pos)
    good()
    assert good.check() == 2 and not _bits(good.pos, pos)
    # cause 1: forces that are not finite at finite positions - TensorNet2 with a total charge that is not a number, written into the
    # charge vector the graph reads between two replays.  (A NaN written into scan.vel would do too, but the move that opens the next
    # replay carries it into the positions before the evaluation, and a neighbour search on positions that are not finite is no
    # part of this test.)
    tn2 = _model("tensornet2")
    charged = tn2.capture_scan(z, pos, CVS, _targets(pos), q=torch.zeros(1, device="cuda"), steps_per_replay=4, fmax=1e-5)
    charged()
    assert charged.check() == 4
    charge = charged.inputs[3]
    charge.fill_(float("nan"))
    charged()  # the move of step 4 is made, then the evaluation of step 5 has no finite force: nothing of it is accepted
    with pytest.raises(RuntimeError, match=r"step 4 the forces are not finite.*frozen"):
        charged.check()
    assert bool(torch.isfinite(charged.pos).all())
    watched = lambda: (charged.pos, charged.vel, charged.forces, charged.projected_forces, charged.epot, charged.fmax, charged.cv,
                       charged.target, charged.multipliers, charged.coef, charged.converged_at, charged.step_size)
    keep = [t.clone() for t in watched()]
    charged()
    with pytest.raises(RuntimeError, match=r"step 4 the forces are not finite.*frozen"):
        charged.check()
    for t, k in zip(watched(), keep):
        assert _bits(t, k)
    assert bool(torch.isfinite(charged.epot).all()) and bool(torch.isfinite(charged.forces).all())
    charge.zero_()
    charged.reset(pos=pos)
    assert charged.check() == 0 and _bits(charged.pos, pos)
    charged()
    assert charged.check() == 4 and not _bits(charged.pos, pos)


def test_refusals_leave_the_model_as_it_was(hip_lib):
    """12. everything capture_neb refuses, D outside 1..4, an index outside the molecule or repeated within a CV, a CV whose atoms are
    all fixed, tol <= 0, max_iter < 1, drive <= 0, shapes that disagree with z, a box per point - raised before anything is staged"""
    from torchmdnet_amd.models.model import create_model

    model = _model("tensornet")
    z, pos = _molecule(n_points=1)
    q = _q("tensornet", 1)
    targets = _targets(pos)
    replay = model.capture(z, pos.reshape(-1, 3), torch.zeros(40, dtype=torch.long, device="cuda"), q=q)
    e0, f0 = (t.clone() for t in replay(pos.reshape(-1, 3)))
    all_fixed = torch.zeros(40, device="cuda")
    all_fixed[[8, 30]] = 1
    for bad in (dict(steps_per_replay=0), dict(fire=dict(timestep=0.1)), dict(fmax=0.0), dict(tol=0.0), dict(tol=-1e-8), dict(max_iter=0),
                dict(drive=0.0), dict(drive=[0.1, -0.05]), dict(drive=[0.1, 0.1, 0.1]), dict(fixed=torch.zeros(3, device="cuda")),
                dict(fixed=all_fixed), dict(q=torch.zeros(2, device="cuda")), dict(box=torch.eye(3).repeat(1, 1, 1).cuda() * 50),
                dict(cvs=[]), dict(cvs=[("distance", 0, 1)] * 5), dict(cvs=[("distance", 0, 40), ("distance", 1, 2)]),
                dict(cvs=[("torsion", 1, 2, 3, 2), ("distance", 1, 2)]), dict(cvs=[("angle", 0, 1), ("distance", 1, 2)]),
                dict(cvs=[("stretch", 0, 1), ("distance", 1, 2)]), dict(targets=torch.zeros(1, 3)), dict(targets=torch.zeros(2)),
                dict(targets=torch.full((1, 2), float("inf")))):
        args = dict(dict(cvs=CVS, targets=targets, q=q), **bad)
        with pytest.raises(ValueError):
            model.capture_scan(z, pos, args.pop("cvs"), args.pop("targets"), **args)
    for bad_pos in (pos[:, :39], pos[0, 0], pos[..., :2], torch.cat([pos, pos])):
        with pytest.raises(ValueError):
            model.capture_scan(z, bad_pos, CVS, targets, q=q)
    with pytest.raises(NotImplementedError):
        model.capture_scan(z, pos.double(), CVS, targets, q=q)
    model.parameter_gradients = True
    try:
        with pytest.raises(NotImplementedError):
            model.capture_scan(z, pos, CVS, targets, q=q)
    finally:
        model.parameter_gradients = False
    torch.manual_seed(0)
    with pytest.raises(NotImplementedError):
        create_model(dict(W.TINY_ARGS, static_shapes=True, output_model="DipoleMoment")).to("cuda").capture_scan(z, pos, CVS, targets)
    with pytest.raises(RuntimeError, match="static_shapes"):
        create_model(dict(W.TINY_ARGS)).to("cuda").capture_scan(z, pos, CVS, targets)
    e1, f1 = replay(pos.reshape(-1, 3))  # the graph captured before the refusals is still valid, and gives the same bits
    assert _bits(e1, e0) and _bits(f1, f0)


class _NeverReplayed:
    """stands in for the graph once the engine has changed: the guard has to raise before it gets here"""

    def replay(self):
        raise AssertionError("a stale graph was replayed")


def test_a_stale_scan_raises_and_replays_nothing(hip_lib):
    """13. once the engine's workspaces are re-created, a replay, a reset and a run raise instead of touching freed memory"""
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(4)
    model = create_model(dict(W.TINY_ARGS, static_shapes=True)).to("cuda")  # (its own model: the test re-creates its workspaces)
    z, pos = _molecule(n_points=1)
    scan = model.capture_scan(z, pos, CVS, _targets(pos), q=_q("tensornet", 1), steps_per_replay=2, fmax=1e-6, warmup=1)
    scan()
    assert scan.check() == 2 == scan.steps_done
    zb, pb, bb = W.synthetic_batch(n_mol=40, n_atoms=60)
    model(zb.cuda() % 19 + 1, pb.cuda(), bb.cuda())  # a larger system: the workspaces grow
    graph, scan.graph = scan.graph, _NeverReplayed()  # (the real graph stays alive, unreplayed, until the test ends)
    stale = r"stale HIP graph.*capture_scan\(\)"
    with pytest.raises(RuntimeError, match=stale):
        scan()
    with pytest.raises(RuntimeError, match=stale):
        scan.reset()
    with pytest.raises(RuntimeError, match=stale):
        scan.run(2)
    assert scan.steps_done == 2
