"""-m gpu: the anisotropic cell barostat of the device-resident MD loop (csrc/tn_md_cell.hip: k_md_ktensor_reduce, k_md_cell_move,
k_md_cell_scale; TorchMD_Net.capture_md_cell).

1. the raw entry, no model: tmdnet_md_advance(CLOSE) then tmdnet_md_barostat_cell on synthetic forces and virials, against
   tests/md_cell_oracle.py (the matrices and the box) and a torch mirror that issues every product and sum as its own kernel
2. a NaN in the virial, the raw refusals
3. the two ensembles of tests/test_md_cell_host.py through the raw entries (the same bounds)
4. through the model: K steps per graph launch are bit-identical to capture(virial=True) + the torch mirror fed the device's matrices
5. the rotation is physical; 6. weak coupling relaxes a stretched cell; 7. seed, overflow, stale graphs, reset(box=), refusals

The helpers of tests/test_gpu_md_barostat.py (the raw-entry wrapper, the water box, the tiny models) are shared, not copied."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import md_baro_oracle as OB
from tests import md_cell_oracle as OC
from tests import test_gpu_md_barostat as B
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

OPEN, MIDDLE, CLOSE = 0, 1, 2
FS = B.FS
CODE = {"anisotropic": 0, "diagonal": 1, "semi-isotropic": 2}
_bits, _np = B._bits, B._np


def _apply(x, M):
    """x [n,3] times M [n,3,3], row vectors: ((x0 M0b) + (x1 M1b)) + (x2 M2b), every product and every sum a kernel of its own"""
    return torch.stack([torch.add(torch.add(torch.mul(x[:, 0], M[:, 0, b]), torch.mul(x[:, 1], M[:, 1, b])), torch.mul(x[:, 2], M[:, 2, b]))
                        for b in range(3)], dim=1)


def _apply_diag(x, M):
    return torch.mul(x, torch.diagonal(M, dim1=1, dim2=2))


def _move_state(coupling, x, v, f, Mx, Mv, Mf):
    """the mirror of k_md_cell_scale<false, .>: -> x, v, f after the move (Mx, Mv, Mf already gathered per atom)"""
    if coupling == "anisotropic":
        return _apply(x, Mx), _apply(v, Mv), _apply(f, Mf)
    return _apply_diag(x, Mx), _apply_diag(v, Mv), f


# ------------------------------------------------------------------------------------------------ 1. the raw entry
class _Raw(B._Raw):
    """tests/test_gpu_md_barostat.py's wrapper plus tmdnet_md_barostat_cell, graph_ws = NULL"""

    def __init__(self, lib, pos, vel, mass, batch, n_mol, dt, box, **kw):
        super().__init__(lib, pos, vel, mass, batch, n_mol, dt, box, **kw)
        nb = C.c_size_t(0)
        assert lib.tmdnet_md_barostat_cell_workspace_bytes(self.n, n_mol, C.byref(nb)) == 0
        self.cell_ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")

    def cell(self, open_next, forces, virial, baro, coupling, axis=2, rows=(None, None, None), keep=None, box_mode=2, expect=0, **over):
        p = self._p
        a = dict(box=self.box, virial=virial, mass=self.mass, code=CODE[coupling], **baro)
        a.update(over)
        rc = self.L.tmdnet_md_barostat_cell(None, self._s(), None, p(self.ws), p(self.cell_ws), self.n, self.n_mol, int(open_next),
                                            p(self.pos), p(self.vel), p(forces), p(self.hk), p(a["mass"]), self.dt, p(self.batch),
                                            p(a["box"]), box_mode, p(a["virial"]), a["pressure"], a["kT"], a["compressibility"], a["tau"],
                                            self.fs, a["seed"], a["code"], axis, p(keep), p(rows[0]), p(rows[1]), p(rows[2]))
        assert rc == expect, rc

    def matrices(self):
        """(Mx, Mv, Mf) [n_mol,3,3] each of the last move, from the scratch (256-aligned, [n_mol,27])"""
        off = (-self.cell_ws.data_ptr()) % 256
        M = self.cell_ws[off:off + 108 * self.n_mol].view(torch.float32).view(self.n_mol, 3, 3, 3)
        return M[:, 0].clone(), M[:, 1].clone(), M[:, 2].clone()

    def ktensor(self):
        """[n_mol,6] float64 of the last move, behind the matrices in the scratch"""
        off = (-self.cell_ws.data_ptr()) % 256 + ((108 * self.n_mol + 255) & ~255)
        return self.cell_ws[off:off + 48 * self.n_mol].view(torch.float64).view(self.n_mol, 6).clone()


def _small(n_mol=3, sizes=(5, 0, 7), seed=21):
    g = torch.Generator().manual_seed(seed)
    n = sum(sizes)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    pos = 10 * torch.randn(n, 3, generator=g)
    vel = 0.05 * torch.randn(n, 3, generator=g)
    f1 = 3 * torch.randn(n, 3, generator=g)
    mass = 1.0 + 39.0 * torch.rand(n, generator=g)
    box = B._triclinic(n_mol, g)
    vir = 300.0 * torch.randn(n_mol, 3, 3, generator=g)
    return [t.cuda() for t in (pos, vel, f1, mass, batch, box, vir)]


# V about 3e4 and W of a few hundred: P about 0.01; a = 0.5 moves the cell by some 1e-3 per step, the noise by 5e-4
RAW_BARO = dict(pressure=0.005, kT=0.025, compressibility=10.0, tau=10.0, seed=2 ** 40 + 11)


def _check_raw(hip_lib, state, n_mol, open_next, coupling, axis=2, batch_arg="given", box_mode=2, baro=RAW_BARO, noise_slack=False):
    """one move through the raw entry against the oracle (host test 1's terms: bit-equal, one ulp, or 1e-12 absolute) and the torch
    mirror.  noise_slack (hundreds of molecules, where some noise-driven entry is small by chance): an entry may also miss by what
    the oracle's own Xi is uncertain by - see _mirror."""
    pos, vel, f1, mass, batch, box, vir = state
    dt = 0.5
    md = _Raw(hip_lib, pos, vel, mass, None if batch_arg is None else batch, n_mol, dt, box, force_scale=FS)
    rows = [torch.full(s, float("nan"), device="cuda") for s in ((n_mol,), (n_mol, 9), (n_mol, 9))]
    keep = f1.clone()
    md.advance(CLOSE, f1)
    md.cell(open_next, f1, vir, baro, coupling, axis, rows, keep, box_mode)
    assert md.status() == (0, 1, 0)
    hk, dt_t = md.hk[:, None], torch.tensor(dt, device="cuda")
    v1 = torch.add(vel, torch.mul(hk, f1))
    Mx, Mv, Mf = md.matrices()
    assert _bits(rows[2].view(n_mol, 3, 3), Mx)
    # the oracle on the device's closed velocities
    a = baro["compressibility"] * dt / baro["tau"]
    Kt = OC.ktensor(_np(batch), _np(mass), _np(v1), n_mol)
    kt = _np(md.ktensor())
    assert np.abs(kt - OC.six(Kt)).max() <= 1e-6 * np.abs(Kt).max()
    ref = OC.moves(_np(box).reshape(-1, 3, 3), _np(vir), Kt, FS, baro["pressure"], baro["kT"], a, coupling, axis, baro["seed"], 0)
    Qt = ref["Q"].transpose(0, 2, 1)
    for name, got, want in (("Mx", Mx, ref["mu"] @ Qt), ("Mv", Mv, ref["nu"] @ Qt), ("Mf", Mf, Qt), ("box", md.box.reshape(-1, 3, 3), ref["L"])):
        ok = OC.close_to_oracle(_np(got), want)
        print(coupling, name, "max ulp distance", OC.ulp_distance(_np(got), want.astype(np.float32)).max(), "max abs", np.abs(_np(got) - want).max())
        if noise_slack:
            tol = 4e-6 * np.sqrt(2.0 * baro["kT"] * a / (3.0 * ref["V"]))[:, None, None] * (float(box.abs().max()) if name == "box" else 1.0)
            print("   entries beyond one ulp:", int((~ok).sum()), "largest miss over the noise slack",
                  float((np.abs(_np(got) - want) / tol)[~ok].max()) if (~ok).any() else 0.0)
            ok |= np.abs(_np(got) - want) <= tol
        assert ok.all(), (name, _np(got)[~ok], want[~ok])
    assert OB.ulp_distance(_np(rows[0]), ref["V"].astype(np.float32)).max() <= 1
    assert OC.close_to_oracle(_np(rows[1]).reshape(-1, 3, 3), ref["P"]).all()
    assert np.abs(_np(Mx) - np.eye(3)).reshape(n_mol, -1).max(1).min() > 1e-5  # every molecule really moved
    if coupling == "anisotropic":
        assert (_np(md.box).reshape(-1, 3, 3)[:, [0, 0, 1], [1, 2, 2]] == 0).all()  # lower triangular, exactly
        assert np.abs(_np(Mf) - np.eye(3)).max() > 1e-3  # the full triclinic boxes are really rotated
    else:
        off = ~np.eye(3, dtype=bool)
        assert (_np(Mf) == np.eye(3, dtype=np.float32)).all() and (_np(Mx)[:, off] == 0).all() and (_np(Mv)[:, off] == 0).all()
    # given the matrices: products and sums one at a time
    x_s, v_s, f_s = _move_state(coupling, pos, v1, f1, Mx[batch], Mv[batch], Mf[batch])
    assert _bits(keep, f_s)
    if open_next:  # then B, A of the next step on the scaled state, with the rotated force
        v_s = torch.add(v_s, torch.mul(hk, f_s))
        x_s = torch.add(x_s, torch.mul(dt_t, v_s))
    assert _bits(md.pos, x_s) and _bits(md.vel, v_s)
    return md


@pytest.mark.parametrize("coupling", OC.COUPLINGS)
@pytest.mark.parametrize("open_next", [0, 1])
def test_raw_move_equals_oracle_and_torch_mirror(hip_lib, open_next, coupling):
    _check_raw(hip_lib, _small(), 3, open_next, coupling, axis=open_next)  # (semi-isotropic: axis 0 and axis 1)


def test_raw_weak_coupling_and_one_shared_box(hip_lib):
    state = _small()
    _check_raw(hip_lib, state, 3, 1, "anisotropic", baro=dict(RAW_BARO, kT=0.0))
    # box_mode 1: one [3,3] box, one molecule, no batch vector
    pos, vel, f1, mass, batch, box, vir = state
    one = [pos, vel, f1, mass, torch.zeros_like(batch), box[0].clone(), vir[:1]]
    md = _check_raw(hip_lib, one, 1, 0, "anisotropic", batch_arg=None, box_mode=1)
    assert md.box.shape == (3, 3)
    _check_raw(hip_lib, one, 1, 1, "semi-isotropic", axis=2, batch_arg=None, box_mode=1)


def test_raw_more_molecules_than_threads(hip_lib):
    """300 molecules for the one block of 256 threads: a thread owns two molecules and pass 2 evaluates their moves again"""
    state = _small(n_mol=300, sizes=(2, 1, 3) * 100)
    _check_raw(hip_lib, state, 300, 1, "anisotropic", baro=dict(RAW_BARO, kT=0.0))  # no noise: the strict terms
    _check_raw(hip_lib, state, 300, 1, "anisotropic", noise_slack=True)
    _check_raw(hip_lib, state, 300, 0, "semi-isotropic", axis=1)


def test_raw_two_stage_reduction_and_unsorted_batch(hip_lib):
    """a molecule of 1 100 atoms: two slices and the finishing launch; two launches give the same bits.  An unsorted batch: the
    filtered path."""
    g = torch.Generator().manual_seed(5)
    n = 1100
    pos, vel, f1 = 10 * torch.randn(n, 3, generator=g), 0.005 * torch.randn(n, 3, generator=g), 0.3 * torch.randn(n, 3, generator=g)
    mass = 1.0 + 39.0 * torch.rand(n, generator=g)
    mass[17] = float("inf")  # a frozen atom is no part of the kinetic tensor
    big = [t.cuda() for t in (pos, vel, f1, mass, torch.zeros(n, dtype=torch.long), B._triclinic(1, g), 300.0 * torch.randn(1, 3, 3, generator=g))]
    nb1, nb2 = C.c_size_t(0), C.c_size_t(0)
    hip_lib.tmdnet_md_barostat_cell_workspace_bytes(1024, 1, C.byref(nb1))
    hip_lib.tmdnet_md_barostat_cell_workspace_bytes(n, 1, C.byref(nb2))
    assert nb2.value > nb1.value  # the slice sums
    a = _check_raw(hip_lib, big, 1, 1, "anisotropic")
    b = _check_raw(hip_lib, big, 1, 1, "anisotropic")
    assert torch.equal(a.ktensor().view(torch.int64), b.ktensor().view(torch.int64)) and _bits(a.pos, b.pos) and _bits(a.box, b.box)
    ref = OC.six(OC.ktensor(np.zeros(n, np.int64), _np(big[3]), _np(torch.add(big[1], torch.mul(a.hk[:, None], big[2]))), 1))
    print("kinetic tensor: largest relative error per entry", (np.abs(_np(a.ktensor()) - ref) / np.abs(ref)).max())
    assert (np.abs(_np(a.ktensor()) - ref) <= 1e-6 * np.abs(ref)).all()
    # three molecules, atoms shuffled
    pos, vel, f1, mass, batch, box, vir = _small(sizes=(40, 23, 61))
    perm = torch.randperm(batch.numel(), generator=g).cuda()
    assert not bool((batch[perm][1:] >= batch[perm][:-1]).all())
    _check_raw(hip_lib, [pos[perm], vel[perm], f1[perm], mass[perm], batch[perm], box, vir], 3, 1, "anisotropic")


# ------------------------------------------------------------------------------------------------ 2. unusable moves, refusals
@pytest.mark.parametrize("coupling", ["anisotropic", "diagonal"])
def test_raw_nan_in_the_virial_latches_status_2(hip_lib, coupling):
    pos, vel, f1, mass, batch, box, vir = _small()
    md = _Raw(hip_lib, pos, vel, mass, batch, 3, 0.5, box, force_scale=FS)
    rows = [torch.full(s, 7.0, device="cuda") for s in ((3,), (3, 9), (3, 9))]
    keep = f1.clone()
    md.advance(CLOSE, f1)
    v1 = md.vel.clone()
    bad = vir.clone()
    bad[1, 2, 2] = float("nan")  # the molecule without atoms
    md.cell(1, f1, bad, RAW_BARO, coupling, 2, rows, keep)
    assert md.status() == (5, 1, 2)  # TMDNET_ERR_STATE, one step completed, status 2
    assert _bits(md.box, box) and _bits(md.pos, pos) and _bits(md.vel, v1) and _bits(keep, f1)
    assert all((r == 7.0).all() for r in rows)
    md.cell(0, f1, vir, RAW_BARO, coupling, 2, rows, keep)  # frozen until a reset
    md.advance(OPEN, f1)
    assert _bits(md.box, box) and _bits(md.pos, pos) and _bits(md.vel, v1) and _bits(keep, f1) and md.status() == (5, 1, 2)
    for broken in ("flat", "left-handed"):
        b2 = box.clone()
        if broken == "flat":
            b2[2, 1] = b2[2, 0]  # a box without volume
        else:
            b2[0, 0] = -b2[0, 0]  # det (h mu) < 0
        md2 = _Raw(hip_lib, pos, vel, mass, batch, 3, 0.5, b2, force_scale=FS)
        md2.advance(CLOSE, f1)
        md2.cell(0, f1, vir, RAW_BARO, coupling)
        assert md2.status() == (5, 1, 2) and _bits(md2.box, b2) and _bits(md2.pos, pos), broken


def test_raw_refusals(hip_lib):
    pos, vel, f1, mass, batch, box, vir = _small()
    md = _Raw(hip_lib, pos, vel, mass, batch, 3, 0.5, box, force_scale=FS)
    md.advance(CLOSE, f1)
    v1 = md.vel.clone()
    cell = lambda **kw: md.cell(kw.pop("open_next", 0), kw.pop("forces", f1), kw.pop("vir", vir), RAW_BARO, "anisotropic", kw.pop("axis", 2),
                                expect=1, **kw)
    cell(box_mode=0)
    cell(box_mode=1)  # one shared box for three molecules
    cell(tau=0.0)
    cell(compressibility=0.0)
    cell(kT=-1.0)
    cell(vir=None)
    cell(box=None)
    cell(mass=None)
    cell(code=3)
    cell(code=-1)
    cell(axis=3)
    cell(axis=-1)
    cell(open_next=1, forces=None)
    assert _bits(md.box, box) and _bits(md.pos, pos) and _bits(md.vel, v1) and md.status() == (0, 1, 0)


# ------------------------------------------------------------------------------------------------ 3. the ensembles
def _device_ensemble(hip_lib, state, e, steps, coupling, axis, baro, kappa=0.0, eps0=0.0):
    """an eager loop on the raw entries, F = 0: -> volumes [steps,R], lengths [steps,R,3] before each move"""
    box, x, v, hk, mass, sigma, c1, c2 = state
    R, n = e["R"], e["n"]
    t = lambda a: torch.from_numpy(a).cuda()
    batch = torch.repeat_interleave(torch.arange(R), n).cuda()
    md = _Raw(hip_lib, t(x), t(v), t(mass), batch, R, e["dt"], t(box), force_scale=1.0, sigma=t(sigma), c1=c1, c2=c2, seed=2024)
    assert _bits(md.hk, t(hk))
    zero, vir = torch.zeros(R * n, 3, device="cuda"), torch.zeros(R, 3, 3, device="cuda")
    vol = torch.full((steps, R), float("nan"), device="cuda")
    length = torch.full((steps, R, 3), float("nan"), device="cuda")
    lens, wdiag = md.box.diagonal(dim1=1, dim2=2), vir.diagonal(dim1=1, dim2=2)
    md.advance(OPEN, zero)
    for s in range(steps):
        md.advance(CLOSE, zero)
        length[s].copy_(lens)
        if kappa > 0.0:  # the synthetic virial W_aa = -kappa (ln L_a - eps0)
            wdiag.copy_(torch.mul(torch.log(lens.double()) - eps0, -kappa))
        md.cell(1, zero, vir, baro, coupling, axis, (vol[s], None, None))
    assert md.status() == (0, steps, 0)
    return _np(vol), _np(length)


@pytest.mark.parametrize("coupling", ["anisotropic", "diagonal"])
def test_ideal_gas_samples_the_npt_ensemble_on_the_device(hip_lib, coupling):
    """The case and the two bounds of tests/test_md_cell_host.py::test_ideal_gas_samples_the_npt_ensemble, per-replica boxes."""
    e = OB.ENSEMBLE
    baro = dict(pressure=e["P0"], kT=e["kT"], compressibility=1.0 / e["P0"], tau=e["tau"], seed=77)
    vol, _ = _device_ensemble(hip_lib, OB.ensemble_state(), e, e["steps"], coupling, 2, baro)
    assert np.isfinite(vol).all()
    m, s = OB.ensemble_bounds(vol)
    print(coupling, "device: mean / ((N+1) kT/P0) =", m, " relative sd * sqrt(N+1) =", s)
    assert abs(m - 1.0) < 0.01 and abs(s - 1.0) < 0.05


@pytest.mark.parametrize("coupling", ["diagonal", "semi-isotropic"])
def test_per_axis_ensemble_on_the_device(hip_lib, coupling):
    """The case and the bounds of tests/test_md_cell_host.py::test_per_axis_ensemble_is_gaussian_in_the_log_lengths."""
    e = OC.PER_AXIS
    baro = dict(pressure=e["P0"], kT=e["kT"], compressibility=e["compressibility"], tau=e["tau"], seed=77)
    _, length = _device_ensemble(hip_lib, OC.per_axis_state(), e, e["steps"], coupling, 2, baro, e["kappa"], e["eps0"])
    assert np.isfinite(length).all()
    r = OC.per_axis_ratios(length, coupling, 2)
    print(coupling, "device: (mean, variance) / theory =", r)
    for m, s in r:
        assert abs(m - 1.0) < 0.05 and abs(s - 1.0) < 0.05


# ------------------------------------------------------------------------------------------------ 4. through the model
_SHEAR = torch.tensor([[1.0, 0.0, 0.0], [0.08, 1.0, 0.0], [-0.05, 0.06, 1.0]])


def _setup(arch, triclinic=False, **over):
    model, (z, pos, batch, box, q), vel, mass = B._setup(arch, **over)
    if triclinic:  # a homogeneous shear of the whole system: box -> box S stays lower triangular
        S = _SHEAR.cuda()
        pos, box = (pos @ S).contiguous(), (box @ S).contiguous()
    return model, (z, pos, batch, box, q), vel, mass


def _pressure(model, inputs, vel, mass):
    """-> P [3,3] (fp64, host), V, dt: the system's own pressure tensor at the start (force_scale 1) and the dt rule of the MD tests"""
    z, pos, batch, box, q = inputs
    _, f, w = model.energy_forces_virial(z, pos, batch, box, q)
    Kt = torch.einsum("n,na,nb->ab", 0.5 * mass.double(), vel.double(), vel.double())
    vol = float(torch.linalg.det(box.double()).abs())
    dt = min(0.05, 0.02 * (12.0 / max(float(f.abs().max()), 1e-6)) ** 0.5)
    return ((2.0 * Kt + w[0].double()) / vol).cpu(), vol, dt


def _baro_for(P, vol, dt, coupling, axis=2, kT=None, seed=99):
    b = B._baro_for(P.diagonal().mean().reshape(1), torch.tensor([vol]), dt, +1, kT=kT, seed=seed)
    return dict(b, coupling=coupling, axis=axis)


def _run(model, inputs, vel, mass, dt, K, replays, baro, collect=False):
    """-> md, logs: epot, volume [K replays, B], scale, pressure_tensor [K replays, B,3,3]; with K = 1 also every step's Mv, Mf and box"""
    z, pos, batch, box, q = inputs
    md = model.capture_md_cell(z, pos, vel, mass, dt, batch=batch, box=box.clone(), q=q, steps_per_replay=K, barostat=baro)
    names = ("epot", "ekin", "volume", "pressure_tensor", "scale")
    logs = {k: [] for k in names + ("Mv", "Mf", "box")}
    for _ in range(replays):
        md()
        for k in names:
            logs[k].append(getattr(md, k).clone())
        if collect:
            assert K == 1
            _, Mv, Mf = md.matrices()
            logs["Mv"].append(Mv[None])
            logs["Mf"].append(Mf[None])
            logs["box"].append(md.box.clone()[None])
    assert md.check() == K * replays == md.steps_done
    return md, {k: torch.cat(v) for k, v in logs.items() if v}


def _mirror(model, inputs, vel0, mass, dt, steps, baro, logs):
    """capture(virial=True) + the scheme in torch, every product and every sum its own rounded kernel; the matrices and the box of
    every step are the device's (logs), checked against the fp64 oracle fed the mirror's own box, virial and velocities.  The
    oracle's Xi is its own libm's: the noise tests bound the difference to the loop's at 1e-6 per normal, D is linear in Xi with
    the coefficient sqrt(2 kT a / 3 V), and no entry of exp(D) Q^T depends on an entry of D with a slope above 2 - so a matrix
    entry may miss one ulp by at most 4e-6 of that coefficient, a box entry by that times the largest box entry."""
    z, pos0, batch, box0, q = inputs
    box = box0.clone()
    replay = model.capture(z, pos0, batch, box, q=q, virial=True)
    hk = (0.5 * dt / mass.double()).float()[:, None]
    dt_t = torch.tensor(dt, dtype=torch.float32, device="cuda")
    a = baro["compressibility"] * float(np.float32(dt)) / baro["tau"]
    pos, vel = pos0.clone(), vel0.clone()
    f = replay(pos)[1].clone()
    epot, vols, worst = [], [], 0.0
    for s in range(steps):
        vel = torch.add(vel, torch.mul(hk, f))
        pos = torch.add(pos, torch.mul(dt_t, vel))
        e, f, w = (t.clone() for t in replay(pos))
        vel = torch.add(vel, torch.mul(hk, f))
        epot.append(e.view(-1))
        Mx, Mv, Mf, newbox = logs["scale"][s], logs["Mv"][s], logs["Mf"][s], logs["box"][s]
        ref = OC.moves(_np(box).reshape(-1, 3, 3), _np(w), OC.ktensor(_np(batch), _np(mass), _np(vel), 1), 1.0, baro["pressure"], baro["kT"], a,
                       baro["coupling"], baro["axis"], baro["seed"], s)
        slack = 4e-6 * math.sqrt(2.0 * baro["kT"] * a / (3.0 * ref["V"][0]))
        Qt = ref["Q"].transpose(0, 2, 1)
        for got, want, tol in ((Mx, ref["mu"] @ Qt, slack), (Mv, ref["nu"] @ Qt, slack), (Mf, Qt, slack),
                               (newbox.reshape(-1, 3, 3), ref["L"], slack * float(box.abs().max()))):
            miss = np.abs(_np(got).astype(np.float64) - want)[~OC.close_to_oracle(_np(got), want)]
            worst = max(worst, float(miss.max() / tol) if miss.size else 0.0)
        vols.append(torch.from_numpy(ref["V"].astype(np.float32)))
        box.copy_(newbox.view_as(box))
        pos, vel, f = _move_state(baro["coupling"], pos, vel, f, Mx[batch], Mv[batch], Mf[batch])
    print("mirror: largest miss of a device matrix entry beyond one ulp, in units of the noise slack:", worst)
    assert worst <= 1.0
    return pos, vel, box, f, torch.stack(epot), torch.stack(vols).cuda()


CASES = {
    "tensornet-anisotropic": dict(arch="tensornet", coupling="anisotropic"),
    "tensornet-semi-isotropic": dict(arch="tensornet", coupling="semi-isotropic", axis=2),
    "equivariant-transformer-anisotropic": dict(arch="equivariant-transformer", coupling="anisotropic"),
    "equivariant-transformer-semi-isotropic": dict(arch="equivariant-transformer", coupling="semi-isotropic", axis=0),
    "tensornet-anisotropic-triclinic": dict(arch="tensornet", coupling="anisotropic", triclinic=True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_cell_npt_is_bit_identical_to_capture_plus_torch_mirror(hip_lib, case):
    c = CASES[case]
    model, inputs, vel, mass = _setup(c["arch"], c.get("triclinic", False))
    P, vol, dt = _pressure(model, inputs, vel, mass)
    baro = _baro_for(P, vol, dt, c["coupling"], c.get("axis", 2))
    print(case, "P", P.tolist(), "V", vol, "dt", dt, baro)
    md, logs = _run(model, inputs, vel, mass, dt, 1, 16, baro, collect=True)
    p_ref, v_ref, b_ref, f_ref, e_ref, vol_ref = _mirror(model, inputs, vel, mass, dt, 16, baro, logs)
    v_end = float(torch.linalg.det(md.box.double()).abs())
    print("V_16 / V_0 - 1 =", v_end / vol - 1.0, "box", md.box.tolist())
    assert abs(v_end / vol - 1.0) > 1e-4  # the volume visibly moved
    assert _bits(md.pos, p_ref) and _bits(md.vel, v_ref) and _bits(md.box, b_ref) and _bits(md.forces, f_ref)
    assert _bits(logs["epot"], e_ref) and _bits(logs["volume"], vol_ref)
    box = md.box.reshape(3, 3)
    assert box[0, 1] == 0 and box[0, 2] == 0 and box[1, 2] == 0  # the upper triangle is exactly zero
    if c["coupling"] == "anisotropic":  # the shape moved: the box is no multiple of the first one
        r = box.diagonal() / inputs[3].reshape(3, 3).diagonal()
        assert float(r.max() - r.min()) > 1e-5 and float(box[1, 0].abs() + box[2, 0].abs() + box[2, 1].abs()) > 1e-4
    else:
        s = logs["scale"][:, 0]
        others = [i for i in range(3) if i != c["axis"]]
        assert _bits(s[:, others[0], others[0]], s[:, others[1], others[1]]) and not _bits(s[:, others[0], others[0]], s[:, c["axis"], c["axis"]])
    # the same bits with 8 steps per launch
    md2, logs2 = _run(model, inputs, vel, mass, dt, 8, 2, baro)
    assert _bits(md2.pos, md.pos) and _bits(md2.vel, md.vel) and _bits(md2.box, md.box) and _bits(md2.forces, md.forces)
    for k in ("epot", "ekin", "volume", "pressure_tensor", "scale"):
        assert _bits(logs2[k], logs[k]), k
    # reset with the first box: the same trajectory again
    md2.reset(pos=inputs[1], vel=vel, box=inputs[3])
    md2(2)
    assert _bits(md2.pos, md.pos) and _bits(md2.box, md.box) and md2.check() == 16


# ------------------------------------------------------------------------------------------------ 5. the rotation is physical
def test_rotated_state_has_the_energy_the_loop_sees_next(hip_lib):
    """After one anisotropic step from a sheared box the state (pos, vel, forces, box) lives in the rotated frame.  Open the next step
    on it in torch, evaluate that geometry with a fresh energy_forces_virial call in the new box, and compare with the epot the loop
    logs for its next step: 1e-4 relative, the fp32 bound of the parity tests.  The fractional coordinates do not know about the
    rotation: x box^-1 before the move equals x' box'^-1 after it."""
    model, inputs, vel, mass = _setup("tensornet", triclinic=True)
    z, pos, batch, box, q = inputs
    P, vol, dt = _pressure(model, inputs, vel, mass)
    baro = _baro_for(P, vol, dt, "anisotropic")
    md = model.capture_md_cell(z, pos, vel, mass, dt, batch=batch, box=box.clone(), q=q, steps_per_replay=1, barostat=baro)
    f0 = md.forces.clone()
    md()
    Mx, _, Mf = md.matrices()
    assert float((Mf[0] - torch.eye(3, device="cuda")).abs().max()) > 1e-5  # a real rotation
    hk, dt_t = (0.5 * dt / mass.double()).float()[:, None], torch.tensor(dt, dtype=torch.float32, device="cuda")
    x1 = torch.add(pos, torch.mul(dt_t, torch.add(vel, torch.mul(hk, f0))))  # where step 1 was evaluated
    frac0 = x1.double() @ torch.linalg.inv(box.double())
    frac1 = md.pos.double() @ torch.linalg.inv(md.box.double())
    print("fractional coordinates: largest change through the move", float((frac1 - frac0).abs().max()))
    assert float((frac1 - frac0).abs().max()) < 1e-5
    v = torch.add(md.vel, torch.mul(hk, md.forces))
    x2 = torch.add(md.pos, torch.mul(dt_t, v))
    e_fresh = model.energy_forces_virial(z, x2, batch, md.box.clone(), q)[0].view(-1)
    md()
    rel = float((md.epot[0] - e_fresh).abs() / e_fresh.abs())
    print("epot of the loop's next step", md.epot[0].tolist(), "fresh evaluation", e_fresh.tolist(), "relative difference", rel)
    assert rel < 1e-4


# ------------------------------------------------------------------------------------------------ 6. weak coupling
@pytest.mark.parametrize("coupling", OC.COUPLINGS)
def test_weak_coupling_relaxes_a_stretched_cell(hip_lib, coupling):
    """kT = 0, 40 steps from a box stretched 3 % along z at fixed volume: L_z / L_x moves towards its unstretched value (the sign).
    The medium has to be one that is known to push back: atoms at rest in the elastic cell of the per-axis ensemble,
    W_aa = -kappa (ln L_a - eps0), through the raw entries.  (The tiny models carry random weights and are no such medium: the next
    test shows that the TensorNet water box answers this stretch with P_zz ABOVE P_xx, and what the loop does then.)"""
    e = OC.PER_AXIS
    side = math.exp(e["eps0"])
    box = torch.diag(torch.tensor([side * 1.03 ** -0.5, side * 1.03 ** -0.5, side * 1.03]))[None].cuda()
    n = 16
    pos = (torch.rand(n, 3, generator=torch.Generator().manual_seed(3)).cuda() * box[0].diagonal()).contiguous()
    zero = torch.zeros(n, 3, device="cuda")
    md = _Raw(hip_lib, pos, zero, torch.ones(n, device="cuda"), torch.zeros(n, dtype=torch.long, device="cuda"), 1, e["dt"], box, force_scale=1.0)
    baro = dict(pressure=0.0, kT=0.0, compressibility=e["compressibility"], tau=e["tau"], seed=0)
    vir = torch.zeros(1, 3, 3, device="cuda")
    lens, wdiag = md.box.diagonal(dim1=1, dim2=2), vir.diagonal(dim1=1, dim2=2)
    ratio = [float(md.box[0, 2, 2] / md.box[0, 0, 0])]
    md.advance(OPEN, zero)
    for _ in range(40):
        md.advance(CLOSE, zero)
        wdiag.copy_(torch.mul(torch.log(lens.double()) - e["eps0"], -e["kappa"]))
        md.cell(1, zero, vir, baro, coupling, 2)
        ratio.append(float(md.box[0, 2, 2] / md.box[0, 0, 0]))
    assert md.status() == (0, 40, 0)
    print(coupling, "L_z / L_x:", ratio[0], "->", ratio[-1], "unstretched 1.0")
    assert all(b < a for a, b in zip(ratio[:-1], ratio[1:])) and 1.0 < ratio[-1] < ratio[0] - 1e-3
    frac = md.pos / md.box[0].diagonal()  # the atoms went with the cell (they are back at rest: the open half moved nothing)
    assert float((frac - pos / box[0].diagonal()).abs().max()) < 1e-5


def test_weak_coupling_follows_the_models_own_deviatoric_pressure(hip_lib):
    """The same stretch on the TensorNet water box, kT = 0 and P0 the box's own mean pressure: over 40 steps L_z / L_x moves the way
    the model's own P_zz - P_xx at the start points (P_zz above P_xx: z grows).  With these random weights that is AWAY from the
    unstretched shape - measured P = diag(-0.02480, -0.02440, -0.02300), L_z / L_x 1.045 -> 1.152 at three times the drive used here -:
    the model is no elastically stable medium, which is a property of its weights and not of the barostat."""
    model, (z, pos, batch, box, q), vel, mass = _setup("tensornet")
    s = torch.tensor([1.03 ** -0.5, 1.03 ** -0.5, 1.03], device="cuda")
    inputs = (z, (pos * s).contiguous(), batch, (box * s).contiguous(), q)
    P, vol, dt = _pressure(model, inputs, vel, mass)
    spread = max(float((P.diagonal() - P.diagonal().mean()).abs().max()), 1e-6)
    # P0 the system's own mean pressure: the volume stays; a / 3 times the largest deviatoric pressure = 3e-4 per step
    baro = dict(pressure=float(P.diagonal().mean()), tau=10.0 * dt, compressibility=10.0 * 9e-4 / spread, kT=0.0, coupling="anisotropic")
    md, logs = _run(model, inputs, vel, mass, dt, 40, 1, baro)
    r0 = float(inputs[3][2, 2] / inputs[3][0, 0])
    r1 = float(md.box[2, 2] / md.box[0, 0])
    print("P at the start", P.tolist(), "L_z / L_x:", r0, "->", r1, "unstretched", float(box[2, 2] / box[0, 0]))
    assert abs(float(P[2, 2] - P[0, 0])) > 1e-5 and abs(r1 - r0) > 1e-4
    assert (r1 > r0) == bool(P[2, 2] > P[0, 0])


# ------------------------------------------------------------------------------------------------ 7. other behaviour
def test_seed_matters_and_the_callers_box_is_the_one_that_moves(hip_lib):
    model, inputs, vel, mass = _setup("tensornet")
    z, pos, batch, box, q = inputs
    P, vol, dt = _pressure(model, inputs, vel, mass)
    baro = _baro_for(P, vol, dt, "anisotropic")
    a, la = _run(model, inputs, vel, mass, dt, 8, 1, baro)
    b, lb = _run(model, inputs, vel, mass, dt, 8, 1, dict(baro, seed=100))
    assert not _bits(a.pos, b.pos) and not _bits(a.box, b.box) and not _bits(la["scale"], lb["scale"])
    mine = box.clone()
    md = model.capture_md_cell(z, pos, vel, mass, dt, batch=batch, box=mine, q=q, steps_per_replay=8, barostat=baro)
    assert md.box is mine
    md()
    assert _bits(mine, a.box) and not _bits(mine, box)
    assert md.volume.shape == (8, 1) and md.pressure_tensor.shape == (8, 1, 3, 3) and md.scale.shape == (8, 1, 3, 3)
    # the isotropic loop is what it was: the same call with capture_md still gives a scalar scale log
    iso = model.capture_md(z, pos, vel, mass, dt, batch=batch, box=box.clone(), q=q, steps_per_replay=2,
                           barostat={k: baro[k] for k in ("pressure", "tau", "compressibility", "kT", "seed")})
    iso()
    assert iso.check() == 2 and iso.scale.shape == (2, 1)


def test_overflow_freezes_box_and_state(hip_lib):
    """The case of tests/test_gpu_md_barostat.py::test_overflow_under_npt_freezes_box_and_state with the cell barostat."""
    model, inputs, vel, mass = _setup("tensornet", max_num_neighbors=72)
    z, pos, batch, box0, q = inputs
    P, vol, _ = _pressure(model, inputs, vel, mass)
    baro = _baro_for(P, vol, 0.01, "anisotropic")
    md = model.capture_md_cell(z, pos, vel, mass, 0.01, batch=batch, box=box0.clone(), q=q, steps_per_replay=4, barostat=baro)
    md()
    assert md.check() == 4 and not _bits(md.box, box0)
    md.box.mul_(0.85)
    md.pos.mul_(0.85)
    state = (md.box, md.pos, md.vel, md.forces, md.epot, md.ekin, md.volume, md.pressure_tensor, md.scale)
    keep = [t.clone() for t in state]
    host = (C.c_uint64 * 2)()
    for _ in range(2):  # the overflowing replay and one more
        md()
        with pytest.raises(RuntimeError, match="max_num_pairs"):
            md.check()
        assert hip_lib.tmdnet_md_status(None, C.c_void_p(md._ws.data_ptr()), host) == 3 and (int(host[0]), int(host[1])) == (4, 1)
        for t, k in zip(state, keep):
            assert _bits(t, k)
    md.reset(pos, vel, box=box0)
    assert _bits(md.box, box0)
    md()
    assert md.check() == 4 and not _bits(md.box, box0) and not _bits(md.pos, keep[1])


def test_a_nan_mass_is_reported_as_the_cell_barostat(hip_lib):
    model, inputs, vel, mass = _setup("tensornet")
    z, pos, batch, box, q = inputs
    P, vol, dt = _pressure(model, inputs, vel, mass)
    md = model.capture_md_cell(z, pos, vel, mass, dt, batch=batch, box=box.clone(), q=q, steps_per_replay=2,
                               barostat=_baro_for(P, vol, dt, "diagonal"))
    md()
    assert md.check() == 2
    md.masses[5] = float("nan")  # the buffer the graph reads: reaches the kinetic tensor of the next step, and with it the pressure
    box_before = md.box.clone()
    md()
    with pytest.raises(RuntimeError, match="cell barostat"):
        md.check()
    assert _bits(md.box, box_before) and torch.isfinite(md.pos).all()
    md.masses[5] = mass[5]
    md.reset(pos, vel, box=box)
    md()
    assert md.check() == 2


class _NeverReplayed:
    """stands in for the graph once the engine has changed: the guard has to raise before it gets here"""

    def replay(self):
        raise AssertionError("a stale graph was replayed")


def test_a_stale_loop_raises_and_replays_nothing(hip_lib):
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(4)
    model = create_model(dict(W.TINY_ARGS, static_shapes=True)).to("cuda")  # (its own model: the test re-creates its workspaces)
    _, (z, pos, batch, box, q), vel, mass = _setup("tensornet")
    baro = dict(pressure=0.0, tau=1.0, compressibility=1e-3, kT=0.0)
    md = model.capture_md_cell(z, pos, vel, mass, 0.01, batch=batch, box=box.clone(), q=q, steps_per_replay=2, barostat=baro, warmup=1)
    md()
    assert md.check() == 2 == md.steps_done
    zb, pb, bb = W.synthetic_batch(n_mol=40, n_atoms=60)
    model(zb.cuda() % 19 + 1, pb.cuda(), bb.cuda())  # a larger system: the workspaces grow
    graph, md.graph = md.graph, _NeverReplayed()  # (the real graph stays alive, unreplayed, until the test ends)
    stale = r"stale HIP graph.*capture_md_cell\(\)"
    with pytest.raises(RuntimeError, match=stale):
        md()
    with pytest.raises(RuntimeError, match=stale):
        md.reset()
    assert md.steps_done == 2
    del graph


def test_refusals_leave_the_model_as_it_was(hip_lib):
    model, inputs, vel, mass = _setup("tensornet")
    z, pos, batch, box, q = inputs
    baro = dict(pressure=0.0, tau=1.0, compressibility=1.0, kT=0.01)
    replay = model.capture(z, pos, batch, box, q=q)
    e0, f0 = (t.clone() for t in replay(pos))
    with pytest.raises(ValueError, match="box"):  # no box (the model is not periodic by itself)
        model.capture_md_cell(z, pos, vel, mass, 0.01, batch=batch, q=q, barostat=baro)
    two = torch.cat([batch, batch + 1])
    with pytest.raises(NotImplementedError, match="own box"):  # one shared box, two molecules
        model.capture_md_cell(torch.cat([z, z]), torch.cat([pos, pos]), torch.cat([vel, vel]), torch.cat([mass, mass]), 0.01, batch=two,
                              box=box, q=torch.zeros(2, device="cuda"), barostat=baro)
    with pytest.raises(ValueError, match="unknown"):
        model.capture_md_cell(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, barostat=dict(baro, beta=1.0))
    with pytest.raises(ValueError, match="coupling"):
        model.capture_md_cell(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, barostat=dict(baro, coupling="isotropic"))
    with pytest.raises(ValueError, match="axis"):
        model.capture_md_cell(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, barostat=dict(baro, coupling="semi-isotropic", axis=3))
    with pytest.raises(ValueError, match="kT"):  # no thermostat to take kT from
        model.capture_md_cell(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, barostat=dict(pressure=0.0, tau=1.0, compressibility=1.0))
    with pytest.raises(ValueError):
        model.capture_md_cell(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, steps_per_replay=0, barostat=baro)
    with pytest.raises(NotImplementedError, match="TensorNet2"):
        B._model("tensornet2").capture_md_cell(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, barostat=baro)
    with pytest.raises(NotImplementedError, match="scalar head"):
        B._model("tensornet", output_model="DipoleMoment").capture_md_cell(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, barostat=baro)
    e1, f1 = replay(pos)  # the graph captured before the refusals replays the same bits
    assert _bits(e1, e0) and _bits(f1, f0)
    # kT and seed default to the thermostat's; the Langevin thermostat runs with the cell barostat
    md = model.capture_md_cell(z, pos, vel, mass, 0.01, batch=batch, box=box.clone(), q=q, steps_per_replay=2,
                               thermostat=dict(friction=1.0, kT=0.02, seed=5), barostat=dict(pressure=0.0, tau=1.0, compressibility=1e-3))
    assert md.cell_barostat["kT"] == 0.02 and md.cell_barostat["seed"] == 5 and md.cell_barostat["coupling"] == "anisotropic"
    md()
    assert md.check() == 2 and torch.isfinite(md.box).all()
