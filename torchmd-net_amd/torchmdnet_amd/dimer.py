"""Device-resident dimer saddle search: K steps per HIP graph launch (``TorchMD_Net.capture_dimer``).

A first-order saddle point from ONE known state by minimum-mode following: the dimer method (Henkelman and Jonsson, J. Chem. Phys.
111, 7010, 1999) with forward differences (Heyden, Bell and Keil, J. Chem. Phys. 123, 224101, 2005) and the rotation from two
curvature rows (Kaestner and Sherwood, J. Chem. Phys. 128, 014106, 2008), driven by FIRE in the form ASE ships with ONE controller per
dimer.  A dimer is three images of the same n atoms - the midpoint R0, R0 + delta N and R0 + delta M with a unit axis N and a unit
partner M at a right angle; the three images of G dimers are evaluated as one batch of 3 G molecules, and the rotation of the axis,
the inverted force, the controller and the per-atom update run as HIP kernels (csrc/tn_dimer.hip, ``tmdnet_dimer_advance``) inside
the captured graph, so nothing is issued from the host between two steps.  With ``translate=False`` the midpoint stays where it is
and the loop only refines N and the curvature C along it: the lowest mode without a Hessian.  The scheme and its rounding are
documented with the C entries in include/tmdnet_amd.h and in DESIGN.md section 19.  The capture sequence, the stale-graph guard,
``dimer(n)``, ``run``, the status read-back and the skeleton of ``reset`` are those of every captured loop:
``torchmdnet_amd.captured``."""
import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from torchmdnet_amd import _C
from torchmdnet_amd.captured import ConvergingLoop
from torchmdnet_amd.minimize import MIN_CLOSE, MIN_MIDDLE, MIN_OPEN, fire_logs, parse_fire
from torchmdnet_amd.models.utils import _ptr, _stream_ptr

_CAUSES = {1: "the forces are not finite (a NaN or an infinite force or FIRE sum)",
           2: "the mode has no length or is not finite",
           3: "an energy of a dimer's three images is not finite"}


def orthonormal_pair(mode: Optional[Tensor], n_dimers: int, n_atoms: int, fixed: Optional[Tensor], seed: int = 0):
    """The start axis N and partner M of every dimer, [G,n,3] fp32 on the CPU, made in fp64: N is ``mode`` ([n,3], shared, or [G,n,3];
    None: a seeded normal draw per dimer) with the fixed atoms zeroed and normalised; M is a seeded normal draw made orthogonal to N
    and normalised.  Raises ValueError for a mode that is zero on the free atoms.  When every atom is fixed both are zero."""
    G, n = int(n_dimers), int(n_atoms)
    gen = torch.Generator().manual_seed(int(seed))
    draw = torch.randn((2, G, n, 3), dtype=torch.float64, generator=gen)
    free = torch.ones(n, dtype=torch.float64) if fixed is None else (fixed.detach().cpu().reshape(-1) == 0).to(torch.float64)
    if mode is None:
        N = draw[0]
    else:
        N = mode.detach().cpu().to(torch.float64)
        N = (N[None] if N.dim() == 2 else N).expand(G, n, 3)
    N, M = N * free[None, :, None], draw[1] * free[None, :, None]
    if not bool(free.any()):
        z = torch.zeros((G, n, 3), dtype=torch.float32)
        return z, z.clone()
    norm = N.pow(2).sum((1, 2)).sqrt()
    if not bool((torch.isfinite(norm) & (norm > 0)).all()):
        raise ValueError("mode must be finite and must not vanish on the atoms that are not fixed")
    N = N / norm[:, None, None]
    M = M - (M * N).sum((1, 2))[:, None, None] * N
    M = M / M.pow(2).sum((1, 2)).sqrt()[:, None, None]
    M = torch.where(torch.isfinite(M), M, torch.zeros_like(M))  # (one free coordinate: there is no direction at a right angle)
    return N.to(torch.float32).contiguous(), M.to(torch.float32).contiguous()


class DeviceDimer(ConvergingLoop):
    """The object ``TorchMD_Net.capture_dimer`` returns.  ``dimer(n)`` replays the captured graph n times (``steps_per_replay`` steps
    each) and returns ``dimer``; nothing is read back.  Static tensors, rewritten by every replay: ``pos`` [G,n,3], the midpoints (a
    view of image 0 in ``images`` [G,3,n,3], the position buffer the graph reads); ``mode`` [G,n,3], the axis N, and ``partner``;
    ``forces`` [G,n,3], the true forces F0 at ``pos`` of the last accepted step, and ``effective_forces``, F_eff there; ``epot``,
    ``curvature``, ``fmax`` and ``residual`` [K,G] (the energy of the midpoint, C, the largest atomic |F_eff| and |T|) after each
    step of the last replay; ``converged_at`` [G] int64, the step at which a dimer's ``fmax`` fell below the bound with C < 0 (-1: not
    yet; such a dimer no longer moves); ``step_size`` [G] fp64, the dimer's current FIRE time step.  ``rotation`` [K,G,2] (co, si),
    ``quad`` [K,G,3] (a, b, c), ``mode_sums`` [K,G,15], ``mode_coef`` [K,G,10], ``sums`` [K,G,4], ``coef`` [K,G,3] and ``alpha`` [G]
    are the device's own logs, and ``epot0 / fmax0 / coef0 / curvature0 / ...`` those of the start.  ``steps_done`` counts on the
    host; ``check()`` reads the device."""

    _capture_name, _noun = "capture_dimer", "the dimer"

    def __init__(self, model, z, pos, mode, partner, box, q, steps_per_replay, fmax, delta, translate, fire, fixed, warmup):
        super().__init__(model, steps_per_replay)
        L = _C.lib()
        dev = pos.device
        G, n = int(pos.shape[0]), int(pos.shape[1])
        K = self.steps_per_replay
        self.n_dimers, self.n_atoms = G, n
        self.fire, self.fmax_bound = parse_fire(fire), float(fmax)
        self.delta, self.translate = float(delta), bool(translate)
        n_mol = 3 * G
        z_all = z.repeat(n_mol).contiguous()
        batch = torch.arange(n_mol, device=dev, dtype=torch.long).repeat_interleave(n).contiguous()
        q_all = None if q is None else q.repeat_interleave(3).contiguous()
        self.inputs = (z_all, batch, box, q_all)  # what the graph reads, kept alive for as long as it can be replayed
        f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
        self.images = torch.zeros((G, 3, n, 3), **f32)
        self._rows = self.images.view(-1, 3)  # the position buffer of the evaluation
        self.pos = self.images[:, 0]
        self.mode = mode.to(**f32).contiguous().clone()
        self.partner = partner.to(**f32).contiguous().clone()
        self.vel = torch.zeros((G, n, 3), **f32)  # FIRE's velocity: the optimiser's own state
        self.fixed = None
        if fixed is not None:
            self.fixed = (fixed.detach().to(dev).reshape(-1) != 0).to(torch.uint8).contiguous()
        self._write_images(pos)
        self.forces, self.effective_forces = torch.zeros((G, n, 3), **f32), torch.zeros((G, n, 3), **f32)
        self.epot, self.fmax = torch.zeros((K, G), **f32), torch.zeros((K, G), **f32)
        self.sums, self.coef = torch.zeros((K, G, 4), **f64), torch.zeros((K, G, 3), **f32)
        self.curvature, self.residual = torch.zeros((K, G), **f64), torch.zeros((K, G), **f64)
        self.rotation, self.quad = torch.zeros((K, G, 2), **f64), torch.zeros((K, G, 3), **f64)
        self.mode_sums, self.mode_coef = torch.zeros((K, G, 15), **f64), torch.zeros((K, G, 10), **f32)
        self.epot0, self.fmax0 = torch.zeros(G, **f32), torch.zeros(G, **f32)
        self._sums0, self.coef0 = torch.zeros((G, 4), **f64), torch.zeros((G, 3), **f32)
        self.curvature0, self.residual0 = torch.zeros(G, **f64), torch.zeros(G, **f64)
        self.rotation0, self.quad0 = torch.zeros((G, 2), **f64), torch.zeros((G, 3), **f64)
        self.mode_sums0, self.mode_coef0 = torch.zeros((G, 15), **f64), torch.zeros((G, 10), **f32)
        self.step_size, self.alpha = torch.zeros(G, **f64), torch.zeros(G, **f64)
        self.converged_at = torch.full((G,), -1, dtype=torch.int64, device=dev)
        nbytes = C.c_size_t(0)
        if L.tmdnet_dimer_workspace_bytes(n, G, C.byref(nbytes)) != _C.OK:
            raise ValueError(f"{G} dimers of {n} atoms are beyond what tmdnet_dimer_workspace_bytes accepts")
        self._ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        self._capture(warmup, lambda out: self._start(*out), lambda: self._advance(MIN_OPEN, self.effective_forces, None, None))

    def _write_images(self, pos):
        """the three images from the midpoints: R0, R0 + fp32(delta) N, R0 + fp32(delta) M, each one rounded product and sum"""
        d = torch.tensor(self.delta, dtype=torch.float32, device=self.images.device)
        x0 = pos.detach().to(device=self.images.device, dtype=torch.float32)
        self.images[:, 0] = x0
        self.images[:, 1] = x0 + d * self.mode
        self.images[:, 2] = x0 + d * self.partner

    def _capture_step(self, k, K, out):
        """The launch that follows evaluation k of a replay (inside the capture): close step k, open step k + 1"""
        self._advance(MIN_MIDDLE if k + 1 < K else MIN_CLOSE, out[1], out[0], k)

    def _evaluate(self):
        z, batch, box, q = self.inputs
        return self._model.energy_and_forces(z, self._rows, batch, box, q, 3 * self.n_dimers, want_forces=True)

    def _start(self, energy, forces):
        """reset, then the control of the start images: the first rotation and coefficients, and dimers that are converged as they stand"""
        dev = self.images.device
        rc = _C.lib().tmdnet_dimer_reset(_stream_ptr(dev), _ptr(self._ws), 0, self.fire["dt"], self.fire["alpha"], int(self.translate))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_dimer_reset failed (code {rc})")
        self._advance(MIN_CLOSE, forces, energy, None)

    def _advance(self, phase, forces, energy, k):
        st = self._model._engine
        dev = self.images.device
        f = self.fire
        if k is None:  # the start images
            rows = (self.curvature0, self.rotation0, self.residual0, self.quad0, self.mode_sums0, self.mode_coef0)
        else:
            rows = (self.curvature[k], self.rotation[k], self.residual[k], self.quad[k], self.mode_sums[k], self.mode_coef[k])
        is_open = phase == MIN_OPEN
        mode_logs = [None] * 6 if is_open else [_ptr(t) for t in rows]
        rc = _C.lib().tmdnet_dimer_advance(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), self.n_atoms, self.n_dimers,
                                           phase, _ptr(self._rows), _ptr(self.vel), _ptr(self.mode), _ptr(self.partner), _ptr(forces),
                                           _ptr(energy), _ptr(self.fixed), None if is_open else _ptr(self.effective_forces),
                                           None if is_open else _ptr(self.forces), f["dt_max"], f["n_min"], f["f_inc"], f["f_dec"],
                                           f["alpha"], f["f_alpha"], f["max_step"], self.fmax_bound, self.delta,
                                           *fire_logs(self, phase, k), *mode_logs)
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_dimer_advance: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def check(self) -> int:
        """Read the device's step counter and status (one synchronisation).  Raises the reference's overflow RuntimeError when an
        evaluation found more neighbours than ``max_num_neighbors`` allows, and a RuntimeError naming the cause when a dimer was
        unusable - forces or an energy that are not finite, or a mode without length: ``pos`` / ``mode`` / ``forces``, the logs and
        the counter are then those of the last valid step, and replays change nothing until ``reset``.  Returns the step counter."""
        rc, (step, status, cause) = self._status(_C.lib().tmdnet_dimer_status, 3)
        return self._verdict("tmdnet_dimer_status", rc, step, status, cause, "dimer search", _CAUSES)

    def reset(self, pos: Optional[Tensor] = None, mode: Optional[Tensor] = None, translate: Optional[bool] = None):
        """New midpoints (None: as they are), a new axis (None: the axis and the partner as they are; given, it is orthonormalised on
        the host with a fresh partner), ``translate`` switched (None: as it is); the images rewritten, forces evaluated there,
        velocity zero, every dimer's controller back to its start values, status cleared, step counters zero.  The captured graph
        serves both uses: find the mode with ``translate=False``, then ``reset(translate=True)`` and go on from it."""
        G, n = self.n_dimers, self.n_atoms

        def copy_in():
            new_pos = self.pos
            if pos is not None:
                if tuple(pos.shape) != (G, n, 3) and not (G == 1 and tuple(pos.shape) == (n, 3)):
                    raise ValueError(f"reset(pos=) needs {(G, n, 3)}" + (f" or {(n, 3)}" if G == 1 else "") + f", got {tuple(pos.shape)}")
                new_pos = pos.reshape(G, n, 3)
            if mode is not None:
                if tuple(mode.shape) not in ((G, n, 3), (n, 3)):
                    raise ValueError(f"reset(mode=) needs {(G, n, 3)} or {(n, 3)}, got {tuple(mode.shape)}")
                N, M = orthonormal_pair(mode, G, n, self.fixed, seed=0)
                self.mode.copy_(N)
                self.partner.copy_(M)
            if translate is not None:
                self.translate = bool(translate)
            self._write_images(new_pos.clone())
            self.vel.zero_()

        return self._reset(copy_in, lambda out: self._start(*out))
