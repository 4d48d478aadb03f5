"""Device-resident nudged elastic band: K band steps per HIP graph launch (``TorchMD_Net.capture_neb``).

A minimum-energy path between two minima and its saddle point: NEB with the improved tangent (Henkelman and Jonsson, J. Chem. Phys.
113, 9978, 2000) and a climbing image, driven by FIRE in the form ASE ships with ONE controller per band.  A band is M images of the
same n atoms; the M images of G bands are evaluated as one batch of G M molecules, and the band-coupled force projection, the
controller and the per-atom update run as HIP kernels (csrc/tn_neb.hip, ``tmdnet_neb_advance``) inside the captured graph, so nothing
is issued from the host between two steps.  Images 0 and M - 1 of every band never move.  No minimum image is applied between
images: the caller supplies an unwrapped path.  The scheme and its rounding are documented with the C entries in
include/tmdnet_amd.h and in DESIGN.md section 15.  The capture sequence, the stale-graph guard, ``neb(n)``, ``run``, the status
read-back and the skeleton of ``reset`` are those of every captured loop: ``torchmdnet_amd.captured``."""
import ctypes as C
import math
from typing import Optional

import torch
from torch import Tensor

from torchmdnet_amd import _C
from torchmdnet_amd.captured import ConvergingLoop
from torchmdnet_amd.minimize import MIN_CLOSE, MIN_MIDDLE, MIN_OPEN, fire_logs, parse_fire
from torchmdnet_amd.models.utils import _ptr, _stream_ptr

#: the band's own parameters and their defaults (``spring`` in E / length^2)
NEB_DEFAULTS = dict(spring=0.1, climb=False)

_CAUSES = {1: "the band forces are not finite (a NaN or an infinite force sum)",
           2: "a tangent has no length or is not finite (coincident images)",
           3: "an energy of a band is not finite"}


def parse_neb(neb):
    """``dict(spring=, climb=)`` or None -> every key of ``NEB_DEFAULTS`` present.  Raises ValueError for an unknown key and for a
    spring constant that is not positive and finite."""
    d = dict(neb or {})
    unknown = set(d) - set(NEB_DEFAULTS)
    if unknown:
        raise ValueError(f"neb: unknown keys {sorted(unknown)} ({', '.join(NEB_DEFAULTS)})")
    out = dict(spring=float(d.get("spring", NEB_DEFAULTS["spring"])), climb=bool(d.get("climb", NEB_DEFAULTS["climb"])))
    if not (out["spring"] > 0 and math.isfinite(out["spring"])):
        raise ValueError(f"neb: spring must be positive and finite, got {out['spring']}")
    return out


def interpolate(initial: Tensor, final: Tensor, n_images: int) -> Tensor:
    """The linear path from ``initial`` to ``final`` ([n,3] each), endpoints included: [n_images, n, 3].  No minimum image."""
    if int(n_images) < 3:
        raise ValueError(f"a band needs at least 3 images, got {n_images}")
    if initial.shape != final.shape or initial.dim() != 2 or initial.shape[1] != 3:
        raise ValueError(f"initial and final must both be [n,3], got {tuple(initial.shape)} and {tuple(final.shape)}")
    t = torch.linspace(0.0, 1.0, int(n_images), dtype=initial.dtype, device=initial.device)[:, None, None]
    path = initial[None] + t * (final - initial)[None]
    path[0], path[-1] = initial, final  # bit for bit
    return path


class DeviceNEB(ConvergingLoop):
    """The object ``TorchMD_Net.capture_neb`` returns.  ``neb(n)`` replays the captured graph n times (``steps_per_replay`` steps
    each) and returns ``neb``; nothing is read back.  Static tensors, rewritten by every replay: ``images`` [G,M,n,3], a view of the
    position buffer the graph reads; ``forces`` [G,M,n,3], the band forces F_neb at ``images`` (zero on the endpoint images);
    ``epot`` [K,G,M], ``fmax`` [K,G] (the largest atomic |F_neb| of the band) and ``climber`` [K,G] (the interior image with the
    largest energy: the one that climbs when climbing is on) after each step of the last replay; ``converged_at`` [G] int64, the step
    at which a band's ``fmax`` fell below the bound (-1: not yet; such a band no longer moves); ``step_size`` [G] fp64, the band's
    current FIRE time step.  ``tangent_coef`` [K,G,M,2] (s+, s- of F_neb = F + s+ d+ + s- d-), ``weights`` [K,G,M,2] (w+, w- of the
    tangent), ``path_sums`` [K,G,M,5], ``sums`` [K,G,4], ``coef`` [K,G,3] (c_v, c_f, d of the move that follows) and ``alpha`` [G] are
    the device's own logs, and ``epot0 / fmax0 / coef0 / tangent_coef0 / climber0`` those of the start path.  ``steps_done`` counts on
    the host; ``check()`` reads the device."""

    _capture_name, _noun = "capture_neb", "the band"

    def __init__(self, model, z, images, box, q, steps_per_replay, fmax, spring, climb, fire, fixed, warmup):
        super().__init__(model, steps_per_replay)
        L = _C.lib()
        dev = images.device
        G, M, n = (int(s) for s in images.shape[:3])
        K = self.steps_per_replay
        self.n_bands, self.n_images, self.n_atoms = G, M, n
        self.fire, self.fmax_bound = parse_fire(fire), float(fmax)
        opts = parse_neb(dict(spring=spring, climb=climb))
        self.spring, self.climb = opts["spring"], opts["climb"]
        n_mol = G * M
        z_all = z.repeat(n_mol).contiguous()
        batch = torch.arange(n_mol, device=dev, dtype=torch.long).repeat_interleave(n).contiguous()
        q_all = None if q is None else q.repeat_interleave(M).contiguous()
        self.inputs = (z_all, batch, box, q_all)  # what the graph reads, kept alive for as long as it can be replayed
        self.pos = images.detach().to(torch.float32).reshape(-1, 3).clone().contiguous()
        self.images = self.pos.view(G, M, n, 3)
        self.vel = torch.zeros_like(self.pos)  # FIRE's velocity: the optimiser's own state
        self.fixed = None
        if fixed is not None:
            self.fixed = (fixed.detach().to(dev).reshape(-1) != 0).to(torch.uint8).contiguous()
        f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
        self.epot, self.fmax = torch.zeros((K, G, M), **f32), torch.zeros((K, G), **f32)
        self.sums, self.coef = torch.zeros((K, G, 4), **f64), torch.zeros((K, G, 3), **f32)
        self.path_sums, self.weights = torch.zeros((K, G, M, 5), **f64), torch.zeros((K, G, M, 2), **f64)
        self.tangent_coef = torch.zeros((K, G, M, 2), **f32)
        self.climber = torch.zeros((K, G), dtype=torch.int32, device=dev)
        self.epot0, self.fmax0 = torch.zeros((G, M), **f32), torch.zeros(G, **f32)
        self._sums0, self.coef0 = torch.zeros((G, 4), **f64), torch.zeros((G, 3), **f32)
        self.path_sums0, self.weights0 = torch.zeros((G, M, 5), **f64), torch.zeros((G, M, 2), **f64)
        self.tangent_coef0 = torch.zeros((G, M, 2), **f32)
        self.climber0 = torch.zeros(G, dtype=torch.int32, device=dev)
        self.step_size, self.alpha = torch.zeros(G, **f64), torch.zeros(G, **f64)
        self.converged_at = torch.full((G,), -1, dtype=torch.int64, device=dev)
        nbytes = C.c_size_t(0)
        if L.tmdnet_neb_workspace_bytes(n, M, G, C.byref(nbytes)) != _C.OK:
            raise ValueError(f"a band of {G} x {M} x {n} rows is beyond what tmdnet_neb_workspace_bytes accepts")
        self._ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)

        def start(out):
            self._forces = torch.zeros_like(out[1])
            self._start(*out)

        self._capture(warmup, start, lambda: self._advance(MIN_OPEN, self._forces, None, None))
        self.forces = self._forces.view(G, M, n, 3)

    def _capture_step(self, k, K, out):
        """The launch that follows evaluation k of a replay (inside the capture): close step k, open step k + 1"""
        self._advance(MIN_MIDDLE if k + 1 < K else MIN_CLOSE, out[1], out[0], k)

    def _evaluate(self):
        z, batch, box, q = self.inputs
        return self._model.energy_and_forces(z, self.pos, batch, box, q, self.n_bands * self.n_images, want_forces=True)

    def _start(self, energy, forces):
        """reset, then the control of the start path: the first coefficients, and bands that are converged as they stand"""
        dev = self.pos.device
        rc = _C.lib().tmdnet_neb_reset(_stream_ptr(dev), _ptr(self._ws), 0, self.fire["dt"], self.fire["alpha"], int(self.climb))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_neb_reset failed (code {rc})")
        self._advance(MIN_CLOSE, forces, energy, None)

    def _advance(self, phase, forces, energy, k):
        st = self._model._engine
        dev = self.pos.device
        f = self.fire
        if k is None:  # the start path
            band = (self.path_sums0, self.weights0, self.tangent_coef0, self.climber0)
        else:
            band = (self.path_sums[k], self.weights[k], self.tangent_coef[k], self.climber[k])
        is_open = phase == MIN_OPEN
        band_logs = [None] * 4 if is_open else [_ptr(t) for t in band]
        rc = _C.lib().tmdnet_neb_advance(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), self.n_atoms, self.n_images,
                                         self.n_bands, phase, _ptr(self.pos), _ptr(self.vel), _ptr(forces), _ptr(energy),
                                         _ptr(self.fixed), None if is_open else _ptr(self._forces), f["dt_max"], f["n_min"], f["f_inc"],
                                         f["f_dec"], f["alpha"], f["f_alpha"], f["max_step"], self.fmax_bound, self.spring,
                                         *fire_logs(self, phase, k), *band_logs)
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_neb_advance: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def check(self) -> int:
        """Read the device's step counter and status (one synchronisation).  Raises the reference's overflow RuntimeError when an
        evaluation found more neighbours than ``max_num_neighbors`` allows, and a RuntimeError naming the cause when a band was
        unusable - band forces or an energy that are not finite, or coincident images: ``images`` / ``forces``, the logs and the
        counter are then those of the last valid step, and replays change nothing until ``reset``.  Returns the step counter."""
        rc, (step, status, cause) = self._status(_C.lib().tmdnet_neb_status, 3)
        return self._verdict("tmdnet_neb_status", rc, step, status, cause, "nudged elastic band", _CAUSES)

    def reset(self, images: Optional[Tensor] = None, climb: Optional[bool] = None):
        """New images (copied into the static buffer; None: the path as it is), ``climb`` switched (None: as it is), forces evaluated
        there, velocity zero, every band's controller back to its start values, status cleared, step counters zero.  The captured
        graph serves both phases: relax with ``climb=False``, then ``reset(climb=True)`` and go on from the relaxed path."""

        def copy_in():
            if images is not None:
                want = tuple(self.images.shape)
                if tuple(images.shape) != want and not (self.n_bands == 1 and tuple(images.shape) == want[1:]):
                    raise ValueError(f"reset(images=) needs {want}" + (f" or {want[1:]}" if self.n_bands == 1 else "") +
                                     f", got {tuple(images.shape)}")
                self.pos.copy_(images.detach().to(device=self.pos.device, dtype=torch.float32).reshape(-1, 3))
            if climb is not None:
                self.climb = bool(climb)
            self.vel.zero_()

        return self._reset(copy_in, lambda out: self._start(*out))

    def barrier(self) -> Tensor:
        """``max_i E_i - E_0`` of every band at the last valid evaluated step, [G] on the host.  The step is the device's counter
        (read as ``check()`` reads it, without raising), so after a replay that froze part-way the row of the step the state is
        frozen at is taken, not the last row of the log; then one read-back of that row."""
        rc, (step, _, _) = self._status(_C.lib().tmdnet_neb_status, 3)
        if rc not in (_C.OK, _C.ERR_OVERFLOW, _C.ERR_STATE):
            raise RuntimeError(f"tmdnet_neb_status failed (code {rc})")
        # step s > 0 was logged in row (s - 1) % K, and nothing was written after it
        e =self.epot0 if step == 0 else self.epot[(step - 1) % self.steps_per_replay]
        return (e.max(dim=1).values - e[:, 0]).cpu()
