"""Device-resident intrinsic reaction coordinate: K steps per HIP graph launch (``TorchMD_Net.capture_irc``).

The path of steepest descent in mass-weighted coordinates from a saddle point, in both directions: the damped velocity Verlet path
follower of Hratchian and Schlegel (J. Phys. Chem. A 106, 165, 2002) - a classical trajectory with a = force_scale F / m whose speed
is put back to a constant v0 after every step, one evaluation per step, one time step per path chosen from an error estimate.  The
G D paths (G saddles, D directions) are evaluated as one batch of G D molecules, and the closing kick, the path sums, the controller
of every path, the damping, the path record and the opening half of the next step run as HIP kernels (csrc/tn_irc.hip,
``tmdnet_irc_advance``) inside the captured graph, so nothing is issued from the host between two steps.  The scheme and its rounding
are documented with the C entries in include/tmdnet_amd.h and in DESIGN.md section 20.  The capture sequence, the stale-graph guard,
``irc(n)``, ``run``, the status read-back and the skeleton of ``reset`` are those of every captured loop: ``torchmdnet_amd.captured``."""
import ctypes as C
import math
from typing import Optional

import torch
from torch import Tensor

from torchmdnet_amd import _C
from torchmdnet_amd.captured import ConvergingLoop
from torchmdnet_amd.minimize import MIN_CLOSE, MIN_MIDDLE, MIN_OPEN
from torchmdnet_amd.models.utils import _ptr, _stream_ptr

_CAUSES = {1: "the forces are not finite (a NaN or an infinite force)",
           2: "the velocity of a path has no length or a path sum is not finite",
           3: "an energy is not finite"}
_DIRECTIONS = {"both": (1.0, -1.0), "forward": (1.0,), "backward": (-1.0,)}


def unit_direction(mode: Tensor, n_saddles: int, n_atoms: int, fixed: Optional[Tensor]) -> Tensor:
    """The unit direction u of every saddle, [G,n,3] fp32 on the CPU, made in fp64: ``mode`` ([n,3], shared, or [G,n,3]) with the
    fixed atoms zeroed, normalised.  Raises ValueError for a mode that vanishes on the atoms that are not fixed."""
    G, n = int(n_saddles), int(n_atoms)
    free = torch.ones(n, dtype=torch.float64) if fixed is None else (fixed.detach().cpu().reshape(-1) == 0).to(torch.float64)
    u = mode.detach().cpu().to(torch.float64)
    u = (u[None] if u.dim() == 2 else u).expand(G, n, 3) * free[None, :, None]
    norm = u.pow(2).sum((1, 2)).sqrt()
    if not bool((torch.isfinite(norm) & (norm > 0)).all()):
        raise ValueError("mode must be finite and must not vanish on the atoms that are not fixed")
    return (u / norm[:, None, None]).to(torch.float32).contiguous()


def record_layout(n_atoms: int, n_paths: int, capacity: int) -> dict:
    """Byte offsets of the path record from the workspace's first address that is a multiple of 256, as include/tmdnet_amd.h states
    them: the 256-byte header, then n_recorded int32 [P], frame_s fp64 [P,C], frame_e fp32 [P,C], frames fp32 [P,C,n,3], each array
    on the next multiple of 256 bytes"""
    up = lambda b: (b + 255) & ~255
    P, Cp, n = int(n_paths), int(capacity), int(n_atoms)
    off, out = 256, {}
    for name, nbytes in (("n_recorded", 4 * P), ("frame_s", 8 * P * Cp), ("frame_e", 4 * P * Cp), ("frames", 12 * P * Cp * n)):
        out[name] = off
        off += up(nbytes)
    out["end"] = off
    return out


def record_views(ws: Tensor, n_atoms: int, n_paths: int, capacity: int):
    """-> n_recorded [P] int32, frame_s [P,C] fp64, frame_e [P,C] fp32, frames [P,C,n,3] fp32: views of the uint8 workspace ``ws``"""
    P, Cp, n = int(n_paths), int(capacity), int(n_atoms)
    lay = record_layout(n, P, Cp)
    base = (-ws.data_ptr()) % 256

    def view(name, dtype, shape):
        count = math.prod(shape)
        start = base + lay[name]
        return ws[start:start + count * torch.empty((), dtype=dtype).element_size()].view(dtype).view(shape)

    return (view("n_recorded", torch.int32, (P,)), view("frame_s", torch.float64, (P, Cp)), view("frame_e", torch.float32, (P, Cp)),
            view("frames", torch.float32, (P, Cp, n, 3)))


class DeviceIRC(ConvergingLoop):
    """The object ``TorchMD_Net.capture_irc`` returns.  ``irc(n)`` replays the captured graph n times (``steps_per_replay`` steps
    each) and returns ``irc``; nothing is read back.  Static tensors, rewritten by every replay: ``pos``, ``vel`` [G,D,n,3], the last
    accepted point of every path and the damped velocity there, and ``forces`` [G,D,n,3], the forces there; ``epot``, ``fmax``
    (fp32), ``arc``, ``dt``, ``power`` (fp64) [K,G,D] after each step of the last replay - the energy, the largest atomic |F|, the
    mass-weighted arc length s from the start image, the next time step and F.v'; ``converged_at`` [G,D] int64, the step at which a
    path finished (-1: not yet; such a path no longer moves) and ``reason`` [G,D] int32 (1: the forces fell below ``fmax``, 2: the
    path turned uphill - the minimum lies within one step behind it); ``step_size``, ``arc_length`` [G,D] fp64 and ``n_recorded``
    [G,D] int32.  ``sums`` [K,G,D,6] (vv, P, fmax2, D2, ds2, the atoms that move) and ``coef`` [K,G,D,2] (fp32(c), fp32(dt_i)) are
    the device's own logs, and ``epot0 / fmax0 / sums0 / coef0`` those of the start images.  ``frames`` [G,D,C,n,3], ``frame_s`` and
    ``frame_energy`` [G,D,C] are views of the record in the workspace.  Direction d = 0 is forward (along ``mode``) unless
    ``direction="backward"``.  ``steps_done`` counts on the host; ``check()`` reads the device."""

    _capture_name, _noun = "capture_irc", "the path"

    def __init__(self, model, z, pos, u, masses, dt, signs, box, q, steps_per_replay, force_scale, fmax, v0, error, initial_step, dt_min,
                 dt_max, every, capacity, fixed, warmup):
        super().__init__(model, steps_per_replay)
        L = _C.lib()
        dev = pos.device
        G, n, D = int(pos.shape[0]), int(pos.shape[1]), len(signs)
        K, P = self.steps_per_replay, G * D
        self.n_saddles, self.n_directions, self.n_paths, self.n_atoms = G, D, P, n
        self.signs = tuple(float(s) for s in signs)
        self.dt0, self.fmax_bound, self.v0, self.error = float(dt), float(fmax), float(v0), float(error)
        self.initial_step, self.dt_min, self.dt_max = float(initial_step), float(dt_min), float(dt_max)
        self.every, self.capacity, self.force_scale = int(every), int(capacity), float(force_scale)
        z_all = z.repeat(P).contiguous()
        batch = torch.arange(P, device=dev, dtype=torch.long).repeat_interleave(n).contiguous()
        q_all = None if q is None else q.repeat_interleave(D).contiguous()
        self.inputs = (z_all, batch, box, q_all)  # what the graph reads, kept alive for as long as it can be replayed
        f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
        m64 = masses.detach().cpu().to(torch.float64).reshape(-1)
        self.masses = m64.to(torch.float32).to(dev).contiguous()
        self._half_inv_mass = (self.force_scale / (2.0 * m64)).to(torch.float32).to(dev).contiguous()  # c_a, rounded once
        self.fixed = None
        if fixed is not None:
            self.fixed = (fixed.detach().to(dev).reshape(-1) != 0).to(torch.uint8).contiguous()
        self.saddle = pos.detach().to(**f32).contiguous().clone()
        self.direction = u.to(**f32).contiguous().clone()
        self.pos, self.vel, self.forces = (torch.zeros((G, D, n, 3), **f32) for _ in range(3))
        self._rows = self.pos.view(-1, 3)  # the position buffer of the evaluation
        self._write_start()
        self.epot, self.fmax = torch.zeros((K, G, D), **f32), torch.zeros((K, G, D), **f32)
        self.arc, self.dt, self.power = (torch.zeros((K, G, D), **f64) for _ in range(3))
        self.sums, self.coef = torch.zeros((K, G, D, 6), **f64), torch.zeros((K, G, D, 2), **f32)
        self.epot0, self.fmax0 = torch.zeros((G, D), **f32), torch.zeros((G, D), **f32)
        self.sums0, self.coef0 = torch.zeros((G, D, 6), **f64), torch.zeros((G, D, 2), **f32)
        self.step_size, self.arc_length = torch.zeros((G, D), **f64), torch.zeros((G, D), **f64)
        self.converged_at = torch.full((G, D), -1, dtype=torch.int64, device=dev)
        self.reason = torch.zeros((G, D), dtype=torch.int32, device=dev)
        self.n_recorded = torch.zeros((G, D), dtype=torch.int32, device=dev)
        nbytes = C.c_size_t(0)
        if L.tmdnet_irc_workspace_bytes(n, P, self.capacity, C.byref(nbytes)) != _C.OK:
            raise ValueError(f"{P} paths of {n} atoms with {self.capacity} frames are beyond what tmdnet_irc_workspace_bytes accepts")
        self._ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        _, s, e, fr = record_views(self._ws, n, P, self.capacity)
        self.frame_s, self.frame_energy = s.view(G, D, self.capacity), e.view(G, D, self.capacity)
        self.frames = fr.view(G, D, self.capacity, n, 3)
        self._capture(warmup, lambda out: self._start(*out), lambda: self._advance(MIN_OPEN, self.forces, None, None))

    def _write_start(self):
        """the start images: x_0 = x_TS + (sigma fp32(initial_step)) u, v_0 = (sigma fp32(v0)) u, each one rounded product (and sum)"""
        dev = self.pos.device
        step = torch.tensor(self.initial_step, dtype=torch.float32, device=dev)
        speed = torch.tensor(self.v0, dtype=torch.float32, device=dev)
        for d, sigma in enumerate(self.signs):
            sg = torch.tensor(sigma, dtype=torch.float32, device=dev)
            self.pos[:, d] = self.saddle + (sg * step) * self.direction
            self.vel[:, d] = (sg * speed) * self.direction

    def _capture_step(self, k, K, out):
        """The launch that follows evaluation k of a replay (inside the capture): close step k, open step k + 1"""
        self._advance(MIN_MIDDLE if k + 1 < K else MIN_CLOSE, out[1], out[0], k)

    def _evaluate(self):
        z, batch, box, q = self.inputs
        return self._model.energy_and_forces(z, self._rows, batch, box, q, self.n_paths, want_forces=True)

    def _start(self, energy, forces):
        """reset, then the control of the start images: the first damping, frame 0, and paths that are finished as they stand"""
        dev = self.pos.device
        rc = _C.lib().tmdnet_irc_reset(_stream_ptr(dev), _ptr(self._ws), 0, self.dt0)
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_irc_reset failed (code {rc})")
        self._advance(MIN_CLOSE, forces, energy, None)

    def _advance(self, phase, forces, energy, k):
        st = self._model._engine
        dev = self.pos.device
        if phase == MIN_OPEN:
            logs = [None] * 12
        elif k is None:  # the start images
            logs = [_ptr(t) for t in (self.epot0, self.fmax0, self.sums0, self.coef0)] + [None] * 3
        else:
            logs = [_ptr(t[k]) for t in (self.epot, self.fmax, self.sums, self.coef, self.dt, self.arc, self.power)]
        if phase != MIN_OPEN:
            logs += [_ptr(t) for t in (self.converged_at, self.reason, self.step_size, self.arc_length, self.n_recorded)]
        rc = _C.lib().tmdnet_irc_advance(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), self.n_atoms, self.n_paths,
                                         self.capacity, self.every, phase, _ptr(self._rows), _ptr(self.vel), _ptr(forces), _ptr(energy),
                                         _ptr(self._half_inv_mass), _ptr(self.masses), _ptr(self.fixed),
                                         None if phase == MIN_OPEN else _ptr(self.forces), self.fmax_bound, self.v0, self.error, self.dt_min,
                                         self.dt_max, *logs)
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_irc_advance: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def check(self) -> int:
        """Read the device's step counter and status (one synchronisation).  Raises the reference's overflow RuntimeError when an
        evaluation found more neighbours than ``max_num_neighbors`` allows, and a RuntimeError naming the cause when a path was
        unusable - forces or an energy that are not finite, or a velocity without length: ``pos`` / ``vel`` / ``forces``, the logs and
        the counter are then those of the last valid step, and replays change nothing until ``reset``.  Returns the step counter."""
        rc, (step, status, cause) = self._status(_C.lib().tmdnet_irc_status, 3)
        return self._verdict("tmdnet_irc_status", rc, step, status, cause, "IRC", _CAUSES)

    @property
    def truncated(self) -> bool:
        """whether a path has taken more frames than ``capacity`` holds (one synchronisation)"""
        return bool((self.n_recorded > self.capacity).any())

    def reset(self, pos: Optional[Tensor] = None, mode: Optional[Tensor] = None):
        """New saddle points (None: as they are), a new direction (None: as it is; given, it is normalised on the host); the start
        images rewritten, forces evaluated there, both generations and the record forgotten, every path's time step back to ``dt``,
        status cleared, step counters zero."""
        G, n = self.n_saddles, self.n_atoms

        def copy_in():
            if pos is not None:
                if tuple(pos.shape) != (G, n, 3) and not (G == 1 and tuple(pos.shape) == (n, 3)):
                    raise ValueError(f"reset(pos=) needs {(G, n, 3)}" + (f" or {(n, 3)}" if G == 1 else "") + f", got {tuple(pos.shape)}")
            if mode is not None:
                if tuple(mode.shape) not in ((G, n, 3), (n, 3)):
                    raise ValueError(f"reset(mode=) needs {(G, n, 3)} or {(n, 3)}, got {tuple(mode.shape)}")
                u = unit_direction(mode, G, n, self.fixed)
                self.direction.copy_(u)
            if pos is not None:
                self.saddle.copy_(pos.detach().reshape(G, n, 3))
            self._write_start()
            self.n_recorded.zero_()

        return self._reset(copy_in, lambda out: self._start(*out))

    def path(self, g: int = 0) -> dict:
        """The recorded path of saddle ``g``, read back (one synchronisation): the backward frames reversed (s < 0), the saddle (s = 0)
        and the forward frames -> dict(s [F] fp64, energy [F] fp32, pos [F,n,3] fp32), s strictly increasing.  A frame's s is the
        device's arc length from its start image plus the mass-weighted length of the initial step.  The energy of the saddle is not
        evaluated by the loop: it is NaN unless a direction's frame 0 lies on it."""
        g = int(g)
        dev = self.pos.device
        counts = self.n_recorded[g].clamp(max=self.capacity).tolist()
        m = self.masses.double()
        moving = torch.isfinite(m) if self.fixed is None else torch.isfinite(m) & (self.fixed == 0)
        saddle = [torch.zeros(1, dtype=torch.float64, device=dev), torch.full((1,), float("nan"), dtype=torch.float32, device=dev),
                  self.saddle[g][None]]
        back, fwd = None, None
        for d, sigma in enumerate(self.signs):
            k = int(counts[d])
            off = (m[moving, None] * self._start_offset(g, d)[moving] ** 2).sum().sqrt()
            part = [sigma * (self.frame_s[g, d, :k] + off), self.frame_energy[g, d, :k], self.frames[g, d, :k]]
            if sigma < 0:
                back = [t.flip(0) for t in part]
            else:
                fwd = part
        pieces = [p for p in (back, saddle, fwd) if p is not None]
        return dict(s=torch.cat([p[0] for p in pieces]).cpu(), energy=torch.cat([p[1] for p in pieces]).cpu(),
                    pos=torch.cat([p[2] for p in pieces]).cpu())

    def _start_offset(self, g, d):
        """x_0 - x_TS of path (g, d) as the start images were written, [n,3] fp64"""
        dev = self.pos.device
        step = torch.tensor(self.initial_step, dtype=torch.float32, device=dev)
        sg = torch.tensor(self.signs[d], dtype=torch.float32, device=dev)
        x0 = self.saddle[g] + (sg * step) * self.direction[g]
        return x0.double() - self.saddle[g].double()
