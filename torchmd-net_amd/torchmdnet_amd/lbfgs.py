"""Device-resident L-BFGS geometry minimisation: K quasi-Newton steps per HIP graph launch
(``TorchMD_Net.capture_minimize(lbfgs=...)``).

ASE's ``LBFGS`` without line search - H0 = 1 / alpha, the last ``memory`` pairs, the step of every atom clamped to ``max_step``,
``damping`` - with one optimiser per molecule (replica): every molecule of a batch has its own history and freezes at its own step.
The one deviation from ASE: a pair (s, y) enters the history only when s.y > 0 (ASE stores every pair and can divide by zero or step
uphill); where every pair passes, the sequence is ASE's.  One step is the move, neighbour list + energy + forces, the scalar products
of the history, the controller (the two-loop recursion in coefficient space) and the direction; all of it runs as HIP kernels
(csrc/tn_lbfgs.hip, ``tmdnet_lbfgs_advance``) inside the captured graph.  The scheme and its rounding are documented with the C entries
in include/tmdnet_amd.h and in DESIGN.md section 14.  The capture sequence, the stale-graph guard, ``opt(n)``, ``run``, the status
read-back and the skeleton of ``reset`` are those of every captured loop: ``torchmdnet_amd.captured``."""
import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from torchmdnet_amd import _C
from torchmdnet_amd.captured import ConvergingLoop
from torchmdnet_amd.minimize import MIN_CLOSE, MIN_MIDDLE, MIN_OPEN
from torchmdnet_amd.models.utils import _ptr, _stream_ptr

#: ASE's LBFGS parameters, under the keys of ``capture_minimize(lbfgs=...)``
LBFGS_DEFAULTS = dict(memory=100, alpha=70.0, max_step=0.2, damping=1.0)

MAX_MEMORY = 512  # tn_lbfgs::kMaxMemory


def parse_lbfgs(lbfgs):
    """``lbfgs=dict(...)`` -> every key of ``LBFGS_DEFAULTS`` present.  Raises ValueError for an unknown key, for memory < 1 (or above
    what the controller's LDS holds, 512) and for an alpha, max_step or damping that is not positive and finite."""
    f = dict(lbfgs or {})
    unknown = set(f) - set(LBFGS_DEFAULTS)
    if unknown:
        raise ValueError(f"lbfgs: unknown keys {sorted(unknown)} ({', '.join(LBFGS_DEFAULTS)})")
    out = {k: (int(f.get(k, v)) if k == "memory" else float(f.get(k, v))) for k, v in LBFGS_DEFAULTS.items()}
    if "memory" in f and float(f["memory"]) != out["memory"]:
        raise ValueError(f"lbfgs: memory must be an integer, got {f['memory']}")
    if not 1 <= out["memory"] <= MAX_MEMORY:
        raise ValueError(f"lbfgs: memory must be between 1 and {MAX_MEMORY}, got {out['memory']}")
    for k in ("alpha", "max_step", "damping"):
        if not (0 < out[k] < float("inf")):
            raise ValueError(f"lbfgs: {k} must be positive and finite, got {out[k]}")
    return out


class DeviceLBFGS(ConvergingLoop):
    """The object ``TorchMD_Net.capture_minimize(lbfgs=...)`` returns.  ``opt(n)`` replays the captured graph n times
    (``steps_per_replay`` steps each) and returns ``opt``; nothing is read back.  Static tensors, rewritten by every replay: ``pos``
    [N,3]; ``forces`` [N,3], the forces at ``pos``; ``direction`` [N,3], the quasi-Newton direction p of the move prepared (0 for a
    fixed atom); ``epot`` and ``fmax`` [K,B], the energy and the largest atomic force norm after each step of the last replay;
    ``accepted`` [K,B] int32, 1 where that step's pair (s, y) entered the history; ``scale`` [K,B], the clamp factor c of the move
    that LED to each step; ``sums`` [K,B,4] fp64 (F.F, max |F_i|^2, s.y of the candidate, g.p of the move prepared); ``pairs`` [B] int32,
    the pairs a molecule holds; ``converged_at`` [B] int64, the step at which a molecule's ``fmax`` fell below the bound (-1: not yet;
    such a molecule no longer moves).  ``epot0 / fmax0`` belong to the start geometry.  ``steps_done`` counts on the host; ``check()``
    reads the device."""

    _capture_name, _noun = "capture_minimize", "the minimiser"

    def __init__(self, model, z, pos, batch, box, q, n_mol, steps_per_replay, fmax, lbfgs, fixed, warmup):
        super().__init__(model, steps_per_replay)
        L = _C.lib()
        dev = pos.device
        n = int(z.shape[0])
        K = self.steps_per_replay
        self.n_atoms, self.n_mol = n, n_mol
        self.lbfgs, self.fmax_bound = parse_lbfgs(lbfgs), float(fmax)
        if not self.fmax_bound > 0:
            raise ValueError(f"fmax must be positive, got {fmax}")
        self.inputs = (z, batch, box, q)  # what the graph reads, kept alive for as long as it can be replayed
        self.pos = pos.detach().to(torch.float32).clone().contiguous()
        self.direction = torch.zeros_like(self.pos)
        self.fixed = None
        if fixed is not None:
            self.fixed = (fixed.detach().to(dev).reshape(-1) != 0).to(torch.uint8).contiguous()
            if self.fixed.numel() != n:
                raise ValueError(f"fixed must have one entry per atom ({n}), got {self.fixed.numel()}")
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.epot, self.fmax, self.scale = (torch.zeros((K, n_mol), **f32) for _ in range(3))
        self.sums = torch.zeros((K, n_mol, 4), dtype=torch.float64, device=dev)
        self.accepted = torch.zeros((K, n_mol), **i32)
        self.epot0, self.fmax0 = torch.zeros(n_mol, **f32), torch.zeros(n_mol, **f32)
        self._sums0 = torch.zeros((n_mol, 4), dtype=torch.float64, device=dev)
        self._accepted0 = torch.zeros(n_mol, **i32)
        self.pairs = torch.zeros(n_mol, **i32)
        self.converged_at = torch.full((n_mol,), -1, dtype=torch.int64, device=dev)
        nbytes = C.c_size_t(0)
        rc = L.tmdnet_lbfgs_workspace_bytes(n, n_mol, self.lbfgs["memory"], C.byref(nbytes))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_lbfgs_workspace_bytes failed (code {rc})")
        self._ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)

        def start(out):
            self.forces = out[1].clone()
            self._start(*out)

        self._capture(warmup, start, lambda: self._advance(MIN_OPEN, self.forces, None, None))

    def _capture_step(self, k, K, out):
        """The launch that follows evaluation k of a replay (inside the capture): close step k, open step k + 1"""
        self._advance(MIN_MIDDLE if k + 1 < K else MIN_CLOSE, out[1], out[0], k)

    def _evaluate(self):
        z, batch, box, q = self.inputs
        return self._model.energy_and_forces(z, self.pos, batch, box, q, self.n_mol, want_forces=True)

    def _start(self, energy, forces):
        """reset, then the control of the start geometry: an empty history, p = F / alpha, and molecules that are converged as they
        stand"""
        rc = _C.lib().tmdnet_lbfgs_reset(_stream_ptr(self.pos.device), _ptr(self._ws), 0)
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_lbfgs_reset failed (code {rc})")
        self._advance(MIN_CLOSE, forces, energy, None)

    def _advance(self, phase, forces, energy, k):
        """One phase; the log rows are those of the start geometry for ``k is None``, row k of the last replay's logs otherwise"""
        st = self._model._engine
        f = self.lbfgs
        if phase == MIN_OPEN:
            logs = [None] * 7
        else:
            rows = (self.epot0, self.fmax0, self._sums0, self.pairs, self._accepted0, None) if k is None else \
                (self.epot[k], self.fmax[k], self.sums[k], self.pairs, self.accepted[k], self.scale[k])
            logs = [_ptr(t) for t in rows] + [_ptr(self.converged_at)]
        rc = _C.lib().tmdnet_lbfgs_advance(st.handle, _stream_ptr(self.pos.device), _ptr(st.graph_ws), _ptr(self._ws), self.n_atoms,
                                           self.n_mol, phase, _ptr(self.pos), _ptr(forces), _ptr(energy), _ptr(self.fixed),
                                           _ptr(self.inputs[1]), None if phase == MIN_OPEN else _ptr(self.forces), _ptr(self.direction),
                                           f["memory"], f["alpha"], f["max_step"], f["damping"], self.fmax_bound, *logs)
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_lbfgs_advance: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def check(self) -> int:
        """Read the device's step counter and status (one synchronisation).  Raises the reference's overflow RuntimeError when an
        evaluation found more neighbours than ``max_num_neighbors`` allows, and a RuntimeError naming the forces when a sum was not
        finite: ``pos`` / ``forces``, the history, the logs and the counter are then those of the last valid step, and replays change
        nothing until ``reset``.  Returns the step counter."""
        rc, (step, status, cause) = self._status(_C.lib().tmdnet_lbfgs_status, 3)
        if status == 2:
            raise RuntimeError(f"minimiser: the forces after step {step} are not finite (a NaN or an infinite force sum); the "
                               "state is frozen at that step")
        return self._verdict("tmdnet_lbfgs_status", rc, step, status)

    def reset(self, pos: Optional[Tensor] = None):
        """New positions (copied into the static buffer), forces evaluated there, the history of every molecule emptied, status
        cleared, step counters zero."""
        dev = self.pos.device

        def copy_in():
            if pos is not None:
                self.pos.copy_(pos.detach().to(device=dev, dtype=torch.float32))

        def start(out):
            self.forces.copy_(out[1])
            self._start(*out)

        return self._reset(copy_in, start)
