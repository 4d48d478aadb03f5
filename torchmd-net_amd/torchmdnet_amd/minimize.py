"""Device-resident geometry minimisation: K FIRE steps per HIP graph launch (``TorchMD_Net.capture_minimize``).

FIRE (Bitzek et al., Phys. Rev. Lett. 97, 170201, 2006) in the form ASE ships - unit masses, the step of a whole molecule clamped
to ``max_step`` - with one controller per molecule (replica): every molecule of a batch has its own time step and freezes at its own
step.  One step is the per-atom update, neighbour list + energy + forces, the per-molecule sums and the controller; all of it runs
as HIP kernels (csrc/tn_min.hip, ``tmdnet_min_advance``) inside the captured graph, so nothing is issued from the host between two
steps.  The box is fixed.  The scheme and its rounding are documented with the C entries in include/tmdnet_amd.h and in DESIGN.md
section 14."""
import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from torchmdnet_amd import _C
from torchmdnet_amd.models.utils import _ptr, _stream_ptr

MIN_OPEN, MIN_MIDDLE, MIN_CLOSE = 0, 1, 2  # TMDNET_MIN_* of include/tmdnet_amd.h

#: ASE's FIRE parameters, under the keys of ``capture_minimize(fire=...)``
FIRE_DEFAULTS = dict(dt=0.1, dt_max=1.0, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, max_step=0.2)


def parse_fire(fire):
    """``fire=dict(...)`` or None -> every key of ``FIRE_DEFAULTS`` present.  Raises ValueError for an unknown key or a value the
    scheme cannot run with."""
    f = dict(fire or {})
    unknown = set(f) - set(FIRE_DEFAULTS)
    if unknown:
        raise ValueError(f"fire: unknown keys {sorted(unknown)} ({', '.join(FIRE_DEFAULTS)})")
    out = {k: (int(f.get(k, v)) if k == "n_min" else float(f.get(k, v))) for k, v in FIRE_DEFAULTS.items()}
    if not (out["dt"] > 0 and out["dt_max"] > 0 and out["max_step"] > 0 and out["f_inc"] >= 1 and 0 < out["f_dec"] < 1
            and 0 <= out["alpha"] <= 1 and 0 < out["f_alpha"] <= 1 and out["n_min"] >= 0):
        raise ValueError("fire: dt, dt_max and max_step must be positive, f_inc >= 1, 0 < f_dec < 1, 0 <= alpha <= 1, "
                         f"0 < f_alpha <= 1 and n_min >= 0, got {out}")
    return out


class DeviceMinimizer:
    """The object ``TorchMD_Net.capture_minimize`` returns.  ``opt(n)`` replays the captured graph n times (``steps_per_replay``
    steps each) and returns ``opt``; nothing is read back.  Static tensors, rewritten by every replay: ``pos`` [N,3]; ``forces``
    [N,3], the forces at ``pos``; ``epot`` and ``fmax`` [K,B], the energy and the largest atomic force norm after each step of the
    last replay; ``converged_at`` [B] int64, the step at which a molecule's ``fmax`` fell below the bound (-1: not yet; such a
    molecule no longer moves); ``step_size`` [B] fp64, the molecule's current FIRE time step.  ``sums`` [K,B,4] (v.F, F.F, v.v,
    max |F_i|^2), ``coef`` [K,B,3] (c_v, c_f, d of the move that follows) and ``alpha`` [B] are the controller's own logs, and
    ``epot0 / fmax0 / coef0`` those of the start geometry.  ``steps_done`` counts on the host; ``check()`` reads the device."""

    def __init__(self, model, z, pos, batch, box, q, n_mol, steps_per_replay, fmax, fire, fixed, warmup):
        L = _C.lib()
        dev = pos.device
        n = int(z.shape[0])
        self._model = model
        self.steps_per_replay = K = int(steps_per_replay)
        self.n_atoms, self.n_mol = n, n_mol
        self.fire, self.fmax_bound = parse_fire(fire), float(fmax)
        if not self.fmax_bound > 0:
            raise ValueError(f"fmax must be positive, got {fmax}")
        self.inputs = (z, batch, box, q)  # what the graph reads, kept alive for as long as it can be replayed
        self.pos = pos.detach().to(torch.float32).clone().contiguous()
        self.vel = torch.zeros_like(self.pos)  # FIRE's velocity: the minimiser's own state
        self.fixed = None
        if fixed is not None:
            self.fixed = (fixed.detach().to(dev).reshape(-1) != 0).to(torch.uint8).contiguous()
            if self.fixed.numel() != n:
                raise ValueError(f"fixed must have one entry per atom ({n}), got {self.fixed.numel()}")
        f32 = dict(dtype=torch.float32, device=dev)
        self.epot, self.fmax = torch.zeros((K, n_mol), **f32), torch.zeros((K, n_mol), **f32)
        self.sums = torch.zeros((K, n_mol, 4), dtype=torch.float64, device=dev)
        self.coef = torch.zeros((K, n_mol, 3), **f32)
        self.epot0, self.fmax0, self.coef0 = torch.zeros(n_mol, **f32), torch.zeros(n_mol, **f32), torch.zeros((n_mol, 3), **f32)
        self._sums0 = torch.zeros((n_mol, 4), dtype=torch.float64, device=dev)
        self.step_size = torch.zeros(n_mol, dtype=torch.float64, device=dev)
        self.alpha = torch.zeros(n_mol, dtype=torch.float64, device=dev)
        self.converged_at = torch.full((n_mol,), -1, dtype=torch.int64, device=dev)
        nbytes = C.c_size_t(0)
        L.tmdnet_min_workspace_bytes(n, n_mol, C.byref(nbytes))
        self._ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        self.steps_done = 0
        with torch.cuda.device(dev):
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(max(warmup, 1)):  # uploads parameters, sizes the workspaces, checks overflow
                    e0, f0 = self._evaluate()
                self.forces = f0.clone()
                self._start(e0, f0)
            torch.cuda.current_stream(dev).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            self._step_outputs = []  # the evaluations' output buffers live in the graph's pool; kept for the graph's lifetime
            with torch.cuda.graph(self.graph):
                self._advance(MIN_OPEN, self.forces, None, None)
                for k in range(K):
                    out = self._evaluate()
                    self._step_outputs.append(out)
                    self._advance(MIN_MIDDLE if k + 1 < K else MIN_CLOSE, out[1], out[0], k)
        self._engine, self._generation = model._engine, model._engine.generation

    def _evaluate(self):
        z, batch, box, q = self.inputs
        return self._model.energy_and_forces(z, self.pos, batch, box, q, self.n_mol, want_forces=True)

    def _start(self, energy, forces):
        """reset, then the control of the start geometry: the first coefficients, and molecules that are converged as they stand"""
        dev = self.pos.device
        rc = _C.lib().tmdnet_min_reset(_stream_ptr(dev), _ptr(self._ws), 0, self.fire["dt"], self.fire["alpha"])
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_min_reset failed (code {rc})")
        self._advance(MIN_CLOSE, forces, energy, None)

    def _advance(self, phase, forces, energy, k):
        st = self._model._engine
        dev = self.pos.device
        f = self.fire
        if k is None:  # the start geometry
            rows = (self.epot0, self.fmax0, self._sums0, self.coef0)
        else:
            rows = (self.epot[k], self.fmax[k], self.sums[k], self.coef[k])
        logs = [None] * 7 if phase == MIN_OPEN else [_ptr(t) for t in rows + (self.step_size, self.alpha, self.converged_at)]
        rc = _C.lib().tmdnet_min_advance(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), self.n_atoms, self.n_mol, phase,
                                         _ptr(self.pos), _ptr(self.vel), _ptr(forces), _ptr(energy), _ptr(self.fixed),
                                         _ptr(self.inputs[1]), None if phase == MIN_OPEN else _ptr(self.forces), f["dt_max"],
                                         f["n_min"], f["f_inc"], f["f_dec"], f["alpha"], f["f_alpha"], f["max_step"], self.fmax_bound,
                                         *logs)
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_min_advance: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def _check_fresh(self):
        # the graph holds raw pointers into the engine's parameter block and workspaces (TorchMD_Net.capture's replay)
        if self._model._engine is not self._engine or self._engine.generation != self._generation:
            raise RuntimeError("stale HIP graph: the model's parameters or workspaces changed after capture_minimize(); capture again")

    def __call__(self, n: int = 1):
        self._check_fresh()
        for _ in range(int(n)):
            self.graph.replay()
        self.steps_done += int(n) * self.steps_per_replay
        return self

    def check(self) -> int:
        """Read the device's step counter and status (one synchronisation).  Raises the reference's overflow RuntimeError when an
        evaluation found more neighbours than ``max_num_neighbors`` allows, and a RuntimeError naming the forces when a force sum
        was not finite: ``pos`` / ``forces``, the logs and the counter are then those of the last valid step, and replays change
        nothing until ``reset``.  Returns the step counter."""
        host = (C.c_uint64 * 2)()
        dev = self.pos.device
        with torch.cuda.device(dev):
            rc = _C.lib().tmdnet_min_status(_stream_ptr(dev), _ptr(self._ws), host)
        if rc == _C.ERR_OVERFLOW:
            raise RuntimeError("Found num_pairs > max_num_pairs, please increase max_num_pairs "
                               f"(max_num_neighbors={self._model.representation_model.max_num_neighbors}; the minimiser is frozen at "
                               f"step {int(host[0])})")
        if int(host[1]) == 2:
            raise RuntimeError(f"minimiser: the forces after step {int(host[0])} are not finite (a NaN or an infinite force sum); the "
                               "state is frozen at that step")
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_min_status failed (code {rc})")
        return int(host[0])

    def reset(self, pos: Optional[Tensor] = None):
        """New positions (copied into the static buffer), forces evaluated there, velocity zero, every molecule's controller back to
        its start values, status cleared, step counters zero."""
        self._check_fresh()
        dev = self.pos.device
        if pos is not None:
            self.pos.copy_(pos.detach().to(device=dev, dtype=torch.float32))
        self.vel.zero_()
        e, f = self._evaluate()  # raises when these positions overflow
        self.forces.copy_(f)
        with torch.cuda.device(dev):
            self._start(e, f)
        self.steps_done = 0
        self._check_fresh()  # the evaluation must not have re-created what the graph points into
        return self

    def run(self, max_steps: int, check_every: int = 1) -> int:
        """Replay until every molecule has converged or another replay would exceed ``max_steps`` steps; ``converged_at`` is read
        back (one synchronisation) before the first replay and then after every ``check_every`` replays.  Steps come in whole
        replays of ``steps_per_replay``.  Returns the number of steps taken by this call; ``check()`` tells whether they were valid."""
        K, every = self.steps_per_replay, max(int(check_every), 1)
        taken = 0
        while not bool((self.converged_at >= 0).all()):
            n = min(every, (int(max_steps) - taken) // K)
            if n < 1:
                break
            self(n)
            taken += n * K
        return taken
