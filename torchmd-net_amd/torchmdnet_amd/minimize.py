"""Device-resident geometry minimisation: K FIRE steps per HIP graph launch (``TorchMD_Net.capture_minimize``).

FIRE (Bitzek et al., Phys. Rev. Lett. 97, 170201, 2006) in the form ASE ships - unit masses, the step of a whole molecule clamped
to ``max_step`` - with one controller per molecule (replica): every molecule of a batch has its own time step and freezes at its own
step.  One step is the per-atom update, neighbour list + energy + forces, the per-molecule sums and the controller; all of it runs
as HIP kernels (csrc/tn_min.hip, ``tmdnet_min_advance``) inside the captured graph, so nothing is issued from the host between two
steps.  The box is fixed unless ``cell=`` is given: then it relaxes with the atoms (ASE's ``UnitCellFilter`` scheme,
``tmdnet_min_advance_cell``).  The scheme and its rounding are documented with the C entries in include/tmdnet_amd.h and in DESIGN.md
section 14.  The capture sequence, the stale-graph guard, ``opt(n)``, ``run``, the status read-back and the skeleton of ``reset`` are
those of every captured loop: ``torchmdnet_amd.captured``."""
import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from torchmdnet_amd import _C
from torchmdnet_amd.captured import ConvergingLoop
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


#: the keys of ``capture_minimize(cell=...)`` and their defaults
CELL_DEFAULTS = dict(mask=None, hydrostatic=False, constant_volume=False, pressure=0.0, cell_factor=None)


def parse_cell(cell):
    """``cell=dict(...)`` -> every key of ``CELL_DEFAULTS`` present, ``mask`` a 3 x 3 list of 0.0 / 1.0.  Raises ValueError for an
    unknown key, a mask that is not a symmetric 3 x 3 matrix of 0 / 1, ``hydrostatic`` together with ``constant_volume``, a pressure
    that is not finite and a ``cell_factor`` that is not positive."""
    c = dict(cell)
    unknown = set(c) - set(CELL_DEFAULTS)
    if unknown:
        raise ValueError(f"cell: unknown keys {sorted(unknown)} ({', '.join(CELL_DEFAULTS)})")
    out = dict(CELL_DEFAULTS, **c)
    mask = torch.ones(3, 3) if out["mask"] is None else torch.as_tensor(out["mask"]).detach().cpu().to(torch.float64)
    if tuple(mask.shape) != (3, 3) or not bool(((mask == 0) | (mask == 1)).all()):
        raise ValueError(f"cell: mask must be a [3,3] matrix of 0 / 1, got {mask.tolist()}")
    if not torch.equal(mask, mask.T):
        raise ValueError(f"cell: mask must be symmetric, got {mask.tolist()}")
    out["mask"] = [[float(v) for v in row] for row in mask.tolist()]
    out["hydrostatic"], out["constant_volume"] = bool(out["hydrostatic"]), bool(out["constant_volume"])
    if out["hydrostatic"] and out["constant_volume"]:
        raise ValueError("cell: hydrostatic and constant_volume exclude each other (an isotropic strain changes the volume)")
    out["pressure"] = float(out["pressure"])
    if out["pressure"] != out["pressure"] or out["pressure"] in (float("inf"), float("-inf")):
        raise ValueError(f"cell: pressure must be finite, got {out['pressure']}")
    if out["cell_factor"] is not None:
        out["cell_factor"] = float(out["cell_factor"])
        if not out["cell_factor"] > 0:
            raise ValueError(f"cell: cell_factor must be positive, got {out['cell_factor']}")
    return out


def fire_logs(loop, phase, k):
    """The seven log pointers of a FIRE advance (``tmdnet_min_advance`` and its cell and band siblings): none for the OPEN phase,
    the rows of the start geometry for ``k is None``, row k of the last replay's logs otherwise, then the controller's state"""
    if phase == MIN_OPEN:
        return [None] * 7
    if k is None:
        rows = (loop.epot0, loop.fmax0, loop._sums0, loop.coef0)
    else:
        rows = (loop.epot[k], loop.fmax[k], loop.sums[k], loop.coef[k])
    return [_ptr(t) for t in rows + (loop.step_size, loop.alpha, loop.converged_at)]


class DeviceMinimizer(ConvergingLoop):
    """The object ``TorchMD_Net.capture_minimize`` returns.  ``opt(n)`` replays the captured graph n times (``steps_per_replay``
    steps each) and returns ``opt``; nothing is read back.  Static tensors, rewritten by every replay: ``pos`` [N,3]; ``forces``
    [N,3], the forces at ``pos``; ``epot`` and ``fmax`` [K,B], the energy and the largest atomic force norm after each step of the
    last replay; ``converged_at`` [B] int64, the step at which a molecule's ``fmax`` fell below the bound (-1: not yet; such a
    molecule no longer moves); ``step_size`` [B] fp64, the molecule's current FIRE time step.  ``sums`` [K,B,4] (v.F, F.F, v.v,
    max |F_i|^2), ``coef`` [K,B,3] (c_v, c_f, d of the move that follows) and ``alpha`` [B] are the controller's own logs, and
    ``epot0 / fmax0 / coef0`` those of the start geometry.  ``steps_done`` counts on the host; ``check()`` reads the device.

    With ``cell=`` the box relaxes too.  ``box`` is the box the graph reads and rewrites ([3,3] for one molecule, [B,3,3] otherwise;
    the caller's tensor when it needed no conversion); ``deform`` [B,3,3] fp64 is the deformation gradient D since the last reset,
    ``box = H0 D^T``; ``stress`` [K,B,3,3] fp64 is -W_s / V of each evaluated step, ``volume`` [K,B] fp64 its V, ``cell_force``
    [K,B,3,3] fp64 the cell rows' force G / cell_factor; ``fmax`` includes the cell rows, ``sums`` are the atoms' alone (the
    controller adds the cell rows' terms); ``stress0 / volume0 / cell_force0`` belong to the start geometry.  The atoms' integrated state is ``pos D^-T``; ``vel`` is its velocity.  A fixed atom
    keeps ``pos D^-T``: it follows the cell affinely.  The neighbour search's minimum image needs a lower-triangular box, so the
    rotation of the cell is not a degree of freedom here: the entries of the cell force below the diagonal are dropped, D stays
    upper triangular and ``H0 D^T`` lower triangular (a shear allowed by ``mask`` acts through the entry above the diagonal)."""

    _capture_name, _noun = "capture_minimize", "the minimiser"

    def __init__(self, model, z, pos, batch, box, q, n_mol, steps_per_replay, fmax, fire, fixed, warmup, cell=None):
        super().__init__(model, steps_per_replay)
        L = _C.lib()
        dev = pos.device
        n = int(z.shape[0])
        K = self.steps_per_replay
        self.n_atoms, self.n_mol = n, n_mol
        self.fire, self.fmax_bound = parse_fire(fire), float(fmax)
        if not self.fmax_bound > 0:
            raise ValueError(f"fmax must be positive, got {fmax}")
        self.inputs = (z, batch, box, q)  # what the graph reads, kept alive for as long as it can be replayed
        self.cell = None if cell is None else parse_cell(cell)
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
        if self.cell is not None:
            self._stage_cell(box, batch)

        def start(out):
            self.forces = out[1].clone()
            self._start(*out)

        self._capture(warmup, start, lambda: self._advance(MIN_OPEN, self.forces, None, None))

    def _capture_step(self, k, K, out):
        """The launch that follows evaluation k of a replay (inside the capture): close step k, open step k + 1"""
        self._advance(MIN_MIDDLE if k + 1 < K else MIN_CLOSE, out[1], out[0], k, *out[2:])

    def _stage_cell(self, box, batch):
        """the cell's state and logs, and the workspace with room for it"""
        dev, B, K = self.pos.device, self.n_mol, self.steps_per_replay
        f64 = dict(dtype=torch.float64, device=dev)
        self.box = box
        self._xt = self.pos.clone()  # pos D^-T: what is integrated
        self.deform = torch.eye(3, **f64).repeat(B, 1, 1).contiguous()
        self._cell_vel = torch.zeros((B, 3, 3), **f64)
        self.stress, self.cell_force = torch.zeros((K, B, 3, 3), **f64), torch.zeros((K, B, 3, 3), **f64)
        self.volume = torch.zeros((K, B), **f64)
        self.stress0, self.cell_force0, self.volume0 = torch.zeros((B, 3, 3), **f64), torch.zeros((B, 3, 3), **f64), torch.zeros(B, **f64)
        c = self.cell["cell_factor"]
        if c is None:  # ASE's: the number of atoms (of that molecule)
            self._cell_factor = torch.bincount(batch, minlength=B)[:B].clamp(min=1).to(torch.float64)
        else:
            self._cell_factor = torch.full((B,), c, **f64)
        # the rotation gauge: only the entries on and above the diagonal move D, so that H0 D^T stays lower triangular
        self._mask = (C.c_double * 9)(*[v if a <= b else 0.0 for a, row in enumerate(self.cell["mask"]) for b, v in enumerate(row)])
        self._flags = int(self.cell["hydrostatic"]) | (int(self.cell["constant_volume"]) << 1)
        nbytes = C.c_size_t(0)
        _C.lib().tmdnet_min_workspace_bytes_cell(self.n_atoms, B, C.byref(nbytes))
        self._ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)

    def _evaluate(self):
        z, batch, box, q = self.inputs
        if self.cell is not None:  # (energy, forces, virial): the gather sibling of the virial replaces the force gather
            return self._model.energy_and_forces(z, self.pos, batch, box, q, self.n_mol, want_forces=True, want_virial=True)
        return self._model.energy_and_forces(z, self.pos, batch, box, q, self.n_mol, want_forces=True)

    def _start(self, energy, forces, virial=None):
        """reset, then the control of the start geometry: the first coefficients, and molecules that are converged as they stand"""
        dev = self.pos.device
        if self.cell is not None:
            rc = _C.lib().tmdnet_min_reset_cell(_stream_ptr(dev), _ptr(self._ws), self.n_atoms, self.n_mol, 0, self.fire["dt"],
                                                self.fire["alpha"], _ptr(self.box), _ptr(self.deform), _ptr(self._cell_vel),
                                                _ptr(self.pos), _ptr(self._xt))
        else:
            rc = _C.lib().tmdnet_min_reset(_stream_ptr(dev), _ptr(self._ws), 0, self.fire["dt"], self.fire["alpha"])
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_min_reset failed (code {rc})")
        self._advance(MIN_CLOSE, forces, energy, None, virial)

    def _advance_cell(self, phase, forces, energy, k, virial):
        st = self._model._engine
        dev = self.pos.device
        f = self.fire
        is_open = phase == MIN_OPEN
        if k is None:  # the start geometry
            cell_rows = (self.stress0, self.volume0, self.cell_force0)
        else:
            cell_rows = (self.stress[k], self.volume[k], self.cell_force[k])
        cell_logs = [None] * 3 if is_open else [_ptr(t) for t in cell_rows]
        rc = _C.lib().tmdnet_min_advance_cell(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), self.n_atoms, self.n_mol,
                                              phase, _ptr(self.pos), _ptr(self.vel), _ptr(forces), _ptr(energy), _ptr(self.fixed),
                                              _ptr(self.inputs[1]), None if is_open else _ptr(self.forces), f["dt_max"], f["n_min"],
                                              f["f_inc"], f["f_dec"], f["alpha"], f["f_alpha"], f["max_step"], self.fmax_bound,
                                              *fire_logs(self, phase, k), _ptr(self._xt), _ptr(self.box), _ptr(self.deform), _ptr(self._cell_vel), _ptr(virial),
                                              _ptr(self._cell_factor), self._mask, self._flags, self.cell["pressure"], *cell_logs)
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_min_advance_cell: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def _advance(self, phase, forces, energy, k, virial=None):
        if self.cell is not None:
            return self._advance_cell(phase, forces, energy, k, virial)
        st = self._model._engine
        dev = self.pos.device
        f = self.fire
        rc = _C.lib().tmdnet_min_advance(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), self.n_atoms, self.n_mol, phase,
                                         _ptr(self.pos), _ptr(self.vel), _ptr(forces), _ptr(energy), _ptr(self.fixed),
                                         _ptr(self.inputs[1]), None if phase == MIN_OPEN else _ptr(self.forces), f["dt_max"],
                                         f["n_min"], f["f_inc"], f["f_dec"], f["alpha"], f["f_alpha"], f["max_step"], self.fmax_bound,
                                         *fire_logs(self, phase, k))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_min_advance: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def check(self) -> int:
        """Read the device's step counter and status (one synchronisation).  Raises the reference's overflow RuntimeError when an
        evaluation found more neighbours than ``max_num_neighbors`` allows, and a RuntimeError naming the forces when a force sum
        was not finite: ``pos`` / ``forces``, the logs and the counter are then those of the last valid step, and replays change
        nothing until ``reset``.  With ``cell=`` the error also names a virial that was not finite or a box without volume, and
        ``box`` / ``deform`` are those of the last valid step as well.  Returns the step counter."""
        L = _C.lib()
        rc, (step, status, cause) = self._status(L.tmdnet_min_status if self.cell is None else L.tmdnet_min_status_cell, 3)
        if status == 2 and cause == 2:
            raise RuntimeError(f"minimiser: the virial after step {step} is not finite; the state, the box included, is frozen "
                               "at that step")
        if status == 2 and cause == 3:
            raise RuntimeError(f"minimiser: the box after step {step} has no volume, or the next move would leave it without "
                               "one or not finite; the state, the box included, is frozen at that step")
        if status == 2:
            raise RuntimeError(f"minimiser: the forces after step {step} are not finite (a NaN or an infinite force sum); the "
                               "state is frozen at that step")
        return self._verdict("tmdnet_min_status", rc, step, status)

    def reset(self, pos: Optional[Tensor] = None, box: Optional[Tensor] = None):
        """New positions (copied into the static buffer), forces evaluated there, velocity zero, every molecule's controller back to
        its start values, status cleared, step counters zero.  With ``cell=``: ``box`` (copied into ``self.box``; None: the box as it
        is) becomes the new reference box and ``deform`` the identity."""
        dev = self.pos.device

        def copy_in():
            if box is not None:
                if self.cell is None:
                    raise ValueError("reset(box=) needs a minimiser captured with cell=...: the box of this one is fixed")
                new = box.detach().to(device=dev, dtype=torch.float32).reshape(self.box.shape)
                if bool((torch.linalg.det(new.double()) == 0).any()):
                    raise ValueError("reset(box=): a box has no volume")
                self.box.copy_(new)
            if pos is not None:
                self.pos.copy_(pos.detach().to(device=dev, dtype=torch.float32))
            self.vel.zero_()

        def start(out):
            self.forces.copy_(out[1])
            self._start(*out)

        return self._reset(copy_in, start)
