"""Device-resident relaxed coordinate scans: K steps of a constrained minimisation per HIP graph launch (``TorchMD_Net.capture_scan``).

A relaxed scan minimises a molecule with chosen internal coordinates - distances, angles, torsions, the collective variables (CVs) of
``capture_md_biased`` - held at exact values: a torsion profile, a bond scan, a first guess of a reaction path.  G points, each a copy
of the same n atoms with its own final targets, are evaluated as one batch.  Per step the force and FIRE's velocity are projected onto
the tangent space of the constraints (Lagrange multipliers from the D x D Gram matrix of the CV gradients), FIRE in the form ASE ships
moves the atoms with ONE controller per point, the targets are driven a bounded step from the CVs of the start geometry towards their
final values, and a Gauss-Newton iteration puts the CV atoms back on the constraint surface; all of it runs as HIP kernels
(csrc/tn_scan.hip, ``tmdnet_scan_advance``) inside the captured graph, so nothing is issued from the host between two steps.  At a
constrained minimum dE/dt_d = -lambda_d, so the logged multiplier is the slope of the profile.  The scheme and its rounding are
documented with the C entries in include/tmdnet_amd.h and in DESIGN.md section 21.  The capture sequence, the stale-graph guard,
``scan(n)``, ``run``, the status read-back and the skeleton of ``reset`` are those of every captured loop: ``torchmdnet_amd.captured``."""
import ctypes as C
import math
from typing import Optional

import torch
from torch import Tensor

from torchmdnet_amd import _C
from torchmdnet_amd.captured import ConvergingLoop
from torchmdnet_amd.minimize import MIN_CLOSE, MIN_MIDDLE, MIN_OPEN, fire_logs, parse_fire
from torchmdnet_amd.models.utils import _ptr, _stream_ptr

CV_KINDS = {"distance": (0, 2), "angle": (1, 3), "torsion": (2, 4)}  # name -> (kind, atoms), as in capture_md_biased
MAX_CVS = 4
_DEFAULT_DRIVE = {0: 0.05, 1: 0.1, 2: 0.1}  # length units for a distance, rad for an angle and a torsion

_CAUSES = {1: "the forces are not finite (a NaN or an infinite energy, force or FIRE sum)",
           2: "a collective variable or its gradient is not finite (coincident atoms, a collinear angle or torsion)",
           3: "the Gram matrix of the CV gradients is not positive definite (two CVs that constrain the same motion)",
           4: "the constraint step did not converge in max_iter corrections"}


def grid(start: float, stop: float, n: int) -> Tensor:
    """``n`` evenly spaced target values from ``start`` to ``stop``, both included, [n,1] fp64: the ``targets`` of a scan along one CV"""
    if int(n) < 1:
        raise ValueError(f"grid needs n >= 1, got {n}")
    return torch.linspace(float(start), float(stop), int(n), dtype=torch.float64).reshape(-1, 1)


def parse_cvs(cvs, n_atoms, fixed=None):
    """``cvs=[("distance", i, j), ("angle", i, j, k), ("torsion", i, j, k, l), ...]`` -> (kinds [D], atoms [D,4] with -1 in the slots
    a kind does not use, the distinct atoms ascending).  Raises ValueError naming the cause: D outside 1..4, an unknown kind, a wrong
    number of atoms, an index outside the molecule or repeated within a CV, a CV whose atoms are all fixed."""
    cvs = list(cvs or [])
    D, n = len(cvs), int(n_atoms)
    if not 1 <= D <= MAX_CVS:
        raise ValueError(f"capture_scan takes 1 to {MAX_CVS} collective variables, got {D}")
    still = None if fixed is None else (torch.as_tensor(fixed).detach().cpu().reshape(-1) != 0)
    kinds, atoms = [], []
    for c, cv in enumerate(cvs):
        name, idx = cv[0], [int(i) for i in cv[1:]]
        if name not in CV_KINDS:
            raise ValueError(f"cv {c} has kind {name!r} ({', '.join(CV_KINDS)})")
        kind, na = CV_KINDS[name]
        if len(idx) != na:
            raise ValueError(f"cv {c} ({name}) takes {na} atoms, got {len(idx)}")
        for i in idx:
            if not 0 <= i < n:
                raise ValueError(f"cv {c} ({name}) names atom {i}, outside the molecule of {n} atoms")
        if len(set(idx)) != na:
            raise ValueError(f"cv {c} ({name}) names an atom twice: {idx}")
        if still is not None and bool(still[idx].all()):
            raise ValueError(f"cv {c} ({name}): all of its atoms {idx} are fixed, so it cannot be driven")
        kinds.append(kind)
        atoms.append(idx + [-1] * (4 - na))
    distinct = sorted({i for row in atoms for i in row if i >= 0})
    return kinds, atoms, distinct


def parse_drive(drive, kinds):
    """``drive`` (None: 0.1 rad for an angle or torsion, 0.05 length units for a distance; a number; one per CV) -> list of D floats"""
    D = len(kinds)
    if drive is None:
        out = [_DEFAULT_DRIVE[k] for k in kinds]
    else:
        d = torch.as_tensor(drive, dtype=torch.float64).detach().cpu().reshape(-1)
        if d.numel() not in (1, D):
            raise ValueError(f"drive must be one value or one per collective variable ({D}), got {d.numel()}")
        out = [float(v) for v in d.expand(D)]
    if not all(v > 0 and math.isfinite(v) for v in out):
        raise ValueError(f"drive must be positive and finite, got {out}")
    return out


class DeviceScan(ConvergingLoop):
    """The object ``TorchMD_Net.capture_scan`` returns.  ``scan(n)`` replays the captured graph n times (``steps_per_replay`` steps
    each) and returns ``scan``; nothing is read back.  Static tensors, rewritten by every replay: ``pos`` [G,n,3]; ``forces`` and
    ``projected_forces`` [G,n,3], F and F_perp at ``pos`` of the last accepted step; ``epot`` and ``fmax`` [K,G], the energy and the
    largest atomic |F_perp| after each step of the last replay; ``cv``, ``target`` and ``multiplier`` [K,G,D], the CVs, the targets
    they are held at and lambda (dE/dt = -lambda at a constrained minimum); ``converged_at`` [G] int64, the step at which a point's
    ``fmax`` fell below the bound with its targets at their final values (-1: not yet; such a point no longer moves); ``step_size``
    [G] fp64, the point's current FIRE time step; ``targets`` [G,D] fp64, the final targets.  ``sums`` [K,G,4], ``coef`` [K,G,3],
    ``alpha`` [G], ``multipliers`` [K,G,2,D] (lambda, mu), ``corrections`` [K,G,A,2,3] (of F and v on the A distinct CV atoms
    ``cv_atoms``), ``constrained`` [K,G,A,3] (row k: the CV atoms as evaluation k saw them) and ``iterations`` [K,G] are the device's
    own logs, and ``epot0 / fmax0 / coef0 / cv0 / ...`` those of the start.  ``steps_done`` counts on the host; ``check()`` reads the
    device."""

    _capture_name, _noun = "capture_scan", "the scan"

    def __init__(self, model, z, pos, kinds, atoms, distinct, targets, box, q, steps_per_replay, fmax, drive, tol, max_iter, fire, fixed,
                 warmup):
        super().__init__(model, steps_per_replay)
        L = _C.lib()
        dev = pos.device
        G, n = int(pos.shape[0]), int(pos.shape[1])
        K, D, A = self.steps_per_replay, len(kinds), len(distinct)
        self.n_points, self.n_atoms, self.n_cv = G, n, D
        self.fire, self.fmax_bound = parse_fire(fire), float(fmax)
        self.tol, self.max_iter = float(tol), int(max_iter)
        self.cv_atoms = torch.tensor(distinct, dtype=torch.long)
        self._kinds = (C.c_int32 * D)(*kinds)
        self._atoms = (C.c_int32 * (4 * D))(*[i for row in atoms for i in row])
        self._drive = (C.c_double * D)(*drive)
        z_all = z.repeat(G).contiguous()
        batch = torch.arange(G, device=dev, dtype=torch.long).repeat_interleave(n).contiguous()
        self.inputs = (z_all, batch, box, q)  # what the graph reads, kept alive for as long as it can be replayed
        f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
        self.pos = pos.detach().to(**f32).clone().contiguous()
        self._rows = self.pos.view(-1, 3)  # the position buffer of the evaluation
        self.vel = torch.zeros((G, n, 3), **f32)  # FIRE's velocity: the optimiser's own state
        self.targets = targets.detach().to(**f64).clone().contiguous()
        self.fixed = None
        if fixed is not None:
            self.fixed = (fixed.detach().to(dev).reshape(-1) != 0).to(torch.uint8).contiguous()
        self.forces, self.projected_forces = torch.zeros((G, n, 3), **f32), torch.zeros((G, n, 3), **f32)
        self.epot, self.fmax = torch.zeros((K, G), **f32), torch.zeros((K, G), **f32)
        self.sums, self.coef = torch.zeros((K, G, 4), **f64), torch.zeros((K, G, 3), **f32)
        self.cv, self.target = torch.zeros((K, G, D), **f64), torch.zeros((K, G, D), **f64)
        self.multipliers = torch.zeros((K, G, 2, D), **f32)
        self.multiplier = self.multipliers[:, :, 0]
        self.corrections = torch.zeros((K, G, A, 2, 3), **f32)
        self.constrained = torch.zeros((K, G, A, 3), **f32)
        self.iterations = torch.zeros((K, G), dtype=torch.int32, device=dev)
        self.epot0, self.fmax0 = torch.zeros(G, **f32), torch.zeros(G, **f32)
        self._sums0, self.coef0 = torch.zeros((G, 4), **f64), torch.zeros((G, 3), **f32)
        self.cv0, self.target0 = torch.zeros((G, D), **f64), torch.zeros((G, D), **f64)
        self.multipliers0, self.corrections0 = torch.zeros((G, 2, D), **f32), torch.zeros((G, A, 2, 3), **f32)
        self.step_size, self.alpha = torch.zeros(G, **f64), torch.zeros(G, **f64)
        self.converged_at = torch.full((G,), -1, dtype=torch.int64, device=dev)
        nbytes = C.c_size_t(0)
        if L.tmdnet_scan_workspace_bytes(n, G, C.byref(nbytes)) != _C.OK:
            raise ValueError(f"{G} points of {n} atoms are beyond what tmdnet_scan_workspace_bytes accepts")
        self._ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        self._capture(warmup, lambda out: self._start(*out), lambda: self._advance(MIN_OPEN, self.projected_forces, None, None))

    def _capture_step(self, k, K, out):
        """The launch that follows evaluation k of a replay (inside the capture): close step k, open step k + 1"""
        self._advance(MIN_MIDDLE if k + 1 < K else MIN_CLOSE, out[1], out[0], k)

    def _evaluate(self):
        z, batch, box, q = self.inputs
        return self._model.energy_and_forces(z, self._rows, batch, box, q, self.n_points, want_forces=True)

    def _start(self, energy, forces):
        """reset, then the control of the start geometry: its CVs become the targets the points start from"""
        dev = self.pos.device
        rc = _C.lib().tmdnet_scan_reset(_stream_ptr(dev), _ptr(self._ws), self.n_atoms, self.n_points, 0, self.fire["dt"], self.fire["alpha"])
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_scan_reset failed (code {rc})")
        self._advance(MIN_CLOSE, forces, energy, None)

    def _advance(self, phase, forces, energy, k):
        st = self._model._engine
        dev = self.pos.device
        f = self.fire
        K = self.steps_per_replay
        if phase == MIN_OPEN:
            logs = [None] * 4
        elif k is None:  # the start geometry
            logs = [_ptr(t) for t in (self.cv0, self.target0, self.multipliers0, self.corrections0)]
        else:
            logs = [_ptr(t) for t in (self.cv[k], self.target[k], self.multipliers[k], self.corrections[k])]
        # the constraint step of OPEN makes what evaluation 0 sees, that of MIDDLE after evaluation k what evaluation k + 1 sees
        row = 0 if phase == MIN_OPEN else (k + 1 if phase == MIN_MIDDLE else None)
        cons = [None, None] if row is None or row >= K else [_ptr(self.constrained[row]), _ptr(self.iterations[row])]
        is_open = phase == MIN_OPEN
        rc = _C.lib().tmdnet_scan_advance(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), self.n_atoms, self.n_points, phase,
                                          _ptr(self._rows), _ptr(self.vel), _ptr(forces), _ptr(energy), _ptr(self.fixed),
                                          None if is_open else _ptr(self.forces), _ptr(self.projected_forces), self.n_cv, self._kinds,
                                          self._atoms, _ptr(self.targets), self._drive, self.tol, self.max_iter, f["dt_max"], f["n_min"],
                                          f["f_inc"], f["f_dec"], f["alpha"], f["f_alpha"], f["max_step"], self.fmax_bound,
                                          *fire_logs(self, phase, k), *logs, *cons)
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_scan_advance: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def check(self) -> int:
        """Read the device's step counter and status (one synchronisation).  Raises the reference's overflow RuntimeError when an
        evaluation found more neighbours than ``max_num_neighbors`` allows, and a RuntimeError naming the cause when a point was
        unusable - forces that are not finite, a CV or gradient that is not finite, a Gram matrix that is not positive definite, a
        constraint step that did not converge: ``pos`` / ``forces``, the logs and the counter are then those of the last valid step,
        and replays change nothing until ``reset``.  Returns the step counter."""
        rc, (step, status, cause) = self._status(_C.lib().tmdnet_scan_status, 3)
        return self._verdict("tmdnet_scan_status", rc, step, status, cause, "scan", _CAUSES)

    def reset(self, pos: Optional[Tensor] = None, targets: Optional[Tensor] = None):
        """New start geometries ([n,3], shared, or [G,n,3]; None: the positions as they are) and new final targets ([G,D]; None: as
        they are); forces evaluated there, velocity zero, every point's controller back to its start values and its targets back to
        the CVs of its start geometry, status cleared, step counters zero."""
        G, n, D = self.n_points, self.n_atoms, self.n_cv

        def copy_in():
            if pos is not None and tuple(pos.shape) not in ((G, n, 3), (n, 3)):
                raise ValueError(f"reset(pos=) needs {(G, n, 3)} or {(n, 3)}, got {tuple(pos.shape)}")
            if targets is not None and tuple(targets.shape) != (G, D):
                raise ValueError(f"reset(targets=) needs {(G, D)}, got {tuple(targets.shape)}")
            if targets is not None and not bool(torch.isfinite(targets).all()):
                raise ValueError("reset(targets=): the targets must be finite")
            if pos is not None:
                self.pos.copy_(pos.detach().to(device=self.pos.device, dtype=torch.float32).expand(G, n, 3))
            if targets is not None:
                self.targets.copy_(targets.detach().to(device=self.pos.device, dtype=torch.float64))
            self.vel.zero_()

        return self._reset(copy_in, lambda out: self._start(*out))

    def profile(self) -> dict:
        """The scan as it stands, on the CPU (one synchronisation): ``target`` and ``cv`` [G,D] fp64, ``energy`` [G] fp32 and
        ``multiplier`` [G,D] fp32 of every point's last controlled step - a point that has converged keeps those of the step it
        converged at - and ``converged`` [G] bool."""
        last = self.steps_per_replay - 1
        started = self.steps_done > 0
        pick = (lambda log, log0: (log[last] if started else log0).detach().cpu().clone())
        return dict(target=pick(self.target, self.target0), cv=pick(self.cv, self.cv0), energy=pick(self.epot, self.epot0),
                    multiplier=pick(self.multipliers, self.multipliers0)[:, 0], converged=(self.converged_at >= 0).cpu())
