"""Device-resident minima hopping: K steps of a conformer search per HIP graph launch (``TorchMD_Net.capture_minima_hopping``).

Minima hopping (Goedecker, J. Chem. Phys. 120, 9911, 2004; parameters named as in ASE's ``MinimaHopping``) leaves a basin by a short
NVE run at kinetic temperature kT, quenches with FIRE, and asks whether the minimum it fell into is new; kT and the acceptance window
ediff are fed back from the answers.  The B molecules of a batch are B independent walkers.  Every walker is in one of four phases -
QUENCH, COMPARE, LAUNCH, MD - and walkers in different phases share the one evaluation of a step; the phase machine, the removal of
momentum and angular momentum of the drawn velocities and the aligned RMSD of a fresh minimum against a history kept on the device run
as HIP kernels (csrc/tn_hop.hip, ``tmdnet_hop_advance``) inside the captured graph, so nothing is issued from the host between two
steps.  The scheme and its rounding are documented with the C entries in include/tmdnet_amd.h and in DESIGN.md section 22.  The capture
sequence, the stale-graph guard, ``hop(n)``, the status read-back and the skeleton of ``reset`` are those of every captured loop:
``torchmdnet_amd.captured``."""
import ctypes as C
import math
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from torchmdnet_amd import _C
from torchmdnet_amd.captured import CapturedLoop
from torchmdnet_amd.minimize import parse_fire
from torchmdnet_amd.models.utils import _ptr, _stream_ptr

PHASES = ("quench", "compare", "launch", "md")  # TMDNET_HOP_* of include/tmdnet_amd.h
QUENCH, COMPARE, LAUNCH, MD = range(4)
OUTCOMES = ("none", "start", "same", "known", "accepted", "rejected", "unconverged", "singular")
(OUT_NONE, OUT_START, OUT_SAME, OUT_KNOWN, OUT_ACCEPTED, OUT_REJECTED, OUT_UNCONVERGED, OUT_SINGULAR) = range(8)
ALIGN = {"none": 0, "translation": 1, "rotation": 2}
MAX_CAPACITY = 64
SUMS_LOG, COEF_LOG, COUNTERS = 16, 10, 7
JACOBI_SWEEPS = 12

#: the parameters of the search under the names of ``capture_minima_hopping``
HOP_DEFAULTS = dict(beta1=1.1, beta2=1.1, beta3=1 / 1.1, alpha1=0.98, alpha2=1 / 0.98, mdmin=2, md_steps=400, opt_steps=2000, fmax=0.05,
                    rmsd_tol=0.1, energy_tol=1e-3, capacity=32, seed=0)


def parse_hop(dt, kT0, ediff0, fire=None, align=None, has_box=False, has_fixed=False, **kw):
    """Every parameter of the search validated and under one dict: ``HOP_DEFAULTS`` overridden by ``kw``, ``dt``, ``kT0``, ``ediff0``,
    ``align`` (0 / 1 / 2; None: rotation without a box and without fixed atoms, translation with a box, none with fixed atoms) and
    ``fire`` (``parse_fire``).  Raises ValueError naming what the scheme cannot run with."""
    unknown = set(kw) - set(HOP_DEFAULTS)
    if unknown:
        raise ValueError(f"minima hopping: unknown parameters {sorted(unknown)}")
    p = dict(HOP_DEFAULTS, **kw)
    p.update(dt=float(dt), kT0=float(kT0), ediff0=float(ediff0), fire=parse_fire(fire))
    for key in ("dt", "kT0", "fmax", "rmsd_tol", "energy_tol"):
        if not (p[key] > 0 and math.isfinite(p[key])):
            raise ValueError(f"{key} must be positive and finite, got {p[key]}")
    if not (p["ediff0"] > 0 and math.isfinite(p["ediff0"])):
        raise ValueError(f"ediff0 must be positive and finite, got {p['ediff0']}")
    for key in ("beta1", "beta2", "beta3", "alpha1", "alpha2"):
        p[key] = float(p[key])
        if not (p[key] > 0 and math.isfinite(p[key])):
            raise ValueError(f"{key} must be positive and finite, got {p[key]}")
    for key in ("mdmin", "md_steps", "opt_steps", "capacity", "seed"):
        p[key] = int(p[key])
    if p["mdmin"] < 1:
        raise ValueError(f"mdmin must be at least 1, got {p['mdmin']}")
    if p["md_steps"] < 1 or p["opt_steps"] < 1:
        raise ValueError(f"md_steps and opt_steps must be at least 1, got {p['md_steps']} and {p['opt_steps']}")
    if not 1 <= p["capacity"] <= MAX_CAPACITY:
        raise ValueError(f"capacity must lie in 1..{MAX_CAPACITY}, got {p['capacity']}")
    if align is None:
        align = "none" if has_fixed else ("translation" if has_box else "rotation")
    if align not in ALIGN:
        raise ValueError(f"align must be one of {sorted(ALIGN)} or None, got {align!r}")
    p["align"] = ALIGN[align]
    return p


def fill_args(args, p):
    """the parameters of ``parse_hop`` into a ``_C.HopArgs``"""
    f = p["fire"]
    args.dt_max, args.f_inc, args.f_dec, args.alpha0 = f["dt_max"], f["f_inc"], f["f_dec"], f["alpha"]
    args.f_alpha, args.max_step, args.fmax, args.dt0, args.n_min = f["f_alpha"], f["max_step"], p["fmax"], f["dt"], f["n_min"]
    for key in ("beta1", "beta2", "beta3", "alpha1", "alpha2", "rmsd_tol", "energy_tol", "dt", "mdmin", "md_steps", "opt_steps",
                "capacity", "align"):
        setattr(args, key, p[key])
    args.seed = p["seed"] & 0xFFFFFFFFFFFFFFFF
    return args


# ---- the host helper: the device's definition of the distance between two geometries, in fp64 ---------------------------------------
def _jacobi_max4(A):
    """largest eigenvalue of a symmetric 4 x 4 matrix by ``JACOBI_SWEEPS`` cyclic Jacobi sweeps (tn_hop::jacobi_max4)"""
    A = np.array(A, dtype=np.float64)
    for _ in range(JACOBI_SWEEPS):
        for p in range(3):
            for q in range(p + 1, 4):
                apq = float(A[p, q])
                if apq == 0.0:
                    continue
                theta = (float(A[q, q]) - float(A[p, p])) / (2.0 * apq)  # (Python floats: a tiny apq gives inf and t = 0)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                J = np.eye(4)
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = s, -s
                A = J.T @ A @ J
    return float(np.max(np.diag(A)))


def rmsd(a, b, align: str = "rotation") -> float:
    """The distance the device compares minima with, on the host in fp64: the root mean square deviation of ``a`` from ``b`` ([n,3]
    each) as they stand (``align="none"``), after the centroids are superposed (``"translation"``) or after the best proper rotation
    as well (``"rotation"``: Horn's quaternion method, the largest eigenvalue of the 4 x 4 matrix of the centred cross-covariance by
    cyclic Jacobi sweeps; a mirror image keeps a positive distance; fewer than 3 atoms: translation only)."""
    if align not in ALIGN:
        raise ValueError(f"align must be one of {sorted(ALIGN)}, got {align!r}")
    a = np.asarray(a.detach().cpu() if isinstance(a, Tensor) else a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b.detach().cpu() if isinstance(b, Tensor) else b, dtype=np.float64).reshape(-1, 3)
    if a.shape != b.shape or a.shape[0] < 1:
        raise ValueError(f"rmsd needs two geometries of the same n >= 1 atoms, got {a.shape} and {b.shape}")
    n = a.shape[0]
    if align == "none":
        return math.sqrt(max(float(((a - b) ** 2).sum()) / n, 0.0))
    a, b = a - a.mean(0), b - b.mean(0)
    S = a.T @ b
    if align == "rotation" and n >= 3:
        N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                      [0.0, S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                      [0.0, 0.0, S[1, 1] - S[0, 0] - S[2, 2], S[1, 2] + S[2, 1]],
                      [0.0, 0.0, 0.0, S[2, 2] - S[0, 0] - S[1, 1]]])
        N = N + np.triu(N, 1).T
        lam = _jacobi_max4(N)
    else:
        lam = float(np.trace(S))
    return math.sqrt(max((float((a * a).sum()) + float((b * b).sum()) - 2.0 * lam) / n, 0.0))


class DeviceHop(CapturedLoop):
    """The object ``TorchMD_Net.capture_minima_hopping`` returns.  ``hop(n)`` replays the captured graph n times (``steps_per_replay``
    steps each) and returns ``hop``; nothing is read back.  Static tensors, rewritten by every replay: ``pos / vel / forces`` [N,3]
    (``vel`` is the MD velocity during an escape and FIRE's during a quench); ``phase`` [B] int32, the phase of every walker's NEXT
    step (``PHASES``); ``kT / ediff`` [B] fp64; ``minimum_pos`` [N,3] and ``minimum_energy`` [B], the accepted minimum each walker
    hops from; ``best_pos / best_energy``, the lowest minimum ever recorded, kept outside the ring; ``n_hops / n_same / n_known /
    n_new / n_accepted / n_unconverged`` [B] int64 (views of ``counters`` [B,7], whose last column counts the ring's writes);
    ``epot / fmax / ekin`` [K,B] fp32, ``phase_log / outcome`` [K,B] int32 (``OUTCOMES``) of the last replay - ``fmax`` is 0 on a
    COMPARE or LAUNCH step, ``ekin`` the kinetic energy of an MD step in the unit of m v^2; ``sums`` [K,B,16] fp64 and ``coef``
    [K,B,10] fp32 are the controller's own logs.  ``ring_pos`` [C,N,3], ``ring_energy / ring_found / ring_visits`` [B,C] hold the
    history; ``minima(b)`` reads it.  ``steps_done`` counts on the host; ``check()`` reads the device."""

    _capture_name, _noun = "capture_minima_hopping", "the search"

    def __init__(self, model, z, pos, masses, batch, box, q, n_mol, steps_per_replay, force_scale, params, fixed, warmup):
        super().__init__(model, steps_per_replay)
        dev = pos.device
        N, B, K = int(z.shape[0]), int(n_mol), self.steps_per_replay
        self.n_atoms, self.n_mol, self.params, self.force_scale = N, B, params, float(force_scale)
        cap = params["capacity"]
        self.inputs = (z, batch, box, q)  # what the graph reads, kept alive for as long as it can be replayed
        f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        self.pos = pos.detach().to(torch.float32).clone().contiguous()
        self.vel = torch.zeros_like(self.pos)
        # per-atom constants in fp64, rounded once, as capture_md stages them; a fixed atom has infinite mass: hk = sig = 0
        m64 = masses.detach().to(device=dev, dtype=torch.float64).reshape(-1).clone()
        still = torch.isinf(m64)
        if fixed is not None:
            still = still | (fixed.detach().to(dev).reshape(-1) != 0)
        m64[still] = float("inf")
        self.fixed = still.to(torch.uint8).contiguous() if bool(still.any()) else None
        self.masses = m64.to(torch.float32).contiguous()
        self.hk = (0.5 * params["dt"] * self.force_scale / m64).to(torch.float32).contiguous()
        self.sig = torch.sqrt(self.force_scale / m64).to(torch.float32).contiguous()
        self.forces = torch.zeros((N, 3), **f32)
        self.minimum_pos, self.best_pos = torch.zeros((N, 3), **f32), torch.zeros((N, 3), **f32)
        self.ring_pos = torch.zeros((cap, N, 3), **f32)
        self.ring_energy = torch.zeros((B, cap), **f64)
        self.ring_found, self.ring_visits = torch.zeros((B, cap), **i64), torch.zeros((B, cap), **i64)
        self.kT, self.ediff = torch.zeros(B, **f64), torch.zeros(B, **f64)
        self.minimum_energy, self.best_energy = torch.zeros(B, **f64), torch.zeros(B, **f64)
        self.phase = torch.zeros(B, **i32)
        self.counters = torch.zeros((B, COUNTERS), **i64)
        (self.n_hops, self.n_same, self.n_known, self.n_new, self.n_accepted, self.n_unconverged) = (self.counters[:, k] for k in range(6))
        self.epot, self.fmax, self.ekin = torch.zeros((K, B), **f32), torch.zeros((K, B), **f32), torch.zeros((K, B), **f32)
        self.phase_log, self.outcome = torch.zeros((K, B), **i32), torch.zeros((K, B), **i32)
        self.sums, self.coef = torch.zeros((K, B, SUMS_LOG), **f64), torch.zeros((K, B, COEF_LOG), **f32)
        self._kT0 = torch.full((B,), params["kT0"], **f64)
        self._ediff0 = torch.full((B,), params["ediff0"], **f64)
        nbytes = C.c_size_t(0)
        if _C.lib().tmdnet_hop_workspace_bytes(N, B, cap, C.byref(nbytes)) != _C.OK:
            raise ValueError(f"{B} walkers, {N} atoms and a capacity of {cap} are beyond what tmdnet_hop_workspace_bytes accepts")
        self._ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        self._args = [self._make_args(k) for k in range(K)]  # one per step of a replay: its log rows and its evaluation's buffers
        self._capture(warmup, lambda out: self._start(0), lambda: None)

    def _make_args(self, k):
        a = fill_args(_C.HopArgs(), self.params)
        for name, t in (("pos", self.pos), ("vel", self.vel), ("hk", self.hk), ("mass", self.masses), ("sig", self.sig),
                        ("fixed", self.fixed), ("batch", self.inputs[1]), ("forces_keep", self.forces), ("cur_pos", self.minimum_pos),
                        ("best_pos", self.best_pos), ("ring_pos", self.ring_pos), ("ring_energy", self.ring_energy),
                        ("ring_found", self.ring_found), ("ring_visits", self.ring_visits), ("kT", self.kT), ("ediff", self.ediff),
                        ("cur_energy", self.minimum_energy), ("best_energy", self.best_energy), ("phase", self.phase),
                        ("counters", self.counters), ("epot_row", self.epot[k]), ("fmax_row", self.fmax[k]), ("ekin_row", self.ekin[k]),
                        ("phase_row", self.phase_log[k]), ("outcome_row", self.outcome[k]), ("sums_row", self.sums[k]),
                        ("coef_row", self.coef[k])):
            setattr(a, name, None if t is None else t.data_ptr())
        return a

    def _evaluate(self):
        z, batch, box, q = self.inputs
        return self._model.energy_and_forces(z, self.pos, batch, box, q, self.n_mol, want_forces=True)

    def _capture_step(self, k, K, out):
        """The launches that follow evaluation k of a replay (inside the capture)"""
        self._advance(out[0], out[1], k)

    def _advance(self, energy, forces, k):
        st = self._model._engine
        dev = self.pos.device
        a = self._args[k]
        a.energy, a.forces = energy.data_ptr(), forces.data_ptr()
        rc = _C.lib().tmdnet_hop_advance(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), self.n_atoms, self.n_mol,
                                         C.byref(a))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_hop_advance: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def step_eager(self, k: int = 0):
        """One step issued from the host - an evaluation and ``tmdnet_hop_advance`` - writing row ``k`` of the logs: what a replay
        does ``steps_per_replay`` times without the host.  For tests and ``tools/hop_bench.py``."""
        self._check_fresh()
        energy, forces = self._evaluate()
        with torch.cuda.device(self.pos.device):
            self._advance(energy, forces, int(k))
        self.steps_done += 1
        return self

    def _start(self, keep):
        dev = self.pos.device
        a = self._args[0]
        rc = _C.lib().tmdnet_hop_reset(_stream_ptr(dev), _ptr(self._ws), self.n_atoms, self.n_mol, C.byref(a), 0, _ptr(self._kT0),
                                       _ptr(self._ediff0), int(keep))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_hop_reset failed (code {rc})")

    def run(self, hops: int, max_steps: int) -> int:
        """Replay until every walker has finished ``hops`` more hops than it had when this was called, or another replay would exceed
        ``max_steps`` steps; ``n_hops`` is read back (one synchronisation) before every replay.  Steps come in whole replays of
        ``steps_per_replay``.  Returns the number of steps taken by this call; ``check()`` tells whether they were valid."""
        K = self.steps_per_replay
        goal = self.n_hops.clone() + int(hops)
        taken = 0
        while not bool((self.n_hops >= goal).all()) and taken + K <= int(max_steps):
            self(1)
            taken += K
        return taken

    def check(self) -> int:
        """Read the device's step counter and status (one synchronisation).  Raises the reference's overflow RuntimeError when an
        evaluation found more neighbours than ``max_num_neighbors`` allows, and a RuntimeError naming the energies and forces when an
        energy or a sum of a walker was not finite: ``pos`` / ``vel``, the walkers' state, the logs and the counter are then those
        of the last valid step, and replays change nothing until ``reset``.  Returns the step counter."""
        rc, (step, status) = self._status(_C.lib().tmdnet_hop_status, 2)
        why = ("an energy or a sum over the forces, velocities or positions of a walker is not finite (a NaN or an infinite energy or "
               "force)")
        return self._verdict("tmdnet_hop_status", rc, step, status, 0, "minima hopping", {0: why})

    def reset(self, pos: Optional[Tensor] = None, kT=None, ediff=None, history: str = "clear"):
        """New start geometries (copied into the static buffer; None: the positions as they are), velocity zero, every walker back
        in the quench of its start geometry with ``kT`` and ``ediff`` (a number or [B]; None: the values of the capture), status
        cleared, step counter zero.  ``history="clear"`` empties the ring, ``best`` and the counters; ``"keep"`` leaves them, and a
        start geometry whose minimum the ring already holds is not recorded twice."""
        if history not in ("clear", "keep"):
            raise ValueError(f"history must be 'clear' or 'keep', got {history!r}")
        dev, B = self.pos.device, self.n_mol

        def staged(value, default, name):
            if value is None:
                return torch.full((B,), default, dtype=torch.float64, device=dev)
            t = torch.as_tensor(value, dtype=torch.float64).detach().to(dev).reshape(-1)
            if t.numel() not in (1, B) or not bool((torch.isfinite(t) & (t > 0)).all()):
                raise ValueError(f"reset({name}=) needs one positive value or one per walker ({B}), got {value}")
            return t.expand(B).contiguous()

        def copy_in():
            kT0, ediff0 = staged(kT, self.params["kT0"], "kT"), staged(ediff, self.params["ediff0"], "ediff")
            if pos is not None and tuple(pos.shape) != tuple(self.pos.shape):
                raise ValueError(f"reset(pos=) needs {tuple(self.pos.shape)}, got {tuple(pos.shape)}")
            if pos is not None:
                self.pos.copy_(pos.detach().to(device=dev, dtype=torch.float32))
            self._kT0.copy_(kT0)
            self._ediff0.copy_(ediff0)
            self.vel.zero_()
            if history == "clear":
                for t in (self.ring_pos, self.ring_energy, self.ring_found, self.ring_visits, self.best_pos, self.minimum_pos):
                    t.zero_()

        return self._reset(copy_in, lambda out: self._start(history == "keep"))

    def minima(self, b: int) -> dict:
        """The live ring entries of walker ``b``, lowest energy first, on the CPU (one synchronisation): ``energy`` [L] fp64, ``pos``
        [L,n_b,3] fp32 (the walker's atoms in the caller's order), ``found_at`` and ``visits`` [L] int64."""
        b = int(b)
        if not 0 <= b < self.n_mol:
            raise ValueError(f"walker {b} is outside 0..{self.n_mol - 1}")
        live = min(int(self.counters[b, 6]), self.params["capacity"])
        e = self.ring_energy[b, :live].cpu()
        order = torch.argsort(e, stable=True)
        atoms = (self.inputs[1] == b).nonzero().reshape(-1)
        pos = self.ring_pos[:live][:, atoms].cpu()
        return dict(energy=e[order], pos=pos[order], found_at=self.ring_found[b, :live].cpu()[order],
                    visits=self.ring_visits[b, :live].cpu()[order])
