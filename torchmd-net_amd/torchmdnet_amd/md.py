"""Device-resident molecular dynamics: K full MD steps per HIP graph launch (``TorchMD_Net.capture_md``).

One step is half-kick, drift, neighbour list + energy + forces, half-kick, optional Langevin O step and the energy bookkeeping; the
integrator runs as HIP kernels (csrc/tn_md.hip, ``tmdnet_md_advance``) inside the captured graph, between the evaluations, so
nothing is issued from the host between two steps.  With ``barostat=`` every step ends with an isotropic stochastic-cell-rescaling
move per molecule (``tmdnet_md_barostat``): box, positions and velocities are scaled inside the graph (NPT).  The scheme, its
rounding contract and the noise generator are documented with the C entries in include/tmdnet_amd.h and in DESIGN.md section 13."""
import ctypes as C
import math
from typing import Optional

import torch
from torch import Tensor

from torchmdnet_amd import _C
from torchmdnet_amd.models.utils import _ptr, _stream_ptr

MD_OPEN, MD_MIDDLE, MD_CLOSE = 0, 1, 2  # TMDNET_MD_* of include/tmdnet_amd.h

#: eV / (Angstrom amu) in Angstrom / fs^2: ``force_scale`` for energies in eV, lengths in Angstrom, masses in amu and dt in fs
FORCE_SCALE_EV_A_AMU_FS = 9.648533e-3
#: 1 bar in eV / Angstrom^3: the barostat's ``pressure`` (and 1 / ``compressibility``) for energies in eV and lengths in Angstrom
BAR_IN_EV_PER_A3 = 6.2415091e-7

_BAROSTAT_KEYS = ("pressure", "tau", "compressibility", "kT", "seed")


def parse_barostat(barostat, thermostat):
    """``barostat=dict(pressure=, tau=, compressibility=, kT=, seed=)`` -> the same with every key present.  ``kT`` defaults to the
    thermostat's and is required without one; ``seed`` defaults to the thermostat's seed, or 0.  Raises ValueError."""
    b = dict(barostat)
    unknown = set(b) - set(_BAROSTAT_KEYS)
    if unknown:
        raise ValueError(f"barostat: unknown keys {sorted(unknown)} ({', '.join(_BAROSTAT_KEYS)})")
    for key in ("pressure", "tau", "compressibility"):
        if key not in b:
            raise ValueError(f"barostat: '{key}' is required")
    th = thermostat or {}
    if "kT" not in b:
        if "kT" not in th:
            raise ValueError("barostat: 'kT' is required when there is no thermostat to take it from (0: weak coupling, no noise)")
        b["kT"] = th["kT"]
    b.setdefault("seed", th.get("seed", 0))
    out = {k: float(b[k]) for k in ("pressure", "tau", "compressibility", "kT")}
    out["seed"] = int(b["seed"]) & (2 ** 64 - 1)
    if not out["tau"] > 0 or not out["compressibility"] > 0 or not out["kT"] >= 0:
        raise ValueError(f"barostat: tau and compressibility must be positive and kT must not be negative, got {out}")
    return out


class DeviceMD:
    """The object ``TorchMD_Net.capture_md`` returns.  ``md(n)`` replays the captured graph n times (``steps_per_replay`` steps
    each) and returns ``md``; nothing is read back.  Static tensors, rewritten by every replay: ``pos``, ``vel``, ``forces``
    [N,3] at the last completed step, ``epot`` and ``ekin`` [K,B] of the last replay's steps (``ekin`` = sum of 0.5 m v^2 in the
    unit of m v^2: divide by ``force_scale`` for the unit of ``epot``).  ``steps_done`` counts on the host; ``check()`` reads the
    device (one synchronisation).  With a barostat: ``box`` is the static box the graph reads AND writes (the caller's own object
    when it needed no conversion), and ``volume`` (before the move), ``pressure`` and ``scale`` (the fp32 factor mu) [K,B] are the
    barostat's logs of the last replay's steps; ``forces`` stay the forces of the last evaluation, at the positions before the move."""

    def __init__(self, model, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, thermostat, warmup,
                 barostat=None):
        L = _C.lib()
        dev = pos.device
        n = int(z.shape[0])
        self._model = model
        self.steps_per_replay = K = int(steps_per_replay)
        self.n_atoms, self.n_mol = n, n_mol
        self.dt, self.force_scale = float(dt), float(force_scale)
        self.inputs = (z, batch, box, q)  # what the graph reads, kept alive for as long as it can be replayed
        self.pos = pos.detach().to(torch.float32).clone().contiguous()
        self.vel = vel.detach().to(device=dev, dtype=torch.float32).clone().contiguous()
        if self.vel.shape != self.pos.shape:
            raise ValueError(f"vel {tuple(self.vel.shape)} must have the shape of pos {tuple(self.pos.shape)}")
        m64 = masses.detach().to(device=dev, dtype=torch.float64).reshape(-1)
        if m64.numel() != n:
            raise ValueError(f"masses must have one entry per atom ({n}), got {m64.numel()}")
        # per-atom constants in fp64, rounded once: hk = dt force_scale / (2 m), sigma = sqrt(kT force_scale / m); m = inf -> 0
        self.masses = m64.to(torch.float32).contiguous()
        self.hk = (0.5 * self.dt * self.force_scale / m64).to(torch.float32).contiguous()
        self.thermostat = None if thermostat is None else dict(thermostat)
        self.sigma, self.c1, self.c2, self.seed = None, 1.0, 0.0, 0
        if self.thermostat is not None:
            unknown = set(self.thermostat) - {"friction", "kT", "seed"}
            if unknown:
                raise ValueError(f"thermostat: unknown keys {sorted(unknown)} (friction, kT, seed)")
            self.c1 = math.exp(-float(self.thermostat["friction"]) * self.dt)
            self.c2 = math.sqrt(1.0 - self.c1 * self.c1)
            self.seed = int(self.thermostat.get("seed", 0)) & (2 ** 64 - 1)
            self.sigma = torch.sqrt(float(self.thermostat["kT"]) * self.force_scale / m64).to(torch.float32).contiguous()
        self.epot = torch.zeros((K, n_mol), dtype=torch.float32, device=dev)
        self.ekin = torch.zeros((K, n_mol), dtype=torch.float32, device=dev)
        self.barostat = None if barostat is None else parse_barostat(barostat, self.thermostat)
        self.box = box
        if self.barostat is not None:
            self.volume, self.pressure, self.scale = (torch.zeros((K, n_mol), dtype=torch.float32, device=dev) for _ in range(3))
            nbytes = C.c_size_t(0)
            L.tmdnet_md_barostat_workspace_bytes(n_mol, C.byref(nbytes))
            self._baro_ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        nbytes = C.c_size_t(0)
        L.tmdnet_md_workspace_bytes(n, n_mol, C.byref(nbytes))
        self._ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        self.steps_done = 0
        with torch.cuda.device(dev):
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(max(warmup, 1)):  # uploads parameters, sizes the workspaces, checks overflow
                    f0 = self._evaluate()[1]
                self.forces = f0.clone()  # forces at the initial positions: what the first OPEN launch reads
                L.tmdnet_md_reset(_stream_ptr(dev), _ptr(self._ws), 0)
            torch.cuda.current_stream(dev).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            self._step_outputs = []  # the evaluations' output buffers live in the graph's pool; kept for the graph's lifetime
            with torch.cuda.graph(self.graph):
                self._advance(MD_OPEN, self.forces, None, 0)
                for k in range(K):
                    out = self._evaluate()
                    self._step_outputs.append(out)
                    if self.barostat is None:
                        self._advance(MD_MIDDLE if k + 1 < K else MD_CLOSE, out[1], out[0], k)
                    else:  # the kinetic energy of the closing half is reduced before the move: CLOSE, then scale (and open)
                        self._advance(MD_CLOSE, out[1], out[0], k)
                        self._barostat_move(k + 1 < K, out[1], out[2], k)
        self._engine, self._generation = model._engine, model._engine.generation

    def _evaluate(self):
        z, batch, box, q = self.inputs
        return self._model.energy_and_forces(z, self.pos, batch, box, q, self.n_mol, want_forces=True,
                                             want_virial=self.barostat is not None)

    def _advance(self, phase, forces, energy, k):
        st = self._model._engine
        dev = self.pos.device
        rc = _C.lib().tmdnet_md_advance(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), self.n_atoms, self.n_mol, phase,
                                        _ptr(self.pos), _ptr(self.vel), _ptr(forces), _ptr(energy), _ptr(self.hk), _ptr(self.masses),
                                        _ptr(self.sigma), self.dt, self.c1, self.c2, self.seed, _ptr(self.inputs[1]),
                                        None if phase == MD_OPEN else _ptr(self.forces), _ptr(self.epot[k]), _ptr(self.ekin[k]))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_md_advance: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def _barostat_move(self, open_next, forces, virial, k):
        st = self._model._engine
        dev = self.pos.device
        b = self.barostat
        rc = _C.lib().tmdnet_md_barostat(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), _ptr(self._baro_ws),
                                         self.n_atoms, self.n_mol, int(open_next), _ptr(self.pos), _ptr(self.vel), _ptr(forces),
                                         _ptr(self.hk), self.dt, _ptr(self.inputs[1]), _ptr(self.box), 1 if self.box.dim() == 2 else 2,
                                         _ptr(virial), _ptr(self.ekin[k]), b["pressure"], b["kT"], b["compressibility"], b["tau"],
                                         self.force_scale, b["seed"], _ptr(self.volume[k]), _ptr(self.pressure[k]), _ptr(self.scale[k]))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_md_barostat: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def _check_fresh(self):
        # the graph holds raw pointers into the engine's parameter block and workspaces (TorchMD_Net.capture's replay)
        if self._model._engine is not self._engine or self._engine.generation != self._generation:
            raise RuntimeError("stale HIP graph: the model's parameters or workspaces changed after capture_md(); capture again")

    def __call__(self, n: int = 1):
        self._check_fresh()
        for _ in range(int(n)):
            self.graph.replay()
        self.steps_done += int(n) * self.steps_per_replay
        return self

    def check(self) -> int:
        """Read the device's step counter and status (one synchronisation).  Raises the reference's overflow RuntimeError when an
        evaluation found more neighbours than ``max_num_neighbors`` allows: ``pos`` / ``vel`` / ``forces`` (and ``box``) and the
        counter are then those of the last valid step, and replays change nothing until ``reset``.  Raises a RuntimeError naming
        the barostat when one of its moves was unusable (zero volume, or a NaN from the virial): the state is frozen before that
        move.  Returns the step counter."""
        host = (C.c_uint64 * 2)()
        dev = self.pos.device
        with torch.cuda.device(dev):
            rc = _C.lib().tmdnet_md_status(_stream_ptr(dev), _ptr(self._ws), host)
        if rc == _C.ERR_OVERFLOW:
            raise RuntimeError("Found num_pairs > max_num_pairs, please increase max_num_pairs "
                               f"(max_num_neighbors={self._model.representation_model.max_num_neighbors}; the MD state is frozen at "
                               f"step {int(host[0])})")
        if int(host[1]) == 2:
            raise RuntimeError(f"barostat: the move after step {int(host[0])} was not finite (zero volume, or a NaN in the virial or "
                               "the kinetic energy); the MD state is frozen before that move")
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_md_status failed (code {rc})")
        return int(host[0])

    def reset(self, pos: Optional[Tensor] = None, vel: Optional[Tensor] = None, step: int = 0, box: Optional[Tensor] = None):
        """New positions and / or velocities (copied into the static buffers), forces evaluated there, status cleared, device step
        counter and ``steps_done`` set to ``step`` (the Langevin noise is a function of (seed, step, atom)).  ``box`` is copied into
        the static box (a barostat has scaled it since the capture)."""
        self._check_fresh()
        dev = self.pos.device
        if box is not None:
            if self.box is None:
                raise ValueError("reset(box=...): this loop was captured without a box")
            self.box.copy_(box.detach().to(device=dev, dtype=torch.float32).reshape(self.box.shape))
        if pos is not None:
            self.pos.copy_(pos.detach().to(device=dev, dtype=torch.float32))
        if vel is not None:
            self.vel.copy_(vel.detach().to(device=dev, dtype=torch.float32))
        f = self._evaluate()[1]  # raises when these positions overflow
        self.forces.copy_(f)
        with torch.cuda.device(dev):
            _C.lib().tmdnet_md_reset(_stream_ptr(dev), _ptr(self._ws), int(step))
        self.steps_done = int(step)
        self._check_fresh()  # the evaluation must not have re-created what the graph points into
        return self
