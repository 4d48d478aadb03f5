"""Committees of models on the device: ``Ensemble.committee`` / ``Ensemble.capture`` / ``Ensemble.capture_md``.

Every member is an engine of its own (its architecture, cutoff, priors and workspaces); its ``energy_and_forces`` runs on the current
stream, one member after the other, and ONE pass (csrc/tn_committee.hip, ``tmdnet_committee_reduce``: two launches) reduces the M
outputs in place: the mean and the unbiased standard deviation of the energies and of every force component, the deviation of atom i
``d_i = sqrt(sum_c std_i,c^2)`` and per molecule ``D_m = max_i d_i`` with the smallest atom index ``a_m`` that attains it.  Sums and
square roots are fp64 (two passes: the mean, then the squared differences), every output is rounded to fp32 once.  The definitions,
their corner cases (a deviation that is not finite is +inf, an empty molecule has D = 0 and a = -1) and the launch list are in
include/tmdnet_amd.h and DESIGN.md.

``DeviceCommitteeMD`` is the device-resident MD loop driven by the committee mean, with a gate on ``D_m`` inside the captured step:
``flag_above`` harvests the first configuration at which a molecule's members disagree, ``stop_above`` freezes the loop at the
completed step (sticky status 6, a result and not an error)."""
import ctypes as C
import math
import struct
from collections import namedtuple
from typing import Optional

import torch
from torch import Tensor

from torchmdnet_amd import _C
from torchmdnet_amd.captured import capture_graph, check_fresh, engine_token
from torchmdnet_amd.md import MD_CLOSE, MD_OPEN, DeviceMD
from torchmdnet_amd.models.utils import _ptr, _stream_ptr

#: what ``Ensemble.committee`` and the replays of ``Ensemble.capture`` return: energy, energy_std, max_deviation [B], max_atom [B]
#: int64, forces, forces_std [N,3], deviation [N]
CommitteeResult = namedtuple("CommitteeResult", "energy forces energy_std forces_std deviation max_deviation max_atom")

MAX_MEMBERS = _C.COMMITTEE_MAX_MEMBERS
_GATE_KEYS = ("flag_above", "stop_above")


def check_members(members, name, captured=False, atom_weights=None, halo_exchange=None):
    """What a committee cannot serve, refused on the host before anything is launched (no GPU is needed to refuse)"""
    members = list(members)
    if not 2 <= len(members) <= MAX_MEMBERS:
        raise ValueError(f"{name}: a committee has 2 to {MAX_MEMBERS} members, this ensemble has {len(members)} (the unbiased spread "
                         "needs two, and the members' output pointers travel in the launch arguments)")
    devices = sorted({str(next(m.parameters()).device) for m in members})
    if len(devices) > 1:
        raise ValueError(f"{name}: the members are on different devices ({', '.join(devices)}); the pass reads all of them on one GPU")
    if atom_weights is not None or halo_exchange is not None:
        raise NotImplementedError(f"{name} has no HIP path with atom weights or the halo exchange (domain decomposition)")
    for k, m in enumerate(members):
        if m._head_kind() != _C.HEAD_SCALAR:
            raise NotImplementedError(f"{name}: member {k} has output_model {type(m.output_model).__name__}; a committee reduces "
                                      "energies and their forces (scalar head)")
        if m.parameter_gradients:
            raise NotImplementedError(f"{name}: member {k} was created with parameter_gradients=True (a training model); create it "
                                      "without it")
        if captured and not getattr(m.representation_model, "static_shapes", False):
            raise ValueError(f"{name}: member {k} was created without static_shapes=True; a captured graph needs static shapes in "
                             "every member")
    return members


def parse_gate(gate):
    """``gate=dict(flag_above=None | float, stop_above=None | float)`` -> (flags, flag_above, stop_above).  Raises ValueError."""
    g = dict(gate or {})
    unknown = set(g) - set(_GATE_KEYS)
    if unknown:
        raise ValueError(f"gate: unknown keys {sorted(unknown)} ({', '.join(_GATE_KEYS)})")
    flags, values = 0, []
    for key, bit in zip(_GATE_KEYS, (_C.COMMITTEE_FLAG, _C.COMMITTEE_STOP)):
        v = g.get(key)
        if v is not None:
            v = float(v)
            if math.isnan(v):
                raise ValueError(f"gate: {key} must not be NaN")
            flags |= bit
        values.append(0.0 if v is None else v)
    return flags, values[0], values[1]


class CommitteePass:
    """The reduction over M members' outputs for n_atoms atoms in n_mol molecules on ``dev``: the zeroed workspace and the call"""

    def __init__(self, n_members, n_atoms, n_mol, dev):
        self.n_members, self.n_atoms, self.n_mol, self.dev = int(n_members), int(n_atoms), int(n_mol), dev
        nbytes = C.c_size_t(0)
        rc = _C.lib().tmdnet_committee_workspace_bytes(self.n_atoms, self.n_mol, C.byref(nbytes))
        if rc != _C.OK:
            raise ValueError(f"tmdnet_committee_workspace_bytes: {n_atoms} atoms in {n_mol} molecules are out of range (code {rc})")
        self.ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)

    def __call__(self, outs, batch, rows=None, members=None, gate=None) -> CommitteeResult:
        """``outs``: the members' (E [B], F [N,3]) fp32 on the device.  ``rows``: (energy_std, max_deviation, max_atom) [B] to write
        instead of new tensors (a loop's log rows).  ``members``: the models, when their overflow flags are to be folded into the
        first one's (static shapes, inside a captured step).  ``gate``: a ``_C.CommitteeGate`` or None."""
        M, n, B, dev = self.n_members, self.n_atoms, self.n_mol, self.dev
        if len(outs) != M:
            raise ValueError(f"the pass was sized for {M} members, got {len(outs)}")
        for e, f in outs:
            if e.dtype != torch.float32 or f.dtype != torch.float32 or e.numel() != B or f.numel() != 3 * n or e.device != dev \
                    or f.device != dev or not e.is_contiguous() or not f.is_contiguous():
                raise ValueError("every member's energy [B] and forces [N,3] must be contiguous fp32 tensors on the pass's device")
        f32 = dict(dtype=torch.float32, device=dev)
        energy, forces = torch.empty(B, **f32), torch.empty((n, 3), **f32)
        forces_std, deviation = torch.empty((n, 3), **f32), torch.empty(n, **f32)
        if rows is None:
            rows = torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, dtype=torch.int64, device=dev)
        energy_std, max_dev, max_atom = rows
        ptrs = lambda ts: (C.c_void_p * M)(*[t.data_ptr() for t in ts])
        handles = graphs = None
        if members is not None:
            handles = (C.c_void_p * M)(*[m._engine.handle.value for m in members])
            graphs = ptrs([m._engine.graph_ws for m in members])
        with torch.cuda.device(dev):
            rc = _C.lib().tmdnet_committee_reduce(_stream_ptr(dev), _ptr(self.ws), self.ws.numel(), M, ptrs([e for e, _ in outs]),
                                                  ptrs([f for _, f in outs]), n, B, _ptr(batch), _ptr(energy), _ptr(forces),
                                                  _ptr(energy_std), _ptr(forces_std), _ptr(deviation), _ptr(max_dev), _ptr(max_atom),
                                                  handles, graphs, None if gate is None else C.byref(gate))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_committee_reduce failed (code {rc})")
        return CommitteeResult(energy, forces, energy_std, forces_std, deviation, max_dev, max_atom)


def _member_inputs(members, name, needs, z, pos, batch, box, q, num_systems, steps_per_replay=1):
    """``TorchMD_Net._capture_inputs`` of every member (each keeps its own box) -> ([(z, batch, box, q)], n_mol, dev)"""
    staged, n_mol, dev = [], num_systems, None
    for m in members:
        zk, bk, boxk, qk, n_mol, dev = m._capture_inputs(name, needs, z, pos, batch, box, q, n_mol, steps_per_replay)
        staged.append((zk, bk, boxk, qk))
    return staged, n_mol, dev


def committee(ensemble, z, pos, batch=None, box=None, q=None, num_systems=None, atom_weights=None, halo_exchange=None):
    """``Ensemble.committee``"""
    from torchmdnet_amd.models.model import _require_cuda

    members = check_members(ensemble, "Ensemble.committee", False, atom_weights, halo_exchange)
    if pos.dtype != torch.float32:
        raise NotImplementedError("torchmdnet_amd computes in fp32; cast positions to float32")
    _require_cuda(pos, "Ensemble.committee")
    dev = pos.device
    batch = torch.zeros_like(z) if batch is None else batch
    n_mol = int(num_systems) if num_systems is not None else (int(batch.max().item()) + 1 if z.numel() else 0)
    batch = batch.to(torch.long).contiguous()
    outs = []
    for m in members:
        rm = m.representation_model
        outs.append(m.energy_and_forces(z, pos, batch, rm.distance.box if box is None and rm.distance.use_periodic else box, q, n_mol))
    key = (len(members), int(z.shape[0]), n_mol, dev)
    cache = ensemble.__dict__.setdefault("_committee_pass", {})
    if key not in cache:
        cache.clear()  # one workspace: that of the last system
        cache[key] = CommitteePass(*key)
    return cache[key](outs, batch)


def capture(ensemble, z, pos, batch=None, box=None, q=None, num_systems=None, warmup=3, atom_weights=None, halo_exchange=None):
    """``Ensemble.capture``"""
    members = check_members(ensemble, "Ensemble.capture", True, atom_weights, halo_exchange)
    staged, n_mol, dev = _member_inputs(members, "Ensemble.capture", "a committee needs", z, pos, batch, box, q, num_systems)
    s_pos = pos.detach().clone().contiguous()
    reduce = CommitteePass(len(members), int(z.shape[0]), n_mol, dev)
    kept = []

    def evaluate():
        outs = [m.energy_and_forces(zk, s_pos, bk, boxk, qk, n_mol) for m, (zk, bk, boxk, qk) in zip(members, staged)]
        return outs, reduce(outs, staged[0][1])

    graph = capture_graph(dev, evaluate, lambda: kept.append(evaluate()), warmup)
    result = kept[0][1]
    tokens = [engine_token(m) for m in members]

    def replay(new_pos: Optional[Tensor] = None) -> CommitteeResult:
        for m, t in zip(members, tokens):
            check_fresh(engine_token(m), t, "Ensemble.capture()")
        if new_pos is not None:
            torch.mul(new_pos.detach(), 1.0, out=s_pos)  # (an elementwise kernel, as in TorchMD_Net.capture)
        graph.replay()
        return result

    replay.graph, replay.pos, replay.inputs = graph, s_pos, staged
    replay.workspace = reduce.ws  # the graph points into it: kept alive for as long as it can be replayed, like the inputs
    replay.member_outputs = kept[0][0]  # the members' own static (E, F), in member order
    replay.n_atoms, replay.n_mol = int(z.shape[0]), n_mol
    return replay


class DeviceCommitteeMD(DeviceMD):
    """The object ``Ensemble.capture_md`` returns: ``DeviceMD``'s surface, driven by the committee mean of the forces, ``epot`` the
    committee mean of the energies.  Logs of the last replay's steps [K,B]: ``energy_std``, ``deviation`` (D_m) and
    ``deviation_atom`` (a_m, int64).  Gate state: ``flagged_at`` [B] int64 (the step at which molecule m was first flagged, -1
    before; steps count from 1 after ``reset(step=0)``, as ``check()`` counts them), ``flagged_pos`` [N,3] (the molecule's atoms at
    that step; other rows as they were), ``flagged_dev`` / ``flagged_atom`` [B], and ``stopped``.

    Per step inside the graph: the M evaluations in member order on the capturing stream, the pass, ``TMDNET_MD_CLOSE`` with the
    committee's forces and energies, the latch (``tmdnet_committee_latch``) and, when another step follows, ``TMDNET_MD_OPEN`` on the
    kept forces.  ``TMDNET_MD_MIDDLE`` is CLOSE then OPEN on the same values, so a committee of copies of one model reproduces that
    model's ``capture_md`` bit for bit.  An overflowed neighbour list in ANY member freezes the loop as in ``DeviceMD`` (status 1)."""

    _capture_name, _noun = "Ensemble.capture_md", "the MD state"

    def __init__(self, members, staged, z, pos, vel, masses, dt, n_mol, steps_per_replay, force_scale, thermostat, warmup, gate):
        dev, n, K = pos.device, int(z.shape[0]), int(steps_per_replay)
        self._members, self._staged = members, staged
        self._gate_values = parse_gate(gate)
        self._pass = CommitteePass(len(members), n, n_mol, dev)
        self._gate, self._kept = None, []
        self.energy_std = torch.zeros((K, n_mol), dtype=torch.float32, device=dev)
        self.deviation = torch.zeros((K, n_mol), dtype=torch.float32, device=dev)
        self.deviation_atom = torch.full((K, n_mol), -1, dtype=torch.int64, device=dev)
        self.flagged_at = torch.full((n_mol,), -1, dtype=torch.int64, device=dev)
        self.flagged_atom = torch.full((n_mol,), -1, dtype=torch.int64, device=dev)
        self.flagged_dev = torch.zeros(n_mol, dtype=torch.float32, device=dev)
        self.flagged_pos = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        zk, bk, boxk, qk = staged[0]
        super().__init__(members[0], zk, pos, vel, masses, dt, bk, boxk, qk, n_mol, steps_per_replay, force_scale, thermostat, warmup)
        self._tokens = [engine_token(m) for m in members]

    def _gate_struct(self):
        if self._gate is None:  # (the MD workspace exists once DeviceMD's constructor has staged it)
            flags, flag_above, stop_above = self._gate_values
            self._gate = _C.CommitteeGate(flags, flag_above, stop_above, self._ws.data_ptr(), self.flagged_at.data_ptr(),
                                          self.flagged_dev.data_ptr(), self.flagged_atom.data_ptr(), self.flagged_pos.data_ptr())
        return self._gate

    def _member_outputs(self):
        return [m.energy_and_forces(zk, self.pos, bk, boxk, qk, self.n_mol)
                for m, (zk, bk, boxk, qk) in zip(self._members, self._staged)]

    def _evaluate(self):
        """Outside a capture (warm-up, ``reset``): the committee's (E, F) at ``pos``, ungated and whatever the loop's status; every
        member polls its own overflow flag there.  Inside: the members' outputs, which ``_capture_step`` reduces into the log rows."""
        outs = self._member_outputs()
        if torch.cuda.is_current_stream_capturing():
            return outs
        res = self._pass(outs, self.inputs[1])
        return res.energy, res.forces

    def _capture_step(self, k, K, outs):
        res = self._pass(outs, self.inputs[1], (self.energy_std[k], self.deviation[k], self.deviation_atom[k]), self._members,
                         self._gate_struct())
        self._kept.append(res)  # the graph's pool holds them; kept for the graph's lifetime
        self._advance(MD_CLOSE, res.forces, res.energy, k)
        dev = self.pos.device
        with torch.cuda.device(dev):
            rc = _C.lib().tmdnet_committee_latch(_stream_ptr(dev), _ptr(self._pass.ws), self.n_atoms, self.n_mol, _ptr(self.inputs[1]),
                                                 _ptr(self.pos), _ptr(self.deviation_atom[k]), C.byref(self._gate_struct()))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_committee_latch failed (code {rc})")
        if k + 1 < K:
            self._advance(MD_OPEN, self.forces, None, 0)

    def _start(self, step):
        dev = self.pos.device
        with torch.cuda.device(dev):
            _C.lib().tmdnet_committee_reset(_stream_ptr(dev), _ptr(self._pass.ws), self.n_mol)

    def _check_fresh(self):
        for m, t in zip(self._members, getattr(self, "_tokens", ())):
            check_fresh(engine_token(m), t, f"{self._capture_name}()")

    @property
    def stopped(self):
        """None, or (step, molecule, atom, value) of the stop: the completed step at which the loop froze, the molecule of the largest
        D_m above ``stop_above`` (the smallest index among equals), its atom a_m and D_m.  One synchronisation."""
        host = (C.c_uint64 * 5)()
        dev = self.pos.device
        with torch.cuda.device(dev):
            rc = _C.lib().tmdnet_committee_status(_stream_ptr(dev), _ptr(self._pass.ws), C.cast(host, C.POINTER(C.c_uint64)))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_committee_status failed (code {rc})")
        if not host[0]:
            return None
        atom = int(host[3]) - (1 << 64) if int(host[3]) >> 63 else int(host[3])
        return int(host[1]), int(host[2]), atom, struct.unpack("<f", struct.pack("<I", int(host[4]) & 0xffffffff))[0]

    def check(self) -> int:
        """``DeviceMD.check`` - the reference's overflow error when ANY member's neighbour list overflowed - except that a stop of
        the gate (status 6) is a result and not an error: the step counter is returned and ``stopped`` tells the rest."""
        rc, (step, status) = self._status(_C.lib().tmdnet_md_status, 2)
        if status == 6:
            return step
        return super().check()

    def run(self, max_steps: int, check_every: int = 1) -> int:
        """Replay until the gate has stopped the loop or another replay would exceed ``max_steps`` steps; ``stopped`` is read back
        (one synchronisation) before the first replay and then after every ``check_every`` replays.  Steps come in whole replays
        of ``steps_per_replay``.  Returns the number of steps enqueued by this call; ``check()`` gives the device's counter."""
        K, every = self.steps_per_replay, max(int(check_every), 1)
        taken = 0
        while self.stopped is None:
            n = min(every, (int(max_steps) - taken) // K)
            if n < 1:
                break
            self(n)
            taken += n * K
        return taken

    def reset(self, pos: Optional[Tensor] = None, vel: Optional[Tensor] = None, step: int = 0, flags: str = "keep"):
        """``DeviceMD.reset`` (the committee's forces at the new positions, status and stop record cleared).  ``flags="keep"`` leaves
        ``flagged_at / flagged_pos / flagged_dev / flagged_atom`` as they are - a flagged molecule is not flagged again -,
        ``"clear"`` starts them over."""
        if flags not in ("keep", "clear"):
            raise ValueError(f"reset(flags=...) must be 'keep' or 'clear', got {flags!r}")
        super().reset(pos, vel, step)
        if flags == "clear":
            self.flagged_at.fill_(-1)
            self.flagged_atom.fill_(-1)
            self.flagged_dev.zero_()
            self.flagged_pos.zero_()
        return self


def capture_md(ensemble, z, pos, vel, masses, dt, batch=None, box=None, q=None, num_systems=None, steps_per_replay=10, force_scale=1.0,
               thermostat=None, warmup=3, gate=None, atom_weights=None, halo_exchange=None, barostat=None, constraints=None, bias=None,
               temperatures=None):
    """``Ensemble.capture_md``"""
    name = "Ensemble.capture_md"
    members = check_members(ensemble, name, True, atom_weights, halo_exchange)
    for what, value, why in (("a barostat", barostat, "the committee has no virial"), ("constraints", constraints,
                             "the constrained integrator is not wired to the committee's forces"),
                             ("a bias", bias, "the bias launch is not wired in"),
                             ("replica exchange", temperatures, "the exchange launch is not wired in")):
        if value is not None:
            raise NotImplementedError(f"{name} has no HIP path with {what} in this version: {why}")
    if thermostat is not None and ("kind" in thermostat or "tau" in thermostat):
        raise NotImplementedError(f"{name} has no HIP path with a global thermostat (CSVR, Nose-Hoover) in this version: None or "
                                  "Langevin, thermostat=dict(friction=, kT=, seed=)")
    parse_gate(gate)
    staged, n_mol, _ = _member_inputs(members, name, "molecular dynamics needs", z, pos, batch, box, q, num_systems, steps_per_replay)
    return DeviceCommitteeMD(members, staged, z, pos, vel, masses, dt, n_mol, steps_per_replay, force_scale, thermostat, warmup, gate)
