"""Device-resident molecular dynamics: K full MD steps per HIP graph launch (``TorchMD_Net.capture_md``).

One step is half-kick, drift, neighbour list + energy + forces, half-kick, optional Langevin O step and the energy bookkeeping; the
integrator runs as HIP kernels (csrc/tn_md.hip, ``tmdnet_md_advance``) inside the captured graph, between the evaluations, so
nothing is issued from the host between two steps.  With ``barostat=`` every step ends with an isotropic stochastic-cell-rescaling
move per molecule (``tmdnet_md_barostat``): box, positions and velocities are scaled inside the graph (NPT).  The scheme, its
rounding contract and the noise generator are documented with the C entries in include/tmdnet_amd.h and in DESIGN.md section 13.
With ``constraints=`` (``TorchMD_Net.capture_md_constrained``) the integrator launches are those of csrc/tn_md_cons.hip
(``tmdnet_md_advance_constrained``): SHAKE after the drift and RATTLE after the closing kick, one group of lanes per cluster of
coupled constraints, still one launch between two evaluations.  ``TorchMD_Net.capture_remd`` (``DeviceREMD``) runs G ladders of R
replicas of one system and exchanges their temperatures inside the graph (csrc/tn_remd.hip, ``tmdnet_md_exchange``).
``TorchMD_Net.capture_md_biased`` (``DeviceBiasedMD``) adds collective-variable restraints and metadynamics: one launch per step
(csrc/tn_bias.hip, ``tmdnet_md_bias``) adds the bias force to the evaluation's forces before the integrator reads them.
``TorchMD_Net.capture_md_global`` (``DeviceGlobalMD``) replaces the Langevin O step by a global thermostat per molecule - stochastic
velocity rescaling or a Nose-Hoover chain - that scales all velocities of a molecule by one factor (csrc/tn_md_thermo.hip,
``tmdnet_md_thermostat``: two launches between the closing and the opening half of a step).
``TorchMD_Net.capture_md_cell`` (``DeviceCellMD``) lets the SHAPE of the cell fluctuate: the barostat's exponent is a 3 x 3 matrix
(anisotropic, diagonal or semi-isotropic coupling; csrc/tn_md_cell.hip, ``tmdnet_md_barostat_cell``: three launches after the closing
half), and in anisotropic mode the box is kept lower triangular by rotating positions, velocities and forces with it.
``Ensemble.capture_md`` (``torchmdnet_amd.committee.DeviceCommitteeMD``) drives the loop with the mean force of a committee of models
and gates it on the members' disagreement inside the graph (csrc/tn_committee.hip).
``TorchMD_Net.capture_md_observed`` attaches an observer (``torchmdnet_amd.observe.Observer``, csrc/tn_observe.hip) to ``DeviceMD`` or
``DeviceGlobalMD``: sample frames, g(r), MSD and the velocity autocorrelation recorded inside the graph at every S-th step, by launches
that read ``pos`` / ``vel`` and write only their own workspace (``md.frames() / rdf() / msd() / vacf() / n_samples``).
The capture sequence, the stale-graph guard, ``md(n)``, the status read-back and the skeleton of ``reset`` are those of every
captured loop: ``torchmdnet_amd.captured``."""
import ctypes as C
import math
from typing import Optional

import torch
from torch import Tensor

from torchmdnet_amd import _C
from torchmdnet_amd.captured import CapturedLoop
from torchmdnet_amd.models.utils import _ptr, _stream_ptr

MD_OPEN, MD_MIDDLE, MD_CLOSE, MD_PROJECT = 0, 1, 2, 3  # TMDNET_MD_* of include/tmdnet_amd.h
#: limits of one cluster of coupled constraints (csrc/tn_md_cons_math.h: one lane per atom of a group of 8)
MAX_CLUSTER_ATOMS, MAX_CLUSTER_CONSTRAINTS = 8, 12

#: eV / (Angstrom amu) in Angstrom / fs^2: ``force_scale`` for energies in eV, lengths in Angstrom, masses in amu and dt in fs
FORCE_SCALE_EV_A_AMU_FS = 9.648533e-3
#: 1 bar in eV / Angstrom^3: the barostat's ``pressure`` (and 1 / ``compressibility``) for energies in eV and lengths in Angstrom
BAR_IN_EV_PER_A3 = 6.2415091e-7

_BAROSTAT_KEYS = ("pressure", "tau", "compressibility", "kT", "seed")
#: ``coupling`` of the cell barostat -> TMDNET_CELL_* of include/tmdnet_amd.h
CELL_COUPLINGS = {"anisotropic": 0, "diagonal": 1, "semi-isotropic": 2}
_CONSTRAINT_KEYS = ("pairs", "lengths", "tol", "max_iter")


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


def parse_cell_barostat(barostat, thermostat):
    """``barostat=dict(pressure=, tau=, compressibility=, kT=, seed=, coupling="anisotropic", axis=2)`` of ``capture_md_cell`` -> the same
    with every key present: ``parse_barostat`` for the first five, ``coupling`` one of ``CELL_COUPLINGS`` and ``axis`` 0, 1 or 2 (the
    axis that moves on its own in "semi-isotropic" mode; ignored by the other two).  Raises ValueError."""
    if barostat is None:
        raise ValueError("capture_md_cell needs barostat=dict(pressure=, tau=, compressibility=, kT=, ...); without one use capture_md")
    b = dict(barostat)
    coupling, axis = b.pop("coupling", "anisotropic"), b.pop("axis", 2)
    out = parse_barostat(b, thermostat)
    if not all(math.isfinite(out[k]) for k in ("pressure", "tau", "compressibility", "kT")):
        raise ValueError(f"barostat: pressure, tau, compressibility and kT must be finite, got {out}")
    if coupling not in CELL_COUPLINGS:
        raise ValueError(f"barostat: coupling must be one of {', '.join(CELL_COUPLINGS)}, got {coupling!r}")
    if isinstance(axis, bool) or not isinstance(axis, int) or not 0 <= axis <= 2:
        raise ValueError(f"barostat: axis must be 0, 1 or 2, got {axis!r}")
    out.update(coupling=coupling, axis=axis)
    return out


def build_clusters(pairs, n_atoms, batch=None, masses=None):
    """Group the constraint pairs [C,2] (caller's atom order) into clusters, the connected components of the constraint graph, as
    ``tmdnet_md_advance_constrained`` takes them.  Clusters come in the order of their smallest atom, the atoms of a cluster in
    ascending order, its constraints in the caller's order; the atoms in no constraint follow, 8 to a cluster without constraints.
    -> dict of CPU tensors: ``cluster_atoms`` [n_clusters,8] int32 (-1: no atom), ``cluster_offsets`` [n_clusters+1] int32,
    ``constraint_ends`` [C,2] int32 (positions in the cluster's row), ``order`` [C] int64 (table row -> row of ``pairs``), and
    ``n_bound``, the number of clusters that have constraints.  Raises ValueError for an index out of range, i == j, a duplicate
    pair, a pair across two molecules, a constraint between two atoms of infinite mass and a cluster over 8 atoms or 12
    constraints."""
    n = int(n_atoms)
    pairs = torch.as_tensor(pairs).detach().cpu()
    if pairs.numel() == 0:
        pairs = pairs.reshape(0, 2)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype.is_floating_point:
        raise ValueError(f"constraints: pairs must be an integer tensor [C,2], got {tuple(pairs.shape)} {pairs.dtype}")
    pl = [(int(i), int(j)) for i, j in pairs.tolist()]
    bl = None if batch is None else torch.as_tensor(batch).detach().cpu().tolist()
    ml = None if masses is None else torch.as_tensor(masses).detach().cpu().reshape(-1).tolist()
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    seen = set()
    for c, (i, j) in enumerate(pl):
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError(f"constraints: pair {c} = ({i}, {j}) has an index outside 0..{n - 1}")
        if i == j:
            raise ValueError(f"constraints: pair {c} = ({i}, {j}) constrains an atom to itself")
        key = (min(i, j), max(i, j))
        if key in seen:
            raise ValueError(f"constraints: pair {c} = ({i}, {j}) is a duplicate")
        seen.add(key)
        if bl is not None and bl[i] != bl[j]:
            raise ValueError(f"constraints: pair {c} = ({i}, {j}) joins molecules {bl[i]} and {bl[j]}")
        if ml is not None and math.isinf(ml[i]) and math.isinf(ml[j]):
            raise ValueError(f"constraints: pair {c} = ({i}, {j}) joins two atoms of infinite mass")
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)  # the root is the component's smallest atom
    members, rows = {}, {}
    for a in sorted({a for p in pl for a in p}):
        members.setdefault(find(a), []).append(a)
    for c, (i, j) in enumerate(pl):
        rows.setdefault(find(i), []).append(c)
    atoms, offsets, ends, order = [], [0], [], []
    for root in sorted(members):
        mem, cons = members[root], rows[root]
        if len(mem) > MAX_CLUSTER_ATOMS or len(cons) > MAX_CLUSTER_CONSTRAINTS:
            raise ValueError(f"constraints: the cluster of atom {root} has {len(mem)} atoms and {len(cons)} constraints (atoms {mem}); "
                             f"a cluster holds at most {MAX_CLUSTER_ATOMS} atoms and {MAX_CLUSTER_CONSTRAINTS} constraints")
        local = {a: l for l, a in enumerate(mem)}
        atoms.append(mem + [-1] * (MAX_CLUSTER_ATOMS - len(mem)))
        for c in cons:
            ends.append([local[pl[c][0]], local[pl[c][1]]])
            order.append(c)
        offsets.append(len(ends))
    n_bound = len(atoms)
    bound = {a for p in pl for a in p}
    free = [a for a in range(n) if a not in bound]
    for k in range(0, len(free), MAX_CLUSTER_ATOMS):
        mem = free[k:k + MAX_CLUSTER_ATOMS]
        atoms.append(mem + [-1] * (MAX_CLUSTER_ATOMS - len(mem)))
        offsets.append(len(ends))
    return dict(cluster_atoms=torch.tensor(atoms, dtype=torch.int32).reshape(-1, MAX_CLUSTER_ATOMS),
                cluster_offsets=torch.tensor(offsets, dtype=torch.int32),
                constraint_ends=torch.tensor(ends, dtype=torch.int32).reshape(-1, 2),
                order=torch.tensor(order, dtype=torch.int64), n_bound=n_bound)


def constraint_residuals(pos, pairs, lengths, tol):
    """Host check (fp64, one read-back): relative residual | |x_i - x_j| - d | / d of every pair and the bound it has to meet,
    tol + 2 * 2^-23 * max|x| / d - the second term is the worst case of rounding the six coordinates to fp32.  -> (res, bound) [C]"""
    x = pos.detach().to(device="cpu", dtype=torch.float64)
    pairs = pairs.detach().cpu()
    d = lengths.detach().to(device="cpu", dtype=torch.float64)
    xi, xj = x[pairs[:, 0]], x[pairs[:, 1]]
    res = ((xi - xj).norm(dim=1) - d).abs() / d
    big = torch.maximum(xi.abs().amax(1), xj.abs().amax(1))
    return res, float(tol) + 2.0 * 2.0 ** -23 * big / d


def _check_positions(pos, con):
    if con["pairs"].shape[0] == 0:
        return
    res, bound = constraint_residuals(pos, con["pairs"], con["lengths"], con["tol"])
    over = res - bound
    over = torch.where(torch.isnan(over), torch.full_like(over, float("inf")), over)
    if bool((over > 0).any()):
        c = int(over.argmax())
        i, j = con["pairs"][c].tolist()
        raise ValueError(f"constraints: the positions do not satisfy the constraints; worst is pair {c} = ({i}, {j}): "
                         f"|r| / d - 1 = {float(res[c]):.3e} against a bound of {float(bound[c]):.3e} (d = {float(con['lengths'][c]):.6g})")


def prepare_constraints(constraints, pos, batch, masses, n_mol):
    """``constraints=dict(pairs=, lengths=None, tol=1e-6, max_iter=64)`` -> everything ``DeviceMD`` needs, on the host, before
    anything is staged: the clusters (``build_clusters``), the lengths (measured from ``pos`` in fp64 when None), the degrees of
    freedom per molecule, and the check that ``pos`` satisfies the constraints.  Raises ValueError."""
    con = dict(constraints)
    unknown = set(con) - set(_CONSTRAINT_KEYS)
    if unknown:
        raise ValueError(f"constraints: unknown keys {sorted(unknown)} ({', '.join(_CONSTRAINT_KEYS)})")
    if "pairs" not in con:
        raise ValueError("constraints: 'pairs' is required")
    tol, max_iter = float(con.get("tol", 1e-6)), int(con.get("max_iter", 64))
    if not tol > 0 or max_iter < 1:
        raise ValueError(f"constraints: tol must be positive and max_iter at least 1, got tol={tol}, max_iter={max_iter}")
    n = int(pos.shape[0])
    m64 = torch.as_tensor(masses).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
    if m64.numel() != n:
        raise ValueError(f"masses must have one entry per atom ({n}), got {m64.numel()}")
    b_cpu = batch.detach().cpu()
    pairs = torch.as_tensor(con["pairs"]).detach().cpu()
    out = build_clusters(pairs, n, b_cpu, m64)
    pairs = pairs.reshape(-1, 2).to(torch.int64)
    x = pos.detach().to(device="cpu", dtype=torch.float64)
    if con.get("lengths") is None:
        lengths = (x[pairs[:, 0]] - x[pairs[:, 1]]).norm(dim=1)
    else:
        lengths = torch.as_tensor(con["lengths"]).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
        if lengths.numel() != pairs.shape[0]:
            raise ValueError(f"constraints: lengths must have one entry per pair ({pairs.shape[0]}), got {lengths.numel()}")
    if pairs.shape[0] and not bool((torch.isfinite(lengths) & (lengths > 0)).all()):
        c = int((~(torch.isfinite(lengths) & (lengths > 0))).nonzero()[0])
        raise ValueError(f"constraints: pair {c} = {tuple(pairs[c].tolist())} has length {float(lengths[c])}; lengths must be positive")
    ndof = torch.zeros(n_mol, dtype=torch.int64).index_add_(0, b_cpu, 3 * torch.isfinite(m64).to(torch.int64))
    if pairs.shape[0]:
        ndof -= torch.bincount(b_cpu[pairs[:, 0]], minlength=n_mol)
    out.update(pairs=pairs, lengths=lengths, tol=tol, max_iter=max_iter, ndof=ndof,
               constraint_d2=(lengths * lengths)[out["order"]].contiguous())
    _check_positions(pos, out)
    return out


def hydrogen_pairs(z, pos, batch=None, cutoff=1.3, rigid_water=False):
    """Constraint pairs that freeze the X-H bonds (host, plain torch, off the hot path): every atom with z == 1 is paired with its
    nearest heavy atom (z > 1) of the same molecule within ``cutoff``; a hydrogen with none is left free.  ``rigid_water``: the H-H
    pair of every oxygen with exactly two hydrogens and no other atom within ``cutoff`` is added, which makes the water rigid.
    Positions are taken as they are (unwrapped: a molecule must not be split across a periodic boundary).
    -> pairs [C,2] int64 in the caller's atom order: (heavy, H) by ascending H, then (H, H) by ascending O."""
    z = z.detach().cpu()
    x = pos.detach().to(device="cpu", dtype=torch.float64)
    b = torch.zeros_like(z) if batch is None else batch.detach().cpu()
    hyd, heavy = (z == 1).nonzero().reshape(-1), (z > 1).nonzero().reshape(-1)
    pairs, partners = [], {}
    if hyd.numel() and heavy.numel():
        for k in range(0, hyd.numel(), 4096):  # [4096, heavy] distances at a time
            h = hyd[k:k + 4096]
            d = torch.cdist(x[h], x[heavy])
            d = torch.where(b[h][:, None] == b[heavy][None, :], d, torch.full_like(d, float("inf")))
            dmin, arg = d.min(dim=1)
            for hi, dm, a in zip(h.tolist(), dmin.tolist(), heavy[arg].tolist()):
                if dm <= cutoff:
                    pairs.append([a, hi])
                    partners.setdefault(a, []).append(hi)
    if rigid_water:
        for o in sorted(a for a, hs in partners.items() if len(hs) == 2 and int(z[a]) == 8):
            d = (x - x[o]).norm(dim=1)
            near = ((d <= cutoff) & (b == b[o])).nonzero().reshape(-1).tolist()
            if sorted(near) == sorted([o] + partners[o]):
                pairs.append(sorted(partners[o]))
    return torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2)


class DeviceMD(CapturedLoop):
    """The object ``TorchMD_Net.capture_md`` returns.  ``md(n)`` replays the captured graph n times (``steps_per_replay`` steps
    each) and returns ``md``; nothing is read back.  Static tensors, rewritten by every replay: ``pos``, ``vel``, ``forces``
    [N,3] at the last completed step, ``epot`` and ``ekin`` [K,B] of the last replay's steps (``ekin`` = sum of 0.5 m v^2 in the
    unit of m v^2: divide by ``force_scale`` for the unit of ``epot``).  ``steps_done`` counts on the host; ``check()`` reads the
    device (one synchronisation).  With a barostat: ``box`` is the static box the graph reads AND writes (the caller's own object
    when it needed no conversion), and ``volume`` (before the move), ``pressure`` and ``scale`` (the fp32 factor mu) [K,B] are the
    barostat's logs of the last replay's steps; ``forces`` stay the forces of the last evaluation, at the positions before the move.
    With constraints (``prepare_constraints``): ``constraints`` is the dict of pairs, lengths, tol, max_iter and cluster tables,
    ``ndof`` [B] int64 the degrees of freedom per molecule (three per atom of finite mass, minus the molecule's constraints), and
    ``vel`` is projected onto the constraints at capture and at every ``reset``."""

    _capture_name, _noun = "capture_md", "the MD state"

    _observer = None  # torchmdnet_amd.observe.Observer of a loop made by capture_md_observed

    def __init__(self, model, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, thermostat, warmup,
                 barostat=None, constraints=None, observer=None):
        super().__init__(model, steps_per_replay)
        self._observer, self._keep_observables = observer, False
        L = _C.lib()
        dev = pos.device
        n = int(z.shape[0])
        K = self.steps_per_replay
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
            self.sigma = self._stage_sigma(m64)
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
        self.constraints = constraints
        if constraints is not None:
            self._tables = tuple(constraints[k].to(dev).contiguous()
                                 for k in ("cluster_atoms", "cluster_offsets", "constraint_ends", "constraint_d2"))
            L.tmdnet_md_constraints_workspace_bytes(n, self._tables[0].shape[0], self._tables[2].shape[0], C.byref(nbytes))
            self._cons_ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)

        def start(out):
            self.forces = out[1].clone()  # forces at the initial positions: what the first OPEN launch reads
            self._restart(0)  # with constraints: velocities drawn from a Maxwell-Boltzmann distribution are consistent before step 1

        self._capture(warmup, start, lambda: self._advance(MD_OPEN, self.forces, None, 0),
                      self.check if constraints is not None else None)

    def _restart(self, step):
        """What follows the evaluation of the start geometry, at capture and at ``reset``: counter and status, the subclass's
        ``_start``, and with constraints their status bits cleared and the velocities projected"""
        _C.lib().tmdnet_md_reset(_stream_ptr(self.pos.device), _ptr(self._ws), step)
        self._start(step)
        if self.constraints is not None:
            self._cons_ws.zero_()
            self._advance(MD_PROJECT, None, None, 0)
        if self._observer is not None and not self._keep_observables:
            self._observer.start(self, step)  # origins = these positions, s0 = step, everything else cleared

    def _stage_sigma(self, m64):
        """[N] fp32 thermal velocities sqrt(kT force_scale / m) the O step reads, from fp64, rounded once"""
        return torch.sqrt(float(self.thermostat["kT"]) * self.force_scale / m64).to(torch.float32).contiguous()

    def _start(self, step):
        """What a subclass enqueues on ``forces`` and its own state after ``tmdnet_md_reset(step)``, at capture and at ``reset``"""

    def _capture_step(self, k, K, out):
        """The launches that follow evaluation k of a replay (inside the capture): close step k, open step k + 1"""
        self._observe(k)
        if self.barostat is None:
            self._advance(MD_MIDDLE if k + 1 < K else MD_CLOSE, out[1], out[0], k)
        else:  # the kinetic energy of the closing half is reduced before the move: CLOSE, then scale (and open)
            self._advance(MD_CLOSE, out[1], out[0], k)
            self._barostat_move(k + 1 < K, out[1], out[2], k)

    def _observe(self, k):
        """The observer's launches after evaluation k, when there is an observer and replay position k is a sampling step; otherwise
        nothing: pos is x at the full step, vel the leapfrog velocity the opening half stored"""
        if self._observer is not None and (k + 1) % self._observer.spec["every"] == 0:
            self._observer.launch(self)

    def _observed(self):
        if self._observer is None:
            raise ValueError("this loop was captured without an observer: use capture_md_observed(..., observe=dict(...))")
        return self._observer

    @property
    def n_samples(self) -> int:
        """Samples the observer has recorded, from the device's step counter (one synchronisation) and not from ``steps_done``: a
        loop frozen by an overflow reports what it recorded"""
        return self._observed().n_samples(self)

    def frames(self):
        """-> (steps [n] int64 (host), pos [n,N,3] [, vel [n,N,3]]) clones of the n = min(capacity, n_samples) newest sampled frames,
        oldest first, in the caller's atom order; ``vel`` is the leapfrog velocity v(s - 1/2)"""
        return self._observed().frames(self)

    def rdf(self):
        """-> (r [bins] bin centres, g [B,P,bins] float64 (host), counts [B,P,bins] int64) of the pair-distance histogram over all
        samples.  With a box g = counts / (n_samples n_pairs shell / V), shell = 4 pi / 3 (r_hi^3 - r_lo^3), n_pairs = N_a N_b or
        N_a (N_a - 1) / 2 for a type whose two selectors are the same; WITHOUT a box there is no density to refer to and g is
        counts / (n_samples n_pairs), the fraction of the type's pairs per bin."""
        return self._observed().rdf(self)

    def msd(self):
        """-> (steps [n] int64 (host), msd [n,B,G] float64): the mean of |x_i(s) - x_i(s0)|^2 over each group's atoms per sample, from
        the unwrapped positions; the origin is the configuration at capture or the last ``reset``"""
        return self._observed().msd(self)

    def vacf(self):
        """-> (lag_times [L] float64 (host), C [B,G,L] float64): the autocorrelation <v(t) . v(t + lag)> of the LEAPFROG velocities
        v(s - 1/2) the loop stores at a sampled step (after the opening kick and, with constraints, after SHAKE's correction),
        averaged over each group's atoms and the n_samples - l origins of lag l; lags are multiples of every * dt; a lag with no
        sample is NaN"""
        return self._observed().vacf(self)

    @property
    def ndof(self) -> Tensor:
        """[B] int64 (host): three degrees of freedom per atom of finite mass, minus the molecule's constraints"""
        if self.constraints is not None:
            return self.constraints["ndof"]
        free = 3 * torch.isfinite(self.masses).to(torch.int64).cpu()
        return torch.zeros(self.n_mol, dtype=torch.int64).index_add_(0, self.inputs[1].cpu(), free)

    def _evaluate(self):
        z, batch, box, q = self.inputs
        return self._model.energy_and_forces(z, self.pos, batch, box, q, self.n_mol, want_forces=True,
                                             want_virial=self.barostat is not None)

    def _advance(self, phase, forces, energy, k):
        st = self._model._engine
        dev = self.pos.device
        if self.constraints is not None:
            return self._advance_constrained(phase, forces, energy, k)
        rc = _C.lib().tmdnet_md_advance(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), self.n_atoms, self.n_mol, phase,
                                        _ptr(self.pos), _ptr(self.vel), _ptr(forces), _ptr(energy), _ptr(self.hk), _ptr(self.masses),
                                        _ptr(self.sigma), self.dt, self.c1, self.c2, self.seed, _ptr(self.inputs[1]),
                                        None if phase == MD_OPEN else _ptr(self.forces), _ptr(self.epot[k]), _ptr(self.ekin[k]))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_md_advance: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def _advance_constrained(self, phase, forces, energy, k):
        st = self._model._engine
        dev = self.pos.device
        atoms, offsets, ends, d2 = self._tables
        con = self.constraints
        rc = _C.lib().tmdnet_md_advance_constrained(
            st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), _ptr(self._cons_ws), self.n_atoms, self.n_mol, phase,
            _ptr(self.pos), _ptr(self.vel), _ptr(forces), _ptr(energy), _ptr(self.hk), _ptr(self.masses), _ptr(self.sigma), self.dt,
            self.c1, self.c2, self.seed, _ptr(self.inputs[1]), None if phase in (MD_OPEN, MD_PROJECT) else _ptr(self.forces),
            _ptr(self.epot[k]), _ptr(self.ekin[k]), atoms.shape[0], ends.shape[0], _ptr(atoms), _ptr(offsets), _ptr(ends), _ptr(d2),
            con["tol"], con["max_iter"])
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_md_advance_constrained: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

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

    def check(self) -> int:
        """Read the device's step counter and status (one synchronisation).  Raises the reference's overflow RuntimeError when an
        evaluation found more neighbours than ``max_num_neighbors`` allows: ``pos`` / ``vel`` / ``forces`` (and ``box``) and the
        counter are then those of the last valid step, and replays change nothing until ``reset``.  Raises a RuntimeError naming
        the barostat when one of its moves was unusable (zero volume, or a NaN from the virial): the state is frozen before that
        move.  Raises a RuntimeError naming the constraints when a cluster did not converge within ``max_iter`` sweeps (or met a
        value that is not finite): that cluster is back at its saved state, the whole state is frozen and finite but is not a point
        of the trajectory - other clusters may be half a step ahead -, and ``reset(pos=, vel=)`` is required.  Raises a RuntimeError
        naming the bias (``DeviceBiasedMD``) when a walker's collective variable, its gradient or its bias was not finite: the state
        is frozen, finite and half a step ahead of the last completed step, and ``reset(pos=, vel=)`` is required.  Raises a
        RuntimeError naming the thermostat (``DeviceGlobalMD``) when a move of the global thermostat was unusable (a kinetic energy
        that is not finite): the state is frozen at the closed step, before that move.  Returns the step counter."""
        rc, (step, status) = self._status(_C.lib().tmdnet_md_status, 2)
        if status == 2:
            raise RuntimeError(f"barostat: the move after step {step} was not finite (zero volume, or a NaN in the virial or "
                               "the kinetic energy); the MD state is frozen before that move")
        if status == 3:
            bits = int(self._cons_ws.view(torch.int32).max().item()) if self.constraints is not None else 0
            stage = " and ".join(n for b, n in ((1, "SHAKE (positions)"), (2, "RATTLE (velocities)")) if bits & b) or "an iteration"
            raise RuntimeError(f"constraints: {stage} did not converge within max_iter={self.constraints['max_iter']} sweeps to "
                               f"tol={self.constraints['tol']:g} after step {step} (or met a value that is not finite); the MD "
                               "state is frozen and finite but is not a point of the trajectory (other clusters may be half a step "
                               "ahead): reset(pos=, vel=) is required")
        if status == 4:
            raise RuntimeError(f"bias: a collective variable, its gradient or the bias of a walker was not finite after step {step} "
                               "(coincident atoms, a collinear angle or torsion, or a NaN position); the MD state is frozen and finite "
                               "but half a step ahead of that step: reset(pos=, vel=) is required")
        if status == 5:
            kind = (getattr(self, "global_thermostat", None) or {}).get("kind", "global")
            raise RuntimeError(f"thermostat: the {kind} move after step {step} was unusable (a kinetic energy, a scale factor or a "
                               "chain value that is not finite, or a scale factor that is not positive); the MD state is frozen "
                               "before that move")
        return self._verdict("tmdnet_md_status", rc, step, status)

    def reset(self, pos: Optional[Tensor] = None, vel: Optional[Tensor] = None, step: int = 0, box: Optional[Tensor] = None,
              observables: str = "clear"):
        """New positions and / or velocities (copied into the static buffers), forces evaluated there, status cleared, device step
        counter and ``steps_done`` set to ``step`` (the Langevin noise is a function of (seed, step, atom)).  ``box`` is copied into
        the static box (a barostat has scaled it since the capture).  With constraints: new positions must satisfy them (ValueError
        naming the worst pair, before anything is changed), and the velocities are projected onto them again.  After a cluster
        did not converge (``check()`` named the constraints) the state is not a point of the trajectory, so both ``pos`` and ``vel``
        are required: a reset without one of them raises RuntimeError and changes nothing.  With an observer
        (``capture_md_observed``): ``observables="clear"`` zeroes the histogram, the logs and the accumulators and takes these
        positions as the new origins and ``step`` as the new s0; ``"keep"`` continues the sums and is refused (ValueError) unless
        ``pos`` and ``vel`` are None and ``step`` is the loop's current step; a new ``box`` must keep r_max within half its height."""
        dev = self.pos.device
        if observables not in ("clear", "keep"):
            raise ValueError(f"reset(observables=...): 'clear' or 'keep', got {observables!r}")
        if self._observer is not None:
            from torchmdnet_amd.observe import refuse_keep

            if observables == "keep":
                refuse_keep(pos, vel, step, self._status(_C.lib().tmdnet_md_status, 2)[1][0])
            if box is not None:
                self._observer.check_box(box)

        def copy_in():
            if self.constraints is not None and (pos is None or vel is None):
                if self._status(_C.lib().tmdnet_md_status, 2)[1][1] == 3:
                    raise RuntimeError("constraints: an iteration did not converge, so the MD state is not a point of the trajectory: "
                                       "reset(pos=, vel=) needs both pos and vel")
            if self.constraints is not None and pos is not None:
                _check_positions(pos, self.constraints)
            if box is not None:
                if self.box is None:
                    raise ValueError("reset(box=...): this loop was captured without a box")
                self.box.copy_(box.detach().to(device=dev, dtype=torch.float32).reshape(self.box.shape))
            if pos is not None:
                self.pos.copy_(pos.detach().to(device=dev, dtype=torch.float32))
            if vel is not None:
                self.vel.copy_(vel.detach().to(device=dev, dtype=torch.float32))

        def start(out):
            self.forces.copy_(out[1])
            self._restart(int(step))

        self._keep_observables = observables == "keep"
        try:
            self._reset(copy_in, start, step)
        finally:
            self._keep_observables = False
        if self.constraints is not None:
            self.check()
        return self


class DeviceCellMD(DeviceMD):
    """The object ``TorchMD_Net.capture_md_cell`` returns: ``DeviceMD`` whose every step ends with an anisotropic, diagonal or
    semi-isotropic stochastic-cell-rescaling move per molecule inside the graph (``tmdnet_md_barostat_cell``, csrc/tn_md_cell.hip; the
    scheme is documented in include/tmdnet_amd.h and DESIGN.md section 13), so the cell's shape fluctuates and not only its volume.
    ``cell_barostat`` is the parsed dict.  ``box`` is the static box the graph reads AND writes (the caller's own object when it needed
    no conversion); in "anisotropic" mode it is lower triangular after every move, the whole system having been rotated with it:
    ``forces`` are the forces of the last evaluation in the frame of ``pos``.  Logs of the last replay's steps: ``volume`` [K,B]
    (before the move), ``pressure_tensor`` [K,B,3,3] and ``scale`` [K,B,3,3], the fp32 matrix Mx that took the positions through the
    move (x <- x Mx).  The minimum image is exact only while the off-diagonal entries of the box stay below half the diagonal ones, as
    for any triclinic box: there is no lattice reduction."""

    _capture_name = "capture_md_cell"

    def __init__(self, model, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, thermostat, warmup, barostat):
        self.cell_barostat = barostat
        self._cell_ready = False
        super().__init__(model, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, thermostat, warmup)

    def _stage_cell(self):
        dev, K, B = self.pos.device, self.steps_per_replay, self.n_mol
        self.volume = torch.zeros((K, B), dtype=torch.float32, device=dev)
        self.pressure_tensor = torch.zeros((K, B, 3, 3), dtype=torch.float32, device=dev)
        self.scale = torch.zeros((K, B, 3, 3), dtype=torch.float32, device=dev)
        nbytes = C.c_size_t(0)
        if _C.lib().tmdnet_md_barostat_cell_workspace_bytes(self.n_atoms, B, C.byref(nbytes)) != _C.OK:
            raise ValueError(f"capture_md_cell: {self.n_atoms} atoms in {B} molecules are not a valid layout")
        self._cell_ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        self._cell_ready = True

    def _start(self, step):
        if not self._cell_ready:
            self._stage_cell()

    def _evaluate(self):
        z, batch, box, q = self.inputs
        return self._model.energy_and_forces(z, self.pos, batch, box, q, self.n_mol, want_forces=True, want_virial=True)

    def matrices(self):
        """-> (Mx, Mv, Mf) [B,3,3] float32 clones of the last move's matrices, from the scratch of ``tmdnet_md_barostat_cell``"""
        off = (-self._cell_ws.data_ptr()) % 256
        M = self._cell_ws[off:off + 108 * self.n_mol].view(torch.float32).view(self.n_mol, 3, 3, 3)
        return M[:, 0].clone(), M[:, 1].clone(), M[:, 2].clone()

    def _cell_move(self, open_next, forces, virial, k):
        st, dev, b = self._model._engine, self.pos.device, self.cell_barostat
        rc = _C.lib().tmdnet_md_barostat_cell(
            st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), _ptr(self._cell_ws), self.n_atoms, self.n_mol, int(open_next),
            _ptr(self.pos), _ptr(self.vel), _ptr(forces), _ptr(self.hk), _ptr(self.masses), self.dt, _ptr(self.inputs[1]), _ptr(self.box),
            1 if self.box.dim() == 2 else 2, _ptr(virial), b["pressure"], b["kT"], b["compressibility"], b["tau"], self.force_scale,
            b["seed"], CELL_COUPLINGS[b["coupling"]], b["axis"], _ptr(self.forces), _ptr(self.volume[k]), _ptr(self.pressure_tensor[k]),
            _ptr(self.scale[k]))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_md_barostat_cell: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def _capture_step(self, k, K, out):
        # the closing half (kick, O step, step counter), then the move: the kinetic tensor is reduced from the closed velocities
        self._advance(MD_CLOSE, out[1], out[0], k)
        self._cell_move(k + 1 < K, out[1], out[2], k)

    def check(self) -> int:
        """``DeviceMD.check``; an unusable move of the cell barostat (status 2) is reported under its own name"""
        step, status = self._status(_C.lib().tmdnet_md_status, 2)[1]
        if status == 2:
            raise RuntimeError(f"cell barostat ({self.cell_barostat['coupling']}): the move after step {step} was unusable (zero volume, a "
                               "NaN in the virial or the kinetic tensor, or a left-handed box); the MD state is frozen before that move")
        return super().check()


def geometric_ladder(kT_min, kT_max, R):
    """R temperatures kT_min (kT_max / kT_min)^(i / (R - 1)), i = 0..R-1: equal ratios between neighbours, which gives equal
    acceptance along the ladder when the heat capacity does not depend on the temperature.  -> [R] float64 (host)"""
    R = int(R)
    if R < 2 or not kT_min > 0 or not kT_max > 0:
        raise ValueError(f"geometric_ladder: needs R >= 2 and positive temperatures, got {kT_min}, {kT_max}, {R}")
    i = torch.arange(R, dtype=torch.float64) / (R - 1)
    return float(kT_min) * (float(kT_max) / float(kT_min)) ** i


class DeviceREMD(DeviceMD):
    """The object ``TorchMD_Net.capture_remd`` returns: ``DeviceMD`` for B = G R replicas of one system in G independent ladders of
    R temperature slots, with a temperature-exchange attempt inside the graph after every ``exchange_every`` steps
    (``tmdnet_md_exchange``; the scheme is documented in include/tmdnet_amd.h and DESIGN.md section 13).  Replicas swap
    temperatures, not coordinates: row b of ``pos`` / ``vel`` stays replica b, and ``slot`` [B] int32 says which temperature it
    has now (``holder`` [G,R] int32 is the inverse); both are the live device tensors.  ``slot_log`` [K/X,B] int32 and ``accepted``
    [K/X,G,R-1] uint8 (pairs not tried in that parity read 0) are the logs of the last replay's attempts; ``attempts`` /
    ``accepts`` [G,R-1] int64 count on the device since the capture or the last ``reset``.  ``temperatures`` [R] float64 (host)."""

    def __init__(self, model, z, pos, vel, masses, dt, temperatures, exchange_every, n_ladders, box, q, steps_per_replay, force_scale,
                 thermostat, warmup):
        kT = torch.as_tensor(temperatures, dtype=torch.float64).detach().cpu().reshape(-1)
        self.temperatures = kT
        self.n_slots, self.n_ladders = R, G = int(kT.numel()), int(n_ladders)
        self.exchange_every = X = int(exchange_every)
        n1 = int(z.shape[0]) // (G * R)
        self._m1 = masses.detach().to(device=pos.device, dtype=torch.float64).reshape(-1)[:n1]
        batch = torch.repeat_interleave(torch.arange(G * R, device=pos.device), n1)
        self._n_attempts = int(steps_per_replay) // X if X else 0
        super().__init__(model, z, pos, vel, masses, dt, batch, box, q, G * R, steps_per_replay, force_scale, thermostat, warmup)

    def _stage_sigma(self, m64):
        # everything the exchange launches read, before the capture: tables per slot in fp64, rounded once
        dev, R, G, kT = m64.device, self.n_slots, self.n_ladders, self.temperatures
        B, n1 = G * R, self._m1.numel()
        self.sigma_table = torch.stack([torch.sqrt(float(t) * self.force_scale / self._m1) for t in kT]).to(torch.float32).contiguous()
        self._beta = (1.0 / kT).to(dev).contiguous()
        self._up = torch.tensor([math.sqrt(float(kT[s + 1]) / float(kT[s])) for s in range(R - 1)], dtype=torch.float64).to(torch.float32).to(dev)
        self._down = torch.tensor([math.sqrt(float(kT[s]) / float(kT[s + 1])) for s in range(R - 1)], dtype=torch.float64).to(torch.float32).to(dev)
        self.slot = torch.arange(R, dtype=torch.int32, device=dev).repeat(G).contiguous()
        self.holder = torch.arange(R, dtype=torch.int32, device=dev).repeat(G, 1).contiguous()
        self.slot_log = torch.zeros((self._n_attempts, B), dtype=torch.int32, device=dev)
        self.accepted = torch.zeros((self._n_attempts, G, R - 1), dtype=torch.uint8, device=dev)
        self._counters = torch.zeros((2, G, R - 1), dtype=torch.int64, device=dev)
        nbytes = C.c_size_t(0)
        if _C.lib().tmdnet_md_exchange_workspace_bytes(B, R, C.byref(nbytes)) != _C.OK:
            raise ValueError(f"capture_remd: {G} ladders of {R} slots are not a valid layout")
        self._ex_ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        return self.sigma_table[self.slot.long()].reshape(-1).contiguous()

    @property
    def attempts(self) -> Tensor:
        return self._counters[0]

    @property
    def accepts(self) -> Tensor:
        return self._counters[1]

    def acceptance(self) -> Tensor:
        """accepts / attempts [G,R-1] float64 on the host (one read-back); NaN for a pair never tried"""
        c = self._counters.cpu().to(torch.float64)
        return c[1] / c[0]

    def _capture_step(self, k, K, out):
        X = self.exchange_every
        if not X or (k + 1) % X:
            return super()._capture_step(k, K, out)
        # CLOSE, the exchange, OPEN: bit for bit MIDDLE (the rounding contract) around an attempt that sees the step's energies
        self._advance(MD_CLOSE, out[1], out[0], k)
        st = self._model._engine
        a = (k + 1) // X - 1
        rc = _C.lib().tmdnet_md_exchange(st.handle, _stream_ptr(self.pos.device), _ptr(st.graph_ws), _ptr(self._ws), _ptr(self._ex_ws),
                                         self.n_atoms, self.n_mol, self.n_slots, X, _ptr(self.vel), _ptr(self.sigma), _ptr(self.epot[k]),
                                         _ptr(self._beta), _ptr(self.sigma_table), _ptr(self._up), _ptr(self._down), self.seed,
                                         _ptr(self.slot), _ptr(self.holder), _ptr(self.slot_log[a]), _ptr(self.accepted[a]),
                                         _ptr(self._counters))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_md_exchange: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")
        if k + 1 < K:
            self._advance(MD_OPEN, self.forces, None, k)

    def by_slot(self, t: Tensor) -> Tensor:
        """Gather a per-replica [B,...] or per-atom [N,...] tensor into slot order [G,R,...] with the current assignment, so that
        ``by_slot(remd.pos)[:, 0]`` is what the first temperature of every ladder holds now."""
        B, G, R = self.n_mol, self.n_ladders, self.n_slots
        if t.shape[0] == self.n_atoms and self.n_atoms != B:
            t = t.reshape(B, self.n_atoms // B, *t.shape[1:])
        elif t.shape[0] != B:
            raise ValueError(f"by_slot: the first dimension must be {B} replicas or {self.n_atoms} atoms, got {tuple(t.shape)}")
        idx = torch.arange(G, device=self.holder.device)[:, None] * R + self.holder.long()
        return t[idx.to(t.device)]

    def reset(self, pos: Optional[Tensor] = None, vel: Optional[Tensor] = None, step: int = 0, slots: Optional[Tensor] = None):
        """``DeviceMD.reset`` (``pos`` / ``vel`` in any shape of B n atoms), plus ``slots`` [B] or [G,R]: the slot of every replica,
        a permutation of 0..R-1 within each ladder (ValueError otherwise, before anything is changed); ``sigma`` is staged again
        for it.  None keeps the current assignment.  The attempt and accept counters are cleared."""
        G, R = self.n_ladders, self.n_slots
        if slots is not None:
            s = torch.as_tensor(slots).detach().cpu()
            if s.dtype.is_floating_point or s.numel() != G * R:
                raise ValueError(f"reset(slots=...): needs {G * R} integers, got {tuple(s.shape)} {s.dtype}")
            s = s.reshape(G, R).to(torch.int64)
            if not bool((s.sort(dim=1).values == torch.arange(R)).all()):
                raise ValueError(f"reset(slots=...): every ladder's slots must be a permutation of 0..{R - 1}, got {s.tolist()}")
        pos = None if pos is None else pos.reshape(-1, 3)
        vel = None if vel is None else vel.reshape(-1, 3)
        if slots is not None:
            dev = self.slot.device
            self.slot.copy_(s.reshape(-1).to(torch.int32).to(dev))
            self.holder.copy_(s.argsort(dim=1).to(torch.int32).to(dev))
            self.sigma.copy_(self.sigma_table[self.slot.long()].reshape(-1))
        self._counters.zero_()
        return super().reset(pos, vel, step)


# ---- collective-variable restraints and metadynamics (csrc/tn_bias.hip) ---------------------------------------------------------------
CV_KINDS = {"distance": (0, 2), "angle": (1, 3), "torsion": (2, 4)}  # name -> (kind of tmdnet_md_bias, number of atoms)
RESTRAINT_KINDS = {"harmonic": 1, "upper": 2, "lower": 3}
MAX_CVS = 8
_BIAS_KEYS = ("cvs", "restraints", "metad", "log_forces")
_METAD_KEYS = ("cvs", "sigma", "height", "pace", "kT", "bias_factor", "walkers_per_group", "capacity")


def prepare_bias(bias, batch, n_atoms, n_mol):
    """``bias=dict(cvs=, restraints=, metad=, log_forces=)`` -> everything ``DeviceBiasedMD`` needs, on the host, before anything is
    staged: the CV tables, the table of distinct atoms and their (cv, slot) entries, kappa and the centres per walker [B,D] and the
    metadynamics parameters.  Raises ValueError naming the cause."""
    b = dict(bias)
    unknown = set(b) - set(_BIAS_KEYS)
    if unknown:
        raise ValueError(f"bias: unknown keys {sorted(unknown)} ({', '.join(_BIAS_KEYS)})")
    B = int(n_mol)
    bt = torch.as_tensor(batch).detach().cpu().to(torch.int64).reshape(-1)
    if bt.numel() != int(n_atoms):
        raise ValueError(f"bias: batch must have one entry per atom ({n_atoms}), got {bt.numel()}")
    if bt.numel() > 1 and bool((bt[1:] < bt[:-1]).any()):
        raise ValueError("bias: batch must be sorted (CV atoms are given relative to each molecule's first atom)")
    sizes = torch.bincount(bt, minlength=B)
    if sizes.numel() != B or int(sizes.min()) < 1:
        raise ValueError(f"bias: every one of the {B} molecules needs at least one atom, got sizes {sizes.tolist()}")
    start = torch.cumsum(sizes, 0) - sizes
    cvs = list(b.get("cvs") or [])
    D = len(cvs)
    if D < 1:
        raise ValueError("bias: 'cvs' needs at least one collective variable")
    if D > MAX_CVS:
        raise ValueError(f"bias: {D} collective variables, at most {MAX_CVS} per walker")
    kinds, atoms = [], []
    smallest = int(sizes.min())
    for c, cv in enumerate(cvs):
        name, idx = cv[0], [int(i) for i in cv[1:]]
        if name not in CV_KINDS:
            raise ValueError(f"bias: cv {c} has kind {name!r} ({', '.join(CV_KINDS)})")
        kind, na = CV_KINDS[name]
        if len(idx) != na:
            raise ValueError(f"bias: cv {c} ({name}) takes {na} atoms, got {len(idx)}")
        for i in idx:
            if not 0 <= i < smallest:
                raise ValueError(f"bias: cv {c} ({name}) names atom {i}, outside its molecule (the smallest molecule has {smallest} atoms; "
                                 "indices are relative to each molecule's first atom)")
        if len(set(idx)) != na:
            raise ValueError(f"bias: cv {c} ({name}) names an atom twice: {idx}")
        kinds.append(kind)
        atoms.append(idx + [-1] * (4 - na))
    distinct = sorted({i for row in atoms for i in row if i >= 0})
    offsets, entries = [0], []
    for a in distinct:
        entries += [(c << 2) | s for c, row in enumerate(atoms) for s, i in enumerate(row) if i == a]
        offsets.append(len(entries))
    res_kind = [0] * D
    kappa, center = torch.zeros((B, D), dtype=torch.float64), torch.zeros((B, D), dtype=torch.float64)
    for r, res in enumerate(b.get("restraints") or []):
        res = dict(res)
        unknown = set(res) - {"cv", "kind", "kappa", "center"}
        if unknown or not {"cv", "kappa", "center"} <= set(res):
            raise ValueError(f"bias: restraint {r} is dict(cv=, kind=, kappa=, center=), got keys {sorted(res)}")
        c, kind = int(res["cv"]), res.get("kind", "harmonic")
        if not 0 <= c < D:
            raise ValueError(f"bias: restraint {r} names cv {c}, outside 0..{D - 1}")
        if kind not in RESTRAINT_KINDS:
            raise ValueError(f"bias: restraint {r} has kind {kind!r} ({', '.join(RESTRAINT_KINDS)})")
        if res_kind[c]:
            raise ValueError(f"bias: cv {c} has two restraints; one per collective variable")
        res_kind[c] = RESTRAINT_KINDS[kind]
        for name, dst in (("kappa", kappa), ("center", center)):
            v = torch.as_tensor(res[name], dtype=torch.float64).detach().cpu().reshape(-1)
            if v.numel() not in (1, B) or not bool(torch.isfinite(v).all()):
                raise ValueError(f"bias: restraint {r}: {name} must be a finite scalar or [{B}] (one per walker), got {tuple(v.shape)}")
            dst[:, c] = v
    out = dict(D=D, kinds=torch.tensor(kinds, dtype=torch.int32), atoms=torch.tensor(atoms, dtype=torch.int32),
               mol_start=start.to(torch.int32), distinct=torch.tensor(distinct, dtype=torch.int32),
               offsets=torch.tensor(offsets, dtype=torch.int32),
               entries=torch.tensor(entries + [0] * (4 * MAX_CVS - len(entries)), dtype=torch.int32), res_kind=torch.tensor(res_kind, dtype=torch.int32),
               kappa=kappa, center=center, log_forces=bool(b.get("log_forces", False)), cvs=[tuple(cv) for cv in cvs],
               dm=0, mcv=(0, 0), sigma=(0.0, 0.0), height=0.0, pace=1, kT=0.0, gamma=0.0, W=1, H=0)
    metad = b.get("metad")
    if metad is not None:
        m = dict(metad)
        unknown = set(m) - set(_METAD_KEYS)
        if unknown:
            raise ValueError(f"bias: metad has unknown keys {sorted(unknown)} ({', '.join(_METAD_KEYS)})")
        for key in ("cvs", "sigma", "height", "pace", "kT", "capacity"):
            if key not in m:
                raise ValueError(f"bias: metad needs '{key}'")
        mcv = [int(c) for c in m["cvs"]]
        if len(mcv) not in (1, 2):
            raise ValueError(f"bias: metadynamics acts on 1 or 2 collective variables, got {len(mcv)}")
        if any(not 0 <= c < D for c in mcv) or len(set(mcv)) != len(mcv):
            raise ValueError(f"bias: metad cvs {mcv} must be distinct indices into the {D} collective variables")
        sigma = [float(s) for s in (m["sigma"] if hasattr(m["sigma"], "__len__") else [m["sigma"]])]
        if len(sigma) != len(mcv) or not all(s > 0 and math.isfinite(s) for s in sigma):
            raise ValueError(f"bias: metad sigma must be {len(mcv)} positive widths, got {sigma}")
        height, pace, kT = float(m["height"]), int(m["pace"]), float(m["kT"])
        if not height >= 0 or not math.isfinite(height):
            raise ValueError(f"bias: metad height must not be negative, got {height}")
        if pace < 1:
            raise ValueError(f"bias: metad pace must be at least 1 step, got {pace}")
        gamma = m.get("bias_factor")
        if gamma is not None and not float(gamma) > 1:
            raise ValueError(f"bias: metad bias_factor must exceed 1 (None: plain metadynamics), got {gamma}")
        if gamma is not None and not kT > 0:
            raise ValueError(f"bias: well-tempered metadynamics needs kT > 0, got {kT}")
        W, H = int(m.get("walkers_per_group", 1)), int(m["capacity"])
        if W < 1 or B % W:
            raise ValueError(f"bias: the {B} walkers are no whole number of groups of walkers_per_group={W}")
        if H < W:
            raise ValueError(f"bias: metad capacity {H} is below walkers_per_group={W}: not one deposit fits")
        out.update(dm=len(mcv), mcv=(mcv[0], mcv[-1]), sigma=(sigma[0], sigma[-1]), height=height, pace=pace, kT=kT,
                   gamma=0.0 if gamma is None else float(gamma), W=W, H=H)
    return out


class DeviceBiasedMD(DeviceMD):
    """The object ``TorchMD_Net.capture_md_biased`` returns: ``DeviceMD`` whose every step adds the force of collective-variable
    restraints and / or metadynamics to the model's force inside the graph (``tmdnet_md_bias``, one launch between the evaluation and
    the integrator launch; the scheme is documented in include/tmdnet_amd.h and DESIGN.md section 13).  The B molecules are walkers;
    consecutive walkers form G = B / W groups that share one list of hills.  ``forces`` is the TOTAL force.  Logs of the last
    replay's steps: ``cv`` [K,B,D], ``restraint_energy`` and ``bias_energy`` [K,B] (float64; the bias each step's force came from),
    and with ``log_forces`` ``bias_forces`` [K,B,A,3] float32 on the atoms ``bias_atoms`` [B,A] (global indices) and
    ``start_bias_forces`` [B,A,3], the bias force in ``forces`` at the capture or the last ``reset``."""

    def __init__(self, model, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, thermostat, warmup, bias):
        self.bias = bias
        self._step0, self._hill_base = 0, 0
        self._bias_ready = False
        super().__init__(model, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, thermostat, warmup)

    def _stage_bias(self):
        bs, dev, K, B = self.bias, self.pos.device, self.steps_per_replay, self.n_mol
        D, A = bs["D"], int(bs["distinct"].numel())
        self._tab = {k: bs[k].to(dev).contiguous() for k in ("kinds", "atoms", "mol_start", "distinct", "offsets", "entries", "res_kind", "kappa", "center")}
        self.cv = torch.zeros((K, B, D), dtype=torch.float64, device=dev)
        self.restraint_energy = torch.zeros((K, B), dtype=torch.float64, device=dev)
        self.bias_energy = torch.zeros((K, B), dtype=torch.float64, device=dev)
        self.bias_forces = torch.zeros((K, B, A, 3), dtype=torch.float32, device=dev) if bs["log_forces"] else None
        self.bias_atoms = (self._tab["mol_start"][:, None] + self._tab["distinct"][None, :]).long()
        self.start_bias_forces = torch.zeros((B, A, 3), dtype=torch.float32, device=dev) if bs["log_forces"] else None
        self._start_row = (torch.zeros((B, D), dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev),
                           torch.zeros(B, dtype=torch.float64, device=dev))
        nbytes = C.c_size_t(0)
        if _C.lib().tmdnet_md_bias_workspace_bytes(B, D, bs["dm"], bs["W"], bs["H"], C.byref(nbytes)) != _C.OK:
            raise ValueError(f"capture_md_biased: {B} walkers, {D} cvs, walkers_per_group={bs['W']}, capacity={bs['H']} are not a valid layout")
        self._bias_ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        self._bias_ready = True

    @property
    def n_groups(self) -> int:
        return self.n_mol // self.bias["W"]

    def _hill_store(self) -> Tensor:
        """[G, dm + 1, H] float64 view of the hills in the workspace: centre 0 [, centre 1], height"""
        bs = self.bias
        off = (-self._bias_ws.data_ptr()) % 256 + 256
        n = self.n_groups * (bs["dm"] + 1) * bs["H"]
        return self._bias_ws[off:off + 8 * n].view(torch.float64).view(self.n_groups, bs["dm"] + 1, bs["H"])

    def _bias_launch(self, deposit, forces, rows, force_row):
        st, dev, bs, tb = self._model._engine, self.pos.device, self.bias, self._tab
        rc = _C.lib().tmdnet_md_bias(
            st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), _ptr(self._bias_ws), self.n_atoms, self.n_mol, int(deposit),
            _ptr(self.pos), _ptr(forces), bs["D"], _ptr(tb["kinds"]), _ptr(tb["atoms"]), _ptr(tb["mol_start"]), int(tb["distinct"].numel()),
            _ptr(tb["distinct"]), _ptr(tb["offsets"]), _ptr(tb["entries"]), _ptr(tb["res_kind"]), _ptr(tb["kappa"]), _ptr(tb["center"]),
            bs["dm"], bs["mcv"][0], bs["mcv"][1], bs["sigma"][0], bs["sigma"][1], bs["height"], bs["kT"], bs["gamma"], bs["pace"], bs["W"],
            bs["H"], _ptr(rows[0]), _ptr(rows[1]), _ptr(rows[2]), _ptr(force_row))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_md_bias: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def _start(self, step):
        # the bias of the start geometry joins ``forces`` (what the first OPEN launch reads): evaluate only, nothing is deposited
        if not self._bias_ready:
            self._stage_bias()
        self._step0 = int(step)
        _C.lib().tmdnet_md_bias_reset(_stream_ptr(self.pos.device), _ptr(self._bias_ws), self._step0, self._hill_base)
        self._bias_launch(0, self.forces, self._start_row, self.start_bias_forces)

    def _capture_step(self, k, K, out):
        self._bias_launch(1, out[1], (self.cv[k], self.restraint_energy[k], self.bias_energy[k]),
                          None if self.bias_forces is None else self.bias_forces[k])
        super()._capture_step(k, K, out)

    def _hills_after(self, steps):
        bs = self.bias
        return self._hill_base + ((int(steps) - self._step0) // bs["pace"]) * bs["W"] if bs["dm"] else 0

    @property
    def n_hills(self) -> int:
        """hills per group that the next step reads (host arithmetic on ``steps_done``; after a frozen replay ``check()`` first)"""
        return min(self.bias["H"], self._hills_after(self.steps_done))

    def __call__(self, n: int = 1):
        after = self._hills_after(self.steps_done + int(n) * self.steps_per_replay)
        if after > self.bias["H"]:
            raise ValueError(f"metad: {int(n)} replay(s) would deposit up to hill {after} of a group, past capacity={self.bias['H']}; "
                             "capture with a larger capacity, or reset(hills='clear')")
        return super().__call__(n)

    def hills(self):
        """-> (centres [G,n,dm], heights [G,n]) float64 clones of the ``n_hills`` hills of every group"""
        bs = self.bias
        if not bs["dm"]:
            raise ValueError("hills(): this loop was captured without metadynamics")
        store, n = self._hill_store(), self.n_hills
        return store[:, :bs["dm"], :n].transpose(1, 2).clone(), store[:, bs["dm"], :n].clone()

    def bias_potential(self, s) -> Tensor:
        """V(s) of every group's hills in torch float64: ``s`` [...,dm] (or [...] for dm = 1) -> [G,...]; a torsion's difference is
        wrapped into (-pi, pi]"""
        bs = self.bias
        c, w = self.hills()
        s = torch.as_tensor(s, dtype=torch.float64).to(c.device)
        if bs["dm"] == 1 and (s.dim() == 0 or s.shape[-1] != 1):
            s = s[..., None]
        if s.shape[-1] != bs["dm"]:
            raise ValueError(f"bias_potential: the last dimension of s must be dm = {bs['dm']}, got {tuple(s.shape)}")
        shape = s.shape[:-1]
        d = s.reshape(1, -1, 1, bs["dm"]) - c[:, None, :, :]  # [G,P,n,dm]
        for k in range(bs["dm"]):
            if int(bs["kinds"][bs["mcv"][k]]) == CV_KINDS["torsion"][0]:
                d[..., k] = d[..., k] - 2.0 * math.pi * torch.ceil((d[..., k] - math.pi) / (2.0 * math.pi))
        sig = torch.tensor(bs["sigma"][:bs["dm"]], dtype=torch.float64, device=c.device)
        V = (w[:, None, :] * torch.exp(-0.5 * ((d / sig) ** 2).sum(-1))).sum(-1)
        return V.reshape(self.n_groups, *shape)

    def free_energy(self, s) -> Tensor:
        """The well-tempered estimate F(s) = -gamma / (gamma - 1) V(s) [G,...], up to a constant.  Plain metadynamics has no such
        factor (its V keeps growing): ValueError."""
        g = self.bias["gamma"]
        if not g > 1:
            raise ValueError("free_energy: needs well-tempered metadynamics (bias_factor > 1); with plain metadynamics use -bias_potential(s)")
        return -(g / (g - 1.0)) * self.bias_potential(s)

    def _device_state(self):
        return tuple(self._status(_C.lib().tmdnet_md_status, 2)[1])

    def reset(self, pos: Optional[Tensor] = None, vel: Optional[Tensor] = None, step: int = 0, hills="keep"):
        """``DeviceMD.reset``, plus the hills: ``"keep"`` (the device's step counter is read first, so the count is the device's also
        after a frozen replay), ``"clear"``, or ``(centres [G,n,dm], heights [G,n])`` to restart from saved hills.  Deposits are
        counted from ``step`` on.  After ``check()`` named the bias (a CV that was not finite) the state is half a step ahead: both
        ``pos`` and ``vel`` are required."""
        self._check_fresh()
        bs = self.bias
        n_dev, status = self._device_state()
        if status == 4 and (pos is None or vel is None):
            raise RuntimeError("bias: a collective variable was not finite, so the MD state is half a step ahead of the last completed "
                               "step: reset(pos=, vel=) needs both pos and vel")
        if isinstance(hills, str):
            if hills not in ("keep", "clear"):
                raise ValueError(f"reset(hills=...): 'keep', 'clear' or (centres, heights), got {hills!r}")
            base = min(bs["H"], self._hills_after(n_dev)) if hills == "keep" else 0
            new = None
        else:
            if not bs["dm"]:
                raise ValueError("reset(hills=(centres, heights)): this loop was captured without metadynamics")
            c = torch.as_tensor(hills[0], dtype=torch.float64)
            w = torch.as_tensor(hills[1], dtype=torch.float64)
            G = self.n_groups
            if c.dim() == 2 and bs["dm"] == 1:
                c = c[..., None]
            if c.dim() != 3 or c.shape[0] != G or c.shape[2] != bs["dm"] or tuple(w.shape) != tuple(c.shape[:2]) or c.shape[1] > bs["H"]:
                raise ValueError(f"reset(hills=...): needs centres [{G},n,{bs['dm']}] and heights [{G},n] with n <= capacity={bs['H']}, got "
                                 f"{tuple(c.shape)} and {tuple(w.shape)}")
            base, new = int(c.shape[1]), (c, w)
        if new is not None and base:
            store = self._hill_store()
            store[:, :bs["dm"], :base] = new[0].to(store.device).transpose(1, 2)
            store[:, bs["dm"], :base] = new[1].to(store.device)
        self._hill_base = base
        return super().reset(pos, vel, step)


# ---- global thermostats: stochastic velocity rescaling and Nose-Hoover chains (csrc/tn_md_thermo.hip) ---------------------------------
THERMOSTAT_KINDS = {"csvr": 0, "nose-hoover": 1}  # name -> kind of tmdnet_md_thermostat
MAX_CHAIN = 8
_GLOBAL_KEYS = {"csvr": ("kind", "kT", "tau", "seed", "ndof"), "nose-hoover": ("kind", "kT", "tau", "chain", "substeps", "ndof")}


def parse_global_thermostat(thermostat):
    """``thermostat=dict(kind="csvr", kT=, tau=, seed=0, ndof=None)`` or ``dict(kind="nose-hoover", kT=, tau=, chain=3, substeps=2,
    ndof=None)`` -> the same with every key present (``chain`` = 0 for CSVR).  ``ndof``: None, an int, or one int per molecule.
    Raises ValueError."""
    if thermostat is None:
        raise ValueError("capture_md_global needs thermostat=dict(kind='csvr' | 'nose-hoover', kT=, tau=, ...); without one use capture_md")
    t = dict(thermostat)
    kind = t.get("kind")
    if kind not in THERMOSTAT_KINDS:
        raise ValueError(f"thermostat: kind must be one of {', '.join(THERMOSTAT_KINDS)}, got {kind!r}")
    unknown = set(t) - set(_GLOBAL_KEYS[kind])
    if unknown:
        raise ValueError(f"thermostat: unknown keys {sorted(unknown)} for kind {kind!r} ({', '.join(_GLOBAL_KEYS[kind])})")
    for key in ("kT", "tau"):
        if key not in t:
            raise ValueError(f"thermostat: '{key}' is required")
    out = dict(kind=kind, kT=float(t["kT"]), tau=float(t["tau"]), seed=int(t.get("seed", 0)) & (2 ** 64 - 1), chain=0, substeps=1)
    if not out["kT"] > 0 or not out["tau"] > 0 or not math.isfinite(out["kT"]) or not math.isfinite(out["tau"]):
        raise ValueError(f"thermostat: kT and tau must be positive, got kT={out['kT']}, tau={out['tau']}")
    if kind == "nose-hoover":
        out["chain"], out["substeps"] = int(t.get("chain", 3)), int(t.get("substeps", 2))
        if not 1 <= out["chain"] <= MAX_CHAIN:
            raise ValueError(f"thermostat: chain must be 1..{MAX_CHAIN} thermostats, got {out['chain']}")
        if out["substeps"] < 1:
            raise ValueError(f"thermostat: substeps must be at least 1, got {out['substeps']}")
    ndof = t.get("ndof")
    if ndof is not None:
        ndof = torch.as_tensor(ndof).detach().cpu().reshape(-1)
        if ndof.dtype.is_floating_point or ndof.dtype == torch.bool:
            raise ValueError(f"thermostat: ndof must be an integer or an integer tensor, got {ndof.dtype}")
        ndof = ndof.to(torch.int64)
        if ndof.numel() < 1 or int(ndof.min()) < 0 or int(ndof.max()) > 2 ** 31 - 1:
            raise ValueError(f"thermostat: ndof must not be negative, got {ndof.tolist()[:8]}")
    out["ndof"] = ndof
    return out


def stage_ndof(ndof, default, n_mol):
    """The thermostat's ``ndof`` (``parse_global_thermostat``: None or a host int64 tensor of 1 or B entries) -> [B] int64 (host);
    None: ``default``, the loop's own count.  Raises ValueError."""
    if ndof is None:
        return default.to(torch.int64).clone()
    if ndof.numel() not in (1, int(n_mol)):
        raise ValueError(f"thermostat: ndof must be one integer or one per molecule ({n_mol}), got {ndof.numel()}")
    return ndof.expand(int(n_mol)).clone()


def count_ndof(masses, batch, n_mol, constraints=None):
    """[B] int64 (host): three degrees of freedom per atom of finite mass, minus the molecule's constraints - ``DeviceMD.ndof``
    before there is a loop"""
    if constraints is not None:
        return constraints["ndof"]
    free = 3 * torch.isfinite(torch.as_tensor(masses).detach().to(torch.float32)).to(torch.int64).cpu().reshape(-1)
    return torch.zeros(int(n_mol), dtype=torch.int64).index_add_(0, batch.detach().cpu(), free)


class DeviceGlobalMD(DeviceMD):
    """The object ``TorchMD_Net.capture_md_global`` returns: ``DeviceMD`` without a Langevin thermostat, whose every step ends with the
    move of a GLOBAL thermostat per molecule inside the graph (``tmdnet_md_thermostat``: stochastic velocity rescaling or a
    Nose-Hoover chain; the scheme is documented in include/tmdnet_amd.h and DESIGN.md section 13): all velocities of a molecule are
    multiplied by one factor alpha, so the relative motion of its atoms is left alone.  ``global_thermostat`` is the parsed dict,
    ``thermostat_ndof`` [B] int64 (host) the degrees of freedom the thermostat counts.  Static tensors rewritten by every replay:
    ``scale`` [K,B] float32, the factor applied after step k, and ``reservoir`` [K,B] float64, the energy the thermostat holds after
    step k in the unit of ``epot``; ``ekin`` [K,B] stays what the closing half's reduction wrote, the kinetic energy BEFORE the
    thermostat's move of that step.  ``chain`` [B,2,M] float64 is the live (xi, v_xi) of the Nose-Hoover chains (M = 0 for CSVR).
    An atom of infinite mass is no degree of freedom and is not scaled."""

    def __init__(self, model, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, warmup, thermostat,
                 constraints=None, observer=None):
        self.global_thermostat = thermostat
        self._thermo_ready = False
        super().__init__(model, z, pos, vel, masses, dt, batch, box, q, n_mol, steps_per_replay, force_scale, None, warmup, None,
                         constraints, observer)

    def _stage_thermostat(self):
        th, dev, K, B = self.global_thermostat, self.pos.device, self.steps_per_replay, self.n_mol
        self.thermostat_ndof = stage_ndof(th["ndof"], self.ndof, B)
        self._ndof32 = self.thermostat_ndof.to(torch.int32).to(dev).contiguous()
        self.scale = torch.zeros((K, B), dtype=torch.float32, device=dev)
        self.reservoir = torch.zeros((K, B), dtype=torch.float64, device=dev)
        nbytes = C.c_size_t(0)
        if _C.lib().tmdnet_md_thermostat_workspace_bytes(B, th["chain"], C.byref(nbytes)) != _C.OK:
            raise ValueError(f"capture_md_global: {B} molecules with a chain of {th['chain']} are not a valid layout")
        self._thermo_ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        # views into the workspace (256-aligned parts: alpha fp32 [B] | reservoir fp64 [B] | chain fp64 [B,2,M])
        up = lambda n: (n + 255) & ~255
        off = (-self._thermo_ws.data_ptr()) % 256
        r0 = off + up(4 * B)
        c0 = r0 + up(8 * B)
        M = th["chain"]
        self._reservoir_now = self._thermo_ws[r0:r0 + 8 * B].view(torch.float64)
        self.chain = self._thermo_ws[c0:c0 + 16 * B * M].view(torch.float64).view(B, 2, M)
        self._thermo_ready = True

    def _start(self, step):
        # the thermostat starts empty, at capture and at every reset: no energy held, chains at rest
        if not self._thermo_ready:
            self._stage_thermostat()
        self._thermo_ws.zero_()

    def _thermostat_move(self, open_next, forces, k):
        st, dev, th = self._model._engine, self.pos.device, self.global_thermostat
        rc = _C.lib().tmdnet_md_thermostat(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(self._ws), _ptr(self._thermo_ws),
                                           self.n_atoms, self.n_mol, THERMOSTAT_KINDS[th["kind"]], int(open_next), _ptr(self.pos),
                                           _ptr(self.vel), _ptr(forces), _ptr(self.hk), self.dt, _ptr(self.inputs[1]), _ptr(self.ekin[k]),
                                           _ptr(self._ndof32), th["kT"], th["tau"], th["chain"], th["substeps"], self.force_scale,
                                           th["seed"], _ptr(self.scale[k]), _ptr(self.reservoir[k]))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_md_thermostat: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def _capture_step(self, k, K, out):
        # CLOSE (kick, kinetic energy, step counter), the thermostat, and the opening half of the next step: fused into the scaling
        # launch, or with constraints the velocity projection and the constrained OPEN launch on the forces the closing half kept
        self._observe(k)
        self._advance(MD_CLOSE, out[1], out[0], k)
        more = k + 1 < K
        self._thermostat_move(more and self.constraints is None, out[1], k)
        if self.constraints is not None:
            # a uniform scaling keeps r.v_rel = 0, but multiplies the residual RATTLE left (within tol) by alpha: project again, which
            # changes nothing in a cluster that is still within tol
            self._advance(MD_PROJECT, None, None, k)
            if more:
                self._advance(MD_OPEN, self.forces, None, k)

    def kinetic_after(self) -> Tensor:
        """``scale``^2 ``ekin`` [K,B] float64: the kinetic energy after the thermostat's move of every step, unit of m v^2"""
        return self.scale.double() ** 2 * self.ekin.double()

    def conserved(self) -> Tensor:
        """``epot + kinetic_after() / force_scale + reservoir`` [K,B] float64: the energy the thermostatted dynamics conserves"""
        return self.epot.double() + self.kinetic_after() / self.force_scale + self.reservoir
