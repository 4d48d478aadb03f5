"""Observables of the device-resident MD loop (``TorchMD_Net.capture_md_observed``): sample frames, the radial distribution function,
the mean-square displacement and the velocity autocorrelation, recorded inside the captured graph by ``tmdnet_md_observe``
(csrc/tn_observe.hip; the scheme is documented in include/tmdnet_amd.h and DESIGN.md section 13, "Observables").

The observer is enqueued after the evaluation of a sampled step and before the integrator launch that closes it, where the bias
launch of ``capture_md_biased`` sits.  It reads ``pos`` (x at the full step s), ``vel`` and static tables and writes only into its own
workspace, so a loop with an observer and a loop without one walk the same trajectory bit for bit.  ``vel`` at that point is the
LEAPFROG velocity v(s - 1/2) - after the opening kick and, with constraints, after SHAKE's correction: the series is stationary and
its lags are whole multiples of ``every * dt``, so its autocorrelation is the velocity autocorrelation function.

This module is the host side: ``prepare_observe`` validates ``observe=dict(...)`` and builds the tables before anything is staged,
``Observer`` owns the workspace and turns the raw sums into the quantities a caller reads."""
import ctypes as C
import math

import torch

from torchmdnet_amd import _C
from torchmdnet_amd.models.utils import _ptr, _stream_ptr

_OBSERVE_KEYS = ("every", "frames", "rdf", "msd", "vacf")
_SUB_KEYS = {"frames": ("capacity", "velocities"), "rdf": ("pairs", "r_max", "bins"), "msd": ("groups", "capacity"),
             "vacf": ("lags", "groups")}
MSD_SHIFT, VACF_SHIFT = 8, 16  # tn_obs::kMsdShift, kVacfShift: where the group bits of the per-atom mask start


def _selector(s, what):
    if s is None:
        return None
    if isinstance(s, bool) or not isinstance(s, int) or s < 0:
        raise ValueError(f"observe: {what} must be an atomic number or None (every species), got {s!r}")
    return int(s)


def _selectors(groups, what):
    groups = list(groups) if groups is not None else []
    if not 1 <= len(groups) <= _C.OBSERVE_MAX_TYPES:
        raise ValueError(f"observe: {what} needs 1 to {_C.OBSERVE_MAX_TYPES} groups, got {len(groups)}")
    return [_selector(g, f"a group of {what}") for g in groups]


def parse_observe(observe, steps_per_replay):
    """``observe=dict(every=S, frames=, rdf=, msd=, vacf=)`` -> the same with every key present and every value checked; nothing here
    needs the system.  Raises ValueError."""
    if not isinstance(observe, dict):
        raise ValueError("capture_md_observed needs observe=dict(every=, frames= | rdf= | msd= | vacf=); without one use capture_md")
    unknown = set(observe) - set(_OBSERVE_KEYS)
    if unknown:
        raise ValueError(f"observe: unknown keys {sorted(unknown)} ({', '.join(_OBSERVE_KEYS)})")
    S, K = observe.get("every", 1), int(steps_per_replay)
    if isinstance(S, bool) or not isinstance(S, int) or S < 1:
        raise ValueError(f"observe: every must be an integer of at least 1 step, got {S!r}")
    if K % S:
        raise ValueError(f"observe: every={S} must divide steps_per_replay={K}: the sampled positions of a replay are fixed at capture")
    out = dict(every=S, frames=None, rdf=None, msd=None, vacf=None)
    for name in ("frames", "rdf", "msd", "vacf"):
        sub = observe.get(name)
        if sub is None:
            continue
        if not isinstance(sub, dict):
            raise ValueError(f"observe: {name} must be a dict({', '.join(k + '=' for k in _SUB_KEYS[name])})")
        unknown = set(sub) - set(_SUB_KEYS[name])
        if unknown:
            raise ValueError(f"observe: {name} has unknown keys {sorted(unknown)} ({', '.join(_SUB_KEYS[name])})")
        out[name] = dict(sub)
    if all(out[k] is None for k in ("frames", "rdf", "msd", "vacf")):
        raise ValueError("observe: needs at least one observable of frames=, rdf=, msd=, vacf=")
    if out["frames"] is not None:
        F = int(out["frames"].get("capacity", 0))
        if not 1 <= F <= 1 << 24:
            raise ValueError(f"observe: frames needs capacity >= 1 frames, got {F}")
        out["frames"] = dict(capacity=F, velocities=bool(out["frames"].get("velocities", False)))
    if out["rdf"] is not None:
        r = out["rdf"]
        pairs = list(r.get("pairs") or [])
        if not 1 <= len(pairs) <= _C.OBSERVE_MAX_TYPES:
            raise ValueError(f"observe: rdf needs 1 to {_C.OBSERVE_MAX_TYPES} pair types, got {len(pairs)}")
        if any(not hasattr(p, "__len__") or len(p) != 2 for p in pairs):
            raise ValueError(f"observe: every rdf pair type is (za, zb), got {pairs}")
        pairs = [(_selector(a, "an rdf selector"), _selector(b, "an rdf selector")) for a, b in pairs]
        if "r_max" not in r or "bins" not in r:
            raise ValueError("observe: rdf needs r_max= and bins=")
        r_max, bins = float(r["r_max"]), int(r["bins"])
        if not (r_max > 0 and math.isfinite(r_max)):
            raise ValueError(f"observe: rdf r_max must be positive, got {r_max}")
        if not 1 <= bins <= _C.OBSERVE_MAX_BINS:
            raise ValueError(f"observe: rdf bins must be 1..{_C.OBSERVE_MAX_BINS}, got {bins}")
        out["rdf"] = dict(pairs=pairs, r_max=r_max, bins=bins)
    if out["msd"] is not None:
        T = int(out["msd"].get("capacity", 0))
        if not 1 <= T <= 1 << 32:
            raise ValueError(f"observe: msd needs capacity >= 1 samples, got {T}")
        out["msd"] = dict(groups=_selectors(out["msd"].get("groups"), "msd"), capacity=T)
    if out["vacf"] is not None:
        L = int(out["vacf"].get("lags", 0))
        if not 1 <= L <= _C.OBSERVE_MAX_LAGS:
            raise ValueError(f"observe: vacf lags must be 1..{_C.OBSERVE_MAX_LAGS}, got {L}")
        out["vacf"] = dict(lags=L, groups=_selectors(out["vacf"].get("groups"), "vacf"))
    return out


def _matches(z, sel):
    return torch.ones_like(z, dtype=torch.bool) if sel is None else z == sel


def selector_masks(z, spec):
    """The per-atom mask ``tmdnet_md_observe`` reads, [N] int32 (host): rdf pair type p - selector a: bit 2p, selector b: bit 2p + 1;
    msd group g: bit 8 + g; vacf group g: bit 16 + g"""
    z = torch.as_tensor(z).detach().cpu().to(torch.int64).reshape(-1)
    mask = torch.zeros_like(z)
    if spec["rdf"] is not None:
        for p, (a, b) in enumerate(spec["rdf"]["pairs"]):
            mask |= _matches(z, a).to(torch.int64) << (2 * p)
            mask |= _matches(z, b).to(torch.int64) << (2 * p + 1)
    for name, shift in (("msd", MSD_SHIFT), ("vacf", VACF_SHIFT)):
        if spec[name] is not None:
            for g, sel in enumerate(spec[name]["groups"]):
                mask |= _matches(z, sel).to(torch.int64) << (shift + g)
    return mask.to(torch.int32)


def tile_table(sizes, tile=_C.OBSERVE_TILE):
    """[n,3] int32 (host): one row (m, it, jt), jt >= it, per pair of ``tile``-atom tiles of molecule m - one block of the histogram
    kernel each"""
    rows = []
    for m, n in enumerate(int(s) for s in sizes):
        nt = (n + tile - 1) // tile
        rows += [(m, i, j) for i in range(nt) for j in range(i, nt)]
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 3)


def box_heights(box):
    """[B,3] float64 (host): the distances between opposite faces of every box [B,3,3] (rows are the cell vectors)"""
    b = torch.as_tensor(box).detach().to(device="cpu", dtype=torch.float64).reshape(-1, 3, 3)
    vol = torch.linalg.det(b).abs()
    cr = torch.stack([torch.linalg.cross(b[:, 1], b[:, 2]), torch.linalg.cross(b[:, 2], b[:, 0]), torch.linalg.cross(b[:, 0], b[:, 1])], 1)
    return vol[:, None] / cr.norm(dim=2)


def check_r_max(r_max, box):
    """The minimum image of the engine is the nearest image only within half the smallest height of the box: ValueError beyond"""
    if box is None:
        return
    h = float(box_heights(box).min())
    if not r_max <= 0.5 * h:
        raise ValueError(f"observe: rdf r_max={r_max:g} exceeds half the smallest box height ({0.5 * h:g}): the minimum image would "
                         "miss pairs")


def refuse_keep(pos, vel, step, step_now):
    """``reset(observables="keep")`` continues the sums, which only means something on the same trajectory: ValueError unless ``pos`` and
    ``vel`` are None and ``step`` is the loop's current step"""
    if pos is not None or vel is not None or int(step) != int(step_now):
        raise ValueError(f"reset(observables='keep'): the sums continue only on an unchanged state - pos and vel must be None and step "
                         f"must stay {int(step_now)} (got pos {'given' if pos is not None else 'None'}, vel "
                         f"{'given' if vel is not None else 'None'}, step {int(step)}); use observables='clear'")


def prepare_observe(observe, z, batch, box, n_mol, steps_per_replay):
    """Everything ``Observer`` needs, on the host, before anything is staged: the parsed dict (``parse_observe``), the per-atom masks,
    the molecules' first atoms, the tile table of the histogram, and the selector and group sizes per molecule.  Raises ValueError."""
    spec = parse_observe(observe, steps_per_replay)
    zc = torch.as_tensor(z).detach().cpu().to(torch.int64).reshape(-1)
    n, B = int(zc.numel()), int(n_mol)
    bt = torch.zeros(n, dtype=torch.int64) if batch is None else torch.as_tensor(batch).detach().cpu().to(torch.int64).reshape(-1)
    if bt.numel() != n:
        raise ValueError(f"observe: batch must have one entry per atom ({n}), got {bt.numel()}")
    sizes = torch.bincount(bt, minlength=B)
    if sizes.numel() != B:
        raise ValueError(f"observe: batch names molecule {int(bt.max())}, outside the {B} molecules")
    out = dict(spec=spec, mask=selector_masks(zc, spec), sizes=sizes, tiles=None, mol_start=None)
    if spec["rdf"] is not None:
        if n > 1 and bool((bt[1:] < bt[:-1]).any()):
            raise ValueError("observe: rdf needs a sorted batch (the pair sweep walks each molecule's atoms as one contiguous range)")
        check_r_max(spec["rdf"]["r_max"], box)
        out["mol_start"] = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)]).to(torch.int32)
        out["tiles"] = tile_table(sizes.tolist())
        onehot = lambda sel: torch.zeros(B, dtype=torch.int64).index_add_(0, bt, _matches(zc, sel).to(torch.int64))  # noqa: E731
        out["n_a"] = torch.stack([onehot(a) for a, _ in spec["rdf"]["pairs"]], 1)  # [B,P]
        out["n_b"] = torch.stack([onehot(b) for _, b in spec["rdf"]["pairs"]], 1)
    for name in ("msd", "vacf"):
        if spec[name] is not None:
            out[name + "_sizes"] = torch.stack([torch.zeros(B, dtype=torch.int64).index_add_(0, bt, _matches(zc, g).to(torch.int64))
                                                for g in spec[name]["groups"]], 1)  # [B,G]
    return out


def normalize_rdf(counts, n_samples, n_a, n_b, same, r_max, volume=None):
    """counts [B,P,bins] int64, n_a / n_b [B,P], same [P] bool, volume [B] or None -> (r [bins], g [B,P,bins]) float64.  With a volume
    g = counts / (n_samples n_pairs shell / V), shell = 4 pi / 3 (r_hi^3 - r_lo^3); without one g = counts / (n_samples n_pairs);
    n_pairs = N_a N_b, or N_a (N_a - 1) / 2 when both selectors of the type are the same."""
    counts = torch.as_tensor(counts).to(torch.float64)
    bins = counts.shape[-1]
    edges = torch.arange(bins + 1, dtype=torch.float64) * (float(r_max) / bins)
    n_a, n_b = torch.as_tensor(n_a).to(torch.float64), torch.as_tensor(n_b).to(torch.float64)
    same = torch.as_tensor(same, dtype=torch.bool)
    n_pairs = torch.where(same[None, :], 0.5 * n_a * (n_a - 1.0), n_a * n_b)  # [B,P]
    ideal = float(n_samples) * n_pairs[:, :, None].expand(-1, -1, bins).clone()
    if volume is not None:
        shell = 4.0 * math.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
        ideal = ideal * shell[None, None, :] / torch.as_tensor(volume, dtype=torch.float64).reshape(-1, 1, 1)
    return 0.5 * (edges[1:] + edges[:-1]), counts.cpu() / ideal


class Observer:
    """The observer of one captured MD loop: the workspace of ``tmdnet_md_observe``, the tables it reads and the accessors behind
    ``md.frames() / rdf() / msd() / vacf() / n_samples``.  ``prep`` is ``prepare_observe``'s result."""

    def __init__(self, prep, n_atoms, n_mol, dt, dev):
        sp = self.spec = prep["spec"]
        self.prep, self.n_atoms, self.n_mol, self.dt, self.s0 = prep, int(n_atoms), int(n_mol), float(dt), 0
        fr, rdf, msd, vacf = sp["frames"], sp["rdf"], sp["msd"], sp["vacf"]
        cs = self.cspec = _C.ObserveSpec()
        cs.every = sp["every"]
        cs.frame_capacity, cs.frame_velocities = (fr["capacity"], int(fr["velocities"])) if fr else (0, 0)
        cs.n_pair_types, cs.bins = (len(rdf["pairs"]), rdf["bins"]) if rdf else (0, 0)
        # r_max^2 and bins / r_max in fp64, rounded once: what the fp32 mirror of the bin uses too
        cs.r_max2 = float(torch.tensor(rdf["r_max"] * rdf["r_max"], dtype=torch.float64).to(torch.float32)) if rdf else 0.0
        cs.inv_dr = float(torch.tensor(rdf["bins"] / rdf["r_max"], dtype=torch.float64).to(torch.float32)) if rdf else 0.0
        cs.n_msd_groups, cs.msd_capacity = (len(msd["groups"]), msd["capacity"]) if msd else (0, 0)
        cs.n_vacf_groups, cs.lags = (len(vacf["groups"]), vacf["lags"]) if vacf else (0, 0)
        nbytes = C.c_size_t(0)
        if _C.lib().tmdnet_md_observe_workspace_bytes(self.n_atoms, self.n_mol, C.byref(cs), C.byref(nbytes)) != _C.OK:
            raise ValueError(f"capture_md_observed: {self.n_atoms} atoms in {self.n_mol} molecules with {sp} are not a valid layout")
        self._ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
        self._mask = prep["mask"].to(dev).contiguous()
        self._mol_start = None if prep["mol_start"] is None else prep["mol_start"].to(dev).contiguous()
        self._tiles = None if prep["tiles"] is None else prep["tiles"].to(dev).contiguous()
        # views into the workspace: the arrays of the layout in its order, each on a multiple of 256 bytes (include/tmdnet_amd.h)
        N, B, F, P, bins, T, L = self.n_atoms, self.n_mol, cs.frame_capacity, cs.n_pair_types, cs.bins, cs.msd_capacity, cs.lags
        Gm, Gv = cs.n_msd_groups, cs.n_vacf_groups
        off = (-self._ws.data_ptr()) % 256 + 256

        def take(count, dtype, shape):
            nonlocal off
            nb = count * torch.empty(0, dtype=dtype).element_size()
            view = self._ws[off:off + nb].view(dtype).view(shape) if count else None
            off += (nb + 255) & ~255
            return view

        self._frame_pos = take(F * N * 3, torch.float32, (F, N, 3))
        self._frame_vel = take(F * N * 3 if cs.frame_velocities else 0, torch.float32, (F, N, 3))
        self._counts = take(B * P * bins, torch.int64, (B, P, bins))
        self._origin = take(N * 3 if Gm else 0, torch.float32, (N, 3))
        self._msd = take(T * B * Gm, torch.float64, (T, B, Gm))
        self._ring = take(L * N * 3 if Gv else 0, torch.float32, (L, N, 3))
        self._acc = take(B * Gv * L, torch.float64, (B, Gv, L))

    def _need(self, name):
        if self.spec[name] is None:
            raise ValueError(f"{name}(): this loop was captured without observe=dict({name}=...)")
        return self.spec[name]

    def start(self, md, step):
        """New origins and a new s0, everything else cleared (capture, and ``reset(observables="clear")``)"""
        self.s0 = int(step)
        dev = md.pos.device
        rc = _C.lib().tmdnet_md_observe_start(_stream_ptr(dev), _ptr(self._ws), self.n_atoms, self.n_mol, C.byref(self.cspec), self.s0,
                                              _ptr(md.pos))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_md_observe_start failed (code {rc})")

    def launch(self, md):
        st, dev = md._model._engine, md.pos.device
        box = md.box
        rc = _C.lib().tmdnet_md_observe(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(md._ws), _ptr(self._ws), self.n_atoms,
                                        self.n_mol, C.byref(self.cspec), _ptr(md.pos), _ptr(md.vel), _ptr(md.inputs[1]), _ptr(box),
                                        0 if box is None else (1 if box.dim() == 2 else 2), _ptr(self._mask), _ptr(self._mol_start),
                                        _ptr(self._tiles), 0 if self._tiles is None else int(self._tiles.shape[0]))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_md_observe: {_C.lib().tmdnet_last_error(st.handle).decode()} (code {rc})")

    def check_box(self, box):
        if self.spec["rdf"] is not None:
            check_r_max(self.spec["rdf"]["r_max"], box)

    def n_samples(self, md) -> int:
        """samples recorded, from the DEVICE's step counter (one synchronisation): a frozen loop reports what it recorded"""
        step = md._status(_C.lib().tmdnet_md_status, 2)[1][0]
        return (step - self.s0) // self.spec["every"] if step > self.s0 else 0

    def _steps(self, j):
        return self.s0 + (j + 1) * self.spec["every"]

    def frames(self, md):
        fr = self._need("frames")
        ns, F = self.n_samples(md), fr["capacity"]
        j = torch.arange(max(ns - F, 0), ns, dtype=torch.int64)  # oldest first
        slots = (j % F).to(self._frame_pos.device)
        out = (self._steps(j), self._frame_pos[slots].clone())
        return out + (self._frame_vel[slots].clone(),) if fr["velocities"] else out

    def rdf(self, md):
        r = self._need("rdf")
        ns = self.n_samples(md)
        counts = self._counts.clone()
        vol = None if md.box is None else torch.linalg.det(md.box.detach().to(device="cpu", dtype=torch.float64).reshape(-1, 3, 3)).abs()
        if vol is not None and vol.numel() == 1:
            vol = vol.expand(self.n_mol)
        same = [a == b for a, b in r["pairs"]]
        centres, g = normalize_rdf(counts.cpu(), ns, self.prep["n_a"], self.prep["n_b"], same, r["r_max"], vol)
        return centres, g, counts

    def msd(self, md):
        m = self._need("msd")
        n = min(self.n_samples(md), m["capacity"])
        steps = self._steps(torch.arange(n, dtype=torch.int64))
        return steps, self._msd[:n].clone() / self.prep["msd_sizes"].to(self._msd.device, torch.float64)[None]

    def vacf(self, md):
        v = self._need("vacf")
        ns, L = self.n_samples(md), v["lags"]
        lags = torch.arange(L, dtype=torch.float64)
        n = torch.clamp(ns - lags, min=0.0)
        n = torch.where(n > 0, n, torch.full_like(n, float("nan"))).to(self._acc.device)
        c = self._acc.clone() / n[None, None, :] / self.prep["vacf_sizes"].to(self._acc.device, torch.float64)[:, :, None]
        return lags * (self.spec["every"] * self.dt), c
