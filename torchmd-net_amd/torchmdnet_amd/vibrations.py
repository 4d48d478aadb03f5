"""Hessians and normal-mode analysis assembled on the device (``TorchMD_Net.hessian`` / ``TorchMD_Net.vibrations``).

The molecules of a batch are independent, so R replicas of the batch, each carrying ONE coordinate of every molecule, give R Hessian
columns of every molecule from one evaluation of the replicated batch: analytically, ``hv = H v`` of the engine's second-order pass
with a unit seed (``method="analytic"``), or as a central difference of the forces of two displaced evaluations
(``method="central"``).  Seeding / displacing the replicated batch, gathering the columns into per-molecule matrices and the fp64
symmetrisation, mass weighting and projection of translations and rotations are HIP kernels (csrc/tn_vib.hip, ``tmdnet_vib_*``);
the eigen-decomposition of the small per-molecule matrices is ``torch.linalg.eigh`` in fp64 on the host.  The scheme and its rounding
are documented with the C entries in include/tmdnet_amd.h and in DESIGN.md section 16."""
import ctypes as C
import math
from typing import List, Optional

import torch
from torch import Tensor

from torchmdnet_amd import _C
from torchmdnet_amd.models.utils import _ptr, _require_cuda, _stream_ptr

METHODS = ("analytic", "central")
#: cm^-1 of sqrt(1 eV / (Angstrom^2 amu)): sqrt(9.648533212e27 s^-2) / (2 pi c)
WAVENUMBER = 521.4709
#: hbar in eV fs (CODATA 2018), the unit of ``zero_point_energy`` under the default ``force_scale``
HBAR_EV_FS = 0.6582119569
MAX_REPLICAS = 65535  # the gather's grid has one row of blocks per replica


def plan_columns(batch: Tensor, fixed: Optional[Tensor], n_mol: int):
    """Host tensors: ``batch`` [N] non-decreasing, ``fixed`` [N] bool or None -> (free_idx [n_free], fstart [n_mol + 1], dims [n_mol]):
    the free atoms in the caller's order, the molecules' offsets into them, and D_b = 3 nfree_b."""
    free = torch.ones(batch.shape, dtype=torch.bool) if fixed is None else ~fixed
    free_idx = torch.nonzero(free).reshape(-1).to(torch.long)
    nfree = torch.bincount(batch[free_idx], minlength=n_mol)[:n_mol] if n_mol else torch.zeros(0, dtype=torch.long)
    fstart = torch.zeros(n_mol + 1, dtype=torch.long)
    fstart[1:] = torch.cumsum(nfree, 0)
    return free_idx, fstart, 3 * nfree


def check_request(z, pos, batch, q, method, delta, fixed, replicas, masses=None):
    """Everything that is refused with ValueError, on host copies, before anything is staged.  -> (batch, fixed, n_mol) on the host."""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    if not (float(delta) > 0 and math.isfinite(float(delta))):
        raise ValueError(f"delta must be positive and finite, got {delta}")
    if replicas is not None and not 1 <= int(replicas) <= MAX_REPLICAS:
        raise ValueError(f"replicas must be between 1 and {MAX_REPLICAS}, got {replicas}")
    n = int(z.shape[0])
    if pos.dim() != 2 or tuple(pos.shape) != (n, 3):
        raise ValueError(f"pos must be [{n},3] for {n} atoms, got {tuple(pos.shape)}")
    bh = torch.zeros(n, dtype=torch.long) if batch is None else batch.detach().reshape(-1).to("cpu", torch.long)
    if bh.numel() != n:
        raise ValueError(f"batch must have one entry per atom ({n}), got {bh.numel()}")
    if n and (int(bh[0]) < 0 or bool((bh[1:] < bh[:-1]).any())):
        raise ValueError("batch must be non-decreasing: the atoms of a molecule are contiguous and the molecules in order")
    n_mol = int(bh[-1]) + 1 if n else 0
    fh = None
    if fixed is not None:
        if fixed.numel() != n:
            raise ValueError(f"fixed must have one entry per atom ({n}), got {fixed.numel()}")
        fh = fixed.detach().reshape(-1).to("cpu") != 0
    if q is not None and q.numel() != n_mol:
        raise ValueError(f"q must have one entry per molecule ({n_mol}), got {q.numel()}")
    if masses is not None:
        if masses.numel() != n:
            raise ValueError(f"masses must have one entry per atom ({n}), got {masses.numel()}")
        mh = masses.detach().reshape(-1).to("cpu", torch.float64)
        free = torch.ones(n, dtype=torch.bool) if fh is None else ~fh
        if not bool((torch.isfinite(mh[free]) & (mh[free] > 0)).all()):
            raise ValueError("masses must be positive and finite on every free atom")
    return bh, fh, n_mol


def _replicate(z, batch, box, q, n_mol, R):
    """z, batch, q and the boxes of R replicas (plumbing): replica r holds the molecules r B .. r B + B - 1"""
    zr = z.repeat(R)
    br = (batch[None, :] + n_mol * torch.arange(R, device=batch.device, dtype=batch.dtype)[:, None]).reshape(-1).contiguous()
    qr = None if q is None else q.reshape(-1).repeat(R)
    boxr = box if box is None or box.dim() == 2 else box.repeat(R, 1, 1)
    return zr, br, boxr, qr


def _pick_replicas(limit, fits):
    """the largest R in [1, limit] with fits(R); 1 when none does (fits is monotone)"""
    lo, hi = 1, max(int(limit), 1)
    if fits(hi):
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid
    return lo


def compute_hessian(model, z, pos, batch, box, q, method, delta, fixed, replicas, max_workspace_bytes, atom_weights=None):
    """``TorchMD_Net.hessian``: -> (H [B,D,D] fp32 on the device, info dict)."""
    if model._head_kind() != _C.HEAD_SCALAR:
        raise NotImplementedError(f"hessian has no HIP path with output_model {type(model.output_model).__name__}: neither route "
                                  "has a property head")
    if method == "analytic" and atom_weights is not None:
        raise NotImplementedError("hessian(method='analytic') has no HIP path with atom weights: the second-order pass takes none")
    if method == "analytic":  # the second-order pass knows the model only; method="central" sees the priors through energy_and_forces
        model._refuse_pair_priors("hessian(method='analytic'); take method='central'")
    bh, fh, n_mol = check_request(z, pos, batch, q, method, delta, fixed, replicas)
    if atom_weights is not None and atom_weights.numel() != z.shape[0]:
        raise ValueError(f"atom_weights must have one entry per atom ({z.shape[0]}), got {atom_weights.numel()}")
    _require_cuda(pos, "TorchMD_Net.hessian")
    if pos.dtype != torch.float32:
        raise NotImplementedError("torchmdnet_amd computes in fp32; cast positions to float32")
    L = _C.lib()
    dev = pos.device
    rm = model.representation_model
    if box is None and rm.distance.use_periodic:
        box = rm.distance.box
    if model._is_et():
        q = None  # TorchMD_ET.forward ignores q
    free_h, fstart_h, dims_h = plan_columns(bh, fh, n_mol)
    N, n_free = int(z.shape[0]), int(free_h.numel())
    D = int(dims_h.max()) if n_mol else 0
    info = dict(method=method, delta=float(delta), n_mol=n_mol, dim=D, dims=[int(d) for d in dims_h], replicas=0, passes=0,
                engine_calls=0, graph_builds=0, workspace_bytes=0)
    with torch.cuda.device(dev):
        z = z.detach().to(device=dev, dtype=torch.long).contiguous()
        p32 = pos.detach().contiguous()
        batch = bh.to(dev)
        box = None if box is None else box.detach().to(device=dev, dtype=torch.float32).contiguous()
        q = None if q is None else q.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        free_idx, fstart = free_h.to(dev), fstart_h.to(dev)
        info.update(batch=batch, free_idx=free_idx, fstart=fstart, box=box)
        H = torch.zeros((n_mol, D, D), dtype=torch.float32, device=dev)  # zeroed once; the passes write the valid entries only
        if D == 0:
            return H, info
        st = model._sync_engine()
        stream = _stream_ptr(dev)
        static = bool(getattr(rm, "static_shapes", False))
        box_mode = 0 if box is None else (1 if box.dim() == 2 else 2)
        counts = (C.c_int64 * 8)()

        def build_graph(zz, pp, bb, xx, n, nm):
            """the exact-count graph of the parameter-gradient passes (brute force inside each molecule) -> (n_pairs, n_edges)"""
            L.tmdnet_set_cell_grid(st.handle, 0, 0, 0)
            nbytes = C.c_size_t(0)
            L.tmdnet_graph_workspace_bytes(st.handle, n, nm, C.byref(nbytes))
            st.graph_ws = model._grow(st.graph_ws, nbytes.value, dev)
            rc = model._build_graph_for_a_training_pass(st, stream, n, nm, pp, bb, zz, xx, box_mode, counts)
            model._raise_bad_indices(counts, L.tmdnet_last_error(st.handle).decode())
            if rc != _C.OK:
                raise RuntimeError(L.tmdnet_last_error(st.handle).decode())
            st.ws_epoch = getattr(st, "ws_epoch", 0) + 1  # the graph workspace was rebuilt: a kept forward half is stale
            info["graph_builds"] += 1
            return int(counts[0]), int(counts[1])

        def workspace(R, pairs1, edges1):
            nb = C.c_size_t(0)
            if method == "analytic":
                rc = L.tmdnet_force_param_workspace_bytes(st.handle, R * N, R * n_mol, R * pairs1, C.byref(nb))
            else:
                rc = L.tmdnet_forward_workspace_bytes(st.handle, R * N, R * n_mol, -1 if static else R * pairs1, -1 if static else R * edges1,
                                                      1, C.byref(nb))
            return nb.value if rc == _C.OK else None

        row_limit = max(min(MAX_REPLICAS, ((2**31 - 1) // 4) // max(N, 1)), 1)
        if replicas is None:
            pairs1, edges1 = (0, 0) if (static and method == "central") else build_graph(z, p32, batch, box, N, n_mol)

            def fits(R):
                w = workspace(R, pairs1, edges1)
                return w is not None and w <= int(max_workspace_bytes)

            R = _pick_replicas(min(D, row_limit), fits)
        else:
            R = int(replicas)
            if R > row_limit:
                raise ValueError(f"replicas = {R} of {N} atoms exceed what one evaluation can index; at most {row_limit}")
        passes = (D + R - 1) // R
        zr, br, boxr, qr = _replicate(z, batch, box, q, n_mol, R)
        seed_args = (N, n_mol, R)
        idx_args = (_ptr(batch), _ptr(free_idx), _ptr(fstart))

        def check(rc, what):
            if rc != _C.OK:
                raise RuntimeError(f"{what} failed (code {rc})")

        if method == "analytic":
            pr = p32.repeat(R, 1).contiguous()
            n_pairs, _ = build_graph(zr, pr, br, boxr, R * N, R * n_mol)  # ONE graph: the positions are the same in every pass
            hb = C.c_size_t(0)
            if L.tmdnet_force_param_workspace_bytes(st.handle, R * N, R * n_mol, n_pairs, C.byref(hb)) != _C.OK:
                raise RuntimeError(L.tmdnet_last_error(st.handle).decode())
            st.hvp_ws = model._grow(getattr(st, "hvp_ws", None), hb.value, dev)
            gfl = C.c_int64(0)
            L.tmdnet_train_workspace_bytes(st.handle, R * N, R * n_mol, n_pairs, None, None, C.byref(gfl))
            flat = torch.empty(gfl.value, dtype=torch.float32, device=dev)  # the weight gradients: allocated once, ignored
            v = torch.empty((R * N, 3), dtype=torch.float32, device=dev)
            hv = torch.empty((R * N, 3), dtype=torch.float32, device=dev)
            info["workspace_bytes"] = hb.value
            for col0 in range(0, D, R):
                check(L.tmdnet_vib_seed(stream, _C.VIB_SEED, *seed_args, col0, None, *idx_args, 0.0, _ptr(v)), "tmdnet_vib_seed")
                rc = L.tmdnet_loss_param_grads(st.handle, stream, _ptr(st.graph_ws), _ptr(st.hvp_ws), st.hvp_ws.numel(), R * N, R * n_mol,
                                               n_pairs, _ptr(zr), _ptr(br), _ptr(qr), _ptr(v), None, _ptr(flat), _ptr(hv))
                if rc != _C.OK:
                    raise RuntimeError(f"tmdnet_loss_param_grads: {L.tmdnet_last_error(st.handle).decode()} (code {rc})")
                info["engine_calls"] += 1
                check(L.tmdnet_vib_gather(stream, _C.VIB_ANALYTIC, N, n_mol, n_free, D, R, col0, *idx_args, _ptr(hv), None, None, None,
                                          _ptr(H)), "tmdnet_vib_gather")
            st.ws_epoch = getattr(st, "ws_epoch", 0) + 1
        else:
            xp = torch.empty((R * N, 3), dtype=torch.float32, device=dev)
            xm = torch.empty((R * N, 3), dtype=torch.float32, device=dev)
            wr = None if atom_weights is None else atom_weights.detach().to(device=dev, dtype=torch.float32).reshape(-1).repeat(R)
            for col0 in range(0, D, R):
                check(L.tmdnet_vib_seed(stream, _C.VIB_PLUS, *seed_args, col0, _ptr(p32), *idx_args, float(delta), _ptr(xp)), "tmdnet_vib_seed")
                check(L.tmdnet_vib_seed(stream, _C.VIB_MINUS, *seed_args, col0, _ptr(p32), *idx_args, float(delta), _ptr(xm)), "tmdnet_vib_seed")
                _, fp = model.energy_and_forces(zr, xp, br, boxr, qr, R * n_mol, want_forces=True, atom_weights=wr)
                _, fm = model.energy_and_forces(zr, xm, br, boxr, qr, R * n_mol, want_forces=True, atom_weights=wr)
                info["engine_calls"] += 2
                check(L.tmdnet_vib_gather(stream, _C.VIB_CENTRAL, N, n_mol, n_free, D, R, col0, *idx_args, _ptr(fp), _ptr(fm), _ptr(xp),
                                          _ptr(xm), _ptr(H)), "tmdnet_vib_gather")
            n_pairs, n_edges = (-1, -1) if static else getattr(st, "counts", (0, 0, 0))[:2]
            nb = C.c_size_t(0)
            L.tmdnet_forward_workspace_bytes(st.handle, R * N, R * n_mol, n_pairs, n_edges, 1, C.byref(nb))
            info["workspace_bytes"] = nb.value  # what the last evaluation asked for
        info.update(replicas=R, passes=passes)
    return H, info


class Vibrations:
    """What ``TorchMD_Net.vibrations`` returns.  B molecules, molecule b with D_b = 3 nfree_b coordinates; E, length, mass are the
    units of the model's energies, the positions and ``masses``.

    ``hessian`` [B,D,D] fp32 on the device (padded, E / length^2); ``eigenvalues``: a list of B fp64 tensors [D_b], ascending, in
    E / (length^2 mass); ``modes``: a list of [D_b,D_b] fp64 tensors whose COLUMNS are the mass-weighted eigenvectors;
    ``omega2 = eigenvalues * force_scale``; ``n_projected`` [B] the rank of the projected translations / rotations (their
    eigenvalues are zero up to rounding); ``asymmetry``, ``drift``, ``hmax`` [B] fp64: max |H_ij - H_ji|, the acoustic sum
    max | sum_j H[i, 3 j + beta] | (meaningful only without fixed atoms) and max |H_ij| of the assembled Hessian; ``amax`` [B]:
    max |A_ij| of the mass-weighted projected matrix; ``dims`` [B]; ``masses`` [N]; ``free_idx`` / ``fstart``: the free atoms and
    the molecules' offsets into them; ``method``, ``replicas``, ``passes``, ``engine_calls``: how the Hessian was assembled."""

    def __init__(self, hessian, info, A, rows, masses, force_scale):
        self.hessian = hessian
        self.method, self.replicas, self.passes, self.engine_calls = info["method"], info["replicas"], info["passes"], info["engine_calls"]
        self.dims = list(info["dims"])
        self.free_idx, self.fstart = info["free_idx"].cpu(), info["fstart"].cpu()
        self.masses = masses.detach().cpu().to(torch.float64)
        self.force_scale = float(force_scale)
        self.hmax, self.asymmetry, self.drift = rows[:, 0].clone(), rows[:, 1].clone(), rows[:, 2].clone()
        self.n_projected = rows[:, 3].to(torch.long)
        self.eigenvalues: List[Tensor] = []
        self.modes: List[Tensor] = []
        amax = []
        for b, d in enumerate(self.dims):
            a = A[b, :d, :d]
            amax.append(float(a.abs().max()) if d else 0.0)
            lam, vec = torch.linalg.eigh(a) if d else (torch.zeros(0, dtype=torch.float64), torch.zeros((0, 0), dtype=torch.float64))
            self.eigenvalues.append(lam)
            self.modes.append(vec)
        self.amax = torch.tensor(amax, dtype=torch.float64)

    @property
    def omega2(self):
        return [lam * self.force_scale for lam in self.eigenvalues]

    def _sqrt_mass(self, b):
        idx = self.free_idx[self.fstart[b]:self.fstart[b + 1]]
        return self.masses[idx].repeat_interleave(3).sqrt()

    def displacements(self):
        """Cartesian displacement patterns: the columns of ``modes`` divided by sqrt(m) of their coordinate (not renormalised)"""
        return [vec / self._sqrt_mass(b)[:, None] for b, vec in enumerate(self.modes)]

    def wavenumbers(self):
        """sign(lambda) sqrt(|lambda|) * 521.4709 cm^-1 for eV, Angstrom and amu; an imaginary mode is negative, as ASE prints it"""
        return [torch.sign(lam) * lam.abs().sqrt() * WAVENUMBER for lam in self.eigenvalues]

    def default_tolerance(self):
        """D_b * 1e-4 * max |A_b|: the bound on an eigenvalue's error when every entry of A is good to 1e-4 of the largest (Weyl)"""
        return [d * 1e-4 * float(a) for d, a in zip(self.dims, self.amax)]

    def n_negative(self, tol=None):
        """per molecule, the number of eigenvalues below -tol (default ``default_tolerance()``): 0 at a minimum, 1 at a first-order
        saddle"""
        tols = self.default_tolerance() if tol is None else [float(tol)] * len(self.dims)
        return [int((lam < -t).sum()) for lam, t in zip(self.eigenvalues, tols)]

    def vibrational(self):
        """per molecule, the eigenvalues outside the projected ones: the n_projected eigenvalues of smallest magnitude are dropped"""
        out = []
        for lam, k in zip(self.eigenvalues, self.n_projected.tolist()):
            keep = torch.ones(lam.numel(), dtype=torch.bool)
            keep[torch.argsort(lam.abs())[:k]] = False
            out.append(lam[keep])
        return out

    def zero_point_energy(self, hbar=HBAR_EV_FS):
        """[B] fp64: hbar / 2 * sum of omega over the positive modes outside the projected ones, omega = sqrt(omega2); ``hbar`` in
        E * (the time unit ``force_scale`` implies) - eV fs for the default ``force_scale``"""
        return torch.stack([0.5 * hbar * (lam[lam > 0] * self.force_scale).sqrt().sum() for lam in self.vibrational()]) \
            if self.dims else torch.zeros(0, dtype=torch.float64)


def compute_vibrations(model, z, pos, batch, box, q, masses, project, force_scale, **hessian_kw):
    """``TorchMD_Net.vibrations``."""
    from torchmdnet_amd.atomic_masses import atomic_masses

    kw = dict(method="analytic", delta=0.01, fixed=None, replicas=None, max_workspace_bytes=8 << 30)
    unknown = set(hessian_kw) - set(kw) - {"atom_weights"}
    if unknown:
        raise TypeError(f"vibrations() got unexpected keyword arguments {sorted(unknown)}")
    kw.update(hessian_kw)
    if masses is None:
        zh = z.detach().reshape(-1).to("cpu", torch.long)
        if zh.numel() and (int(zh.min()) < 0 or int(zh.max()) >= len(atomic_masses)):
            raise ValueError(f"z holds an element outside the mass table (0 .. {len(atomic_masses) - 1}); pass masses=")
        masses = torch.from_numpy(atomic_masses)[zh]
    # the masses are checked with the rest, before anything is staged
    check_request(z, pos, batch, q, kw["method"], kw["delta"], kw["fixed"], kw["replicas"], masses=masses)
    H, info = compute_hessian(model, z, pos, batch, box, q, **kw)
    L = _C.lib()
    dev = pos.device
    n_mol, D, N = info["n_mol"], info["dim"], int(z.shape[0])
    with torch.cuda.device(dev):
        m32 = masses.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        p32 = pos.detach().contiguous()
        A = torch.empty((n_mol, D, D), dtype=torch.float64, device=dev)
        rows = torch.zeros((n_mol, _C.VIB_INFO), dtype=torch.float64, device=dev)
        nb = C.c_size_t(0)
        if L.tmdnet_vib_workspace_bytes(n_mol, D, C.byref(nb)) != _C.OK:
            raise ValueError(f"{n_mol} molecules of {D} coordinates are beyond what tmdnet_vib_workspace_bytes accepts")
        ws = torch.empty(max(nb.value, 8), dtype=torch.uint8, device=dev)
        mol_atoms = torch.bincount(info["batch"], minlength=n_mol)[:n_mol].contiguous() if n_mol else torch.zeros(0, dtype=torch.long, device=dev)
        mode = _C.VIB_PROJECT_NONE if not project else (_C.VIB_PROJECT_TRANS if info["box"] is not None else _C.VIB_PROJECT_TRANS_ROT)
        rc = L.tmdnet_vib_finish(_stream_ptr(dev), _ptr(ws), ws.numel(), N, n_mol, D, mode, _ptr(H), _ptr(p32), _ptr(m32), _ptr(info["free_idx"]),
                                 _ptr(info["fstart"]), _ptr(mol_atoms), _ptr(A), _ptr(rows))
        if rc != _C.OK:
            raise RuntimeError(f"tmdnet_vib_finish failed (code {rc})")
        A_h, rows_h = A.cpu(), rows.cpu()  # the one read-back: B small matrices for the host eigensolver
    return Vibrations(H, info, A_h, rows_h, m32, force_scale)
