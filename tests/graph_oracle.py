"""TEST INFRASTRUCTURE ONLY -- float64 numpy specification of the neighbour graph that tmdnet_build_graph[_static] leaves in its
workspace (csrc/tn_graph_wave.hip, tn_kernels.hip, tn_cell.hip; read back through tmdnet_debug_graph): the deterministic pair list
pair_i / pair_j / pd / pdelta / prhat (lower pairs i > j sorted by (i, j), the self pair at index P with pd[P] = 0), the symmetric
CSR rowptr / col / epair / esign (columns ascending, the self edge with pair id P and sign 0, a lower edge +1, an upper edge -1
with the id of the lower edge), the per-row counts and their prefix sums, the flags counts[0..5] = (P, E, overflow, unsorted
batch, z out of range, batch out of range) and, on the cell route, the renumbering perm (stable sort by cell id) with z_c and bat_c.

The minimum image is the engine's and the reference's statement - sequential rounding z -> y -> x (reference
tests/test_neighbors.py:19-27) - not the true nearest image; the two differ in strongly skewed boxes, and the engine is kept as the
reference has it.  Inputs are the fp32 positions and box widened to float64.  `margins` reports how far the case stays from every
decision a rounding could flip (tests/test_graph_oracle.py asserts them), so that the device comparison can be exact."""
import numpy as np


def min_image(d, box, margins=None, tie=None):
    """d [n, 3] float64, box [3, 3] (rows a, b, c of the reduced lower-triangular form) or None; tie [n] (optional) receives
    the smallest distance of a scaled difference from a half-integer, where roundf could go either way."""
    if box is None:
        return d
    d = d.copy()
    for ax in (2, 1, 0):
        s = d[:, ax] / box[ax, ax]
        if len(s):
            t = np.abs(np.abs(s - np.floor(s)) - 0.5)
            if margins is not None:
                margins["round"] = min(margins["round"], float(t.min()))
            if tie is not None:
                np.minimum(tie, t, out=tie)
        d -= np.outer(np.round(s), box[ax])
    return d


def grid_cap(n_atoms):
    ncap = 1
    while (ncap + 1) ** 3 <= 8 * n_atoms:
        ncap += 1
    return ncap


def cell_grid(pos, box, up, explicit=None, margins=None):
    """-> (grid [nx, ny, nz, cells], boxd [3, 3]) of the cell route: the box itself or, without one, the fictitious orthorhombic box
    around the bounding box; n = floor(perpendicular width / cutoff) unless given, every axis clamped to [1, ncap]."""
    n = len(pos)
    if box is not None:
        boxd = np.array(box, dtype=np.float64)
        a, b, c = boxd
        vol = abs(a[0] * b[1] * c[2])
        w = [vol / np.linalg.norm(np.cross(b, c)), vol / np.linalg.norm(np.cross(c, a)), abs(c[2])]
    else:
        ext = pos.max(0) - pos.min(0) if n else np.zeros(3)
        w = [max(e + 1.01 * up + 1e-3 * e, 3.0 * up) for e in ext]
        boxd = np.diag(w)
    ncap = grid_cap(n)
    grid = []
    for ax in range(3):
        if explicit is not None and explicit[ax] > 0:
            v = int(explicit[ax])
        else:
            q = w[ax] / up
            if margins is not None:
                margins["grid"] = min(margins["grid"], abs(q - round(q)))
            v = int(np.floor(q))
        grid.append(min(max(v, 1), ncap))
    return np.array(grid + [grid[0] * grid[1] * grid[2]], dtype=np.int64), boxd


def cell_keys(pos, boxd, grid, margins=None):
    """cell id of every atom from its wrapped fractional position (solved back to front), clamped into the grid."""
    fz = pos[:, 2] / boxd[2, 2]
    fy = (pos[:, 1] - fz * boxd[2, 1]) / boxd[1, 1]
    fx = (pos[:, 0] - fy * boxd[1, 0] - fz * boxd[2, 0]) / boxd[0, 0]
    c = []
    for f, n in zip((fx, fy, fz), grid[:3]):
        f = f - np.floor(f)
        t = f * n
        if margins is not None:  # interior cell faces only: at the top face the clamp gives n - 1 on either side
            k = np.round(t)
            dist = np.abs(t - k)[(k >= 1) & (k <= n - 1)]
            margins["on_face"] += int((dist == 0).sum())
            dist = dist[dist > 0]
            if len(dist):
                margins["cell"] = min(margins["cell"], float(dist.min()))
        c.append(np.minimum(t.astype(np.int64), n - 1))
    return (c[0] * grid[1] + c[1]) * grid[2] + c[2]


TOL_CUT, TOL_ROUND, TOL_CELL = 1e-5, 1e-4, 1e-4  # relative to the squared cutoff; of a scaled difference; of a scaled coordinate


def new_margins():
    """cut / round / grid / cell: the smallest distance from a decision (squared cutoffs, roundf ties, floor of the grid, interior cell
    faces); on_face / exact_cut: atoms placed on a cell face and pairs placed on a cutoff on purpose (exactly representable);
    offenders: atoms (caller's numbering) of pairs inside TOL_CUT or TOL_ROUND - what a case generator nudges."""
    return {"cut": np.inf, "round": np.inf, "grid": np.inf, "cell": np.inf, "on_face": 0, "exact_cut": 0, "offenders": set()}


def build(pos, batch, n_mol, lo, up, mnn, box=None, box_mode=0, z=None, max_z=None, cell=None, weights=None):
    """The graph of one build.  pos [N, 3] fp32, batch [N] int64, box [3, 3] (mode 1) / [B, 3, 3] (mode 2) fp32, lo / up the cutoffs as
    the engine holds them (fp32 values), mnn = max_num_neighbors, cell = None (brute force) / "auto" / (nx, ny, nz) explicit grid,
    weights [N] (ghost atoms have weight 0; cell route with a halo exchange set).  -> dict of arrays, plus "margins"."""
    pos = np.asarray(pos, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    batch = np.asarray(batch, dtype=np.int64)
    N, B = len(pos), int(n_mol)
    lo, up = float(np.float32(lo)), float(np.float32(up))
    lo2, up2 = float(np.float32(lo * lo)), float(np.float32(up * up))  # the engine squares in fp32 (exact for the cutoffs used)
    if box is not None:
        box = np.asarray(box, dtype=np.float32).astype(np.float64)
    mg = new_margins()
    ecap = mnn * N
    pcap = ecap // 2 + 1
    out = {"margins": mg, "ecap": ecap, "pcap": pcap, "N": N, "B": B}
    bad_b = (batch < 0) | (batch >= B)
    unsorted = bool(np.any(batch[1:] < batch[:-1])) or bool(bad_b.any())
    # the engine's own decision (csrc/tn_api.hip cell_applicable): per-molecule boxes and oversized explicit grids take brute force
    use_cell = cell is not None and B >= 1 and box_mode != 2 and N >= 1 and (
        cell == "auto" or (min(cell) >= 1 and cell[0] * cell[1] * cell[2] <= 8 * N))
    out["route_cell"] = bool(use_cell)
    if use_cell:
        grid, boxd = cell_grid(pos, box if box_mode == 1 else None, up, None if cell == "auto" else cell, mg)
        key = cell_keys(pos, boxd, grid, mg)
        perm = np.argsort(key, kind="stable")
        out.update(cgrid=grid.astype(np.int32), boxd=boxd, perm=perm.astype(np.int32), cell_key_sorted=key[perm].astype(np.int32))
        if B > 1:
            out["bat_c"] = np.clip(batch[perm], 0, B - 1)
        pbox = boxd  # mode 0: the fictitious box never moves a pair inside the cutoff (edge >= extent + 1.01 cutoff)
        box_mode_eff = 1
    else:
        perm = np.arange(N)
        pbox, box_mode_eff = box, box_mode
    p_in, b_in = pos[perm], batch[perm]
    w_in = None if weights is None or not use_cell else np.asarray(weights, dtype=np.float64)[perm]
    if z is not None:
        zz = np.asarray(z, dtype=np.int64)[perm]
        out["z_c"] = np.clip(zz, 0, max_z - 1)
    c4 = int(z is not None and bool(((np.asarray(z) < 0) | (np.asarray(z) >= max_z)).any()))
    c5 = int(bad_b.any())
    # pairs, molecule by molecule (members in ascending internal index)
    PI, PJ, PD = [], [], []
    order = np.argsort(b_in, kind="stable")
    bounds = np.flatnonzero(np.diff(b_in[order])) + 1
    for members in np.split(order, bounds):
        m = int(b_in[members[0]]) if len(members) else -1
        if m < 0 or m >= B or len(members) < 2:
            continue
        if use_cell and c5:
            raise ValueError("the specification does not cover an out-of-range batch on the cell route")
        a, b = np.tril_indices(len(members), -1)
        i, j = members[a], members[b]
        bx = None if box_mode_eff == 0 else (pbox if box_mode_eff == 1 else pbox[m])
        real_box = box_mode_eff and not (use_cell and box_mode == 0)
        tie = np.full(len(i), np.inf)
        d = min_image(p_in[i] - p_in[j], bx, mg if real_box else None, tie if real_box else None)
        d2 = (d * d).sum(1)
        bad = tie < TOL_ROUND
        for c2 in (lo2, up2):
            if c2 > 0:
                rel = np.abs(d2 - c2) / c2
                bad |= rel < TOL_CUT
                mg["exact_cut"] += int((rel == 0).sum())
                rel = rel[rel > 0]
                if len(rel):
                    mg["cut"] = min(mg["cut"], float(rel.min()))
        mg["offenders"].update(perm[i[bad]].tolist())
        keep = (d2 >= lo2) & (d2 < up2)
        if w_in is not None:
            keep &= ~((w_in[i] == 0) & (w_in[j] == 0))
        PI.append(i[keep]); PJ.append(j[keep]); PD.append(d[keep])
    pi = np.concatenate(PI) if PI else np.zeros(0, dtype=np.int64)
    pj = np.concatenate(PJ) if PJ else np.zeros(0, dtype=np.int64)
    pdl = np.concatenate(PD) if PD else np.zeros((0, 3))
    o = np.lexsort((pj, pi))
    pi, pj, pdl = pi[o], pj[o], pdl[o]
    P = len(pi)
    dist = np.sqrt((pdl * pdl).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        rhat = np.where(dist[:, None] > 0, pdl / dist[:, None], 0.0)
    # symmetric CSR with self edges (an atom with an out-of-range molecule index has an empty row)
    selfs = np.flatnonzero(~((b_in < 0) | (b_in >= B)))
    row = np.concatenate([pi, pj, selfs])
    col = np.concatenate([pj, pi, selfs])
    ep = np.concatenate([np.arange(P), np.arange(P), np.full(len(selfs), P)])
    sg = np.concatenate([np.ones(P), -np.ones(P), np.zeros(len(selfs))])
    o = np.lexsort((col, row))
    row, col, ep, sg = row[o], col[o], ep[o], sg[o]
    ntot = np.bincount(row, minlength=N)[:N] if N else np.zeros(0, dtype=np.int64)
    nlow = np.bincount(pi, minlength=N)[:N] if N else np.zeros(0, dtype=np.int64)
    E = len(row)
    overflow = int(E > ecap or P > pcap or c5)
    c3 = (1 if B > 1 else 0) if use_cell else int(unsorted)
    out.update(counts=np.array([P, E, overflow, c3, c4, c5], dtype=np.int32), nlow=nlow.astype(np.int32), ntot=ntot.astype(np.int32),
               rowptr=np.concatenate([[0], np.cumsum(ntot)]).astype(np.int32),
               pairptr=np.concatenate([[0], np.cumsum(nlow)]).astype(np.int32), col=col.astype(np.int32), epair=ep.astype(np.int32),
               esign=sg.astype(np.float32), pair_i=pi.astype(np.int32), pair_j=pj.astype(np.int32), pd=np.concatenate([dist, [0.0]]),
               pdelta=pdl, prhat=rhat)
    if use_cell and B == 1:
        out.update(mstart=np.array([0], dtype=np.int32), mend=np.array([N], dtype=np.int32))
    elif not use_cell and not unsorted:
        ms, me = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        for m in np.unique(batch):
            idx = np.flatnonzero(batch == m)
            ms[m], me[m] = idx[0], idx[-1] + 1
        out.update(mstart=ms, mend=me)
    out["_geom"] = (p_in, pbox, box_mode_eff, b_in)
    # scale of the float arrays' bounds (the same statement in numpy fp32): |pos_i|inf + |pos_j|inf + sum |box|
    if P:
        s_box = 0.0 if box_mode_eff == 0 else (np.abs(pbox).sum() if box_mode_eff == 1 else np.abs(pbox).sum((1, 2))[b_in[pi]])
        out["scale"] = np.abs(p_in[pi]).max(1) + np.abs(p_in[pj]).max(1) + s_box
    else:
        out["scale"] = np.zeros(0)
    return out


def fp32_statement(spec):
    """The engine's pair geometry (csrc/tn_common.h pair_geometry and the fill pass) restated in numpy fp32 on the pairs of the
    specification: one subtraction, fused shifts z -> y -> x (a fused multiply-add is the exactly formed a * b + c rounded once:
    the product of two fp32 values is exact in float64), d = sqrt(d2), rhat = delta * (1 / d).  -> pdelta, pd, prhat (fp32).
    Its distance from the float64 specification is the floor no fp32 engine can be asked to beat."""
    f32 = np.float32
    p_in, pbox, mode, b_in = spec["_geom"]
    pi, pj = spec["pair_i"].astype(np.int64), spec["pair_j"].astype(np.int64)
    pos = p_in.astype(f32)
    d = pos[pi] - pos[pj]
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)  # noqa: E731
    if mode and len(pi):
        bx = (pbox[None] if mode == 1 else pbox[b_in[pi]]).astype(f32)
        bx = np.broadcast_to(bx, (len(pi), 3, 3))
        for ax in (2, 1, 0):
            s = -np.round(d[:, ax] / bx[:, ax, ax])
            for k in range(ax + 1):
                d[:, k] = fma(s, bx[:, ax, k], d[:, k])
    d2 = fma(d[:, 2], d[:, 2], fma(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))
    dist = np.sqrt(d2)
    with np.errstate(divide="ignore"):
        inv = np.where(dist > 0, f32(1.0) / dist, f32(0.0)).astype(f32)
    return d, np.concatenate([dist, np.zeros(1, dtype=f32)]), d * inv[:, None]


def pair_set_original(spec_or_arrays, perm=None):
    """{(hi, lo): index} of the pair list in the caller's numbering, with the sign that turns the stored delta into pos[hi] - pos[lo]."""
    pi, pj = np.asarray(spec_or_arrays["pair_i"]), np.asarray(spec_or_arrays["pair_j"])
    if perm is not None:
        pi, pj = np.asarray(perm)[pi], np.asarray(perm)[pj]
    sign = np.where(pi > pj, 1.0, -1.0)
    hi, lo_ = np.maximum(pi, pj), np.minimum(pi, pj)
    o = np.lexsort((lo_, hi))
    return hi[o], lo_[o], sign[o], o
