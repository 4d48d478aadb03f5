"""TEST INFRASTRUCTURE ONLY -- the cases of the kernel-level unit tests of the TensorNet2 kernels (tmdnet_debug_tn2): hand-built
graphs, seeded inputs, launches and the figures the tests assert on.  One statement serves three users:
tests/test_gpu_tn2_unit.py (asserts), tools/tn2_unit_floor.py (the fp32 rounding floor of the reference on these very inputs
without a device, and the errors observed on the device, into profiles/tn2_unit_floor.json, from which the test reads its
bounds) and tests/test_tn2_unit_oracle.py (statements against oracle/tn2_torch.py and autograd, branch census; no device).
"""
import ctypes as C
import json
import os

import torch

from tests import tn2_unit_oracle as O
from tests.kernel_unit_cases import SENTINEL, TAIL, bits, sentinel
from tests.message_unit_cases import worse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR_JSON = os.path.join(ROOT, "profiles", "tn2_unit_floor.json")
# restated from csrc/tn_tn2.hip (tests/test_tn2_unit_oracle.py parses the source and compares)
COULOMB_ROUND, QEQ_BLOCK, EDGE_TRIP, ROW_THREADS_CAP, WAVE, ATOMS_PER_BLOCK, MAX_QC = 64, 256, 4, 256, 64, 4, 64

# graph name -> (atoms, undirected edges, molecule of every atom)
GRAPHS = {
    # rows of 1, 2, 3, 4, 5, 8 and 9 entries (self edge included): atom 0 alone, hubs 1 (eight neighbours) and 10 (seven)
    "rows": (23, [(1, k) for k in range(2, 10)] + [(10, k) for k in range(11, 18)] +
             [(2, 3), (4, 5), (5, 6), (7, 8), (8, 9), (8, 11), (18, 19), (20, 21), (21, 22), (20, 22)], [0] * 23),
    # a complete molecule of five, a chain of four and an atom without a neighbour
    "two_mols": (10, [(a, b) for a in range(5) for b in range(a)] + [(5, 6), (6, 7), (7, 8)], [0] * 5 + [1] * 5),
}
EDGE_F = (32, 96, 128, 320)
CP_F = (32, 96)
EDGE_OPS = ("edge_pre1", "edge_gw", "edge_reduce", "pair_gd")
QEQ_QD = (1, 3, 8, 24, 64)
QEQ_VARIANTS = ("q", "noq", "perm", "neutral")  # total charges given / NULL / atoms permuted (counts[3] = 1) / all f ~ 1e-4
COULOMB_SIZES = (1, 2, 63, 64, 65, 130)  # and one more atom whose `batch` is out of range
COULOMB_QC = (1, 8, 9, 24, 64)
COULOMB_MODES = ("a2a", "rf", "rf_box", "rf_molbox")  # all-to-all / reaction field: no box, one triclinic box, a box per molecule
COULOMB_ORDERS = ("sorted", "perm")
COULOMB_CUT, COULOMB_EPS, COULOMB_SCALE = 6.0, 78.3, 1.7
MIN_DIST, CLASS_MARGIN = 0.9, 1e-3
PAIR_CAP_EXTRA = 2  # PAIR_GD is launched over this many pairs more than counts[0]

OPS = {"edge_reverse": 0, "cp_feat": 1, "cp_feat_bwd": 2, "qeq_fwd": 3, "qeq_bwd": 4, "edge_pre1": 5, "edge_gw": 6, "edge_reduce": 7,
       "pair_gd": 8, "coulomb": 9}
OUTPUTS = {"edge_reverse": ["erev", "eid", "pair_edge"], "cp_feat": ["feat"], "cp_feat_bwd": ["G"], "qeq_fwd": ["charges", "Fu", "dQ"],
           "qeq_bwd": ["g_out"], "edge_pre1": ["pre1", "he1", "Ce"], "edge_gw": ["g_pre3", "slots"], "edge_reduce": ["gB", "gCs", "gAp"],
           "pair_gd": ["gd"], "coulomb": ["ec", "g_q", "fpos"]}
EXACT = ("erev", "eid", "pair_edge", "Ce")  # integer outputs and plain copies: bit for bit


def all_cases():
    """[(op, variant, size)]: variant = graph / equilibration variant / Coulomb mode-order, size = F / qd / QC"""
    out = [("edge_reverse", gname, 0) for gname in GRAPHS]
    out += [(op, "rows", F) for F in CP_F for op in ("cp_feat", "cp_feat_bwd")]
    out += [(op, v, qd) for qd in QEQ_QD for v in QEQ_VARIANTS for op in ("qeq_fwd", "qeq_bwd")]
    out += [(op, gname, F) for gname in GRAPHS for F in EDGE_F for op in EDGE_OPS]
    out += [("coulomb", f"{m}-{o}", QC) for m in COULOMB_MODES for o in COULOMB_ORDERS for QC in COULOMB_QC]
    return out


def case_id(case):
    return "%s-%s-%d" % case


def _gen(case):
    op, variant, size = case
    names = sorted(GRAPHS) + list(QEQ_VARIANTS) + [f"{m}-{o}" for m in COULOMB_MODES for o in COULOMB_ORDERS]
    return torch.Generator().manual_seed(7919 * OPS[op] + 104729 * names.index(variant) + size)


# ====================================================================================== graphs
_graph_cache = {}


def build_graph(name):
    """the CSR of GRAPHS[name] in the engine's form (int64 tensors on the CPU): pairs (i, j), i > j, numbered in the order of (i, j)"""
    if name in _graph_cache:
        return _graph_cache[name]
    N, edges, batch = GRAPHS[name]
    adj = torch.eye(N, dtype=torch.bool)
    for a, b in edges:
        assert a != b and not adj[a, b]
        adj[a, b] = adj[b, a] = True
    rows, cols = torch.nonzero(adj, as_tuple=True)  # sorted by (row, column)
    lower = rows > cols
    P = int(lower.sum())
    pid = torch.full((N * N,), -1, dtype=torch.int64)
    pid[(rows * N + cols)[lower]] = torch.arange(P)
    epair = torch.where(rows == cols, torch.tensor(P), pid[torch.maximum(rows, cols) * N + torch.minimum(rows, cols)])
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.bincount(rows, minlength=N).cumsum(0)
    batch = torch.tensor(batch)
    g = dict(N=N, P=P, E=rows.numel(), rowptr=rowptr, rows=rows, col=cols, epair=epair, batch=batch, B=int(batch.max()) + 1)
    _graph_cache[name] = g
    return g


def row_lengths(name):
    g = build_graph(name)
    return (g["rowptr"][1:] - g["rowptr"][:-1]).tolist()


# ====================================================================================== inputs
def qeq_sizes(qd):
    """one atom fewer than, exactly as many as, one more than the groups of a block, and a single atom"""
    groups = QEQ_BLOCK // qd
    return [n for n in (groups - 1, groups, groups + 1, 1) if n >= 1]


def _mol_index(sizes):
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    mend = torch.tensor(sizes).cumsum(0)
    return batch, mend - torch.tensor(sizes), mend


def _boxes(mode, B, gen):
    """lower-triangular boxes, every length >= 2 cut"""
    if mode in ("a2a", "rf"):
        return None, 0
    n = 1 if mode == "rf_box" else B
    box = torch.zeros(n, 3, 3, dtype=torch.float64)
    for k in range(n):
        box[k] = torch.diag(2 * COULOMB_CUT + 0.3 + 1.5 * torch.rand(3, generator=gen, dtype=torch.float64))
        box[k, 1, 0], box[k, 2, 0], box[k, 2, 1] = (2.0 * torch.rand(3, generator=gen, dtype=torch.float64) - 1.0).tolist()
    return box.float(), (1 if mode == "rf_box" else 2)


def _image_steps(delta, box):
    """the three quotients the minimum image rounds, and the image itself (float64)"""
    q = []
    for a in (2, 1, 0):
        q.append(delta[..., a] / box[a, a])
        delta = delta - torch.round(q[-1])[..., None] * box[a]
    return torch.stack(q, -1), delta


def _place(n, box, cut, gen):
    """n points whose pairs satisfy the conditions of coulomb_conditions with twice the margin (rejection sampling, float32 values).
    The single pair of a two-atom molecule stays within 2 A per axis: the reaction-field g(d) goes to zero at the cutoff as a
    difference of terms of 0.2 .. 0.3, and a molecule whose only pair sat there would have nothing else to be measured against."""
    pts = torch.zeros(0, 3, dtype=torch.float64)
    while pts.shape[0] < n:
        c = torch.rand(3, generator=gen, dtype=torch.float64)
        c = (c * (10.0 if n > 2 else 2.0) if box is None else (c if n > 2 else 0.15 * c) @ box).float().double()
        delta = c[None] - pts
        if box is not None:
            q, delta = _image_steps(delta, box)
            if bool((((q - torch.floor(q)) - 0.5).abs() < CLASS_MARGIN).any()):
                continue
        d = delta.norm(dim=-1)
        if bool((d < MIN_DIST + 0.05).any()) or (cut > 0 and bool(((d / cut - 1).abs() < 2 * CLASS_MARGIN).any())):
            continue
        pts = torch.cat([pts, c[None]])
    return pts


def coulomb_conditions(pos, batch, B, box, box_mode, cut):
    """the conditions on a Coulomb case's inputs, asserted on the float32 values themselves (in float64): what keeps a float32 /
    float64 difference in the CLASS of a pair (inside the cutoff, which image) from being hidden as a tolerance"""
    pos, N = pos.double(), pos.shape[0]
    valid = (batch >= 0) & (batch < B)
    same = (batch[:, None] == batch[None, :]) & valid[:, None] & valid[None, :] & ~torch.eye(N, dtype=torch.bool)
    delta = pos[:, None] - pos[None, :]
    if box_mode:
        bx = box.double().reshape(-1, 3, 3)
        assert bool((torch.diagonal(bx, dim1=1, dim2=2) >= 2 * cut).all()), "a box length below twice the cutoff"
        for m in range(B):
            sel = batch == m
            q, img = _image_steps(delta[sel][:, sel], bx[0 if box_mode == 1 else m])
            assert bool((((q - torch.floor(q)) - 0.5).abs() > 0.5 * CLASS_MARGIN).all()), "a minimum-image component at half a box vector"
            idx = torch.nonzero(sel).flatten()
            delta[idx[:, None], idx[None, :]] = img
    d = delta.norm(dim=-1)[same]
    assert float(d.min()) >= MIN_DIST, "two atoms closer than the minimum distance"
    assert bool((d < O.R_DAMP).any()) and bool((d > O.R_DAMP).any()), "no pair on one side of the damping radius"
    if cut > 0:
        assert bool((d < cut).any()) and bool((d > cut).any()), "no pair on one side of the cutoff"
        assert bool(((d / cut - 1).abs() > CLASS_MARGIN).all()), "a pair at the cutoff"


_coulomb_geom = {}


def coulomb_geometry(mode):
    """positions (float32), batch, mstart, mend, box, box_mode of a mode: built once, shared by its QC values and both orders"""
    if mode in _coulomb_geom:
        return _coulomb_geom[mode]
    gen = torch.Generator().manual_seed(4242 + COULOMB_MODES.index(mode))
    sizes, B = list(COULOMB_SIZES), len(COULOMB_SIZES)
    batch, mstart, mend = _mol_index(sizes)
    box, box_mode = _boxes(mode, B, gen)
    cut = 0.0 if mode == "a2a" else COULOMB_CUT
    pos = torch.cat([_place(n, None if box is None else box[0 if box_mode == 1 else m].double(), cut, gen) for m, n in enumerate(sizes)] +
                    [torch.tensor([[3.0, 4.0, 5.0]], dtype=torch.float64)]).float()
    batch = torch.cat([batch, torch.tensor([B])])  # the last atom belongs to no molecule
    coulomb_conditions(pos, batch, B, box, box_mode, cut)
    geo = dict(pos=pos, batch=batch, mstart=mstart, mend=mend, box=box, box_mode=box_mode, cut=cut, B=B, N=pos.shape[0])
    _coulomb_geom[mode] = geo
    return geo


def make_inputs(case):
    """the fp32 operands of a case on the CPU (and its integers): a dict"""
    op, variant, size = case
    gen = _gen(case)
    rn = lambda *s: torch.randn(*s, generator=gen)
    if op == "edge_reverse":
        return {}
    if op in ("cp_feat", "cp_feat_bwd"):
        N = GRAPHS[variant][0]
        return dict(X=rn(N, 9, size) * 0.5, g_feat=rn(N, 3, size), old=rn(N, 9, size))
    if op in ("qeq_fwd", "qeq_bwd"):
        qd, sizes = size, qeq_sizes(size)
        batch, mstart, mend = _mol_index(sizes)
        N, B = int(batch.numel()), len(sizes)
        out = rn(N, 2 * qd)
        if variant == "neutral":
            out[:, qd:] = 1e-4 * (1 + 0.3 * rn(N, qd))
        d = dict(out=out, Qmol=torch.randint(-2, 3, (B,), generator=gen).float(), g_c=rn(N, qd), batch=batch, mstart=mstart, mend=mend,
                 N=N, B=B, unsorted=0)
        if variant == "perm":
            perm = torch.randperm(N, generator=gen)
            d.update(out=out[perm].contiguous(), g_c=d["g_c"][perm].contiguous(), batch=batch[perm].contiguous(), unsorted=1,
                     mstart=torch.zeros_like(mstart), mend=torch.zeros_like(mend))
            assert bool((d["batch"][1:] < d["batch"][:-1]).any())
        _, Fu, dQ = O.qeq_fwd(d["out"], None if variant == "noq" else d["Qmol"], d["batch"], B, qd)
        d.update(Fu=Fu, dQ=dQ)  # the backward kernel's input: the fp32 statement's, not the forward kernel's
        return d
    if op == "coulomb":
        mode, order = variant.split("-")
        geo = dict(coulomb_geometry(mode))
        N = geo["N"]
        # one sign per atom over its channels: the channel sum s_ij of a pair then has no cancelling terms, so the single pair of the
        # two-atom molecule is not a rounding residue (the sums over the partners j still carry both signs)
        sign = torch.where(torch.rand(N, 1, generator=gen) < 0.5, -1.0, 1.0)
        geo.update(charges=sign * rn(N, size).abs() * 0.3, wq=torch.rand(size, generator=gen) + 0.5, unsorted=0)
        if order == "perm":
            perm = torch.randperm(N, generator=gen)
            geo.update(pos=geo["pos"][perm].contiguous(), batch=geo["batch"][perm].contiguous(), charges=geo["charges"][perm].contiguous(),
                       unsorted=1, mstart=torch.zeros_like(geo["mstart"]), mend=torch.zeros_like(geo["mend"]))
        return geo
    g = build_graph(variant)
    N, P, E, F = g["N"], g["P"], g["E"], size
    if op == "edge_pre1":
        return dict(Ap=rn(P + 1, F), Bt=rn(N, F), Cs=rn(N, F), C=torch.rand(P + 1, generator=gen))
    if op == "edge_gw":
        return dict(gMi=rn(N, 9, F), Pn=rn(N, 9, F) * 0.5, pre3=rn(E, 3 * F), Ce=torch.rand(E, generator=gen))
    if op == "edge_reduce":
        return dict(g_pre1=rn(E, F))
    assert op == "pair_gd"
    return dict(gAp=rn(P, F), dAp=rn(P + 1, F), slots=rn((F + WAVE - 1) // WAVE, E), dC=rn(P + 1), old=rn(P))


def graph_of(case, d):
    return build_graph(case[1]) if case[0] == "edge_reverse" or case[0] in EDGE_OPS else None


def reference(case, g, d):
    """output name -> expected tensor in the dtype of d, or (value, scale) where the error is normalised by the sum of the absolute
    values of the terms (slots, g_out)"""
    op, variant, size = case
    if op == "edge_reverse":
        return dict(zip(OUTPUTS[op], O.edge_reverse(g)))
    if op == "cp_feat":
        return {"feat": O.cp_feat(d["X"])}
    if op == "cp_feat_bwd":
        return {"G": d["old"] + O.cp_feat_bwd(d["X"], d["g_feat"])}
    if op == "qeq_fwd":
        return dict(zip(OUTPUTS[op], O.qeq_fwd(d["out"], None if variant == "noq" else d["Qmol"], d["batch"], d["B"], size, want_scale=True)))
    if op == "qeq_bwd":
        return {"g_out": O.qeq_bwd(d["out"], d["Fu"], d["dQ"], d["g_c"], d["batch"], size, want_scale=True)}
    if op == "edge_pre1":
        return dict(zip(OUTPUTS[op], O.edge_pre1(g, d["Ap"], d["Bt"], d["Cs"], d["C"])))
    if op == "edge_gw":
        g_pre3, slots, scale = O.edge_gw(g, d["gMi"], d["Pn"], d["pre3"], d["Ce"])
        return {"g_pre3": g_pre3, "slots": (slots, scale)}
    if op == "edge_reduce":
        return dict(zip(OUTPUTS[op], O.edge_reduce(g, d["g_pre1"])))
    if op == "pair_gd":
        return {"gd": d["old"] + O.pair_gd(g, d["gAp"], d["dAp"], d["slots"], d["dC"])}
    return O.coulomb(d["pos"], d["batch"], d["B"], d["box"], d["box_mode"], d["charges"], d["wq"], d["cut"], COULOMB_EPS, COULOMB_SCALE)


def error_groups(case, g, d, name):
    """the rows over which an output's error is normalised together: None = every row (atom, edge) on its own, else a group index
    per row (the molecule of the atom, or of the pair)"""
    op = case[0]
    if op in ("qeq_fwd", "qeq_bwd"):
        return d["batch"] if name in ("charges", "g_out") else None
    if op == "coulomb":
        return torch.where((d["batch"] >= 0) & (d["batch"] < d["B"]), d["batch"], torch.full_like(d["batch"], d["B"]))
    if name == "gd":
        lower = g["col"] < g["rows"]
        mol = torch.zeros(g["P"], dtype=torch.int64, device=g["col"].device)
        mol[g["epair"][lower]] = g["batch"][g["rows"][lower]]
        return mol
    return None


def errors(case, g, d, got, ref):
    out = {}
    for k, r in ref.items():
        if k in EXACT:
            out[k] = 0.0 if torch.equal(got[k].to(r.device).to(r.dtype), r) else float("inf")
        elif k == "slots":
            out[k] = O.slot_rel_err(got[k], r[0], r[1])
        elif isinstance(r, tuple):
            out[k] = O.group_rel_err(got[k], r[0], error_groups(case, g, d, k), scale=r[1])
        else:
            out[k] = O.group_rel_err(got[k], r, error_groups(case, g, d, k))
    return out


def _to(d, f):
    return {k: (f(v) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


def floor_of(case):
    """rounding floor per output: the statements in float32 against themselves in float64 on the case's own inputs (CPU)"""
    d = make_inputs(case)
    g = graph_of(case, d)
    lo, hi = reference(case, g, d), reference(case, g, _to(d, lambda v: v.double()))
    return {k: e for k, e in errors(case, g, d, {k: (v[0] if isinstance(v, tuple) else v) for k, v in lo.items()}, hi).items()}


def load_bounds():
    with open(FLOOR_JSON) as fh:
        return json.load(fh)


# ====================================================================================== launches
def _ptr(t):
    return None if t is None else t.data_ptr()


def _isent(shape, device):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=device)


def fresh_outputs(case, g, d, device):
    """every output buffer of the op, all sentinel (accumulating outputs: the case's old contents in their rows), with TAIL sentinel
    rows behind the last row the op may write; slot arrays: one more than the kernel's count, TAIL slots behind entry E"""
    op, variant, size = case
    if op == "edge_reverse":
        return {"erev": _isent((g["E"] + TAIL,), device), "eid": _isent((g["E"] + TAIL,), device), "pair_edge": _isent((g["P"] + TAIL,), device)}
    if op == "cp_feat":
        return {"feat": sentinel((d["X"].shape[0] + TAIL, 3, size), device)}
    if op == "cp_feat_bwd":
        G = sentinel((d["X"].shape[0] + TAIL, 9, size), device)
        G[:d["X"].shape[0]] = d["old"]
        return {"G": G}
    if op == "qeq_fwd":
        return {"charges": sentinel((d["N"] + TAIL, size), device), "FuQ": sentinel((d["B"] + TAIL, 2 * size), device)}
    if op == "qeq_bwd":
        return {"g_out": sentinel((d["N"] + TAIL, 2 * size), device)}
    if op == "edge_pre1":
        return {"pre1": sentinel((g["E"] + TAIL, size), device), "he1": sentinel((g["E"] + TAIL, size), device), "Ce": sentinel((g["E"] + TAIL,), device)}
    if op == "edge_gw":
        return {"g_pre3": sentinel((g["E"] + TAIL, 3 * size), device), "slots": sentinel(((size + WAVE - 1) // WAVE + 1, g["E"] + TAIL), device)}
    if op == "edge_reduce":
        return {"gB": sentinel((g["N"] + TAIL, size), device), "gCs": sentinel((g["N"] + TAIL, size), device),
                "gAp": sentinel((g["P"] + 1 + TAIL, size), device)}  # row P is the self pair's: no entry with j < i, never written
    if op == "pair_gd":
        gd = sentinel((g["P"] + TAIL,), device)
        gd[:g["P"]] = d["old"]
        return {"gd": gd}
    N = d["N"]
    return {"ec": sentinel((N + TAIL,), device), "g_q": sentinel((N + TAIL, size), device), "fpos": sentinel((N + TAIL, 3), device)}


def unit_args(case, g, d, out, dev, overflow=False, forces=True):
    """tmdnet_tn2_unit_args of a case; `dev` holds the device copies (graph arrays as int32) and keeps them alive"""
    from torchmdnet_amd import _C

    op, variant, size = case
    x = _C.Tn2UnitArgs()
    x.op = OPS[op]
    if g is not None:
        x.N, x.B, x.P, x.E, x.F = g["N"], g["B"], g["P"], g["E"], size
        x.rowptr, x.col, x.epair = _ptr(dev["rowptr"]), _ptr(dev["col"]), _ptr(dev["epair"])
        x.counts = _ptr(dev["counts_overflow" if overflow else "counts"])
    if op == "edge_reverse":
        x.erev, x.eid, x.pair_edge = _ptr(out["erev"]), _ptr(out["eid"]), _ptr(out["pair_edge"])
    elif op in ("cp_feat", "cp_feat_bwd"):
        x.N, x.F, x.X = d["X"].shape[0], size, _ptr(dev["X"])
        if op == "cp_feat":
            x.feat = _ptr(out["feat"])
        else:
            x.g_feat, x.G = _ptr(dev["g_feat"]), _ptr(out["G"])
    elif op in ("qeq_fwd", "qeq_bwd"):
        x.N, x.B, x.qd = d["N"], d["B"], size
        x.counts, x.mstart, x.mend, x.batch, x.out = (_ptr(dev[k]) for k in ("counts", "mstart", "mend", "batch", "out"))
        if op == "qeq_fwd":
            x.Qmol, x.charges, x.FuQ = (None if variant == "noq" else _ptr(dev["Qmol"])), _ptr(out["charges"]), _ptr(out["FuQ"])
        else:
            x.FuQ, x.g_c, x.g_out = _ptr(dev["FuQ"]), _ptr(dev["g_c"]), _ptr(out["g_out"])
    elif op == "edge_pre1":
        x.Ap, x.Bt, x.Cs, x.C = (_ptr(dev[k]) for k in ("Ap", "Bt", "Cs", "C"))
        x.pre1, x.he1, x.Ce = _ptr(out["pre1"]), _ptr(out["he1"]), _ptr(out["Ce"])
    elif op == "edge_gw":
        x.gMi, x.Pn, x.pre3, x.Ce = (_ptr(dev[k]) for k in ("gMi", "Pn", "pre3", "Ce"))
        x.g_pre3, x.slots, x.slot_stride = _ptr(out["g_pre3"]), _ptr(out["slots"]), out["slots"].shape[1]
    elif op == "edge_reduce":
        x.g_pre1, x.erev = _ptr(dev["g_pre1"]), _ptr(dev["erev"])
        x.gB, x.gCs, x.gAp = _ptr(out["gB"]), _ptr(out["gCs"]), _ptr(out["gAp"])
    elif op == "pair_gd":
        x.P = g["P"] + PAIR_CAP_EXTRA  # the launch covers more pairs than counts[0]: those may not be touched
        x.gAp, x.dAp, x.slots, x.slot_stride, x.dC = _ptr(dev["gAp"]), _ptr(dev["dAp"]), _ptr(dev["slots"]), g["E"], _ptr(dev["dC"])
        x.pair_edge, x.erev, x.gd = _ptr(dev["pair_edge"]), _ptr(dev["erev"]), _ptr(out["gd"])
    else:
        x.N, x.B, x.QC, x.box_mode = d["N"], d["B"], size, d["box_mode"]
        x.cut, x.eps_solvent, x.scale = d["cut"], COULOMB_EPS, COULOMB_SCALE
        x.counts, x.mstart, x.mend, x.batch = (_ptr(dev[k]) for k in ("counts", "mstart", "mend", "batch"))
        x.pos, x.box, x.charges, x.wq, x.ec = _ptr(dev["pos"]), _ptr(dev.get("box")), _ptr(dev["charges"]), _ptr(dev["wq"]), _ptr(out["ec"])
        if forces:
            x.g_q, x.fpos = _ptr(out["g_q"]), _ptr(out["fpos"])
    return x


def device_copies(case, g, d, device):
    """device copies of the inputs: floats as they are, graph and molecule index arrays as int32, batch as int64"""
    dev = {k: v.to(device).contiguous() for k, v in d.items() if torch.is_tensor(v) and v.is_floating_point()}
    src = dict(d)
    counts = [0] * 8
    if g is not None:
        src.update(rowptr=g["rowptr"], col=g["col"], epair=g["epair"])
        counts[0], counts[1] = g["P"], g["E"]
        erev, _, pair_edge = O.edge_reverse(g)
        src.update(erev=erev, pair_edge=pair_edge)
    counts[3] = int(d.get("unsorted", 0))
    for k in ("rowptr", "col", "epair", "mstart", "mend", "erev", "pair_edge"):
        if k in src:
            dev[k] = src[k].to(torch.int32).to(device)
    if "batch" in d:
        dev["batch"] = d["batch"].to(torch.int64).to(device)
    if "Fu" in d:
        dev["FuQ"] = torch.cat([d["Fu"], d["dQ"]], 1).to(device).contiguous()
    dev["counts"] = torch.tensor(counts, dtype=torch.int32, device=device)
    counts[2] = 1
    dev["counts_overflow"] = torch.tensor(counts, dtype=torch.int32, device=device)
    return dev


def call(lib, x):
    """one call of tmdnet_debug_tn2 -> (rc, slot arrays)"""
    ns = C.c_int32(-1)
    x.slot_arrays_out = C.pointer(ns)
    rc = lib.tmdnet_debug_tn2(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(x))
    torch.cuda.synchronize()
    return rc, ns.value


def _written(case, g, d, out):
    """output name -> (the part the op owns, the parts it may not touch)"""
    op, variant, size = case
    if op == "qeq_fwd":
        B = d["B"]
        return {"charges": (out["charges"][:d["N"]], [out["charges"][d["N"]:]]), "Fu": (out["FuQ"][:B, :size], [out["FuQ"][B:]]),
                "dQ": (out["FuQ"][:B, size:], [])}
    n = {"erev": "E", "eid": "E", "pair_edge": "P", "pre1": "E", "he1": "E", "Ce": "E", "g_pre3": "E", "gB": "N", "gCs": "N", "gAp": "P", "gd": "P"}
    res = {}
    for k, t in out.items():
        if k == "slots":
            cnt = (size + WAVE - 1) // WAVE
            res[k] = (t[:cnt, :g["E"]], [t[:cnt, g["E"]:], t[cnt:]])
        else:
            rows = g[n[k]] if k in n else (d["X"].shape[0] if "X" in d else d["N"])
            res[k] = (t[:rows], [t[rows:]])
    return res


def run_case(lib, case, device="cuda"):
    """Launch one case twice (the Coulomb head also without forces), and once with the pair-overflow flag where the kernel has one
    -> dict(err={output: figure}, finite, slot_arrays_ok, tail_ok, deterministic, overflow_ok, energy_only_ok)."""
    op, variant, size = case
    d = make_inputs(case)
    g = graph_of(case, d)
    dev = device_copies(case, g, d, device)
    d64 = {k: (v.to(device).double() if torch.is_tensor(v) and v.is_floating_point() else (v.to(device) if torch.is_tensor(v) else v))
           for k, v in d.items()}
    g64 = None if g is None else {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in g.items()}
    ref = reference(case, g64, d64)  # fp64 on the device, once, left unchanged
    res = dict(err={}, finite=True, slot_arrays_ok=True, tail_ok=True, deterministic=True, overflow_ok=True, energy_only_ok=True)
    runs = []
    for _ in range(2):
        out = fresh_outputs(case, g, d, device)
        rc, ns = call(lib, unit_args(case, g, d, out, dev))
        assert rc == 0, f"tmdnet_debug_tn2 returned {rc}"
        res["slot_arrays_ok"] &= ns == ((size + WAVE - 1) // WAVE if x_has_channels(op) else 0)
        runs.append(out)
    a, b = runs
    w = _written(case, g, d, a)
    got = {k: v[0] for k, v in w.items()}
    gd_ = None if g is None else g64
    dd_ = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in d.items()}
    for k, e in errors(case, gd_, dd_, got, ref).items():
        res["err"][k] = worse(res["err"].get(k), e)
        res["finite"] &= bool(torch.isfinite(got[k].float()).all())
    res["tail_ok"] = all(bool((bits(p) == SENTINEL).all()) for v in w.values() for p in v[1])
    res["deterministic"] = all(bool(torch.equal(bits(a[k]), bits(b[k]))) for k in a)
    if op == "coulomb":  # energy only (g_q NULL): the same energies bit for bit, the gradient buffers untouched
        out = fresh_outputs(case, g, d, device)
        rc, _ = call(lib, unit_args(case, g, d, out, dev, forces=False))
        assert rc == 0
        res["energy_only_ok"] = bool(torch.equal(bits(out["ec"]), bits(a["ec"]))) and all(bool((bits(out[k]) == SENTINEL).all()) for k in ("g_q", "fpos"))
    if op == "edge_reverse" or op in EDGE_OPS:  # pair overflow (counts[2] != 0): every edge kernel returns without a write
        out = {k: (sentinel(tuple(v.shape), device) if v.dtype == torch.float32 else _isent(tuple(v.shape), device))
               for k, v in fresh_outputs(case, g, d, device).items()}
        rc, _ = call(lib, unit_args(case, g, d, out, dev, overflow=True))
        assert rc == 0
        res["overflow_ok"] = all(bool((bits(v) == SENTINEL).all()) for v in out.values())
    return res


def x_has_channels(op):
    return op not in ("edge_reverse", "qeq_fwd", "qeq_bwd", "coulomb")
