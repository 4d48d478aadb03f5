"""TEST INFRASTRUCTURE ONLY -- plain torch statements of what the kernels only the TensorNet2 + ScalarPlusWeightedCoulomb path has
compute (csrc/tn_tn2.hip: k_edge_reverse, k_cp_feat, k_cp_feat_bwd, k_qeq, k_tn2_edge_pre1, k_tn2_edge_gw, k_tn2_edge_reduce,
k_tn2_pair_gd, k_coulomb), in the precision of their inputs: float64 inputs give the reference of tests/test_gpu_tn2_unit.py,
float32 inputs the rounding floor its bounds are derived from (tools/tn2_unit_floor.py).

Written from the formulas (tensornet2.py:99-150, output_modules.py:440-606, the comments above each kernel), not from the
kernels' loops: sums over molecules and rows are index_add over `batch` / `rows` / `col` / `epair`, the Coulomb sum is a dense
masked N x N table.  A graph is a dict in the engine's form as in tests/message_oracle.py (rowptr, rows, col, epair, N, P; a self
edge with pair id P in every row).  tests/test_tn2_unit_oracle.py pins the equilibration and the Coulomb energy to
oracle/tn2_torch.py and every adjoint to torch.autograd of its forward statement.
"""
import math

import torch

from oracle import tensornet_torch as TT
from oracle.tensornet_adjoint import TYPE_OF, compose
from tests import message_oracle as MO

COULOMB_FACTOR = 0.5 * 27.211386024367243 * 0.5291772105638411  # output_modules.py:399-403
R_DAMP = 4.6
WAVE = 64  # channels per slot array of the cutoff-gradient partial sums


def silu(x):
    return x * torch.sigmoid(x)


def silu_grad(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


# ---------------------------------------------------------------------------------------------- graph extras
def edge_reverse(g):
    """-> (erev [E]: the entry (j <- i) of entry (i <- j); eid [E] = e; pair_edge [P]: the entry with j < i of each pair)"""
    N, rows, col = g["N"], g["rows"], g["col"]
    key = rows * N + col  # ascending: rows in order, the columns of a row ascending
    erev = torch.searchsorted(key, col * N + rows)
    eid = torch.arange(col.numel(), device=col.device)
    lower = col < rows
    pair_edge = torch.full((g["P"],), -1, dtype=torch.int64, device=col.device)
    pair_edge[g["epair"][lower]] = eid[lower]
    return erev, eid, pair_edge


# ---------------------------------------------------------------------------------------------- charge prediction
def cp_feat(X):
    """[I ; |A|^2 ; |S|^2] [N, 3, F] of the stored components X [N, 9, F] (tensornet2.py:139-150: I itself)."""
    I, A, S = TT.decompose(compose(X))
    return torch.stack([I, TT.tnorm(A), TT.tnorm(S)], 1)


def cp_feat_bwd(X, g_feat):
    """(d feat / d X)^T g_feat [N, 9, F]: what the kernel ADDS to G."""
    I, v0, v1, v2, s0, s1, s2, s3, s4 = X.unbind(1)
    gI, gA, gS = g_feat.unbind(1)
    return torch.stack([gI, 4 * v0 * gA, 4 * v1 * gA, 4 * v2 * gA, (4 * s0 + 2 * s3) * gS, 4 * s1 * gS, 4 * s2 * gS,
                        (4 * s3 + 2 * s0) * gS, 4 * s4 * gS], 1)


def qeq_fwd(out, Qmol, batch, B, qd, want_scale=False):
    """per-molecule charge equilibration (tensornet2.py:99-138) -> (charges [N, qd], Fu [B, qd], dQ [B, qd]); with want_scale the
    charges and dQ come as (value, sum of the absolute values of the terms): r and its correction cancel (exactly, but for the
    1e-6, in a molecule of one atom without a total charge), and so may Q and the sum of r"""
    r, f = out[:, :qd], out[:, qd:]
    fu = f ** 2
    z = lambda: torch.zeros(B, qd, dtype=out.dtype, device=out.device)
    Fu = z().index_add(0, batch, fu) + 1.0e-6
    Qu = z().index_add(0, batch, r)
    Q = torch.zeros(B, dtype=out.dtype, device=out.device) if Qmol is None else Qmol
    dQ = Q[:, None] - Qu
    corr = fu / Fu[batch] * dQ[batch]
    if not want_scale:
        return r + corr, Fu, dQ
    return (r + corr, r.abs() + corr.abs()), Fu, (dQ, Q.abs()[:, None] + z().index_add(0, batch, r.abs()))


def qeq_bwd(out, Fu, dQ, g_c, batch, qd, want_scale=False):
    """gradient of sum(g_c * charges) wrt out = [r | f] -> [N, 2 qd]; with want_scale also the sum of the absolute values of the
    two terms of each entry (g_c and S1 cancel: exactly, but for the 1e-6, in a molecule of one atom)"""
    f = out[:, qd:]
    S1 = torch.zeros_like(Fu).index_add(0, batch, g_c * f * f) / Fu
    gr = g_c - S1[batch]
    k = 2 * f * dQ[batch] / Fu[batch]
    g_out = torch.cat([gr, k * gr], 1)
    if not want_scale:
        return g_out
    ab = g_c.abs() + S1[batch].abs()
    return g_out, torch.cat([ab, k.abs() * ab], 1)


# ---------------------------------------------------------------------------------------------- edge MLP
def edge_pre1(g, Ap, Bt, Cs, C):
    """-> (pre1 [E, F] = Ap[pair] + Bt[target] + Cs[source], he1 = silu(pre1), Ce [E] = C[pair])"""
    pre1 = Ap[g["epair"]] + Bt[g["rows"]] + Cs[g["col"]]
    return pre1, silu(pre1), C[g["epair"]]


def edge_message(g, pre3, Ce, Pn):
    """M[i] = sum_{e in row i} w[e, type(c)] Pn[col(e), c] with the per-edge weights w = silu(pre3) Ce (tensornet2.py:548-600)"""
    E = g["col"].numel()
    w = silu(pre3.reshape(E, 3, -1)) * Ce[:, None, None]
    return MO.gather(dict(g, epair=torch.arange(E, device=pre3.device)), w, Pn)


def edge_gw(g, gMi, Pn, pre3, Ce):
    """gradient of sum(gMi * edge_message) wrt pre3 and Ce -> (g_pre3 [E, 3 F], slots [ceil(F / 64), E], scale of the slots);
    slot a holds the part of g_Ce of the channels 64 a .. 64 a + 63, scale the sum of the absolute values of its terms"""
    E, F = g["col"].numel(), gMi.shape[2]
    t = gMi[g["rows"]] * Pn[g["col"]]  # [E, 9, F]
    p3 = pre3.reshape(E, 3, F)
    g_w = torch.stack([t[:, 0], t[:, 1:4].sum(1), t[:, 4:9].sum(1)], 1)
    g_pre3 = g_w * Ce[:, None, None] * silu_grad(p3)
    ns = (F + WAVE - 1) // WAVE
    pad = lambda h: torch.nn.functional.pad(h, (0, ns * WAVE - F)).reshape(E, ns, WAVE).sum(2).t().contiguous()
    slots = pad((g_w * silu(p3)).sum(1))
    scale = pad((t.abs() * silu(p3).abs()[:, TYPE_OF, :]).sum(1))
    return g_pre3.reshape(E, 3 * F), slots, scale


def edge_reduce(g, g_pre1):
    """gradient of sum(g_pre1 * pre1) wrt Bt, Cs and the pair rows of Ap -> (gB [N, F], gCs [N, F], gAp [P, F])"""
    N, P, F = g["N"], g["P"], g_pre1.shape[1]
    z = lambda n: torch.zeros(n, F, dtype=g_pre1.dtype, device=g_pre1.device)
    off = g["rows"] != g["col"]
    return z(N).index_add(0, g["rows"], g_pre1), z(N).index_add(0, g["col"], g_pre1), z(P).index_add(0, g["epair"][off], g_pre1[off])


def pair_gd(g, gAp, dAp, slots, dC):
    """sum_f gAp[p, f] dAp[p, f] + g_C[p] dC[p] with g_C[p] the sum of g_Ce over both entries of pair p and all slot arrays: what
    the kernel ADDS to gd [P]"""
    P = g["P"]
    off = g["rows"] != g["col"]
    gC = torch.zeros(P, dtype=gAp.dtype, device=gAp.device).index_add(0, g["epair"][off], slots.sum(0)[off])
    return (gAp * dAp[:P]).sum(1) + gC * dC[:P]


# ---------------------------------------------------------------------------------------------- Coulomb head
def rf_constants(cut, eps):
    """(k_rf, c_rf) of the reaction field (output_modules.py:470-480)"""
    return (1.0 / cut ** 3) * (eps - 1.0) / (2.0 * eps + 1.0), (1.0 / cut) * (3.0 * eps) / (2.0 * eps + 1.0)


def min_image(delta, box_i):
    """triclinic minimum image, z -> y -> x in turn; delta [N, N, 3], box_i [N, 3, 3] the box of atom i"""
    for a in (2, 1, 0):
        delta = delta - torch.round(delta[..., a] / box_i[:, None, a, a])[..., None] * box_i[:, None, a]
    return delta


def coulomb_table(pos, batch, B, box, box_mode, cut):
    """-> (mask [N, N] of the pairs that count, delta [N, N, 3], d [N, N] (1 where masked out))"""
    N = pos.shape[0]
    valid = (batch >= 0) & (batch < B)
    mask = (batch[:, None] == batch[None, :]) & valid[:, None] & valid[None, :] & ~torch.eye(N, dtype=torch.bool, device=pos.device)
    delta = pos[:, None] - pos[None, :]
    if box_mode:
        delta = min_image(delta, box.reshape(1, 3, 3).expand(N, 3, 3) if box_mode == 1 else box.reshape(-1, 3, 3)[batch.clamp(0, B - 1)])
    d2 = (delta * delta).sum(-1)
    if cut > 0:
        mask = mask & (d2 < cut * cut)
    return mask, delta, torch.sqrt(torch.where(mask, d2, torch.ones_like(d2)))


def coulomb(pos, batch, B, box, box_mode, charges, wq, cut, eps, scale, want_grad=True):
    """damped pair Coulomb energy of all charge channels per atom (each pair in both atoms; output_modules.py:504-603) ->
    dict(ec [N]; and with want_grad g_q [N, QC] = d (scale sum ec) / d charges, fpos [N, 3] = - d (scale sum ec) / d pos)"""
    mask, delta, d = coulomb_table(pos, batch, B, box, box_mode, cut)
    u = (d / R_DAMP).clamp(max=1.0 - 1e-6)
    om = 1.0 - u * u
    hexp = torch.exp(-1.0 / om) / math.exp(-1.0)
    fc = 1.0 - hexp
    g, dg = 1.0 / d, -1.0 / (d * d)
    if cut > 0:
        k_rf, c_rf = rf_constants(cut, eps)
        g, dg = g + k_rf * d * d - c_rf, dg + 2.0 * k_rf * d
    W = wq.sum()
    s = torch.einsum("ik,jk,k->ij", charges, charges, wq) / W
    a = torch.where(mask, COULOMB_FACTOR * fc * g, torch.zeros_like(d))
    res = {"ec": (a * s).sum(1)}
    if want_grad:
        dfc = torch.where(d / R_DAMP < 1.0 - 1e-6, 2.0 * u * hexp / (om * om) / R_DAMP, torch.zeros_like(d))
        res["g_q"] = 2.0 * scale * wq[None, :] / W * (a @ charges)
        fr = torch.where(mask, -2.0 * scale * COULOMB_FACTOR * s * (dfc * g + fc * dg) / d, torch.zeros_like(d))
        res["fpos"] = (fr[:, :, None] * delta).sum(1)
    return res


# ---------------------------------------------------------------------------------------------- error figures
def group_rel_err(got, ref, groups=None, scale=None):
    """max over the groups (rows when None) of max|got - ref| / max|scale|, each group normalised by its own largest magnitude of
    `scale` (the reference itself when None); a group whose scale is all zero counts its absolute error"""
    n = ref.shape[0]
    if n == 0:
        return 0.0
    d = (got.reshape(n, -1).double() - ref.reshape(n, -1).double()).abs().amax(1)
    s = (ref if scale is None else scale).reshape(n, -1).double().abs().amax(1)
    if groups is not None:
        groups = groups.to(d.device)
        sel = [groups == m for m in torch.unique(groups).tolist()]
        d, s = torch.stack([d[m].max() for m in sel]), torch.stack([s[m].max() for m in sel])
    return float((d / torch.where(s > 0, s, torch.ones_like(s))).max())


slot_rel_err = MO.slot_rel_err
