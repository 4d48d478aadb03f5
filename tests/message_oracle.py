"""TEST INFRASTRUCTURE ONLY -- plain torch statements of what TensorNet's neighbour sweeps compute (csrc/tn_kernels.hip:
k_message, k_message_split, k_message_adjoint, k_message_adjoint_gd, k_message_dual; csrc/tn_message_pair.hip: k_message_rows8,
k_message_adjoint_rows8), in the precision of their inputs: float64 inputs give the reference of tests/test_gpu_message.py,
float32 inputs the rounding floor its bounds are derived from (tools/message_unit_floor.py).

A graph is a dict in the engine's own form: rowptr [N + 1], col / epair / esign / rows per entry (int64 here), N, P; symmetric,
the columns of a row ascending, a self edge with pair id P in every row, esign +1 where the row atom is the pair's first atom
(col < row), -1 where it is the second, 0 on the self edge.  The 3x3 algebra is oracle/tensornet_adjoint.py's.
tests/test_message_oracle.py checks the adjoint, the distance-gradient halves and the tangent against autograd.
"""
import torch

from oracle.tensornet_adjoint import TYPE_OF, compose, dec, mm, quad

CHUNK = 2048  # entries per step of the per-entry statements (bounds the [entries, 9, F] intermediates)


def gather(g, w, src):
    """Mi[i, c, f] = sum_{e in row(i)} w[epair(e), type(c), f] * src[col(e), c, f]  (tensornet.py:757-806)."""
    out = torch.zeros_like(src)
    E = g["col"].numel()
    for a in range(0, E, CHUNK):
        s = slice(a, min(E, a + CHUNK))
        out.index_add_(0, g["rows"][s], w[g["epair"][s]][:, TYPE_OF, :] * src[g["col"][s]])
    return out


def kappa(q, batch, N, like):
    """both conventions of the kernels: 1 + 0.1 q[batch[i]] with `batch`, q[i] without it, 1 without q."""
    if q is None:
        return torch.ones(N, dtype=like.dtype, device=like.device)
    return 1 + 0.1 * q[batch] if batch is not None else q


def group_product(Y, M, kap, o3):
    """Ch = dec(C) / (quad(C) + 1),  C = kap (Y M + M Y) for O(3), 2 Y M for SO(3)  (tensornet.py:795-806)."""
    Yf, Mf = compose(Y), compose(M)
    C = kap[:, None, None, None] * (mm(Yf, Mf) + mm(Mf, Yf)) if o3 else 2 * mm(Yf, Mf)
    u = dec(C)
    return u / (quad(u) + 1)[:, None]


def forward(g, w, src, q, batch, o3):
    """-> (Mi, Ch) of the forward sweep."""
    Mi = gather(g, w, src)
    return Mi, group_product(src, Mi, kappa(q, batch, src.shape[0], src), o3)


def adjoint(g, w, gMi):
    """sum_e w * gMi[col(e)]: what the adjoint sweeps ADD to gPn (the graph and the pair rows are symmetric)."""
    return gather(g, w, gMi)


def pair_halves(g, dw, gMi, Pn, group):
    """h(i <- j) = sum_{k, f} dw[p, k, f] * sum_{c in k} gMi[j, c, f] * Pn[i, c, f], one partial sum per group of `group` channels.
    -> (slots [F / group, 2 P], scale [F / group, 2 P]): slot 2 p + 0 holds the half of the row with col < row (esign +1), slot
    2 p + 1 the other; scale is the sum of the absolute values of the terms of each half (the halves cancel heavily)."""
    F, P = gMi.shape[2], g["P"]
    ng = F // group
    slots = torch.zeros(ng, 2 * P + 2, dtype=gMi.dtype, device=gMi.device)
    scale = torch.zeros_like(slots)
    E = g["col"].numel()
    for a in range(0, E, CHUNK):
        s = slice(a, min(E, a + CHUNK))
        i, j, p = g["rows"][s], g["col"][s], g["epair"][s]
        t = dw[p][:, TYPE_OF, :] * gMi[j] * Pn[i]  # [e, 9, F]
        idx = 2 * p + (j > i).long()  # the self edge lands in 2 P (+ 0), cut off below
        slots.index_add_(1, idx, t.sum(1).reshape(-1, ng, group).sum(2).t().contiguous())
        scale.index_add_(1, idx, t.abs().sum(1).reshape(-1, ng, group).sum(2).t().contiguous())
    return slots[:, :2 * P], scale[:, :2 * P]


def dual(g, w, w_t, src, src_t):
    """value and tangent of the neighbour sum: (sum_e w src, sum_e w src_t + sum_e w_t src)."""
    return gather(g, w, src), gather(g, w, src_t) + gather(g, w_t, src)


def per_atom_rel_err(got, ref):
    """max over atoms of max|got - ref| / max|ref|, each atom's block normalised by its own maximum."""
    N = ref.shape[0]
    d = (got.reshape(N, -1).double() - ref.reshape(N, -1).double()).abs().amax(1)
    s = ref.reshape(N, -1).double().abs().amax(1).clamp_min(1e-300)
    return float((d / s).max())


def slot_rel_err(got, ref, scale):
    """max over the slot arrays (each on its own) and their slots of |got - ref| / (sum of the absolute terms of that half)."""
    if ref.numel() == 0:
        return 0.0
    return float(((got.double() - ref.double()).abs() / scale.double().clamp_min(1e-300)).max())
