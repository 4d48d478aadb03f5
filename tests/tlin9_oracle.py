"""TEST INFRASTRUCTURE ONLY -- plain torch statements of what the fused nine-component tensor linears (csrc/tn_tlin9.hip,
k_tlin9<PRO, EPI>) and the GEMM epilogues (csrc/tn_gemm_epi.h, epilogue_store) compute, in the precision of their inputs:
float64 inputs give the reference of the GPU unit tests, float32 inputs give the rounding floor that their tolerances are
derived from (tools/tlin9_gemm_unit_floor.py).

The specification is csrc/tn_tlin9.h and the stand-alone kernels of csrc/tn_kernels.hip that the unfused schedule runs
(k_norm_x, k_update, k_update_bwd, k_norm_bwd, k_embed_gate_bwd, k_embed_bwd_atom); the 3x3 algebra is
oracle/tensornet_adjoint.py's.  tests/test_tlin9_oracle.py checks every adjoint written here against autograd of the forward
statement it inverts.
"""
import torch

from oracle.tensornet_adjoint import TYPE_OF, compose, compose_T, dec, dec_T, dquad, mm, quad, silu_grad, tensor_linear, tr_

# name -> (pro, epi) of tmdnet_debug_tlin9: the eight launched combinations
COMBOS = {
    "plain": (0, 0),
    "norm": (1, 0),
    "mulgate": (0, 1),
    "update": (0, 2),
    "updbwd": (2, 0),
    "normbwd": (0, 3),
    "normbwd_gate": (0, 4),
    "embbwd": (0, 5),
}
# inputs each combination reads besides A and the three weights, and the outputs it defines (name -> components per atom)
READS = {
    "plain": (), "norm": (), "mulgate": ("e3",), "update": ("e0",), "updbwd": ("A2",), "normbwd": ("e0", "e1"),
    "normbwd_gate": ("e0", "e1", "e2", "e3", "e4"), "embbwd": ("e0", "e1"),
}
WRITES = {
    "plain": {"C": 9}, "norm": {"C": 9}, "mulgate": {"C": 9, "o1": 9}, "update": {"C": 9, "o1": 9, "o2": 3},
    "updbwd": {"C": 9}, "normbwd": {"C": 9}, "normbwd_gate": {"C": 9, "o1": 3}, "embbwd": {"o1": 10},
}
USES_KAP = ("update", "updbwd")
# components per atom of every operand ([N, comps, F])
OPERAND_COMPS = {"A": 9, "A2": 9, "e0": 9, "e1": 9, "e2": 9, "e3": 3, "e4": 3}


def lin(A, Ws):
    """C[n, c, :] = A[n, c, :] @ W_type(c)^T  (tensornet.py:595-617, 752-754, 808-810)."""
    return tensor_linear(A, Ws)


def norm(X):
    """X / (||X||^2 + 1) per atom and channel (k_norm_x; tensornet.py:745)."""
    return X / (quad(X) + 1)[:, None]


def _kap(kap, ndim):
    return 1.0 if kap is None else kap.reshape((-1,) + (1,) * (ndim - 1))


def gate(X, gates):
    """X[n, c, f] * gates[n, type(c), f]."""
    return X * gates[:, TYPE_OF]


def update(X, dX, kap=None):
    """new X = dec(compose(X_hat) + compose(dX) + kap compose(dX) compose(dX)), X_hat = norm(X)  (k_update; tensornet.py:808-812)."""
    D = compose(dX)
    return dec(compose(norm(X)) + D + _kap(kap, 4) * mm(D, D))


def invariants(u):
    """[N, 9, F] -> [N, 3, F]: ||I 1||^2, ||A||^2, ||S||^2 of the three irreducible parts (tensornet.py:144-146 per part)."""
    I, v0, v1, v2, s0, s1, s2, s3, s4 = u.unbind(1)
    return torch.stack([3 * I * I, 2 * (v0 * v0 + v1 * v1 + v2 * v2),
                        s0 * s0 + s3 * s3 + (s0 + s3) ** 2 + 2 * (s1 * s1 + s2 * s2 + s4 * s4)], 1)


def update_bwd(G, dX, kap=None):
    """adjoint of `update` with respect to dX (in stored components): compose^T(Gf + kap (Gf D^T + D^T Gf)), Gf = dec^T(G)."""
    Gf = dec_T(G)
    Dt = tr_(compose(dX))
    return compose_T(Gf + _kap(kap, 4) * (mm(Gf, Dt) + mm(Dt, Gf)))


def norm_bwd(X, g):
    """adjoint of `norm` at X contracted with the incoming gradient g (k_norm_bwd<0>)."""
    inv = 1 / (quad(X) + 1)
    dot = (g * X).sum(1)
    return g * inv[:, None] + dquad(X) * (-dot * inv * inv)[:, None]


def gate_bwd(G, UX, gates, a2):
    """adjoint of X1 = gate(UX, gates) with gates = silu(a2): (g_UX [N, 9, F], g_a2 [N, 3, F])  (k_embed_gate_bwd)."""
    g_gate = torch.zeros_like(gates)
    g_gate.index_add_(1, torch.tensor(TYPE_OF, device=G.device), G * UX)
    return gate(G, gates), g_gate * silu_grad(a2)


def embed_atom_inputs_to_u0(I0, v, T):
    """forward the embedding atom adjoint inverts: (I0 [N, F], v [N, 3, F], T [N, 6, F] = T00 T01 T02 T11 T12 T22 of a symmetric
    3x3) -> stored components [N, 9, F]; the trace of T is removed from the two stored diagonal entries."""
    third = (T[:, 0] + T[:, 3] + T[:, 5]) / 3
    return torch.cat([I0[:, None], v, torch.stack([T[:, 0] - third, T[:, 1], T[:, 2], T[:, 3] - third, T[:, 4]], 1)], 1)


def embed_bwd_atom(g_lin, u0, g_s0n):
    """[N, 10, F]: gradient with respect to (I0, v[3], T00, T01, T02, T11, T12, T22) of <g_lin, u0> + <g_s0n, quad(u0)>
    (k_embed_bwd_atom)."""
    g = g_lin + dquad(u0) * g_s0n[:, None]
    third = (g[:, 4] + g[:, 7]) / 3
    return torch.stack([g[:, 0], g[:, 1], g[:, 2], g[:, 3], g[:, 4] - third, g[:, 5], g[:, 6], g[:, 7] - third, g[:, 8], -third], 1)


def reference(name, t, Ws, kap=None):
    """Outputs of combination `name` as a dict (keys of WRITES[name]); t: dict of operands in one dtype, Ws: (W_I, W_A, W_S)."""
    A = t["A"]
    if name == "plain":
        return {"C": lin(A, Ws)}
    if name == "norm":
        return {"C": lin(norm(A), Ws)}
    if name == "mulgate":
        o1 = lin(A, Ws)
        return {"o1": o1, "C": gate(o1, t["e3"])}
    if name == "update":
        dX = lin(A, Ws)
        o1 = update(t["e0"], dX, kap)
        return {"C": dX, "o1": o1, "o2": invariants(o1)}
    if name == "updbwd":
        return {"C": lin(update_bwd(A, t["A2"], kap), Ws)}
    if name == "normbwd":
        return {"C": norm_bwd(t["e0"], t["e1"] + lin(A, Ws))}
    if name == "normbwd_gate":
        G = norm_bwd(t["e0"], t["e1"] + lin(A, Ws))
        gUX, g_a2 = gate_bwd(G, t["e2"], t["e3"], t["e4"])
        return {"C": gUX, "o1": g_a2}
    if name == "embbwd":
        return {"o1": embed_bwd_atom(lin(A, Ws), t["e0"], t["e1"][:, 0])}
    raise KeyError(name)


def make_inputs(name, N, F, seed, random_kap):
    """fp32 operands of one case: per-atom scale spread over (0, 2) on every [N, *, F] operand (as test_mfma_gemm_unit scales
    its rows; one exception below), weights ~ N(0, 1/F), kap None or uniform in [-0.5, 1.5].  Returns (t, Ws, kap) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    Ws = tuple(rn(F, F) / F ** 0.5 for _ in range(3))
    # update: spread (0, 1) on A.  With (0, 2) the float32 reference alone is 2.9e-6 off its float64 self in o2 (the squares of an
    # o1 that dX dominates wherever the atom's X is small), and four times that is past the 1e-5 cap of the unit tests' bounds.
    t = {"A": rn(N, 9, F) * (ru(N, 1, 1) * (1 if name == "update" else 2))}
    for k in READS[name]:
        comps = OPERAND_COMPS[k]
        if name == "embbwd" and k == "e1":
            comps = 1  # [N, F]: the gradient of the scalar embedding's norm input
        t[k] = rn(N, comps, F) * (ru(N, 1, 1) * 2)
    if name == "normbwd_gate":
        t["e3"] = torch.nn.functional.silu(t["e4"])  # the gates are silu of their pre-activations, as in the model
    kap = (ru(N) * 2 - 0.5) if (random_kap and name in USES_KAP) else None
    return t, Ws, kap


def per_atom_rel_err(got, ref):
    """max over atoms of max|got - ref| / max|ref| with each atom's block normalised by its own maximum."""
    N = ref.shape[0]
    d = (got.reshape(N, -1).double() - ref.reshape(N, -1).double()).abs().amax(1)
    s = ref.reshape(N, -1).double().abs().amax(1).clamp_min(1e-300)
    return float((d / s).max())


# ------------------------------------------------------------------------------ GEMM epilogues
GEMM_ACT_SILU, GEMM_MUL_AUX, GEMM_MUL_DSILU_AUX, GEMM_ACCUM, GEMM_ROWSCALE = 1, 2, 4, 8, 16


def gemm_epilogue_reference(A, W, bias, C_old, aux, rowscale, lay, rows):
    """The EPI_GENERIC branch of epilogue_store, literally, over groups and offsets.  Every specialised kind is one flag set of it.

    A [M, lda], C_old [M, ldc], aux [M, ldaux] or None are the whole row-major buffers; W / bias: one per group ([N, K] / [N] or
    None); lay: dict(N, K, groups, flags, a_off, c_off, pre_off, aux_off, ldpre, want_pre); rows: number of rows computed.
    Returns (C, pre): copies of the buffers with rows [0, rows) of every group's column window overwritten (pre: a NaN buffer
    [M, ldpre] with the windows written, or None)."""
    N, K, flags = lay["N"], lay["K"], lay["flags"]
    C = C_old.clone()
    pre = torch.full((A.shape[0], lay["ldpre"]), float("nan"), dtype=A.dtype, device=A.device) if lay["want_pre"] else None
    r = slice(0, rows)
    for g in range(lay["groups"]):
        v = A[r, lay["a_off"][g]:lay["a_off"][g] + K] @ W[g].t()
        if bias[g] is not None:
            v = v + bias[g]
        if pre is not None:
            pre[r, lay["pre_off"][g]:lay["pre_off"][g] + N] = v
        if flags & GEMM_ACT_SILU:
            v = v * torch.sigmoid(v)
        if flags & GEMM_ROWSCALE:
            v = v * rowscale[r, None]
        if flags & (GEMM_MUL_AUX | GEMM_MUL_DSILU_AUX):
            x = aux[r, lay["aux_off"][g]:lay["aux_off"][g] + N]
            if flags & GEMM_MUL_AUX:
                v = v * x
            if flags & GEMM_MUL_DSILU_AUX:
                v = v * silu_grad(x)
        if flags & GEMM_ACCUM:
            v = v + C_old[r, lay["c_off"][g]:lay["c_off"][g] + N]
        C[r, lay["c_off"][g]:lay["c_off"][g] + N] = v
    return C, pre


def per_row_rel_err(got, ref, cols):
    """max over rows of max|got - ref| / max|ref| over the column index list `cols`, every row normalised by its own maximum."""
    if ref.shape[0] == 0:
        return 0.0
    g, r = got[:, cols].double(), ref[:, cols].double()
    d = (g - r).abs().amax(1)
    s = r.abs().amax(1).clamp_min(1e-300)
    return float((d / s).max())
