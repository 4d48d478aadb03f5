"""Keeps tests/tlin9_oracle.py honest without a device: every adjoint it states must equal torch.autograd.grad of the forward
statement it inverts, in float64, to 1e-12 (per-atom max-norm relative); the forward statements are tied to the 3x3 algebra of
oracle/tensornet_adjoint.py.  The GPU tests (tests/test_gpu_tlin9.py, tests/test_gpu_gemm_epilogues.py) compare the kernels
with these functions."""
import pytest
import torch

from oracle.tensornet_adjoint import compose, quad
from tests import tlin9_oracle as O

TOL = 1e-12
N, F = 7, 5


def _rn(*s, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*s, generator=g, dtype=torch.float64)


def _kap(random_kap):
    return (torch.rand(N, generator=torch.Generator().manual_seed(9), dtype=torch.float64) * 2 - 0.5) if random_kap else None


def _Ws():
    return tuple(_rn(F, F, seed=20 + k) / F ** 0.5 for k in range(3))


def test_forward_statements_agree_with_the_3x3_algebra():
    u = _rn(N, 9, F, seed=1)
    frob = (compose(u) ** 2).sum((1, 2))
    assert O.per_atom_rel_err(quad(u), frob) < TOL
    assert O.per_atom_rel_err(O.invariants(u).sum(1), frob) < TOL  # the three parts are orthogonal
    y = O.norm(u)
    assert O.per_atom_rel_err(compose(y), compose(u) / (frob + 1)[:, None, None]) < TOL
    Ws = _Ws()
    C = O.lin(u, Ws)
    for c in range(9):
        assert torch.equal(C[:, c], u[:, c] @ Ws[O.TYPE_OF[c]].t())
    gates = _rn(N, 3, F, seed=2)
    X1 = O.gate(u, gates)
    for c in range(9):
        assert torch.equal(X1[:, c], u[:, c] * gates[:, O.TYPE_OF[c]])


@pytest.mark.parametrize("random_kap", [False, True])
def test_update_is_the_reference_layer_update(random_kap):
    """update() restated with full 3x3 matrices: X_hat + dX + kap dX dX (kap None = factor 1)."""
    X, dX, kap = _rn(N, 9, F, seed=3), _rn(N, 9, F, seed=4), _kap(random_kap)
    Xf, Df = compose(X), compose(dX)
    k = 1.0 if kap is None else kap[:, None, None, None]
    full = Xf / ((Xf ** 2).sum((1, 2)) + 1)[:, None, None] + Df + k * torch.einsum("nabf,nbcf->nacf", Df, Df)
    assert O.per_atom_rel_err(compose(O.update(X, dX, kap)), full) < TOL


def test_normbwd_is_the_gradient_of_the_normalisation():
    X, A, e1 = _rn(N, 9, F, seed=5).requires_grad_(), _rn(N, 9, F, seed=6), _rn(N, 9, F, seed=7)
    Ws = _Ws()
    g_in = e1 + O.lin(A, Ws)
    (auto,) = torch.autograd.grad((O.norm(X) * g_in).sum(), X)
    ref = O.reference("normbwd", {"A": A, "e0": X.detach(), "e1": e1}, Ws)
    assert set(ref) == set(O.WRITES["normbwd"])
    assert O.per_atom_rel_err(ref["C"], auto) < TOL


@pytest.mark.parametrize("random_kap", [False, True])
def test_updbwd_prologue_is_the_gradient_of_the_update_wrt_dX(random_kap):
    X, dX, G, kap = _rn(N, 9, F, seed=8), _rn(N, 9, F, seed=9).requires_grad_(), _rn(N, 9, F, seed=10), _kap(random_kap)
    (auto,) = torch.autograd.grad((O.update(X, dX, kap) * G).sum(), dX)
    assert O.per_atom_rel_err(O.update_bwd(G, dX.detach(), kap), auto) < TOL
    # the whole combination: the tensor linear of that, and (chained) the gradient with respect to the linear's input
    Ws = _Ws()
    ref = O.reference("updbwd", {"A": G, "A2": dX.detach()}, Ws, kap)
    assert O.per_atom_rel_err(ref["C"], O.lin(auto, Ws)) < TOL
    Y = _rn(N, 9, F, seed=11).requires_grad_()
    WT = tuple(w.t() for w in Ws)
    (auto_y,) = torch.autograd.grad((O.update(X, O.lin(Y, WT), kap) * G).sum(), Y)  # dX = lin(Y, W^T) -> g_Y = lin(g_dX, W)
    ref_y = O.reference("updbwd", {"A": G, "A2": O.lin(Y, WT).detach()}, Ws, kap)
    assert O.per_atom_rel_err(ref_y["C"], auto_y) < TOL


def test_gate_adjoint_is_the_gradient_of_the_gate_multiply():
    UX, a2, G = _rn(N, 9, F, seed=12).requires_grad_(), _rn(N, 3, F, seed=13).requires_grad_(), _rn(N, 9, F, seed=14)
    gates = torch.nn.functional.silu(a2)
    auto_ux, auto_a2 = torch.autograd.grad((O.gate(UX, gates) * G).sum(), (UX, a2))
    g_ux, g_a2 = O.gate_bwd(G, UX.detach(), gates.detach(), a2.detach())
    assert O.per_atom_rel_err(g_ux, auto_ux) < TOL
    assert O.per_atom_rel_err(g_a2, auto_a2) < TOL


def test_normbwd_gate_is_the_gradient_of_gate_then_normalise():
    """whole combination: X1 = gate(UX, silu(a2)) is normalised; incoming gradient e1 + lin(A) on the normalised tensor."""
    UX, a2 = _rn(N, 9, F, seed=15).requires_grad_(), _rn(N, 3, F, seed=16).requires_grad_()
    A, e1, Ws = _rn(N, 9, F, seed=17), _rn(N, 9, F, seed=18), _Ws()
    gates = torch.nn.functional.silu(a2)
    X1 = O.gate(UX, gates)
    auto_ux, auto_a2 = torch.autograd.grad((O.norm(X1) * (e1 + O.lin(A, Ws))).sum(), (UX, a2))
    ref = O.reference("normbwd_gate", {"A": A, "e0": X1.detach(), "e1": e1, "e2": UX.detach(), "e3": gates.detach(), "e4": a2.detach()}, Ws)
    assert set(ref) == set(O.WRITES["normbwd_gate"])
    assert O.per_atom_rel_err(ref["C"], auto_ux) < TOL
    assert O.per_atom_rel_err(ref["o1"], auto_a2) < TOL


def test_embbwd_is_the_gradient_wrt_the_ten_atom_inputs_with_the_trace_removed():
    I0, v, T = _rn(N, F, seed=19).requires_grad_(), _rn(N, 3, F, seed=30).requires_grad_(), _rn(N, 6, F, seed=31).requires_grad_()
    A, gs, Ws = _rn(N, 9, F, seed=32), _rn(N, 1, F, seed=33), _Ws()
    u0 = O.embed_atom_inputs_to_u0(I0, v, T)
    assert O.per_atom_rel_err((u0[:, 4] + u0[:, 7])[:, None].detach(), (T[:, 0] + T[:, 3] - 2 * (T[:, 0] + T[:, 3] + T[:, 5]) / 3)[:, None].detach()) < TOL
    g_lin = O.lin(A, Ws)
    gi, gv, gT = torch.autograd.grad((g_lin * u0).sum() + (gs[:, 0] * quad(u0)).sum(), (I0, v, T))
    # T = (T00, T01, T02, T11, T12, T22): the same order as rows 4..9 of the kernel's output
    auto = torch.cat([gi[:, None], gv, gT], 1)
    ref = O.reference("embbwd", {"A": A, "e0": u0.detach(), "e1": gs}, Ws)
    assert ref["o1"].shape == (N, 10, F)
    assert O.per_atom_rel_err(ref["o1"], auto) < TOL


@pytest.mark.parametrize("name", list(O.COMBOS))
@pytest.mark.parametrize("random_kap", [False, True])
def test_reference_defines_exactly_the_declared_outputs(name, random_kap):
    t, Ws, kap = O.make_inputs(name, 5, 8, seed=1, random_kap=random_kap)
    assert set(t) == {"A", *O.READS[name]}
    assert (kap is not None) == (random_kap and name in O.USES_KAP)
    if kap is not None:
        assert kap.min() >= -0.5 and kap.max() <= 1.5
    out = O.reference(name, {k: x.double() for k, x in t.items()}, tuple(w.double() for w in Ws), None if kap is None else kap.double())
    assert {k: x.shape[1] for k, x in out.items()} == O.WRITES[name]
    assert all(x.dtype == torch.float64 and torch.isfinite(x).all() for x in out.values())


def test_update_with_unit_kap_equals_no_kap():
    X, dX = _rn(N, 9, F, seed=3), _rn(N, 9, F, seed=4)
    one = torch.ones(N, dtype=torch.float64)
    assert torch.equal(O.update(X, dX, one), O.update(X, dX, None))
    assert torch.equal(O.update_bwd(X, dX, one), O.update_bwd(X, dX, None))


def test_gemm_epilogue_reference_orders_its_steps_and_honours_offsets_and_rows():
    M, Nn, K, G = 6, 3, 4, 2
    A = _rn(M, G * K + 1, seed=40)
    W = [_rn(Nn, K, seed=41 + g) for g in range(G)]
    b = [_rn(Nn, seed=43), None]
    Cold = _rn(M, G * Nn + 2, seed=44)
    aux = _rn(M, G * Nn + 1, seed=45)
    rs = _rn(M, seed=46)
    lay = dict(N=Nn, K=K, groups=G, flags=O.GEMM_ACT_SILU | O.GEMM_ROWSCALE | O.GEMM_MUL_AUX | O.GEMM_MUL_DSILU_AUX | O.GEMM_ACCUM,
               a_off=[1, 1 + K], c_off=[0, Nn + 2], pre_off=[1, 1 + Nn], aux_off=[0, Nn + 1], ldpre=G * Nn + 1, want_pre=True)
    rows = 4
    C, pre = O.gemm_epilogue_reference(A, W, b, Cold, aux, rs, lay, rows)
    for g in range(G):
        v = A[:rows, lay["a_off"][g]:lay["a_off"][g] + K] @ W[g].t() + (b[g] if b[g] is not None else 0)
        x = aux[:rows, lay["aux_off"][g]:lay["aux_off"][g] + Nn]
        s = torch.sigmoid(x)
        want = torch.nn.functional.silu(v) * rs[:rows, None] * x * (s * (1 + x * (1 - s))) + Cold[:rows, lay["c_off"][g]:lay["c_off"][g] + Nn]
        assert torch.allclose(C[:rows, lay["c_off"][g]:lay["c_off"][g] + Nn], want, rtol=1e-13, atol=0)
        assert torch.equal(pre[:rows, lay["pre_off"][g]:lay["pre_off"][g] + Nn], v)
    # untouched: rows past the count, and every column outside the groups' windows
    assert torch.equal(C[rows:], Cold[rows:]) and torch.isnan(pre[rows:]).all()
    assert torch.equal(C[:, Nn:Nn + 2], Cold[:, Nn:Nn + 2]) and torch.isnan(pre[:, 0]).all()
