"""The single-product GEMM family behind launch_gemm (csrc/tn_gemm.hip, tn_gemm_skinny.hip, tn_gemm_sb1.hip) through
tmdnet_debug_gemm_ex: every kernel of the family x every epilogue kind of epi_kind() (and one mixed flag set of the generic
one) x one group, three groups, three groups at offsets that are no multiples of 4, and the nine interleaved groups of the
tensor linears; padded leading dimensions; the device-side row count; the ends of the activation range.

Every case asserts the route it means to test (the value of gemm_route, which the launchers branch on): the routing thresholds
are performance choices, and a shape that silently reached another kernel would test nothing.  Reference: the generic branch of
epilogue_store restated in float64 (tests/tlin9_oracle.py: gemm_epilogue_reference).  Comparison per ROW, each row normalised
by its own maximum; everything outside rows [0, rows) x the groups' column windows must keep its bits (a NaN sentinel, or the
old value for the accumulating epilogue); two launches bit-identical.

Bounds: profiles/tlin9_gemm_unit_floor.json, max(2e-6, 4 x the float32 rounding floor of the reference itself on these inputs),
never above 1e-5 (tools/tlin9_gemm_unit_floor.py)."""
import ctypes as C

import pytest
import torch

from tests import kernel_unit_cases as K

pytestmark = pytest.mark.gpu

CASES = [(route, i) for route, cases in K.gemm_cases().items() for i in range(len(cases))]
CASE_IDS = [f"{route}-{K.gemm_cases()[route][i][0]}-{i}" for route, i in CASES]


@pytest.fixture(scope="module")
def bounds():
    return K.load_bounds()["gemm"]


def _case(hip_lib, route, i, extreme=False):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    layout, M, N, Kk = K.gemm_cases(n_cu)[route][i]
    # fp32 routes are offered no split image, except in the unaligned layout, which a split-bf16 kernel must decline
    split = route.startswith("sb1") or (layout == "g3u" and not extreme)
    return K.GemmCase(hip_lib, layout, M, N, Kk, split, extreme), (route, layout, M, N, Kk)


def _check(r, route, b, what, keys=None):
    print(what, r["route"], "rows", r["rows"], {k: f"{e:.3g}" for k, e in r["err"].items()}, {k: b[k]["bound"] for k in r["err"]})
    assert r["route"] == route, (what, "reached", r["route"])
    for k, e in r["err"].items():
        assert 2e-6 <= b[k]["bound"] <= 1e-5
        assert e < b[k]["bound"], (what, k, e, b[k]["bound"])
    assert r["finite"], what
    assert r["untouched_ok"], (what, "wrote outside the computed rows / column windows")
    assert r["deterministic"], (what, "two launches differ")


@pytest.mark.parametrize("route,i", CASES, ids=CASE_IDS)
def test_gemm_epilogues_vs_fp64(hip_lib, bounds, route, i):
    case, what = _case(hip_lib, route, i)
    if what[1] == "g3u":
        assert case.img is not None and any(o % 4 for o in case.lay["a_off"] + case.lay["c_off"])
    for epi in K.EPILOGUES:
        r = case.run(epi)
        assert set(r["err"]) == ({"C", "pre"} if K.EPILOGUES[epi][1] else {"C"})
        _check(r, route, bounds[route][epi], what + (epi,))


@pytest.mark.parametrize("route", list(K.gemm_cases()))
def test_gemm_device_row_count(hip_lib, bounds, route):
    """rows = min(M, *m_dev + m_add): rows below match, rows at or above keep the sentinel in C and pre (their old value for
    the accumulating epilogue)."""
    case, what = _case(hip_lib, route, 0)
    M = what[2]
    counts = K.m_dev_counts(M)
    assert {c + a for c, a in counts} >= {0, 1, M, M + 1000} and {a for _, a in counts} == {0, 1}
    for epi in ("silu_pre", "accum"):
        for (m_dev, m_add) in counts:
            r = case.run(epi, m_dev=m_dev, m_add=m_add)
            assert r["rows"] == max(0, min(M, m_dev + m_add))
            # with no row to compute the launch may still be sized for M: the route is that of the capacity
            _check(r, route, bounds[route][epi], what + (epi, m_dev, m_add))


@pytest.mark.parametrize("route", list(K.gemm_cases()))
def test_gemm_activation_range_ends(hip_lib, bounds, route):
    """pre-activations of +-30, +-88, +-1e4 through silu (from the bias) and through silu' (the aux operand): finite, and at the
    right limit.  fast_sigmoid is rcp(1 + __expf(-x)): it overflows to the right limit only if nothing on the way makes a NaN."""
    case, what = _case(hip_lib, route, 0, extreme=True)
    for epi in ("silu_pre", "muldsilu"):
        b = bounds[route]["extreme_" + epi]
        r = case.run(epi)
        _check(r, route, b, what + ("extreme", epi))
        assert r["elem_err"] < b["C"]["bound"], (what, epi, "element-wise, in units of max(1, |ref|)", r["elem_err"])
    aux = case.d["aux"][:, :what[3]]
    assert {float(x) for x in aux.unique()} == set(K.EXTREMES)


def test_gemm_ex_rejects_what_is_outside_the_contract(hip_lib):
    from torchmdnet_amd import _C

    M, N, Kk = 40, 32, 16
    A, W = torch.randn(M, Kk, device="cuda"), torch.randn(N, Kk, device="cuda")
    Cb = K.sentinel((M, N), "cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**over):
        x = _C.GemmExArgs()
        x.A, x.C, x.W[0] = A.data_ptr(), Cb.data_ptr(), W.data_ptr()
        x.lda, x.ldw, x.ldc, x.M, x.N, x.K, x.groups = Kk, Kk, N, M, N, Kk, 1
        for k, v in over.items():
            if k in ("W0", "a_off0", "c_off0"):
                getattr(x, k[:-1])[0] = v
            else:
                setattr(x, k, v)
        route = C.c_int32(-1)
        return hip_lib.tmdnet_debug_gemm_ex(s, C.byref(x), C.byref(route)), route.value

    for over in (dict(N=0), dict(K=0), dict(M=-1), dict(groups=0), dict(groups=10), dict(flags=32), dict(A=None), dict(C=None),
                 dict(W0=None), dict(flags=_C.GEMM_ROWSCALE), dict(flags=_C.GEMM_MUL_AUX), dict(flags=_C.GEMM_MUL_DSILU_AUX),
                 dict(lda=Kk - 1), dict(ldw=Kk - 1), dict(ldc=N - 1), dict(pre=Cb.data_ptr(), ldpre=N - 1), dict(a_off0=-1), dict(c_off0=-4)):
        assert call(**over)[0] == _C.ERR_INVALID, over
    assert hip_lib.tmdnet_debug_gemm_ex(s, None, None) == _C.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((K.bits(Cb) == K.SENTINEL).all()), "a rejected call launched"
    assert call(M=0) == (_C.OK, _C.GEMM_ROUTE_NONE)
    torch.cuda.synchronize()
    assert bool((K.bits(Cb) == K.SENTINEL).all())
    assert call() == (_C.OK, _C.GEMM_ROUTE_SKINNY4)
    torch.cuda.synchronize()
    assert torch.allclose(Cb, A @ W.t(), rtol=1e-4, atol=1e-4)
