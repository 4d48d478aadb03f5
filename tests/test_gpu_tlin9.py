"""The fused nine-component tensor linears (csrc/tn_tlin9.hip, k_tlin9<PRO, EPI>) in isolation, through tmdnet_debug_tlin9,
against the float64 statements of tests/tlin9_oracle.py (kept honest by autograd in tests/test_tlin9_oracle.py).

Every one of the eight launched combinations runs at the smallest sizes that reach each mechanism of the kernel
(kernel_unit_cases.tlin9_shapes: a single clamped row, the 32-atom tile boundary on both sides, two and three column tiles, a
partial epilogue group of eight atoms, and more tiles than compute units so that a persistent block walks a second tile).
Per case: every output against float64 PER ATOM (each atom's block normalised by its own maximum, so a bad tile cannot hide
behind a large atom elsewhere); 64 sentinel atoms behind row N and every output the combination does not define bit-unchanged;
two launches bit-identical; the normalisation adjoint also with C aliasing e1, as the reverse pass runs it.

Bounds: profiles/tlin9_gemm_unit_floor.json, max(2e-6, 4 x the float32 rounding floor of the reference itself on these inputs),
never above 1e-5 (tools/tlin9_gemm_unit_floor.py; the errors observed on the MI355X are recorded beside them)."""
import ctypes as C

import pytest
import torch

from tests import kernel_unit_cases as K
from tests import tlin9_oracle as O

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["one_row", "tile_minus_1", "tile", "tile_plus_1", "two_col_tiles_partial_group", "three_col_tiles", "second_tile_per_block"]


@pytest.fixture(scope="module")
def bounds():
    return K.load_bounds()["tlin9"]


@pytest.mark.parametrize("shape", range(len(SHAPE_IDS)), ids=SHAPE_IDS)
@pytest.mark.parametrize("name", list(O.COMBOS))
def test_tlin9_vs_fp64(hip_lib, bounds, name, shape):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    N, F = K.tlin9_shapes(n_cu)[shape]
    if SHAPE_IDS[shape] == "second_tile_per_block":
        assert (N + 31) // 32 * (F // 128) > n_cu and N % 32
    for (random_kap, want_feat, alias) in K.tlin9_variants(name):
        r = K.run_tlin9(hip_lib, name, N, F, random_kap, want_feat, alias)
        what = (name, N, F, dict(random_kap=random_kap, want_feat=want_feat, alias=alias))
        print(what, {k: f"{e:.3g}" for k, e in r["err"].items()}, {k: bounds[name][k]["bound"] for k in r["err"]})
        assert set(r["err"]) == set(O.WRITES[name]) - ({"o2"} if (name == "update" and not want_feat) else set())
        for k, e in r["err"].items():
            b = bounds[name][k]["bound"]
            assert 2e-6 <= b <= 1e-5
            assert e < b, (what, k, e, b)
        assert r["tail_ok"], (what, "rows behind N were written")
        assert r["undefined_ok"], (what, "an output this combination does not define was written")
        assert r["deterministic"], (what, "two launches differ")


def test_tlin9_rejects_what_is_outside_the_contract(hip_lib):
    """TMDNET_ERR_INVALID and no launch: F % 128, N < 1, an unknown (pro, epi) pair, a missing operand, a short scratch."""
    from torchmdnet_amd import _C

    N, F = 5, 128
    t, Ws, _ = O.make_inputs("normbwd_gate", N, F, 1, False)
    dev = {k: v.cuda() for k, v in t.items()}
    W = [w.cuda() for w in Ws]
    out = {k: K.sentinel((N + K.TAIL, 9, F), "cuda") for k in ("C", "o1", "o2")}
    scratch, n = K.tlin9_scratch(hip_lib, F, "cuda")
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(pro=0, epi=0, N=N, F=F, n=n, scratch=scratch, **over):
        o = dict(A=dev["A"], A2=dev["A"], C=out["C"], e0=dev["e0"], e1=dev["e1"], e2=dev["e2"], e3=dev["e3"], e4=dev["e4"],
                 o1=out["o1"], o2=out["o2"], kap=None)
        o.update(over)
        return hip_lib.tmdnet_debug_tlin9(s, pro, epi, N, F, *[p(o[k]) for k in ("A", "A2", "C", "e0", "e1", "e2", "e3", "e4", "o1", "o2", "kap")],
                                          1, p(W[0]), p(W[1]), p(W[2]), p(scratch), C.byref(n))

    assert call(F=96) == _C.ERR_INVALID and call(F=0) == _C.ERR_INVALID and call(F=192) == _C.ERR_INVALID
    assert call(N=0) == _C.ERR_INVALID and call(N=-3) == _C.ERR_INVALID
    for pro, epi in [(1, 1), (2, 2), (1, 5), (3, 0), (0, 6), (-1, 0), (0, -1)]:
        assert call(pro, epi) == _C.ERR_INVALID, (pro, epi)
    assert call(A=None) == _C.ERR_INVALID and call(C=None) == _C.ERR_INVALID
    assert call(2, 0, A2=None) == _C.ERR_INVALID
    assert call(0, 1, e3=None) == _C.ERR_INVALID and call(0, 1, o1=None) == _C.ERR_INVALID
    assert call(0, 2, e0=None) == _C.ERR_INVALID and call(0, 2, o2=None) == _C.ERR_INVALID
    assert call(0, 3, e1=None) == _C.ERR_INVALID
    for k in ("e0", "e1", "e2", "e3", "e4", "o1"):
        assert call(0, 4, **{k: None}) == _C.ERR_INVALID, k
    assert call(0, 5, o1=None) == _C.ERR_INVALID
    assert call(n=C.c_int64(n.value - 1)) == _C.ERR_INVALID
    torch.cuda.synchronize()
    assert all(bool((K.bits(x) == K.SENTINEL).all()) for x in out.values()), "a rejected call launched"
    assert call(0, 0) == _C.OK  # and the same arguments, within the contract, run
    torch.cuda.synchronize()
    assert torch.isfinite(out["C"][:N]).all() and bool((K.bits(out["C"][N:]) == K.SENTINEL).all())
