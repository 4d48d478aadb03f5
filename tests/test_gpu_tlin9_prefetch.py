"""The epilogue of the fused tensor linears (csrc/tn_tlin9.hip) requests the operands of atom group G + 1 while it works on
group G, and the update adjoint requests its second prologue operand one double chunk behind the first.  The sizes here are the
ones at which a request that runs ahead can go wrong, which tests/test_gpu_tlin9.py does not have:

    (7, 128)                        groups 1-3 wholly behind N: every request that runs ahead is a clamped row
    (8, 128), (9, 128), (17, 128)   the last valid atom on either side of a group boundary
    (25, 128)                       group 3 partial
    (32 n_cu + 9, 128)              one tile more than there are blocks: a block walks on to a second tile (group 3 of a tile
                                    must not ask for the next tile), and that last tile has one valid group and one atom more

for every combination that carries an operand, in every variant of kernel_unit_cases.tlin9_variants (the normalisation adjoint
with C aliasing e1, the update with and without the invariants, with and without per-atom kappa).

Per case, what run_tlin9 reports: nothing behind row N written, nothing the combination does not define written, two launches
bit-identical, and every output per atom against float64 within the bound tests/test_gpu_tlin9.py applies to that output
(profiles/tlin9_gemm_unit_floor.json) AND within kernel_unit_cases.bound_of of this case's own float32 rounding floor."""
import functools

import pytest
import torch

from tests import kernel_unit_cases as K
from tests import tlin9_oracle as O

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["groups_1_to_3_behind_N", "group_0_full", "group_1_one_atom", "group_2_one_atom", "group_3_one_atom",
             "second_tile_one_group"]
NAMES = [n for n in O.COMBOS if n not in ("plain", "norm")]  # the combinations with an operand besides A and the weights


def shapes(n_cu):
    return [(7, 128), (8, 128), (9, 128), (17, 128), (25, 128), (32 * n_cu + 9, 128)]


@pytest.fixture(scope="module")
def bounds():
    return K.load_bounds()["tlin9"]


@functools.lru_cache(maxsize=None)
def floor_of(name, N, F, random_kap):
    return K.tlin9_floor(name, N, F, random_kap)


@pytest.mark.parametrize("shape", range(len(SHAPE_IDS)), ids=SHAPE_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_tlin9_requests_ahead(hip_lib, bounds, name, shape):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    N, F = shapes(n_cu)[shape]
    if SHAPE_IDS[shape] == "second_tile_one_group":
        assert (N + 31) // 32 * (F // 128) == n_cu + 1 and 8 < N % 32 <= 16
    variants = K.tlin9_variants(name)
    if name == "normbwd":
        assert (False, 1, True) in variants  # C is e1: a lane reads atom n + 8 while it writes atom n
    if name == "update":
        assert {w for (_, w, _) in variants} == {0, 1}
    for (random_kap, want_feat, alias) in variants:
        r = K.run_tlin9(hip_lib, name, N, F, random_kap, want_feat, alias)
        floor = floor_of(name, N, F, random_kap)
        what = (name, N, F, dict(random_kap=random_kap, want_feat=want_feat, alias=alias))
        print(what, {k: f"{e:.3g}" for k, e in r["err"].items()}, {k: f"{floor[k]:.3g}" for k in r["err"]},
              {k: bounds[name][k]["bound"] for k in r["err"]})
        assert set(r["err"]) == set(O.WRITES[name]) - ({"o2"} if (name == "update" and not want_feat) else set())
        for k, e in r["err"].items():
            b = min(bounds[name][k]["bound"], K.bound_of(floor[k]))
            assert 2e-6 <= b <= 1e-5
            assert e < b, (what, k, e, b)
        assert r["tail_ok"], (what, "rows behind N were written")
        assert r["undefined_ok"], (what, "an output this combination does not define was written")
        assert r["deterministic"], (what, "two launches differ")
