"""The reverse tile sweep with the adjoint of the group product in its prologue (k_message_adjoint_rows8_fold), in isolation,
through tmdnet_debug_message_fold, on hand-built graphs whose 64-row tiles are all closed, against float64: gM, gY = autograd
gradients of sum(gCh * group_product(Pn, Mi, kap, o3)) (tests/message_oracle.py), gPn = gY + adjoint(g, w, gM), slots =
pair_halves(g, dw, gM, Pn, 32).

Graphs (tests/message_fold_cases.py): one complete 64-atom molecule (4096 adjacency entries exactly); 64 + 37 atoms (a partial
last tile whose dead rows help); molecules of 20 + 44, 64 and 1 + 63 atoms (several molecules per tile, a one-atom molecule that
walks the tails of the long rows); a star (one row of 64 entries, the others of 2).  F = 32 and 128; O(3) with per-molecule q,
O(3) with per-atom kappa, SO(3).

Per case and mode: every gPn row per atom and every slot array on its own against float64; the slots bit-identical to, and gPn
within the bound of, the sequence the kernel replaces (k_message_bwd_node, then k_message_adjoint_rows8) run through the same
entry; 64 sentinel rows behind row N, the slots no edge owns and the slot array beyond the kernel's count bit-unchanged; two
launches bit-identical; nothing written with the pair-overflow flag set; the gMi buffer untouched.

Bounds: profiles/message_fold_floor.json, max(2e-6, 4 x the float32 rounding floor of the reference itself on the case's inputs),
never above 1e-5 (tools/message_fold_floor.py; the errors observed on the MI355X are recorded beside them)."""
import ctypes as C
import math

import pytest
import torch

from tests import kernel_unit_cases as K
from tests import message_fold_cases as M

pytestmark = pytest.mark.gpu

CASES = M.all_cases()


@pytest.fixture(scope="module")
def bounds():
    return M.load_bounds()["cases"]


@pytest.mark.parametrize("case", CASES, ids=[M.case_id(c) for c in CASES])
def test_folded_sweep_vs_fp64_and_parent_sequence(hip_lib, bounds, case):
    r = M.run_case(hip_lib, case)
    ent = bounds[M.case_id(case)]
    for mode, errs in r["err"].items():
        print(M.case_id(case), mode, {k: f"{e:.3g}" for k, e in errs.items()}, {k: ent[mode][k]["bound"] for k in errs},
              "gPn vs parent sequence %.3g" % r["vs_parent"][mode], "bit-identical" if r["gPn_bit_identical"][mode] else "not bit-identical")
    assert r["finite"], (case, "an output row or a slot the kernel owns was left at the NaN sentinel, or is not finite")
    for mode, errs in r["err"].items():
        assert set(errs) == {"gPn", "slots"}
        for k, e in errs.items():
            b = ent[mode][k]["bound"]
            assert b == K.bound_of(ent[mode][k]["floor"]) and 2e-6 <= b <= 1e-5
            assert math.isfinite(e) and e < b, (case, mode, k, e, b)
        e = r["vs_parent"][mode]
        assert math.isfinite(e) and e < ent[mode]["gPn"]["bound"], (case, mode, "gPn against the parent sequence", e)
    assert r["slots_equal_parent"], (case, "the slots differ from the parent sequence's")
    assert r["tail_ok"], (case, "rows behind N were written")
    assert r["unowned_ok"], (case, "a slot no edge owns or a slot array beyond the kernel's count was written")
    assert r["deterministic"], (case, "two launches differ")
    assert r["overflow_ok"], (case, "written although the pair-overflow flag is set")
    assert r["gMi_untouched"], (case, "the folded kernel wrote gMi")


def test_fold_entry_rejects_what_is_outside_the_contract(hip_lib):
    """TMDNET_ERR_INVALID and no launch: a graph whose tiles are not closed, F % 32, N < 1, a NULL operand, short slot arrays."""
    from torchmdnet_amd import _C
    from tests import message_unit_cases as U

    F = 32
    g = M.build_graph("partial")
    d = {k: v.cuda().contiguous() for k, v in M.make_inputs("partial", F).items()}
    gd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in g.items()}
    csr = dict(rowptr=gd["rowptr"].int(), col=gd["col"].int(), epair=gd["epair"].int(), esign=gd["esign"].contiguous(),
               counts=torch.zeros(8, dtype=torch.int32, device="cuda"))
    out = M.fresh_outputs(g, F, "cuda")
    assert hip_lib.tmdnet_debug_message_fold(None, None) == _C.ERR_INVALID
    # a 65-atom chain: atom 64's neighbours lie in the tile before it
    og = U.build_graph("chain65")
    ogd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in og.items()}
    ocsr = dict(rowptr=ogd["rowptr"].int(), col=ogd["col"].int(), epair=ogd["epair"].int(), esign=ogd["esign"].contiguous(),
                counts=csr["counts"])
    od = {k: v.cuda().contiguous() for k, v in U.make_inputs("chain65", F).items()}
    od.update(Mi=od["src"], gCh=od["gMi"])
    oout = M.fresh_outputs(og, F, "cuda")
    assert M.launch(hip_lib, ogd, ocsr, od, F, "so3", oout, True) == _C.ERR_INVALID
    assert M.launch(hip_lib, ogd, ocsr, od, F, "so3", oout, False) == _C.OK  # the parent sequence takes any graph
    assert bool((K.bits(oout["gPn"][og["N"]:]) == K.SENTINEL).all()) and bool(torch.isfinite(oout["gPn"][:og["N"]]).all())

    def rejected(edit):
        from torchmdnet_amd._C import MessageFoldArgs
        x = MessageFoldArgs()
        x.N, x.F, x.P, x.o3, x.folded = g["N"], F, g["P"], 1, 1
        x.rowptr, x.col, x.epair, x.esign, x.counts = (csr[k].data_ptr() for k in ("rowptr", "col", "epair", "esign", "counts"))
        x.w, x.dw, x.gCh, x.Pn, x.Mi = (d[k].data_ptr() for k in ("w", "dw", "gCh", "Pn", "Mi"))
        x.gPn, x.slots, x.slot_stride = out["gPn"].data_ptr(), out["slots"].data_ptr(), out["slots"].shape[1]
        edit(x)
        rc = hip_lib.tmdnet_debug_message_fold(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(x))
        assert rc == _C.ERR_INVALID, rc

    for field, bad in (("N", 0), ("F", 48), ("F", 0), ("P", -1), ("slot_stride", 2 * g["P"] - 1)):
        rejected(lambda x, f=field, v=bad: setattr(x, f, v))
    for field in ("rowptr", "col", "epair", "esign", "counts", "w", "dw", "gCh", "Pn", "Mi", "gPn", "slots"):
        rejected(lambda x, f=field: setattr(x, f, None))
    rejected(lambda x: setattr(x, "folded", 0))  # the parent sequence needs gMi
    torch.cuda.synchronize()
    assert all(bool((K.bits(t) == K.SENTINEL).all()) for t in out.values()), "a rejected call launched"
