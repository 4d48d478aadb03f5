"""TensorNet's neighbour sweeps and their adjoints in isolation, through tmdnet_debug_message, on hand-built graphs, against the
float64 statements of tests/message_oracle.py (kept honest by autograd in tests/test_message_oracle.py).

Every stored-row kernel the launchers can pick runs by explicit selection, so the tile kernels (k_message_rows8<8, 4>,
k_message_adjoint_rows8, which the engine reaches from 8 192 atoms on at F = 128) run on graphs of 1 to 209 atoms built to hit
each of their block-uniform branches and boundaries: staged / unstaged window, adjacency slice in LDS / walked from global
memory, wn == 64 and nE == 4096 exactly and one past, partial last tiles whose dead rows help the longest rows, rows longer than
eight records per lane, equal rows (no helper), a window of dozens of molecules, a block count that is no multiple of 8.  The row
kernels run on a ladder of complete molecules of 1 .. 26 atoms (every row length: every unroll tail) and on the mixed batch.
tests/test_message_oracle.py asserts, without a device, that the case list as a whole contains a tile of every class.

Per case: every output row against float64 PER ATOM (each atom's [9, F] block normalised by its own maximum); every slot array of
the distance-gradient halves on its own against the float64 partial sum of its channel group, each half normalised by the sum
of the absolute values of its terms; 64 sentinel rows behind row N, every slot no edge owns and every slot array beyond the
kernel's count bit-unchanged; accumulating kernels start from random contents; two launches bit-identical; the forward kernels in
O(3) with per-molecule q, O(3) with per-atom kappa, and SO(3); the forward tile kernel with and without the balanced walk; with
the pair-overflow flag set nothing is written; *route_out is the selected kernel.

Bounds: profiles/message_unit_floor.json, max(2e-6, 4 x the float32 rounding floor of the reference itself on the case's
inputs), never above 1e-5 (tools/message_unit_floor.py; the errors observed on the MI355X are recorded beside them)."""
import ctypes as C
import math

import pytest
import torch

from tests import kernel_unit_cases as K
from tests import message_oracle as O
from tests import message_unit_cases as M

pytestmark = pytest.mark.gpu

CASES = M.all_cases()


@pytest.fixture(scope="module")
def bounds():
    return M.load_bounds()["cases"]


@pytest.mark.parametrize("case", CASES, ids=[M.case_id(c) for c in CASES])
def test_message_kernel_vs_fp64(hip_lib, bounds, case):
    r = M.run_case(hip_lib, case)
    ent = bounds[M.case_id(case)]
    print(M.case_id(case), {k: f"{e:.3g}" for k, e in r["err"].items()}, {k: ent[k]["bound"] for k in r["err"]})
    assert set(r["err"]) == set(M.outputs_of(case[0]))
    assert r["finite"], (case, "an output row or a slot the kernel owns was left at the NaN sentinel, or is not finite")
    for k, e in r["err"].items():
        b = ent[k]["bound"]
        assert b == K.bound_of(ent[k]["floor"]) and 2e-6 <= b <= 1e-5
        assert math.isfinite(e) and e < b, (case, k, e, b)
    assert r["route_ok"], (case, "*route_out is not the selected kernel")
    assert r["slot_arrays_ok"], (case, "number of slot arrays")
    assert r["tail_ok"], (case, "rows behind N were written")
    assert r["unowned_ok"], (case, "a slot no edge owns, a slot array beyond the kernel's count or an output of another sweep was written")
    assert r["deterministic"], (case, "two launches differ")
    assert r["overflow_ok"], (case, "written although the pair-overflow flag is set")


def test_auto_is_the_launchers_own_choice(hip_lib):
    """TMDNET_MSG_AUTO goes through launch_message* with (N, F, small_mols): the route reported is the selection function's, the
    slot-array count is message_adjoint_gd_waves', and the result is the selected kernel's, bit for bit.  The dual sweep's
    small-system route (zero fill + three split sweeps) has no selector: it is compared with float64 here, bound by the same rule."""
    from torchmdnet_amd import _C

    for (gname, F, want) in [("ladder", 64, {"fwd": _C.MSG_FWD_SPLIT, "adj": _C.MSG_ADJ_SPLIT, "gd": _C.MSG_GD_SPLIT, "dual": _C.MSG_DUAL_SPLIT3}),
                             ("ladder", 192, {"fwd": _C.MSG_FWD_ROW, "adj": _C.MSG_ADJ_ROW, "gd": _C.MSG_GD_ROW, "dual": _C.MSG_DUAL})]:
        g, d, csr, d64, _ = M._device_case(gname, F, "cuda")
        for kernel in ("fwd_row", "adj_row", "gd_row", "dual"):
            op = kernel.split("_")[0]
            outs = []
            for sel in (_C.MSG_AUTO, want[op]):
                if sel == _C.MSG_DUAL_SPLIT3:  # a route, not a selector
                    continue
                x = M.message_args(kernel, g, csr, F, small_mols=1)
                x.kernel = sel
                out = M.fresh_outputs(kernel, g, d, F, "cuda")
                rc, route, ns = M.launch(hip_lib, kernel, x, d, out, "o3_mol", g)
                assert rc == _C.OK and route == want[op], (gname, F, kernel, sel, rc, route)
                assert ns == (F // 64 if op == "gd" else 0)
                outs.append(out)
            if len(outs) == 2:
                assert all(torch.equal(K.bits(outs[0][k]), K.bits(outs[1][k])) for k in outs[0])
            assert torch.isfinite(outs[0]["out"][:g["N"]]).all()
            if want[op] == _C.MSG_DUAL_SPLIT3:  # no selector reaches this route: the launcher's zero fill + three split sweeps vs fp64
                lo = M.reference("dual", M.build_graph(gname), M.make_inputs(gname, F))
                ref = M.reference("dual", g, d64)
                for k, name in (("out", "out"), ("out2", "out_t")):
                    floor = O.per_atom_rel_err(lo[name], ref[name].cpu())  # fp32 statement on THESE inputs (CPU), the rule as everywhere
                    e = O.per_atom_rel_err(outs[0][k][:g["N"]], ref[name])
                    print("auto dual_split3", name, f"err {e:.3g} floor {floor:.3g}")
                    assert math.isfinite(e) and e < K.bound_of(floor), (name, e, floor)
                    assert bool((K.bits(outs[0][k][g["N"]:]) == K.SENTINEL).all())
    # below the tile threshold the hint changes nothing; the tile route itself is pinned in tests/test_gpu_bench_scale.py
    g, d, csr, _, _ = M._device_case("mixed", 256, "cuda")
    for hint in (0, 1):
        x = M.message_args("gd_row", g, csr, 256, small_mols=hint)
        x.kernel = _C.MSG_AUTO
        rc, route, ns = M.launch(hip_lib, "gd_row", x, d, M.fresh_outputs("gd_row", g, d, 256, "cuda"))
        assert (rc, route, ns) == (_C.OK, _C.MSG_GD_ROW, 4)


def test_message_rejects_what_is_outside_the_contract(hip_lib):
    """TMDNET_ERR_INVALID and no launch: N < 1, an F outside the selected kernel's contract, an unknown selector or one of another
    sweep, a NULL graph array or operand, slot arrays shorter than the pair list."""
    from torchmdnet_amd import _C

    F = 64
    g, d, csr, _, _ = M._device_case("chain65", F, "cuda")
    outs = {k: M.fresh_outputs(k, g, d, F, "cuda") for k in ("fwd_tile", "gd_tile", "dual")}
    for o in outs.values():  # all sentinel, the accumulating output too
        for k in o:
            o[k] = K.sentinel(tuple(o[k].shape), "cuda")

    def call(kernel, edit, base=None):
        x = M.message_args(base or kernel, g, csr, F)
        out = outs["fwd_tile" if kernel.startswith("fwd") else ("dual" if kernel.startswith("dual") else "gd_tile")]
        x.out, x.out2, x.w, x.w2, x.src, x.src2 = (M._ptr(t) for t in (out["out"], out["out2"], d["w"], d["dw"], d["gMi"], d["Pn"]))
        x.slots, x.slot_stride = M._ptr(outs["gd_tile"]["slots"]), outs["gd_tile"]["slots"].shape[1]
        edit(x)
        route, ns = C.c_int32(-7), C.c_int32(-7)
        rc = hip_lib.tmdnet_debug_message(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(x), C.byref(route), C.byref(ns))
        return rc, route.value, ns.value

    def rejected(kernel, edit):
        rc, route, ns = call(kernel, edit)
        assert rc == _C.ERR_INVALID and route == -7 and ns == -7, (kernel, rc, route, ns)

    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip_lib.tmdnet_debug_message(s, None, None, None) == _C.ERR_INVALID
    every = ("fwd_row", "fwd_split", "fwd_tile", "adj_row", "adj_split", "gd_row", "gd_split", "gd_tile", "dual", "dual_acc")
    for kernel in every:
        rejected(kernel, lambda x: setattr(x, "N", 0))
        rejected(kernel, lambda x: setattr(x, "N", -5))
        rejected(kernel, lambda x: setattr(x, "F", 0))
        rejected(kernel, lambda x: setattr(x, "P", -1))
        for field in ("rowptr", "col", "epair", "esign", "counts", "w", "src", "out"):
            rejected(kernel, lambda x, f=field: setattr(x, f, None))
        rejected(kernel, lambda x: setattr(x, "op", (x.op + 1) % 4))  # a kernel of another sweep
    for kernel in ("fwd_tile", "gd_tile"):
        for bad in (48, 16, 33):
            rejected(kernel, lambda x, v=bad: setattr(x, "F", v))
    for kernel in ("fwd_split", "adj_split", "gd_split"):
        for bad in (32, 96, 192, 256):
            rejected(kernel, lambda x, v=bad: setattr(x, "F", v))
    for bad in (32, 96, 1088):
        rejected("gd_row", lambda x, v=bad: setattr(x, "F", v))
    for kernel in ("fwd_row", "fwd_split", "fwd_tile", "dual", "dual_acc"):
        rejected(kernel, lambda x: setattr(x, "out2", None))
    for kernel in ("gd_row", "gd_split", "gd_tile", "dual", "dual_acc"):
        rejected(kernel, lambda x: setattr(x, "w2", None))
        rejected(kernel, lambda x: setattr(x, "src2", None))
    for kernel in ("gd_row", "gd_split", "gd_tile"):
        rejected(kernel, lambda x: setattr(x, "slots", None))
        rejected(kernel, lambda x: setattr(x, "slot_stride", 2 * g["P"] - 1))
    for sel in (-1, 11, 12, 16, 17, 99):  # unknown selectors, and routes that are no selectable kernel
        for op in range(4):
            rejected("fwd_row", lambda x, v=sel, o=op: (setattr(x, "kernel", v), setattr(x, "op", o)))
    rejected("fwd_row", lambda x: setattr(x, "op", 4))
    torch.cuda.synchronize()
    assert all(bool((K.bits(t) == K.SENTINEL).all()) for o in outs.values() for t in o.values()), "a rejected call launched"
    # and the same arguments, within the contract, run
    rc, route, ns = call("fwd_tile", lambda x: (setattr(x, "src", M._ptr(d["src"])), setattr(x, "q", None), setattr(x, "batch", None)))
    torch.cuda.synchronize()
    assert (rc, route, ns) == (_C.OK, _C.MSG_FWD_TILE, 0)
    o = outs["fwd_tile"]
    assert torch.isfinite(o["out"][:g["N"]]).all() and torch.isfinite(o["out2"][:g["N"]]).all()
    assert bool((K.bits(o["out"][g["N"]:]) == K.SENTINEL).all()) and bool((K.bits(o["out2"][g["N"]:]) == K.SENTINEL).all())
