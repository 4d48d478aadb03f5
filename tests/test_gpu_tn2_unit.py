"""The kernels only the TensorNet2 + ScalarPlusWeightedCoulomb path has (csrc/tn_tn2.hip) in isolation, through tmdnet_debug_tn2
and their own launchers, on hand-built inputs, against the float64 statements of tests/tn2_unit_oracle.py (pinned to
oracle/tn2_torch.py and to autograd in tests/test_tn2_unit_oracle.py, which also holds the branch census of the case list).

One parametrised test per op over tests/tn2_unit_cases.py: k_edge_reverse, k_tn2_edge_pre1, k_tn2_edge_gw, k_tn2_edge_reduce and
k_tn2_pair_gd on two hand-built graphs (rows of 1, 2, 3, 4, 5, 8 and 9 entries; two molecules and an atom without a neighbour;
atom and pair counts that leave a partial last block) at F = 32, 96, 128 and 320; k_cp_feat and its adjoint at F = 32 and 96;
k_qeq<false> and k_qeq<true> for q_dim 1, 3, 8, 24 and 64 on molecules of one atom fewer than, exactly as many as and one more than
256 / q_dim atoms and of one atom, with and without total charges, with permuted atoms (counts[3] = 1) and with all f ~ 1e-4;
k_coulomb<1..8> on molecules of 1, 2, 63, 64, 65 and 130 atoms plus one atom outside every molecule, for 1, 8, 9, 24 and 64 charge
channels, all-to-all and as reaction field without a box, in one triclinic box and in a box per molecule, sorted and permuted,
with forces and energy only.

Per case: integer outputs and plain copies exact; every float output against float64, normalised per row (edge or atom) or per
molecule by the largest magnitude of the reference there, or, where an output is a difference of terms that may cancel (the
cutoff-gradient slots, the equilibrated charges and their adjoint), by the sum of the absolute values of the terms; TAIL
sentinel rows behind the last row, the slots behind entry E, the slot array beyond the kernel's count, the pairs from counts[0]
on and the self pair's row of gAp bit-unchanged; accumulating outputs start from random contents; with the pair-overflow flag set
the edge kernels write nothing; two launches bit-identical (deterministic: no atomics).

Bounds: profiles/tn2_unit_floor.json, max(2e-6, 4 x the float32 rounding floor of the reference itself on the case's inputs),
never above 1e-5 (tools/tn2_unit_floor.py; the errors observed on the MI355X are recorded beside them)."""
import ctypes as C
import math

import pytest
import torch

from tests import kernel_unit_cases as K
from tests import tn2_unit_cases as M

pytestmark = pytest.mark.gpu

CASES = M.all_cases()


@pytest.fixture(scope="module")
def bounds():
    return M.load_bounds()["cases"]


def _check(hip_lib, bounds, case):
    r = M.run_case(hip_lib, case)
    ent = bounds[M.case_id(case)]
    print(M.case_id(case), {k: f"{e:.3g}" for k, e in r["err"].items()}, {k: ent[k]["bound"] for k in r["err"]})
    assert set(r["err"]) == set(M.OUTPUTS[case[0]])
    assert r["finite"], (case, "an output the kernel owns was left at the NaN sentinel, or is not finite")
    for k, e in r["err"].items():
        if k in M.EXACT:
            assert e == 0, (case, k, "not exact")
            continue
        b = ent[k]["bound"]
        assert b == K.bound_of(ent[k]["floor"]) and 2e-6 <= b <= 1e-5
        assert math.isfinite(e) and e < b, (case, k, e, b)
    assert r["slot_arrays_ok"], (case, "number of slot arrays")
    assert r["tail_ok"], (case, "a row, slot or pair the kernel does not own was written")
    assert r["deterministic"], (case, "two launches differ")
    assert r["overflow_ok"], (case, "written although the pair-overflow flag is set")
    assert r["energy_only_ok"], (case, "the energy-only launch differs, or wrote a gradient buffer")


def _of(*ops):
    cs = [c for c in CASES if c[0] in ops]
    return pytest.mark.parametrize("case", cs, ids=[M.case_id(c) for c in cs])


@_of("edge_reverse")
def test_edge_reverse_exact(hip_lib, bounds, case):
    _check(hip_lib, bounds, case)


@_of("cp_feat", "cp_feat_bwd")
def test_cp_feat_and_adjoint_vs_fp64(hip_lib, bounds, case):
    _check(hip_lib, bounds, case)


@_of("qeq_fwd")
def test_qeq_fwd_vs_fp64(hip_lib, bounds, case):
    _check(hip_lib, bounds, case)


@_of("qeq_bwd")
def test_qeq_bwd_vs_fp64(hip_lib, bounds, case):
    _check(hip_lib, bounds, case)


@_of("edge_pre1")
def test_edge_pre1_vs_fp64(hip_lib, bounds, case):
    _check(hip_lib, bounds, case)


@_of("edge_gw")
def test_edge_gw_vs_fp64(hip_lib, bounds, case):
    _check(hip_lib, bounds, case)


@_of("edge_reduce")
def test_edge_reduce_vs_fp64(hip_lib, bounds, case):
    _check(hip_lib, bounds, case)


@_of("pair_gd")
def test_pair_gd_vs_fp64(hip_lib, bounds, case):
    _check(hip_lib, bounds, case)


@_of("coulomb")
def test_coulomb_vs_fp64(hip_lib, bounds, case):
    _check(hip_lib, bounds, case)


def test_tn2_unit_rejects_what_is_outside_the_contract(hip_lib):
    """TMDNET_ERR_INVALID and no launch: N < 1, F < 1 (F > 1024 for EDGE_GW), qd < 1, QC > 64, a NULL operand the op reads or
    writes, slot arrays shorter than E, an unknown op; the out-field stays untouched."""
    from torchmdnet_amd import _C

    dev = "cuda"
    outs = []

    def setup(case):
        d = M.make_inputs(case)
        g = M.graph_of(case, d)
        out = {k: (K.sentinel(tuple(v.shape), dev) if v.dtype == torch.float32 else M._isent(tuple(v.shape), dev))
               for k, v in M.fresh_outputs(case, g, d, dev).items()}
        outs.append(out)
        return g, d, out, M.device_copies(case, g, d, dev)

    def rejected(case, ctx, edit):
        g, d, out, devc = ctx
        x = M.unit_args(case, g, d, out, devc)
        edit(x)
        ns = C.c_int32(-7)
        x.slot_arrays_out = C.pointer(ns)
        rc = hip_lib.tmdnet_debug_tn2(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(x))
        assert rc == _C.ERR_INVALID and ns.value == -7, (case, rc, ns.value)

    assert hip_lib.tmdnet_debug_tn2(None, None) == _C.ERR_INVALID
    needs = {"edge_reverse": ("rowptr", "col", "epair", "counts", "erev", "eid", "pair_edge"), "cp_feat": ("X", "feat"),
             "cp_feat_bwd": ("X", "g_feat", "G"), "qeq_fwd": ("counts", "mstart", "mend", "batch", "out", "charges", "FuQ"),
             "qeq_bwd": ("counts", "mstart", "mend", "batch", "out", "FuQ", "g_c", "g_out"),
             "edge_pre1": ("rowptr", "col", "epair", "counts", "Ap", "Bt", "Cs", "C", "pre1", "he1", "Ce"),
             "edge_gw": ("rowptr", "col", "epair", "counts", "gMi", "Pn", "pre3", "Ce", "g_pre3", "slots"),
             "edge_reduce": ("rowptr", "col", "epair", "counts", "g_pre1", "erev", "gB", "gCs", "gAp"),
             "pair_gd": ("counts", "gAp", "dAp", "slots", "pair_edge", "erev", "dC", "gd"),
             "coulomb": ("counts", "mstart", "mend", "pos", "charges", "wq", "ec", "fpos")}
    pick = {"edge_reverse": ("edge_reverse", "two_mols", 0), "cp_feat": ("cp_feat", "rows", 32), "cp_feat_bwd": ("cp_feat_bwd", "rows", 32),
            "qeq_fwd": ("qeq_fwd", "q", 24), "qeq_bwd": ("qeq_bwd", "q", 24), "coulomb": ("coulomb", "rf_box-sorted", 9)}
    pick.update({op: (op, "two_mols", 96) for op in M.EDGE_OPS})
    for op, case in pick.items():
        ctx = setup(case)
        rejected(case, ctx, lambda x: setattr(x, "N", 0))
        rejected(case, ctx, lambda x: setattr(x, "N", -3))
        for field in needs[op]:
            rejected(case, ctx, lambda x, f=field: setattr(x, f, None))
        if M.x_has_channels(op):
            rejected(case, ctx, lambda x: setattr(x, "F", 0))
        if op in ("qeq_fwd", "qeq_bwd"):
            rejected(case, ctx, lambda x: setattr(x, "qd", 0))
            rejected(case, ctx, lambda x: setattr(x, "B", 0))
        if op == "edge_gw":
            rejected(case, ctx, lambda x: setattr(x, "F", 1025))
        if op in ("edge_gw", "pair_gd"):
            rejected(case, ctx, lambda x: setattr(x, "slot_stride", x.E - 1))
        if op == "coulomb":
            rejected(case, ctx, lambda x: setattr(x, "QC", 65))
            rejected(case, ctx, lambda x: setattr(x, "QC", 0))
            rejected(case, ctx, lambda x: setattr(x, "box", None))
            rejected(case, ctx, lambda x: setattr(x, "box_mode", 3))
        rejected(case, ctx, lambda x: setattr(x, "op", 10))
        rejected(case, ctx, lambda x: setattr(x, "op", -1))
    torch.cuda.synchronize()
    assert all(bool((K.bits(t) == K.SENTINEL).all()) for o in outs for t in o.values()), "a rejected call launched"
    # and within the contract the same arguments run, and report the launcher's own number of slot arrays
    case = pick["edge_gw"]
    g, d, out, devc = setup(case)
    rc, ns = M.call(hip_lib, M.unit_args(case, g, d, out, devc))
    assert (rc, ns) == (_C.OK, 2) and torch.isfinite(out["g_pre3"][:g["E"]]).all()
