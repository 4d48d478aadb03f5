"""Rounding floors, bounds and observed device errors of the ET edge-sweep unit tests (tests/test_gpu_et_unit.py)
-> profiles/et_unit_floor.json.

    python tools/et_unit_floor.py            # no device needed: floors and bounds
    python tools/et_unit_floor.py --gpu      # on the MI355X: adds the errors the kernels actually make

The floor of a check is the error of its own reference (tests/et_unit_oracle.py) evaluated in float32 on the CPU against the same
code in float64, on the case's own graph, inputs and seed (tests/et_unit_cases.py): node outputs per atom, each block (xagg, a
component of vagg, one of the five blocks of g_qkv, g_vec) normalised by that atom's maximum; the slot arrays of gd2 and gr2 each
on its own, every slot normalised by the sum of the absolute values of its terms.  bound = max(2e-6, 4 x floor), never above 1e-5
(kernel_unit_cases.bound_of); the factor covers the sweeps' other summation orders (rotated and slot-order walks, DPP head sums,
two channels per lane) and fused against separate multiply-adds.  The bounds depend on the reference alone; the observed errors
are recorded beside them for the reader and are not used by any test.

The hardware sigmoid of the tile kernels (v_exp_f32 and v_rcp_f32, each documented to 1 ulp, in place of expf and an IEEE divide)
gets NO term of its own here: sigma = rcp(1 + exp2(-a log2 e)) carries at most (|a| log2 e + 3) ulp of relative error, which for
the ordinary cases (|a| <= 4, asserted in tests/test_et_unit_oracle.py) is below 9 ulp = 5.4e-7 on ONE edge's weight, inside the
factor 4 over floors of 3e-7 .. 6e-7 of sums over dozens of edges; the errors observed on the device (recorded beside the
bounds) confirm that none is needed.  In the extremes cases the weights of |a| >= 30 are exactly 0 or 1 in float32 either way.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "torchmd-net_amd"))

from tests import et_unit_cases as U  # noqa: E402
from tests import kernel_unit_cases as K  # noqa: E402


def _entry(fl):
    fl = {k: U.floor_kept(e) for k, e in fl.items()}  # (what the file keeps, and what the bound is taken from)
    return {k: {"floor": e, "bound": K.bound_of(e), "observed_gpu": None} for k, e in fl.items()}


def floors():
    doc = {"cases": {}}
    memo = {}  # the statement of a case does not depend on the kernel that runs it, but the slot groups do
    for c in U.all_cases():
        key = (U.slot_group(c), c.graph, c.F, c.hd, c.combo, c.bf16, c.variant == "extreme")
        if key not in memo:
            memo[key] = U.floor_of(c)
        doc["cases"][U.case_id(c)] = _entry(memo[key])
        print(U.case_id(c), {k: f"{e:.2e}" for k, e in memo[key].items()}, flush=True)
    for gname in U.OTHER_GRAPHS:
        for F in U.OTHER_F:
            fl = {f"{op}.{k}": e for op, d in U.other_floor(gname, F).items() for k, e in d.items()}
            doc["cases"][U.other_id(gname, F)] = _entry(fl)
            print(U.other_id(gname, F), {k: f"{e:.2e}" for k, e in fl.items()}, flush=True)
    for fc in U.FILTER_CASES:
        doc["cases"][U.filter_id(fc)] = _entry(U.filter_floor(fc))
        print(U.filter_id(fc), flush=True)
    return doc


def observe(doc):
    """the errors of the kernels themselves, same cases as the test"""
    from torchmdnet_amd import _C

    lib = _C.lib()
    for c in U.all_cases():
        r = U.run_case(lib, c)
        for k, e in r["err"].items():
            doc["cases"][U.case_id(c)][k]["observed_gpu"] = e
        print(U.case_id(c), {k: f"{e:.2e}" for k, e in r["err"].items()}, {k: v for k, v in r.items() if k != "err" and not v}, flush=True)
    for gname in U.OTHER_GRAPHS:
        for F in U.OTHER_F:
            r = U.run_other(lib, gname, F)
            for op, d in r["err"].items():
                for k, e in d.items():
                    doc["cases"][U.other_id(gname, F)][f"{op}.{k}"]["observed_gpu"] = e
            print(U.other_id(gname, F), r["err"], flush=True)
    for fc in U.FILTER_CASES:
        r = U.run_filter(lib, fc)
        for k, e in r["err"].items():
            doc["cases"][U.filter_id(fc)][k]["observed_gpu"] = e
        print(U.filter_id(fc), r["err"], flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true", help="add the errors observed on the device to the existing file")
    ap.add_argument("--out", default=U.FLOOR_JSON)
    a = ap.parse_args()
    if a.gpu:
        doc = observe(U.load_bounds())
    else:
        doc = floors()
        doc["rule"] = ("bound = max(2e-6, 4 x floor) <= 1e-5 (kernel_unit_cases.bound_of); floor = reference in float32 (CPU) against "
                       "float64 on the test's own inputs, rounded up; floor and observed_gpu in `unit`, in the order of `outputs` or `names`")
        if os.path.exists(U.FLOOR_JSON):  # keep what was measured on the device for the entries that still exist
            old = U.load_bounds()["cases"]
            for cid, d in doc["cases"].items():
                for k, v in d.items():
                    v["observed_gpu"] = old.get(cid, {}).get(k, {}).get("observed_gpu")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    U.save_bounds(doc, a.out)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
