"""Rounding floors, bounds and observed device errors of the folded reverse tile sweep's unit test
(tests/test_gpu_message_fold.py) -> profiles/message_fold_floor.json.

    python tools/message_fold_floor.py            # no device needed: floors and bounds
    python tools/message_fold_floor.py --gpu      # on the MI355X: adds the errors the kernel actually makes

The floor of a check is the error of its own reference (tests/message_fold_cases.py: autograd through the group product of
tests/message_oracle.py, then the adjoint sweep and the distance-gradient halves) evaluated in float32 on the CPU against the same
code in float64, on the case's own graph, fp32 inputs and seed: gPn per atom, normalised by that atom's maximum; the halves per
slot array, normalised by the sum of the absolute values of each half's terms.  bound = max(2e-6, 4 x floor), never above 1e-5
(kernel_unit_cases.bound_of, which asserts the cap: a case whose reference alone needs more has to shrink its inputs).  The
bounds depend on the reference alone; the observed errors are recorded beside them for the reader and are not used by any test.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "torchmd-net_amd"))

from tests import kernel_unit_cases as K  # noqa: E402
from tests import message_fold_cases as M  # noqa: E402


def floors():
    doc = {"cases": {}}
    for case in M.all_cases():
        fl = M.floor_of(case)
        doc["cases"][M.case_id(case)] = {mode: {k: {"floor": e, "bound": K.bound_of(e), "observed_gpu": None} for k, e in f.items()}
                                         for mode, f in fl.items()}
        print(M.case_id(case), {mode: {k: f"{e:.2e}" for k, e in f.items()} for mode, f in fl.items()}, flush=True)
    return doc


def observe(doc):
    """the errors of the kernel itself, same cases as the test"""
    from torchmdnet_amd import _C

    lib = _C.lib()
    for case in M.all_cases():
        r = M.run_case(lib, case)
        assert r["finite"], (case, "an output row or a slot the kernel owns was not written, or is not finite")
        for mode, errs in r["err"].items():
            for k, e in errs.items():
                doc["cases"][M.case_id(case)][mode][k]["observed_gpu"] = e
            doc["cases"][M.case_id(case)][mode]["gPn"]["observed_gpu_vs_parent_sequence"] = r["vs_parent"][mode]
            doc["cases"][M.case_id(case)][mode]["gPn"]["bit_identical_to_parent_sequence"] = r["gPn_bit_identical"][mode]
        print(M.case_id(case), {mode: {k: f"{e:.2e}" for k, e in errs.items()} for mode, errs in r["err"].items()},
              {k: v for k, v in r.items() if isinstance(v, bool) and not v}, flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true", help="add the errors observed on the device to the existing file")
    ap.add_argument("--out", default=M.FLOOR_JSON)
    a = ap.parse_args()
    if a.gpu:
        doc = observe(M.load_bounds())
    else:
        doc = floors()
        doc["rule"] = "bound = max(2e-6, 4 x floor) <= 1e-5; floor = reference in float32 (CPU) against float64 on the test's own inputs"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
