"""Rounding floors, bounds and observed device errors of the TensorNet2 kernel unit tests (tests/test_gpu_tn2_unit.py)
-> profiles/tn2_unit_floor.json.

    python tools/tn2_unit_floor.py            # no device needed: floors and bounds
    python tools/tn2_unit_floor.py --gpu      # on the MI355X: adds the errors the kernels actually make

The floor of a check is the error of its own reference (tests/tn2_unit_oracle.py) evaluated in float32 on the CPU against the
same code in float64, on the case's own graph, fp32 inputs and seed (tests/tn2_unit_cases.py): per edge or atom row, per
molecule for the per-molecule kernels (equilibration, Coulomb head, pair gradient), each normalised by the largest magnitude of
the reference there; the cutoff-gradient slot arrays by the sum of the absolute values of each slot's terms.
bound = max(2e-6, 4 x floor), never above 1e-5 (kernel_unit_cases.bound_of); integer outputs and plain copies are exact
(floor 0, bound 0).  The bounds depend on the reference alone; the observed errors are recorded beside them for the reader and
are not used by any test.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "torchmd-net_amd"))

from tests import kernel_unit_cases as K  # noqa: E402
from tests import tn2_unit_cases as M  # noqa: E402


def floors():
    doc = {"cases": {}}
    for case in M.all_cases():
        fl = M.floor_of(case)
        doc["cases"][M.case_id(case)] = {k: {"floor": e, "bound": 0.0 if k in M.EXACT else K.bound_of(e), "observed_gpu": None}
                                         for k, e in fl.items()}
        print(M.case_id(case), {k: f"{e:.2e}" for k, e in fl.items()}, flush=True)
    return doc


def observe(doc):
    """the errors of the kernels themselves, same cases as the test"""
    from torchmdnet_amd import _C

    lib = _C.lib()
    for case in M.all_cases():
        r = M.run_case(lib, case)
        assert r["finite"], (case, "an output the kernel owns was not written, or is not finite")
        for k, e in r["err"].items():
            doc["cases"][M.case_id(case)][k]["observed_gpu"] = e
        print(M.case_id(case), {k: f"{e:.2e}" for k, e in r["err"].items()},
              {k: v for k, v in r.items() if k != "err" and not v}, flush=True)
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
        if os.path.exists(M.FLOOR_JSON):  # keep what was measured on the device for the entries that still exist
            old = M.load_bounds()["cases"]
            for cid, d in doc["cases"].items():
                for k, v in d.items():
                    v["observed_gpu"] = old.get(cid, {}).get(k, {}).get("observed_gpu")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
