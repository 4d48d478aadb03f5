#!/usr/bin/env python
"""Writes profiles/et_bf16_oracle_floor.json: effect and noise floor of the rounding-aware ET oracle on the tile-sweep cases
(oracle/et_bf16_floor.py; CPU, fp64, about 15 s) and the bound tests/test_gpu_et.py takes from them.

    python tools/et_bf16_oracle_floor.py [--bound 3.5e-4]

The bound is a choice between 4 x the largest floor and half the smallest effect; the tool refuses one outside."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torchmd-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import et_bf16_floor as B  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bound", type=float, default=None, help="default: the geometric mean of the two limits")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "et_bf16_oracle_floor.json"))
    a = ap.parse_args()
    cases = {}
    for case in B.TILE_CASES:
        cases[B.case_name(case)] = r = B.measure(case)
        print(f"{B.case_name(case):32s} effect {r['effect']:.3e}  floor {r['floor']:.3e}", flush=True)
    lo = 4 * max(r["floor"] for r in cases.values())
    hi = 0.5 * min(r["effect"] for r in cases.values())
    bound = a.bound if a.bound is not None else float(f"{(lo * hi) ** 0.5:.1e}")  # two digits
    print(f"4 x floor = {lo:.3e} <= bound = {bound:.3e} <= effect / 2 = {hi:.3e}")
    if not lo <= bound <= hi:
        sys.exit("no bound separates the floor from the effect")
    rec = {"what": "relative max-norm force differences of oracle/et_torch.py in fp64, two molecules per case: effect = rounded vs "
                   "unrounded rows, floor = rounded vs rounded after a +-2^-22 perturbation of the rows before rounding; "
                   "bound = BF16_ORACLE_REL of tests/test_gpu_et.py",
           "perturbation": B.PERTURB, "bound": bound, "four_times_largest_floor": lo, "half_smallest_effect": hi, "cases": cases}
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
