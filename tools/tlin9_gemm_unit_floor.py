"""Rounding floors, bounds and observed device errors of the kernel-level unit tests (tests/test_gpu_tlin9.py,
tests/test_gpu_gemm_epilogues.py) -> profiles/tlin9_gemm_unit_floor.json.

    python tools/tlin9_gemm_unit_floor.py            # no device needed: floors and bounds
    python tools/tlin9_gemm_unit_floor.py --gpu      # on the MI355X: adds the errors the kernels actually make

The floor of a check is the error of its own reference evaluated in float32 on the CPU against the same code in float64, on
the test's own fp32 inputs, shapes and seeds (tests/kernel_unit_cases.py), per atom / per row and normalised by that atom's /
row's maximum.  bound = max(2e-6, 4 x floor), never above 1e-5 (kernel_unit_cases.bound_of).  The bounds depend on the
reference alone; the observed errors are recorded beside them for the reader and are not used by any test.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "torchmd-net_amd"))

import torch  # noqa: E402

from tests import kernel_unit_cases as K  # noqa: E402
from tests import tlin9_oracle as O  # noqa: E402


def _entry(floor):
    return {"floor": floor, "bound": K.bound_of(floor), "observed_gpu": None}


def _merge_max(dst, key, val):
    dst[key] = val if key not in dst else max(dst[key], val)


def floors():
    out = {"tlin9": {}, "gemm": {}}
    for name in O.COMBOS:
        fl = {}
        for (N, F) in K.tlin9_shapes():
            for rk in sorted({v[0] for v in K.tlin9_variants(name)}):
                for k, e in K.tlin9_floor(name, N, F, rk).items():
                    _merge_max(fl, k, e)
        out["tlin9"][name] = {k: _entry(e) for k, e in fl.items()}
        print("tlin9", name, {k: f"{e:.2e}" for k, e in fl.items()}, flush=True)
    for route, cases in K.gemm_cases().items():
        out["gemm"][route] = {}
        for epi in K.EPILOGUES:
            fl = {}
            for (layout, M, N, Kk) in cases:
                for k, e in K.gemm_floor(layout, M, N, Kk, epi).items():
                    _merge_max(fl, k, e)
            out["gemm"][route][epi] = {k: _entry(e) for k, e in fl.items()}
        layout, M, N, Kk = cases[0]
        for epi in ("silu_pre", "muldsilu"):
            out["gemm"][route]["extreme_" + epi] = {k: _entry(e) for k, e in K.gemm_floor(layout, M, N, Kk, epi, extreme=True).items()}
        print("gemm", route, {e: {k: f"{v['floor']:.2e}" for k, v in d.items()} for e, d in out["gemm"][route].items()}, flush=True)
    return out


def observe(doc):
    """the errors of the kernels themselves, same cases as the tests"""
    from torchmdnet_amd import _C

    lib = _C.lib()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for name in O.COMBOS:
        ob = {}
        for (N, F) in K.tlin9_shapes(n_cu):
            for (rk, wf, alias) in K.tlin9_variants(name):
                for k, e in K.run_tlin9(lib, name, N, F, rk, wf, alias)["err"].items():
                    _merge_max(ob, k, e)
        for k, e in ob.items():
            doc["tlin9"][name][k]["observed_gpu"] = e
        print("tlin9", name, {k: f"{e:.2e}" for k, e in ob.items()}, flush=True)
    for route, cases in K.gemm_cases(n_cu).items():
        for i, (layout, M, N, Kk) in enumerate(cases):
            case = K.GemmCase(lib, layout, M, N, Kk, split=route.startswith("sb1") or layout == "g3u")
            for epi in K.EPILOGUES:
                r = case.run(epi)
                assert r["route"] == route, (route, layout, r["route"])
                for k, e in r["err"].items():
                    d = doc["gemm"][route][epi][k]
                    d["observed_gpu"] = e if d["observed_gpu"] is None else max(d["observed_gpu"], e)
            if i == 0:
                ext = K.GemmCase(lib, layout, M, N, Kk, split=route.startswith("sb1"), extreme=True)
                for epi in ("silu_pre", "muldsilu"):
                    for k, e in ext.run(epi)["err"].items():
                        doc["gemm"][route]["extreme_" + epi][k]["observed_gpu"] = e
        print("gemm", route, {e: {k: (None if v["observed_gpu"] is None else f"{v['observed_gpu']:.2e}") for k, v in d.items()}
                              for e, d in doc["gemm"][route].items()}, flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true", help="add the errors observed on the device to the existing file")
    ap.add_argument("--out", default=K.FLOOR_JSON)
    a = ap.parse_args()
    if a.gpu:
        doc = observe(K.load_bounds())
    else:
        doc = floors()
        doc["rule"] = "bound = max(2e-6, 4 x floor) <= 1e-5; floor = reference in float32 (CPU) against float64 on the tests' own inputs"
        if os.path.exists(K.FLOOR_JSON):  # keep what was measured on the device for the entries that still exist
            old = K.load_bounds()
            for fam in ("tlin9", "gemm"):
                for a1, d1 in doc[fam].items():
                    for a2, d2 in d1.items():
                        try:
                            if fam == "tlin9":
                                d2["observed_gpu"] = old[fam][a1][a2]["observed_gpu"]
                            else:
                                for a3, d3 in d2.items():
                                    d3["observed_gpu"] = old[fam][a1][a2][a3]["observed_gpu"]
                        except KeyError:
                            pass
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
