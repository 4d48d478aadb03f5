"""Bit-level digests of what the tile sweeps of csrc/tn_message_pair.hip write (k_message_rows8<8, 4>, k_message_adjoint_rows8,
k_message_adjoint_rows8_fold), for changes that must not move a bit: a refactor, a compiler flag, a new walk helper.

    python tools/message_tile_digest.py --out before.json                # on the MI355X, library of the tree
    python tools/message_tile_digest.py --out after.json [--lib OTHER.so]
    python tools/message_tile_digest.py --compare before.json after.json  # no device needed; exit status 1 on a difference

The launches are those of the unit tests, through the cases' own launch / fresh_outputs functions: every tile case of
tests/message_unit_cases.py (routes fwd_tile - three group-product modes, balance off and on - and gd_tile, which has no balance
switch) and every case of tests/message_fold_cases.py (three modes, the folded kernel and the sequence it replaces).  Their graphs
hold the smallest tiles at which each block-uniform branch of the kernels is taken (tests/test_message_oracle.py keeps that true).
One SHA-256 per output array and slot array, over the whole allocation: the sentinel rows behind row N and the slot arrays the
kernel does not own are part of it.  The digests depend on the compiler and are not a fixture: compare two builds of one toolchain.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "torchmd-net_amd"))


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def unit_digests(lib, device="cuda"):
    from tests import message_unit_cases as M

    doc = {}
    for case in M.all_cases():
        kernel, gname, F = case
        if kernel not in ("fwd_tile", "gd_tile"):
            continue
        g, d, csr, _, _ = M._device_case(gname, F, device)
        x = M.message_args(kernel, g, csr, F)
        modes = M.FWD_MODES if kernel == "fwd_tile" else (None,)
        balances = (0, 1) if kernel == "fwd_tile" else (-1,)
        for mode in modes:
            for bal in balances:
                out = M.fresh_outputs(kernel, g, d, F, device)
                rc, route, _ = M.launch(lib, kernel, x, d, out, mode, g, bal)
                assert rc == 0 and route == M.KERNELS[kernel][1], (case, rc, route)
                key = "unit/%s/%s/balance=%d" % (M.case_id(case), mode, bal)
                doc[key] = {k: _sha(v) for k, v in sorted(out.items())}
    return doc


def fold_digests(lib, device="cuda"):
    import torch

    from tests import message_fold_cases as M
    from tests.message_unit_cases import FWD_MODES

    doc = {}
    for case in M.all_cases():
        gname, F = case
        g = M.build_graph(gname)
        gd = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in g.items()}
        d = {k: v.to(device).contiguous() for k, v in M.make_inputs(gname, F).items()}
        csr = dict(rowptr=gd["rowptr"].int(), col=gd["col"].int(), epair=gd["epair"].int(), esign=gd["esign"].contiguous(),
                   counts=torch.tensor([g["P"], g["col"].numel(), 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=device))
        for mode in FWD_MODES:
            for folded in (True, False):
                out = M.fresh_outputs(g, F, device)
                assert M.launch(lib, gd, csr, d, F, mode, out, folded) == 0, (case, mode, folded)
                key = "fold/%s/%s/%s" % (M.case_id(case), mode, "folded" if folded else "sequence")
                doc[key] = {k: _sha(v) for k, v in sorted(out.items())}
    return doc


def compare(path_a, path_b):
    a, b = (json.load(open(p))["digests"] for p in (path_a, path_b))
    assert sorted(a) == sorted(b), "the two files hold different cases"
    total = equal = 0
    for key in sorted(a):
        assert sorted(a[key]) == sorted(b[key]), key
        for name in a[key]:
            total += 1
            if a[key][name] == b[key][name]:
                equal += 1
            else:
                print("DIFFERENT", key, name)
    print(json.dumps({"launches": len(a), "arrays_compared": total, "arrays_equal": equal}))
    return total == equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the digests of the library to this file")
    ap.add_argument("--lib", help="another build of libtmdnet_amd.so (default: the tree's)")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two digest files")
    a = ap.parse_args()
    if a.compare:
        sys.exit(0 if compare(*a.compare) else 1)
    assert a.out, "--out or --compare"
    import torch  # noqa: F401  before the library: both need the HIP runtime, and the process must hold one copy of it - torch's

    from torchmdnet_amd import _C

    if a.lib:
        _C.LIB_PATH = os.path.abspath(a.lib)
    lib = _C.lib()
    doc = {"library": os.path.basename(_C.LIB_PATH), "digests": {}}
    doc["digests"].update(unit_digests(lib))
    doc["digests"].update(fold_digests(lib))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", a.out, len(doc["digests"]), "launches")


if __name__ == "__main__":
    main()
