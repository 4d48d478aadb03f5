#!/usr/bin/env python
"""What the ZBL / D2 pair pass (csrc/tn_prior.hip) costs: ms per energy+force step, timed with device events around blocks of
steps (the final event inside the clock), median and min / max over ``--rounds`` blocks after one that warms up, alternating
the legs in one process:

  c2      the step of BASELINE configs[1] - TensorNet F = 128, L = 2 on 256 molecules of 64 atoms - without priors and with
          [ZBL(cutoff 5 A), D2(cutoff 10 A)], and the pass alone (``tmdnet_pair_priors_add`` on the same inputs)
  water   the 10 125-atom periodic water box (one molecule: the brute-force pass pairs every atom with every other) without
          priors and with ZBL(cutoff 5 A), and the pass alone

Every leg is an eager ``TorchMD_Net.energy_and_forces`` call (dynamic shapes: the neighbour count is read back each step, as in
bench.py's throughput leg).  ``--parent-root DIR``: also time the prior-free legs with the package of another checkout (the
parent commit, built), in a child process.  Writes profiles/priors.json; ``--accuracy FILE`` adds the worst |got - oracle| / S
lines of a tests/test_gpu_priors.py log.  No threshold is asserted."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, EV = 1e-10, 1.602176634e-19


def timed(fn, steps, rounds):
    import torch

    fn()
    torch.cuda.synchronize()
    out = []
    for r in range(rounds + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(steps):
            fn()
        t1.record()
        t1.synchronize()
        if r:
            out.append(t0.elapsed_time(t1) / steps)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def legs(root, with_priors, steps, rounds):
    sys.path.insert(0, os.path.join(root, "torchmd-net_amd"))
    import ctypes as C

    import torch
    from torchmdnet_amd import _C, workloads as W
    from torchmdnet_amd.models.model import create_model
    from torchmdnet_amd.models.utils import _ptr, _stream_ptr

    an = [1] + list(range(1, W.C2_ARGS["max_z"]))
    pa = lambda cutoff: dict(cutoff_distance=cutoff, max_num_neighbors=128, atomic_number=an, distance_scale=A, energy_scale=EV)
    res = {}
    z, pos, batch = (t.cuda() for t in W.synthetic_batch(n_mol=256, n_atoms=64))
    wz, wpos, wbox = (t.cuda() for t in W.water_box(n_side=15))
    systems = {"c2": (z, pos, batch, None, 256, (["ZBL", "D2"], [pa(5.0), pa(10.0)])),
               "water": (wz, wpos.float(), torch.zeros_like(wz), wbox.float(), 1, ("ZBL", [pa(5.0)]))}
    for name, (z, pos, batch, box, n_mol, (pm, pargs)) in systems.items():
        torch.manual_seed(0)
        plain = create_model(dict(W.C2_ARGS)).to("cuda")
        run = {"prior_free": lambda m=plain: m.energy_and_forces(z, pos, batch, box, None, n_mol)}
        if with_priors:
            torch.manual_seed(0)
            model = create_model(dict(W.C2_ARGS, prior_model=pm, prior_args=pargs)).to("cuda")
            run["with_priors"] = lambda m=model: m.energy_and_forces(z, pos, batch, box, None, n_mol)
            E, F = model.energy_and_forces(z, pos, batch, box, None, n_mol)
            st, L, n = model._engine, _C.lib(), int(z.shape[0])
            nb = C.c_size_t(0)
            L.tmdnet_pair_priors_workspace_bytes(st.handle, n, n_mol, C.byref(nb))
            ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")
            mode = 0 if box is None else 1
            run["pass_alone"] = lambda: L.tmdnet_pair_priors_add(st.handle, _stream_ptr(pos.device), _ptr(ws), ws.numel(), n, n_mol, _ptr(pos),
                                                                 _ptr(z), _ptr(batch), _ptr(box), mode, None, _ptr(E), _ptr(F), None)
        res[name] = {"n_atoms": int(z.shape[0]), "n_mol": n_mol}
        for _ in range(2):  # alternate the legs: the second pass is the record
            for leg, fn in run.items():
                res[name][leg] = timed(fn, steps, rounds)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--child", action="store_true", help="internal: print the prior-free legs of --root as JSON")
    ap.add_argument("--root", default=ROOT, help="internal: the checkout whose package the child imports")
    ap.add_argument("--accuracy", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "priors.json"))
    a = ap.parse_args()
    if a.child:
        print("__JSON__" + json.dumps(legs(a.root, False, a.steps, a.rounds)))
        return
    import torch

    out = {"device": torch.cuda.get_device_name(0), "model": "TensorNet F=128 L=2 (BASELINE configs[1])", "steps_per_block": a.steps,
           "rounds": a.rounds, "timing": legs(ROOT, True, a.steps, a.rounds),
           "launches_of_the_pass": ["k_prior_ranges", "k_prior_pairs", "k_prior_mol_sum"], "synchronisations_of_the_pass": 0}
    if a.parent_root:  # a fresh child process: it imports the other checkout's package and library
        txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--root", os.path.abspath(a.parent_root), "--steps",
                              str(a.steps), "--rounds", str(a.rounds)], capture_output=True, text=True, timeout=600).stdout
        out["parent_commit"] = json.loads(txt.split("__JSON__")[1])
    for name, t in out["timing"].items():
        t["pass_share_of_step"] = t["pass_alone"]["median_ms"] / t["with_priors"]["median_ms"]
        t["with_over_prior_free"] = t["with_priors"]["median_ms"] / t["prior_free"]["median_ms"]
        if "parent_commit" in out:
            t["prior_free_over_parent"] = t["prior_free"]["median_ms"] / out["parent_commit"][name]["prior_free"]["median_ms"]
    if a.accuracy and os.path.exists(a.accuracy):
        rows = re.findall(r"\[priors\] (\w+): worst ratio ([0-9.e+-]+)", open(a.accuracy).read())
        out["accuracy"] = {"bound": 1e-5, "measure": "max |got - fp64 oracle| / S over e_i, E, F, W; S = sum of absolute pair terms",
                           "worst_ratio_per_case": {k: float(v) for k, v in rows}, "worst_ratio": max(float(v) for _, v in rows)}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out["timing"], indent=1))


if __name__ == "__main__":
    main()
