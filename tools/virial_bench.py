"""Cost of the virial: energy+force step time with and without want_virial on
  C2      256 molecules x 64 atoms, TensorNet F = 128 (BASELINE configs[1])
  water   the 10 125-atom periodic water box, TensorNet F = 128, cell list (bench.py's water leg)
  C4      256 x 64 atoms, Equivariant Transformer (BASELINE configs[3])

    python tools/virial_bench.py [--steps 40] [--repeats 5] [--warmup 10] [--out profiles/virial_cost.json]

Method: both variants are warmed up, then timed in alternating blocks (plain, virial, plain, ...) of `steps` eager calls, each block
between two device events; `repeats` blocks per variant.  Reported per variant: the median block's ms per step and the spread
(min .. max over the blocks); the overhead is the difference of the medians.  The expected extra traffic is 12 B per pair (pdelta)
plus 36 B per atom written and read again (the per-atom partials), against the step's own traffic: printed as `model_extra_us` at
an achievable 4 TB/s so that a measured overhead far above it stands out (the extra reduction launch costs a few microseconds by
itself whatever the size).  One JSON object goes to --out and to stdout."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "torchmd-net_amd")]

from torchmdnet_amd import workloads as W  # noqa: E402
from torchmdnet_amd.models.model import create_model  # noqa: E402


def block_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def measure(model, z, pos, batch, box, n_mol, steps, repeats, warmup):
    plain = lambda: model.energy_and_forces(z, pos, batch, box, None, n_mol)
    virial = lambda: model.energy_and_forces(z, pos, batch, box, None, n_mol, want_virial=True)
    for _ in range(warmup):
        plain()
        virial()
    torch.cuda.synchronize()
    t = {"plain": [], "virial": []}
    for _ in range(repeats):
        t["plain"].append(block_ms(plain, steps))
        t["virial"].append(block_ms(virial, steps))
    e0, f0 = plain()
    e1, f1, w = virial()
    assert torch.equal(e0, e1) and torch.equal(f0, f1) and torch.isfinite(w).all()
    n, pairs = int(z.shape[0]), int(model._engine.counts[0])
    out = {"atoms": n, "molecules": n_mol, "pairs": pairs}
    for k, v in t.items():
        out[k] = {"ms_per_step_median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    d = out["virial"]["ms_per_step_median"] - out["plain"]["ms_per_step_median"]
    out["overhead_us"] = round(1e3 * d, 2)
    out["overhead_pct"] = round(100 * d / out["plain"]["ms_per_step_median"], 3)
    out["extra_bytes_model"] = 12 * pairs + 2 * 36 * n
    out["model_extra_us"] = round(out["extra_bytes_model"] / 4e12 * 1e6, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default="C2,water,C4")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "virial_bench.py measures on the GPU only"
    res = {"device": torch.cuda.get_device_name(0), "steps_per_block": a.steps, "blocks_per_variant": a.repeats, "legs": {}}
    zb, pb, bb = (t.cuda() for t in W.synthetic_batch(n_mol=256, n_atoms=64))
    for leg in a.legs.split(","):
        torch.manual_seed(0)
        if leg == "C2":
            model = create_model(dict(W.C2_ARGS)).cuda()
            r = measure(model, zb, pb, bb, None, 256, a.steps, a.repeats, a.warmup)
        elif leg == "C4":
            model = create_model(dict(W.C4_ARGS)).cuda()
            r = measure(model, zb, pb, bb, None, 256, a.steps, a.repeats, a.warmup)
        elif leg == "water":
            model = create_model(dict(W.C2_ARGS, max_num_neighbors=96)).cuda()
            z, pos, box = (t.cuda() for t in W.water_box(n_side=15))
            r = measure(model, z, pos, torch.zeros_like(z), box, 1, a.steps, a.repeats, a.warmup)
        else:
            raise SystemExit(f"unknown leg {leg}")
        res["legs"][leg] = r
        print(json.dumps({leg: r}), flush=True)
        del model
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
