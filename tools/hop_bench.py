#!/usr/bin/env python
"""ms per step of minima hopping, captured against the same loop stepped from the host:

  ``hop_K10``    ``capture_minima_hopping`` with K = 10 steps per graph launch,
  ``hop_eager``  the same object stepped by ``step_eager`` - an evaluation and ``tmdnet_hop_advance`` issued from the host per step,
  ``min_K10``    ``capture_minimize`` (FIRE) and ``md_K10`` ``capture_md`` (NVE) at the same shape in the same run,

for 1 x 64 and 256 x 64 atoms, TensorNet F = 128, L = 2.  Alternating blocks in one process, each block at least ``--seconds`` of
stepping with the final synchronise inside the clock; median and min / max over ``--rounds`` blocks.  The random-weight potential is no
force field, so the steps are kept tiny and fmax is far below what is reached: every walker stays in the quench of its start geometry
(which has no step budget), so a hop step here is a FIRE step plus the reduce launch - the expectation this file records next to the
numbers.  Writes the ``bench`` block of profiles/hop.json and keeps what else the file holds."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torchmd-net_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from min_bench import _block  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hop.json"))
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.hop import QUENCH
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    K, n, fmax = 10, 64, 1e-9
    fire = dict(dt=1e-4, dt_max=1e-3, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, max_step=1e-4)
    bench = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes", "steps_per_replay": K,
             "seconds_per_block": a.seconds, "rounds": a.rounds, "fire": fire, "fmax": fmax, "sizes": {}}
    torch.manual_seed(0)
    model = create_model(dict(W.C2_ARGS, static_shapes=True)).to(dev)
    for B in (1, 256):
        z, pos, batch = (t.to(dev) for t in W.synthetic_batch(n_mol=B, n_atoms=n))
        pos = pos.float().contiguous()
        m = torch.full((B * n,), 12.0, device=dev)
        hop = model.capture_minima_hopping(z, pos, m, 1e-3, batch=batch, steps_per_replay=K, kT0=1e-4, ediff0=1e-4, fmax=fmax, fire=fire)
        opt = model.capture_minimize(z, pos, batch=batch, steps_per_replay=K, fmax=fmax, fire=fire)
        md = model.capture_md(z, pos, torch.zeros_like(pos), m, 1e-3, batch=batch, steps_per_replay=K, force_scale=9.648533e-3)
        legs = {"hop_K10": (hop, K), "hop_eager": (hop.step_eager, 1), "min_K10": (opt, K), "md_K10": (md, K)}
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        for loop in (hop, opt, md):
            loop.check()  # raises if a loop overflowed or was unusable: its timings would be of a frozen loop
        entry = {k: {"ms_per_step": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        entry["n_walkers"], entry["n_atoms"] = B, n
        entry["walkers_in_quench"] = int((hop.phase == QUENCH).sum())
        entry["hop_minus_min_ms"] = entry["hop_K10"]["ms_per_step"] - entry["min_K10"]["ms_per_step"]
        entry["captured_over_eager"] = entry["hop_K10"]["ms_per_step"] / entry["hop_eager"]["ms_per_step"]
        bench["sizes"][f"{B}x{n}"] = entry
        print(f"{B}x{n}", json.dumps(entry), flush=True)
        del hop, opt, md, legs
    result = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            result = json.load(fh)
    result["bench"] = bench
    result["bench_note"] = "measured by tools/hop_bench.py; every walker stays in QUENCH (see the tool's docstring)"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
