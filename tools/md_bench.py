#!/usr/bin/env python
"""A/B of the MD loop: ms per step of

  (a) the loop a caller can build on ``capture()``: one graph launch per step, the integrator as eager torch ops on
      ``replay.pos`` between the launches - ``a_inplace`` is the leanest form (three in-place ops per step, no energies read),
      ``a_test_loop`` is ``_nve`` of tests/test_gpu_md.py as written (four ops, two clones, the total energy read every step);
  (b) ``capture_md``: K steps per graph launch, integrator, kinetic energy and energy logs inside the graph, K in {1, 10, 50},
      NVE and Langevin,

for one system of 64, 256 and 1 024 atoms, TensorNet F = 128, L = 2 (bench.py's md_latency model).  Alternating blocks of (a) and
(b) in one process, each block at least ``--seconds`` of stepping with the final synchronise inside the clock; median and
min / max over ``--rounds`` blocks.  dt is tiny (the random-weight potential is not a force field: the atoms must not travel);
ns/day is quoted at 1 fs per step, as bench.py does.  Writes profiles/md_loop.json."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torchmd-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _block(step_fn, steps_per_call, seconds, sync):
    """ms per step of one block: calls until `seconds` have passed, the synchronise inside the clock"""
    step_fn()
    sync()
    calls = 0
    t0 = time.perf_counter()
    while True:
        for _ in range(max(1, 200 // steps_per_call)):
            step_fn()
            calls += 1
        sync()  # the queue must not run ahead of the clock
        t = time.perf_counter() - t0
        if t >= seconds:
            return 1e3 * t / (calls * steps_per_call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "md_loop.json"))
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    dt, mass_amu, fs = 1e-3, 12.0, 9.648533e-3
    result = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes",
              "seconds_per_block": a.seconds, "rounds": a.rounds, "dt_for_ns_per_day_fs": 1.0, "sizes": {}}
    for n in a.sizes:
        torch.manual_seed(0)
        model = create_model(dict(W.C2_ARGS, static_shapes=True, max_num_neighbors=64 if n <= 64 else 128)).to(dev)
        z, pos, batch = W.synthetic_batch(n_mol=1, n_atoms=n)
        z, pos, batch = z.to(dev), pos.to(dev), batch.to(dev)
        vel0 = torch.zeros_like(pos)
        masses = torch.full((n,), mass_amu, device=dev)
        hk = 0.5 * dt * fs / mass_amu
        legs = {}

        replay = model.capture(z, pos, batch)
        vel = vel0.clone()
        _, forces = replay(pos)

        def a_inplace():
            vel.add_(forces, alpha=hk)
            replay.pos.add_(vel, alpha=dt)
            replay()
            vel.add_(forces, alpha=hk)

        legs["a_inplace"] = (a_inplace, 1)
        state = {"pos": pos.clone(), "vel": vel0.clone(), "f": forces.clone()}

        def a_test_loop():  # tests/test_gpu_md.py::_nve, one step
            s = state
            s["vel"] = s["vel"] + 0.5 * dt * fs * s["f"] / mass_amu
            s["pos"] = s["pos"] + dt * s["vel"]
            e, f = replay(s["pos"])
            s["f"] = f.clone()
            s["vel"] = s["vel"] + 0.5 * dt * fs * s["f"] / mass_amu
            s["tot"] = float(e.sum()) + 0.5 * mass_amu * float((s["vel"] * s["vel"]).sum())

        legs["a_test_loop"] = (a_test_loop, 1)
        mds = []
        for K in (1, 10, 50):
            for name, th in (("nve", None), ("langevin", dict(friction=0.01, kT=0.0259, seed=1))):
                md = model.capture_md(z, pos, vel0, masses, dt, batch=batch, steps_per_replay=K, force_scale=fs, thermostat=th)
                mds.append(md)
                legs[f"b_K{K}_{name}"] = (md, K)
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        for md in mds:
            md.check()  # raises if a trajectory overflowed: its timings would be of a frozen loop
        entry = {}
        for k, v in times.items():
            ms = statistics.median(v)
            entry[k] = {"ms_per_step": ms, "min": min(v), "max": max(v), "ns_per_day_at_1fs": 86400.0 / ms * 1e3 * 1e-6}
        base = entry["a_inplace"]["ms_per_step"]
        entry["ratio_b_over_a_inplace"] = {k: entry[k]["ms_per_step"] / base for k in entry if k.startswith("b_")}
        entry["ratio_b_over_a_test_loop"] = {k: entry[k]["ms_per_step"] / entry["a_test_loop"]["ms_per_step"] for k in entry
                                             if k.startswith("b_")}
        slower = [k for k in ("b_K10_nve", "b_K10_langevin") if entry[k]["ms_per_step"] > base]
        entry["b_K10_not_slower_than_a"] = not slower
        result["sizes"][str(n)] = entry
        print(n, json.dumps(entry), flush=True)
        del replay, mds, legs
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
