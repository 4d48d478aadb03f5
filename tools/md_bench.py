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
ns/day is quoted at 1 fs per step, as bench.py does.  Writes profiles/md_loop.json.

``--npt``: the constant-pressure loop instead, on the 192-atom water box and on the 1 024-atom system above inside a cubic box that
holds it with a cutoff of margin (same atoms, same pairs):

  (a) ``a_eager_npt``: the loop a caller builds on ``capture(virial=True)`` - one graph launch per step, Langevin integrator and an
      isotropic stochastic-cell-rescaling move as eager torch ops on the device, nothing read back;
  (b) ``b_K10_npt``: ``capture_md(thermostat=, barostat=)`` with K = 10, and ``b_K10_nvt``: the same without the barostat,

same alternating blocks, median and min / max.  The coupling is weak enough that the box stays where it is (the random-weight
potential is no force field).  Records the NPT / NVT ratio and NPT against the eager loop per size; writes profiles/md_npt.json."""
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


def _summary(times):
    out = {}
    for k, v in times.items():
        ms = statistics.median(v)
        out[k] = {"ms_per_step": ms, "min": min(v), "max": max(v), "ns_per_day_at_1fs": 86400.0 / ms * 1e3 * 1e-6}
    return out


def npt_main(a):
    import math

    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    dt, mass_amu, fs, kT, friction, K = 1e-3, 12.0, 9.648533e-3, 0.0259, 0.01, 10
    baro = dict(pressure=0.0, tau=1000.0 * dt, compressibility=1e-6, kT=kT, seed=2)
    result = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes", "steps_per_replay": K,
              "seconds_per_block": a.seconds, "rounds": a.rounds, "dt_for_ns_per_day_fs": 1.0, "barostat": baro, "sizes": {}}
    for name in ("water192", "synthetic1024"):
        torch.manual_seed(0)
        model = create_model(dict(W.C2_ARGS, static_shapes=True, max_num_neighbors=128)).to(dev)
        if name == "water192":
            z, pos, box = W.water_box(n_side=4)
        else:
            z, pos, _ = W.synthetic_batch(n_mol=1, n_atoms=1024)
            cut = float(W.C2_ARGS["cutoff_upper"])
            pos = pos - pos.min(0).values + cut
            box = torch.eye(3) * (float(pos.max()) + cut)
        z, pos, box = z.to(dev), pos.to(dev).float().contiguous(), box.to(dev).float().contiguous()
        n = int(z.shape[0])
        batch = torch.zeros_like(z)
        vel0 = torch.zeros_like(pos)
        masses = torch.full((n,), mass_amu, device=dev)
        th = dict(friction=friction, kT=kT, seed=1)
        hk = 0.5 * dt * fs / mass_amu
        c1 = math.exp(-friction * dt)
        c2s = math.sqrt(1.0 - c1 * c1) * math.sqrt(kT * fs / mass_amu)
        acoef = baro["compressibility"] * dt / baro["tau"]

        ebox = box.clone()
        replay = model.capture(z, pos, batch, ebox, virial=True)
        vel = vel0.clone()
        _, forces, virial = replay(pos)

        def a_eager_npt():
            vel.add_(forces, alpha=hk)
            replay.pos.add_(vel, alpha=dt)
            replay()
            vel.add_(forces, alpha=hk)
            vel.mul_(c1).add_(torch.randn_like(vel), alpha=c2s)
            ke = (vel * vel).sum() * (0.5 * mass_amu / fs)
            vol = torch.linalg.det(ebox).abs()
            p = (2.0 * ke + virial[0].diagonal().sum()) / (3.0 * vol)
            d = (p - baro["pressure"]) * acoef + torch.sqrt(2.0 * kT * acoef / vol) * torch.randn((), device=dev)
            mu = torch.exp(d / 3.0)
            ebox.mul_(mu)
            replay.pos.mul_(mu)
            vel.div_(mu)

        legs = {"a_eager_npt": (a_eager_npt, 1)}
        mds = []
        for leg, b in (("b_K10_nvt", None), ("b_K10_npt", baro)):
            md = model.capture_md(z, pos, vel0, masses, dt, batch=batch, box=box.clone(), steps_per_replay=K, force_scale=fs, thermostat=th,
                                  barostat=b)
            mds.append(md)
            legs[leg] = (md, K)
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        for md in mds:
            md.check()  # raises if a trajectory overflowed or a move was not finite: its timings would be of a frozen loop
        entry = _summary(times)
        entry["n_atoms"] = n
        entry["volume_ratio_end"] = {"eager": float(torch.linalg.det(ebox).abs() / torch.linalg.det(box).abs()),
                                     "capture_md": float(torch.linalg.det(mds[1].box).abs() / torch.linalg.det(box).abs())}
        entry["ratio_npt_over_nvt"] = entry["b_K10_npt"]["ms_per_step"] / entry["b_K10_nvt"]["ms_per_step"]
        entry["ratio_npt_over_eager_npt"] = entry["b_K10_npt"]["ms_per_step"] / entry["a_eager_npt"]["ms_per_step"]
        entry["b_K10_npt_not_slower_than_eager"] = entry["b_K10_npt"]["ms_per_step"] <= entry["a_eager_npt"]["ms_per_step"]
        result["sizes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del replay, mds, legs
    out = a.out if a.out else os.path.join(ROOT, "profiles", "md_npt.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--npt", action="store_true", help="time the constant-pressure loop instead (profiles/md_npt.json)")
    ap.add_argument("--out", default=None, help="default: profiles/md_loop.json, with --npt profiles/md_npt.json")
    a = ap.parse_args()
    if a.npt:
        return npt_main(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "md_loop.json")

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
