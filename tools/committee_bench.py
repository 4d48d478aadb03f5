#!/usr/bin/env python
"""What a committee of M = 4 TensorNet members costs inside the captured MD loop: ms per MD step, timed with device events around
blocks of replays (the final event inside the clock), median and min / max over ``--rounds`` blocks after one that warms up,
alternating the legs in one process:

  c2      BASELINE configs[1] - TensorNet F = 128, L = 2 on 256 molecules of 64 atoms
  mol64   the single 64-atom molecule

  committee_step   ``Ensemble.capture_md`` (K steps per graph, gate armed but never firing): M evaluations, the pass, CLOSE, the latch, OPEN
  members_sum      the members' own ``TorchMD_Net.capture_md`` loops (the code path of the parent commit: one MIDDLE launch between two
                   evaluations), each timed alone in this run, summed
  pass_alone       ``tmdnet_committee_reduce`` on the four members' outputs: its two launches, 20 passes captured back to back in
                   one graph (pass_alone_eager: one call at a time from the host, which is bound by the host's launch rate)

Writes profiles/committee.json.  No threshold is asserted."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torchmd-net_amd"))


def timed(fn, calls, rounds, per_call=1):
    import torch

    fn()
    torch.cuda.synchronize()
    out = []
    for r in range(rounds + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        if r:
            out.append(t0.elapsed_time(t1) / (calls * per_call))
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--steps-per-replay", type=int, default=10)
    ap.add_argument("--replays", type=int, default=10, help="replays per timed block")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "committee.json"))
    a = ap.parse_args()
    import torch
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.committee import CommitteePass
    from torchmdnet_amd.models.model import Ensemble, create_model

    M, K = a.members, a.steps_per_replay
    members = []
    for s in range(M):
        torch.manual_seed(s)
        members.append(create_model(dict(W.C2_ARGS, static_shapes=True)).to("cuda"))
    systems = {"c2": W.synthetic_batch(n_mol=256, n_atoms=64), "mol64": W.synthetic_batch(n_mol=1, n_atoms=64)}
    out = {"device": torch.cuda.get_device_name(0), "model": f"{M} x TensorNet F=128 L=2 (BASELINE configs[1]), static shapes",
           "steps_per_replay": K, "replays_per_block": a.replays, "rounds": a.rounds, "timing": {},
           "launches_of_the_pass": ["k_committee_atoms", "k_committee_mols"],
           "launches_added_per_step": ["k_committee_atoms", "k_committee_mols", "k_committee_latch",
                                       "k_md_atoms<OPEN> (MIDDLE split into CLOSE and OPEN)"]}
    for name, (z, pos, batch) in systems.items():
        z, pos, batch = z.cuda(), pos.cuda(), batch.cuda()
        n, B = int(z.shape[0]), int(batch.max()) + 1
        vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
        mass = torch.where(z == 1, 1.008, 12.0).float()
        kw = dict(batch=batch, steps_per_replay=K, warmup=2)
        run = {}
        loop = Ensemble(members).capture_md(z, pos, vel, mass, 0.001, gate=dict(flag_above=1e30, stop_above=1e30), **kw)
        run["committee_step"] = (loop, K)
        for k, m in enumerate(members):
            run[f"member_{k}_step"] = (m.capture_md(z, pos, vel, mass, 0.001, **kw), K)
        outs = [m.energy_and_forces(z, pos, batch, None, None, B) for m in members]
        red = CommitteePass(M, n, B, pos.device)
        run["pass_alone_eager"] = (lambda: red(outs, batch), 1)  # (bounded by the host's launch rate)
        red(outs, batch)
        torch.cuda.synchronize()
        graph, kept = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(graph):  # 20 passes back to back in one graph: what the pass costs as nodes of a captured step
            kept.extend(red(outs, batch) for _ in range(20))
        run["pass_alone"] = (graph.replay, 20)
        t = out["timing"][name] = {"n_atoms": n, "n_mol": B}
        for _ in range(2):  # alternate the legs: the second pass is the record
            for leg, (fn, per) in run.items():
                t[leg] = timed(fn, a.replays, a.rounds, per)
        assert loop.check() > 0 and loop.stopped is None
        t["members_sum"] = {"median_ms": sum(t[f"member_{k}_step"]["median_ms"] for k in range(M))}
        t["committee_minus_members_ms"] = t["committee_step"]["median_ms"] - t["members_sum"]["median_ms"]
        t["committee_over_members"] = t["committee_step"]["median_ms"] / t["members_sum"]["median_ms"]
        t["pass_bytes"] = {"in": 12 * M * n + 4 * M * B, "out": 28 * n + 20 * B}
        del loop, run
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out["timing"], indent=1))


if __name__ == "__main__":
    main()
