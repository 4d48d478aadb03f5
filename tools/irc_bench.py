#!/usr/bin/env python
"""A/B of the IRC follower: ms per step of

  (a) ``a_eager``: a host loop of the same kernels - one graph launch of ``capture()`` on the stacked paths per step and then
      ``tmdnet_irc_advance(MIDDLE)`` issued from the host, everything on the device and nothing read back;
  (b) ``b_K10``: ``capture_irc`` with K = 10 steps per graph launch,

for one saddle of 64 atoms and for 16 such saddles, both directions (2 and 32 paths), TensorNet F = 128, L = 2.  For context,
``md_K10``: ``capture_md`` (NVE, K = 10) on the same batch of 2 / 32 molecules in the same process - the MD loop is what the IRC step
adds its two launches to.  Alternating blocks of the legs in one process, each block at least ``--seconds`` of stepping with the final
synchronise inside the clock; median and min / max over ``--rounds`` blocks.  The random-weight potential has no saddle at hand: every
start point is a displaced copy of the molecule and the mode is the force there, so the forward path runs downhill and the backward one
has turned uphill at its start image and is finished at step 0 - its evaluation stays in the batch (the batch is fixed), only its
per-atom work is skipped, in both legs alike.  fmax is far below what is reached and the speed is small, so no forward path finishes.
Writes profiles/irc.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torchmd-net_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from min_bench import _block  # noqa: E402


def eager_irc(torch, model, irc, replay):
    """-> step(): one graph launch of the evaluation, then the three launches of tmdnet_irc_advance(MIDDLE) from the host, on the
    start state and the parameters of ``irc`` and on a workspace of its own"""
    from torchmdnet_amd import _C
    from torchmdnet_amd.minimize import MIN_CLOSE, MIN_MIDDLE, MIN_OPEN
    from torchmdnet_amd.models.utils import _ptr, _stream_ptr

    L, st, dev = _C.lib(), model._engine, replay.pos.device
    n, P = irc.n_atoms, irc.n_paths
    ws = torch.zeros_like(irc._ws)
    vel, forces = irc.vel.clone().view(-1, 3), torch.zeros_like(replay.pos)
    conv = torch.full((P,), -1, dtype=torch.int64, device=dev)

    def advance(phase, f, e):
        rc = L.tmdnet_irc_advance(st.handle, _stream_ptr(dev), _ptr(st.graph_ws), _ptr(ws), n, P, irc.capacity, irc.every, phase,
                                  _ptr(replay.pos), _ptr(vel), _ptr(f), _ptr(e), _ptr(irc._half_inv_mass), _ptr(irc.masses), _ptr(irc.fixed),
                                  None if phase == MIN_OPEN else _ptr(forces), irc.fmax_bound, irc.v0, irc.error, irc.dt_min, irc.dt_max,
                                  *([None] * 7), None if phase == MIN_OPEN else _ptr(conv), *([None] * 4))
        assert rc == _C.OK, rc

    assert L.tmdnet_irc_reset(_stream_ptr(dev), _ptr(ws), 0, irc.dt0) == _C.OK
    e, f = replay()
    advance(MIN_CLOSE, f, e)
    advance(MIN_OPEN, forces, None)

    def step():
        e, f = replay()
        advance(MIN_MIDDLE, f, e)

    def status():
        host = (C.c_uint64 * 3)()
        rc = L.tmdnet_irc_status(_stream_ptr(dev), _ptr(ws), C.cast(host, C.POINTER(C.c_uint64)))
        return rc, [int(w) for w in host]

    return step, conv, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irc.json"))
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    K, n = 10, 64
    prm = dict(dt=0.05, fmax=1e-9, v0=1e-4, error=1.5e-3, initial_step=0.01, dt_max=0.1, record=dict(every=10, capacity=64))
    result = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes", "steps_per_replay": K,
              "seconds_per_block": a.seconds, "rounds": a.rounds, "parameters": prm, "sizes": {}}
    torch.manual_seed(0)
    model = create_model(dict(W.C2_ARGS, static_shapes=True)).to(dev)
    z, pos, _ = W.synthetic_batch(n_mol=1, n_atoms=n)
    z, pos = z.to(dev), pos.to(dev).float().contiguous()
    masses = torch.full((n,), 12.0)
    for G in (1, 16):
        starts = []
        for g in range(G):  # every start point a copy of the molecule displaced smoothly by at most 0.1 per atom
            gen = torch.Generator().manual_seed(100 + g)
            k, ph = torch.rand(3, 3, generator=gen).to(dev), (6.28 * torch.rand(3, generator=gen)).to(dev)
            starts.append(pos + (0.1 / 3 ** 0.5) * torch.sin(pos @ k + ph))
        x0 = torch.stack(starts).contiguous()
        _, f0 = model.energy_and_forces(z.repeat(G), x0.reshape(-1, 3), torch.arange(G, device=dev).repeat_interleave(n), None, None, G,
                                        want_forces=True)
        mode = f0.detach().view(G, n, 3).clone()
        P = 2 * G
        batch = torch.arange(P, device=dev).repeat_interleave(n)
        rows = x0.repeat_interleave(2, 0).reshape(-1, 3).contiguous()
        replay = model.capture(z.repeat(P), rows, batch)
        md = model.capture_md(z.repeat(P), rows.clone(), torch.zeros(P * n, 3, device=dev), masses.repeat(P).to(dev), 1e-3, batch=batch,
                              steps_per_replay=K, force_scale=9.648533e-3)
        irc = model.capture_irc(z, x0, mode, masses, steps_per_replay=K, **prm)  # (last: its start state seeds the eager leg)
        replay.pos.copy_(irc.pos.reshape(-1, 3))
        eager, eager_conv, eager_status = eager_irc(torch, model, irc, replay)
        legs = {"a_eager": (eager, 1), "b_K10": (irc, K), "md_K10": (md, K)}
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        irc.check()  # raises if a path overflowed or was unusable: its timings would be of a frozen loop
        md.check()
        assert eager_status()[0] == 0, eager_status()
        entry = {k: {"ms_per_step": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        entry["n_saddles"], entry["n_paths"], entry["n_atoms"] = G, P, n
        entry["finished"] = {"eager": int((eager_conv >= 0).sum()), "capture_irc": int((irc.converged_at >= 0).sum())}
        entry["finished_at_step_0"] = int((irc.converged_at == 0).sum())
        entry["displacement_max"] = {"eager": float((replay.pos.view(G, 2, n, 3)[:, 0] - x0).abs().max()),
                                     "capture_irc": float((irc.pos[:, 0] - x0).abs().max())}
        entry["ratio_b_over_a"] = entry["b_K10"]["ms_per_step"] / entry["a_eager"]["ms_per_step"]
        entry["b_K10_not_slower_than_eager"] = entry["b_K10"]["ms_per_step"] <= entry["a_eager"]["ms_per_step"]
        entry["b_K10_minus_md_K10_us"] = 1e3 * (entry["b_K10"]["ms_per_step"] - entry["md_K10"]["ms_per_step"])
        result["sizes"][f"{G}x2x{n}"] = entry
        print(f"{G}x2x{n}", json.dumps(entry), flush=True)
        del replay, irc, md, legs, eager
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
