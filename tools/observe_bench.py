#!/usr/bin/env python
"""What the MD loop's observer costs: ms per step of

  (a) ``observed``: ``capture_md_observed`` with K = 10, S = 10 and rdf + msd + vacf (one sample per replay);
  (b) ``plain``: ``capture_md`` at K = 10 - the yardstick, the loop as it is without an observer;
  (c) ``eager_rdf``: the alternative a caller has without the observer - ``capture_md`` at K = 10 plus, after every replay, the pair
      histogram as eager torch ops on ``md.pos`` (pairwise differences, the orthorhombic minimum image with a box, ``histc``), on the
      device, nothing read back,

for one 64-atom molecule, the 192-atom water box and 256 x 64 atoms (TensorNet F = 128, L = 2, bench.py's md_latency model; NVE, a tiny
dt: the random-weight potential is no force field and the atoms must not travel).  Alternating blocks of the three legs in one process,
as tools/md_bench.py does: each block at least ``--seconds`` of stepping with the final synchronise inside the clock; median and
min / max over ``--rounds`` blocks.  Records the cost of the observer per step and per sample and its ratio to the plain loop and to the
eager histogram.  Writes profiles/md_observe.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torchmd-net_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from md_bench import _block, _summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["mol64", "water192", "batch256x64"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "md_observe.json"))
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    dt, mass_amu, fs, K, bins = 1e-3, 12.0, 9.648533e-3, 10, 256
    result = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes", "steps_per_replay": K,
              "every": K, "bins": bins, "seconds_per_block": a.seconds, "rounds": a.rounds, "dt_for_ns_per_day_fs": 1.0, "shapes": {}}
    for shape in a.shapes:
        torch.manual_seed(0)
        box = None
        if shape == "water192":
            model = create_model(dict(W.C2_ARGS, static_shapes=True, max_num_neighbors=128)).to(dev)
            z, pos, box = W.water_box(n_side=4)
            batch, n_mol, r_max = torch.zeros_like(z), 1, 6.0
            box = box.to(dev)
        else:
            n_mol = 1 if shape == "mol64" else 256
            model = create_model(dict(W.C2_ARGS, static_shapes=True, max_num_neighbors=64)).to(dev)
            z, pos, batch = W.synthetic_batch(n_mol=n_mol, n_atoms=64)
            r_max = 8.0
        z, pos, batch = z.to(dev), pos.to(dev), batch.to(dev)
        n = int(z.shape[0])
        vel0, masses = torch.zeros_like(pos), torch.full((n,), mass_amu, device=dev)
        za = int(z[0])
        observe = dict(every=K, rdf=dict(pairs=[(None, None), (za, za)], r_max=r_max, bins=bins), msd=dict(groups=[None], capacity=1 << 20),
                       vacf=dict(lags=64, groups=[None]))
        kw = dict(batch=batch, box=box, steps_per_replay=K, force_scale=fs)
        observed = model.capture_md_observed(z, pos, vel0, masses, dt, observe=observe, **kw)
        plain = model.capture_md(z, pos, vel0, masses, dt, **kw)
        eager = model.capture_md(z, pos, vel0, masses, dt, **kw)
        hist = torch.zeros(n_mol, bins, device=dev)
        per = n // n_mol
        iu = torch.triu_indices(per, per, 1, device=dev)
        edge = None if box is None else torch.diagonal(box)
        wide = torch.zeros(n_mol, bins + 1, device=dev)  # (the last column takes what lies beyond r_max)
        offset = (bins + 1) * torch.arange(n_mol, device=dev)[:, None]
        ones = torch.ones(n_mol * iu.shape[1], device=dev)

        def eager_rdf():
            eager()
            x = eager.pos.view(n_mol, per, 3)
            d = x[:, iu[1]] - x[:, iu[0]]
            if edge is not None:
                d = d - edge * torch.round(d / edge)
            r = d.norm(dim=2)
            if n_mol == 1:
                hist[0] += torch.histc(r[0], bins=bins, min=0.0, max=r_max)
            else:  # one scatter over the batch with the molecule as an offset: a loop of 256 histc calls would time the launches
                idx = (r * (bins / r_max)).long().clamp_(max=bins) + offset
                wide.view(-1).scatter_add_(0, idx.reshape(-1), ones)

        legs = {"observed": (observed, K), "plain": (plain, K), "eager_rdf": (eager_rdf, K)}
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        for md in (observed, plain, eager):
            md.check()  # raises if a trajectory overflowed: its timings would be of a frozen loop
        assert observed.n_samples > 0 and int(observed.rdf()[2].sum()) > 0
        entry = _summary(times)
        base = entry["plain"]["ms_per_step"]
        entry.update(n_atoms=n, n_mol=n_mol, r_max=r_max, tiles=int(observed._observer._tiles.shape[0]),
                     observer_us_per_sample=1e3 * K * (entry["observed"]["ms_per_step"] - base),
                     ratio_observed_over_plain=entry["observed"]["ms_per_step"] / base,
                     ratio_eager_over_plain=entry["eager_rdf"]["ms_per_step"] / base,
                     ratio_observed_over_eager=entry["observed"]["ms_per_step"] / entry["eager_rdf"]["ms_per_step"])
        result["shapes"][shape] = entry
        print(shape, json.dumps(entry), flush=True)
        del observed, plain, eager, legs
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
