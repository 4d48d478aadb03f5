#!/usr/bin/env python
"""A/B of the nudged elastic band: ms per band step of

  (a) ``a_eager``: the loop a caller builds on ``capture()`` - one graph launch on the stacked images per step, and the path sums,
      the improved tangents, the band force and FIRE (one controller per band) as eager torch ops between the launches, everything
      on the device and nothing read back;
  (b) ``b_K10``: ``capture_neb`` with K = 10 steps per graph launch,

for one band of 7 images x 64 atoms and for 16 such bands, TensorNet F = 128, L = 2.  Alternating blocks of (a) and (b) in one process,
each block at least ``--seconds`` of stepping with the final synchronise inside the clock; median and min / max over ``--rounds``
blocks.  The random-weight potential is no force field, so the steps are kept tiny (dt, dt_max and max_step scaled down: the images
must not travel) and fmax is far below what is reached: no band freezes and both legs do the full work at every step.  Writes
profiles/neb.json."""
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


def eager_neb(torch, replay, shape, fire, fmax, spring, climb):
    """-> step(): one band step of every band as eager torch ops on replay.pos, then one graph launch"""
    G, M, n = shape
    dev = replay.pos.device
    f64 = dict(dtype=torch.float64, device=dev)
    x = replay.pos.view(G, M, n, 3)
    out = replay()
    energy, forces = out[0].view(G, M), out[1].view(G, M, n, 3)
    vel = torch.zeros(G, M - 2, n, 3, device=dev)
    s = dict(dt=torch.full((G,), fire["dt"], **f64), alpha=torch.full((G,), fire["alpha"], **f64),
             n_pos=torch.zeros(G, dtype=torch.int64, device=dev), done=torch.zeros(G, dtype=torch.bool, device=dev))
    zero = torch.zeros(G, **f64)
    inner = torch.arange(1, M - 1, device=dev)

    def step():
        f = forces[:, 1:-1]
        dp, dm = x[:, 2:] - x[:, 1:-1], x[:, 1:-1] - x[:, :-2]
        tot = lambda t: t.double().sum((2, 3))  # [G, M-2]
        a, b, c, p, q = tot(dp * dp), tot(dm * dm), tot(dp * dm), tot(f * dp), tot(f * dm)
        e = energy.double()
        e_prev, e_mid, e_next = e[:, :-2], e[:, 1:-1], e[:, 2:]
        up, dn = (e_next - e_mid).abs(), (e_prev - e_mid).abs()
        hi, lo = torch.maximum(up, dn), torch.minimum(up, dn)
        rising, falling = (e_next > e_mid) & (e_mid > e_prev), (e_next < e_mid) & (e_mid < e_prev)
        wp = torch.where(rising, 1.0, torch.where(falling, 0.0, torch.where(e_next > e_prev, hi, lo)))
        wm = torch.where(rising, 0.0, torch.where(falling, 1.0, torch.where(e_next > e_prev, lo, hi)))
        tau2 = wp * wp * a + 2.0 * wp * wm * c + wm * wm * b
        ft = wp * p + wm * q
        tau = tau2.sqrt()
        g = (-(ft / tau) + spring * (a.sqrt() - b.sqrt())) / tau
        if climb:
            top = e_mid.argmax(1, keepdim=True) + 1
            g = torch.where(inner[None, :] == top, -2.0 * ft / tau2, g)
        sp, sm = (g * wp).float()[..., None, None], (g * wm).float()[..., None, None]
        fneb = f + sp * dp + sm * dm
        band = lambda t: t.double().sum((1, 2, 3))  # [G]
        vf, ff, vv = band(vel * fneb), band(fneb * fneb), band(vel * vel)
        fmax2 = (fneb * fneb).sum(3).amax((1, 2)).double()
        s["done"] |= fmax2.sqrt() < fmax
        down = vf > 0
        c_v = torch.where(down, 1.0 - s["alpha"], zero)
        mix = torch.where(down & (ff > 0) & (vv > 0), s["alpha"] * torch.sqrt(vv / ff.clamp_min(1e-300)), zero)
        grow = down & (s["n_pos"] > fire["n_min"])
        s["dt"] = torch.where(grow, (s["dt"] * fire["f_inc"]).clamp_max(fire["dt_max"]), torch.where(down, s["dt"], s["dt"] * fire["f_dec"]))
        s["alpha"] = torch.where(grow, s["alpha"] * fire["f_alpha"], torch.where(down, s["alpha"], torch.full_like(zero, fire["alpha"])))
        s["n_pos"] = torch.where(down, s["n_pos"] + 1, torch.zeros_like(s["n_pos"]))
        c_f = mix + s["dt"]
        n2 = c_v * c_v * vv + 2.0 * c_v * c_f * vf + c_f * c_f * ff
        length = s["dt"] * torch.sqrt(n2.clamp_min(0.0))
        d = s["dt"] * (fire["max_step"] / length.clamp_min(1e-300)).clamp_max(1.0)
        moving = (~s["done"]).to(torch.float32)
        coef = (torch.stack([c_v, c_f, d], 1).to(torch.float32) * moving[:, None])[:, None, None, :]
        vel.mul_(coef[..., 0:1]).addcmul_(coef[..., 1:2], fneb)
        x[:, 1:-1].addcmul_(coef[..., 2:3], vel)
        replay()

    return step, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neb.json"))
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model
    from torchmdnet_amd.neb import interpolate

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    K, M, n, fmax, spring, climb = 10, 7, 64, 1e-9, 0.1, True
    fire = dict(dt=1e-4, dt_max=1e-3, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, max_step=1e-4)
    result = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes", "steps_per_replay": K,
              "seconds_per_block": a.seconds, "rounds": a.rounds, "fire": fire, "fmax": fmax, "spring": spring, "climb": climb,
              "sizes": {}}
    torch.manual_seed(0)
    model = create_model(dict(W.C2_ARGS, static_shapes=True)).to(dev)
    z, pos, _ = W.synthetic_batch(n_mol=1, n_atoms=n)
    z, pos = z.to(dev), pos.to(dev).float().contiguous()
    for G in (1, 16):
        bands = []
        for b in range(G):  # every band from the molecule to a copy displaced smoothly by at most 0.3 per atom
            g = torch.Generator().manual_seed(100 + b)
            k, ph = torch.rand(3, 3, generator=g).to(dev), (6.28 * torch.rand(3, generator=g)).to(dev)
            bands.append(interpolate(pos, pos + (0.3 / 3 ** 0.5) * torch.sin(pos @ k + ph), M))
        images = torch.stack(bands).contiguous()
        batch = torch.arange(G * M, device=dev).repeat_interleave(n)
        replay = model.capture(z.repeat(G * M), images.reshape(-1, 3), batch)
        replay(images.reshape(-1, 3))
        eager, state = eager_neb(torch, replay, (G, M, n), fire, fmax, spring, climb)
        neb = model.capture_neb(z, images, steps_per_replay=K, fmax=fmax, spring=spring, climb=climb, fire=fire)
        legs = {"a_eager": (eager, 1), "b_K10": (neb, K)}
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        neb.check()  # raises if the band overflowed or was unusable: its timings would be of a frozen loop
        entry = {k: {"ms_per_step": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        entry["n_bands"], entry["n_images"], entry["n_atoms_per_image"] = G, M, n
        entry["converged"] = {"eager": int(state["done"].sum()), "capture_neb": int((neb.converged_at >= 0).sum())}
        start = images.reshape(-1, 3)
        entry["displacement_max"] = {"eager": float((replay.pos - start).abs().max()), "capture_neb": float((neb.pos - start).abs().max())}
        entry["ratio_b_over_a"] = entry["b_K10"]["ms_per_step"] / entry["a_eager"]["ms_per_step"]
        entry["b_K10_not_slower_than_eager"] = entry["b_K10"]["ms_per_step"] <= entry["a_eager"]["ms_per_step"]
        result["sizes"][f"{G}x{M}x{n}"] = entry
        print(f"{G}x{M}x{n}", json.dumps(entry), flush=True)
        del replay, neb, legs
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
