#!/usr/bin/env python
"""A/B of the dimer saddle search: ms per dimer step of

  (a) ``a_eager``: the loop a caller builds on ``capture()`` - one graph launch on the stacked images per step, and the curvature
      rows, the 2 x 2 rotation, the inverted force, the next partner and FIRE (one controller per dimer) as eager torch ops between
      the launches, everything on the device and nothing read back;
  (b) ``b_K10``: ``capture_dimer`` with K = 10 steps per graph launch,

for one dimer of 64 atoms and for 16 such dimers, TensorNet F = 128, L = 2.  Alternating blocks of (a) and (b) in one process, each
block at least ``--seconds`` of stepping with the final synchronise inside the clock; median and min / max over ``--rounds`` blocks.
The random-weight potential is no force field, so the steps are kept tiny (dt, dt_max and max_step scaled down: the midpoints must
not travel) and fmax is far below what is reached: no dimer freezes and both legs do the full work at every step.  It also measures,
on a 7-atom molecule with ``translate=False``, how far the logged curvature is from N'^T H N' of the central Hessian.  Writes
profiles/dimer.json."""
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


def eager_dimer(torch, replay, shape, N, M, fire, fmax, delta):
    """-> step(): one dimer step of every dimer as eager torch ops on replay.pos, then one graph launch"""
    G, n = shape
    dev = replay.pos.device
    f64 = dict(dtype=torch.float64, device=dev)
    x = replay.pos.view(G, 3, n, 3)
    out = replay()
    forces = out[1].view(G, 3, n, 3)
    vel = torch.zeros(G, n, 3, device=dev)
    s = dict(dt=torch.full((G,), fire["dt"], **f64), alpha=torch.full((G,), fire["alpha"], **f64),
             n_pos=torch.zeros(G, dtype=torch.int64, device=dev), done=torch.zeros(G, dtype=torch.bool, device=dev), N=N.clone(), M=M.clone())
    zero = torch.zeros(G, **f64)
    tot = lambda t: t.double().sum((1, 2))  # [G]

    def step():
        N, M = s["N"], s["M"]
        f0 = forces[:, 0]
        hn, hm = (f0 - forces[:, 1]) / delta, (f0 - forces[:, 2]) / delta
        a, b, c = tot(N * hn), 0.5 * (tot(N * hm) + tot(M * hn)), tot(M * hm)
        theta = 0.5 * torch.atan2(-2.0 * b, c - a)
        co, si = torch.cos(theta), torch.sin(theta)
        u = co[:, None, None] * N.double() + si[:, None, None] * M.double()
        nu = u.pow(2).sum((1, 2)).sqrt()
        cn, sn = (co / nu).float()[:, None, None], (si / nu).float()[:, None, None]
        Np, Hp = cn * N + sn * M, cn * hn + sn * hm
        C = (co * co * a + 2.0 * co * si * b + si * si * c) / (nu * nu)
        p = (co * tot(f0 * N) + si * tot(f0 * M)) / nu
        T = Hp - C.float()[:, None, None] * Np
        feff = torch.where((C < 0)[:, None, None], f0 - (2.0 * p).float()[:, None, None] * Np, -p.float()[:, None, None] * Np)
        kt = tot(T * Np) / tot(Np * Np)
        T = T - kt.float()[:, None, None] * Np
        s["N"], s["M"] = Np, T / tot(T * T).sqrt().float()[:, None, None]
        vf, ff, vv = tot(vel * feff), tot(feff * feff), tot(vel * vel)
        fmax2 = (feff * feff).sum(2).amax(1).double()
        s["done"] |= (fmax2.sqrt() < fmax) & (C < 0)
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
        coef = (torch.stack([c_v, c_f, d], 1).to(torch.float32) * moving[:, None])[:, None, :]
        vel.mul_(coef[..., 0:1]).addcmul_(coef[..., 1:2], feff)
        x[:, 0].addcmul_(coef[..., 2:3], vel)
        x[:, 1] = x[:, 0] + delta * s["N"]
        x[:, 2] = x[:, 0] + delta * s["M"]
        replay()

    return step, s


def curvature_check(torch, model, z, pos, delta):
    """translate=False on the first 7 atoms: the logged C against N'^T H N' of the central Hessian at the same delta"""
    z7, p7 = z[:7].contiguous(), pos[:7].contiguous()
    dimer = model.capture_dimer(z7, p7, steps_per_replay=10, translate=False, delta=delta, seed=2)
    dimer(2)
    dimer.check()
    H, _ = model.hessian(z7, p7, method="central", delta=delta)
    Np = dimer.mode[0].double().reshape(-1)
    ritz = float(Np @ H[0].double() @ Np)
    C = float(dimer.curvature[-1, 0])
    return {"n_atoms": 7, "steps": 20, "delta": delta, "C_logged": C, "ritz_value_central_hessian": ritz, "abs_deviation": abs(C - ritz),
            "lowest_eigenvalue": float(torch.linalg.eigvalsh(0.5 * (H[0] + H[0].T).double())[0]), "residual": float(dimer.residual[-1, 0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dimer.json"))
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.dimer import orthonormal_pair
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    K, n, fmax, delta = 10, 64, 1e-9, 0.01
    fire = dict(dt=1e-4, dt_max=1e-3, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, max_step=1e-4)
    result = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes", "steps_per_replay": K,
              "seconds_per_block": a.seconds, "rounds": a.rounds, "fire": fire, "fmax": fmax, "delta": delta, "sizes": {}}
    torch.manual_seed(0)
    model = create_model(dict(W.C2_ARGS, static_shapes=True)).to(dev)
    z, pos, _ = W.synthetic_batch(n_mol=1, n_atoms=n)
    z, pos = z.to(dev), pos.to(dev).float().contiguous()
    for G in (1, 16):
        mids = []
        for g in range(G):  # every dimer at a copy of the molecule displaced smoothly by at most 0.1 per atom
            gen = torch.Generator().manual_seed(100 + g)
            k, ph = torch.rand(3, 3, generator=gen).to(dev), (6.28 * torch.rand(3, generator=gen)).to(dev)
            mids.append(pos + (0.1 / 3 ** 0.5) * torch.sin(pos @ k + ph))
        x0 = torch.stack(mids).contiguous()
        N, M = (t.to(dev) for t in orthonormal_pair(None, G, n, None, seed=0))
        images = torch.stack([x0, x0 + delta * N, x0 + delta * M], 1).contiguous()
        batch = torch.arange(3 * G, device=dev).repeat_interleave(n)
        replay = model.capture(z.repeat(3 * G), images.reshape(-1, 3), batch)
        replay(images.reshape(-1, 3))
        eager, state = eager_dimer(torch, replay, (G, n), N, M, fire, fmax, delta)
        dimer = model.capture_dimer(z, x0, steps_per_replay=K, fmax=fmax, delta=delta, fire=fire, seed=0)
        legs = {"a_eager": (eager, 1), "b_K10": (dimer, K)}
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        dimer.check()  # raises if the search overflowed or was unusable: its timings would be of a frozen loop
        entry = {k: {"ms_per_step": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        entry["n_dimers"], entry["n_atoms_per_image"] = G, n
        entry["converged"] = {"eager": int(state["done"].sum()), "capture_dimer": int((dimer.converged_at >= 0).sum())}
        entry["displacement_max"] = {"eager": float((replay.pos.view(G, 3, n, 3)[:, 0] - x0).abs().max()),
                                     "capture_dimer": float((dimer.pos - x0).abs().max())}
        entry["curvature_last"] = [float(c) for c in dimer.curvature[-1].cpu()]
        entry["ratio_b_over_a"] = entry["b_K10"]["ms_per_step"] / entry["a_eager"]["ms_per_step"]
        entry["b_K10_not_slower_than_eager"] = entry["b_K10"]["ms_per_step"] <= entry["a_eager"]["ms_per_step"]
        result["sizes"][f"{G}x{n}"] = entry
        print(f"{G}x{n}", json.dumps(entry), flush=True)
        del replay, dimer, legs
    result["curvature_vs_central_hessian"] = curvature_check(torch, model, z, pos, delta)
    print("curvature", json.dumps(result["curvature_vs_central_hessian"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
