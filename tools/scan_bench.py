#!/usr/bin/env python
"""A/B of the relaxed coordinate scan: ms per step of

  (a) ``a_eager``: the loop a caller builds on ``capture()`` - one graph launch on the stacked points per step, and the torsion with
      its gradient, the multipliers, the projection of force and velocity, FIRE (one controller per point), the drive of the target
      and two Gauss-Newton corrections as eager torch ops between the launches, everything on the device and nothing read back;
  (b) ``b_K10``: ``capture_scan`` with K = 10 steps per graph launch,

for one point of 64 atoms and for a 24-point torsion scan of 64 atoms, TensorNet F = 128, L = 2.  Alternating blocks of (a) and (b) in
one process, each block at least ``--seconds`` of stepping with the final synchronise inside the clock; median and min / max over
``--rounds`` blocks.  The random-weight potential is no force field, so the steps are kept tiny (dt, dt_max and max_step scaled down)
and fmax is far below what is reached: no point freezes and both legs do the full work at every step; the targets lie far enough away
that the drive works at every step too.  Writes profiles/scan.json and keeps what else the file holds; ``--slope-records DIR`` takes the
slope figures that test 9 of tests/test_gpu_scan.py recorded into its ``slope_check`` block (``--slope-only``: that alone, without a GPU)."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torchmd-net_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from min_bench import _block  # noqa: E402


def torsion(torch, x):
    """x [G,4,3] fp64 -> phi [G], grad [G,4,3]"""
    b1, b2, b3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 1], x[:, 3] - x[:, 2]
    n1, n2 = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
    l2 = b2.norm(dim=1)
    phi = torch.atan2(l2 * (b1 * n2).sum(1), (n1 * n2).sum(1))
    gi = -(l2 / (n1 * n1).sum(1))[:, None] * n1
    gl = (l2 / (n2 * n2).sum(1))[:, None] * n2
    p, q = ((b1 * b2).sum(1) / (l2 * l2))[:, None], ((b3 * b2).sum(1) / (l2 * l2))[:, None]
    return phi, torch.stack([gi, -gi - p * gi + q * gl, -gl + p * gi - q * gl, gl], 1)


def eager_scan(torch, replay, shape, idx, t_fin, fire, fmax, drive):
    """-> step(): one scan step of every point as eager torch ops on replay.pos, then one graph launch"""
    G, n = shape
    dev = replay.pos.device
    f64 = dict(dtype=torch.float64, device=dev)
    x = replay.pos.view(G, n, 3)
    out = replay()
    forces = out[1].view(G, n, 3)
    vel = torch.zeros(G, n, 3, device=dev)
    s = dict(dt=torch.full((G,), fire["dt"], **f64), alpha=torch.full((G,), fire["alpha"], **f64),
             n_pos=torch.zeros(G, dtype=torch.int64, device=dev), done=torch.zeros(G, dtype=torch.bool, device=dev),
             t=torsion(torch, x[:, idx].double())[0])
    zero = torch.zeros(G, **f64)
    tot = lambda t: t.double().sum((1, 2))
    wrap = lambda d: d - 2.0 * math.pi * torch.ceil((d - math.pi) / (2.0 * math.pi))

    def step():
        _, g = torsion(torch, x[:, idx].double())
        gg = (g * g).sum((1, 2))
        lam = ((g * forces[:, idx].double()).sum((1, 2)) / gg).float()
        mu = ((g * vel[:, idx].double()).sum((1, 2)) / gg).float()
        fp, vp = forces.clone(), vel.clone()
        fp[:, idx] += (-lam.double()[:, None, None] * g).float()
        vp[:, idx] += (-mu.double()[:, None, None] * g).float()
        vf, ff, vv = tot(vp * fp), tot(fp * fp), tot(vp * vp)
        fmax2 = (fp * fp).sum(2).amax(1).double()
        s["done"] |= (fmax2.sqrt() < fmax) & (s["t"] == t_fin)
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
        vel.copy_(vp * coef[..., 0:1] + coef[..., 1:2] * fp)
        x.addcmul_(coef[..., 2:3], vel)
        gap = wrap(t_fin - s["t"])
        s["t"] = torch.where(gap.abs() <= drive, t_fin, wrap(s["t"] + gap.clamp(-drive, drive)))
        y = x[:, idx].double()
        for _ in range(2):  # two Gauss-Newton corrections: quadratic convergence from a drive of 1e-3 rad
            phi, g = torsion(torch, y)
            y = y - (wrap(phi - s["t"]) / (g * g).sum((1, 2)))[:, None, None] * g
        x[:, idx] = torch.where(s["done"][:, None, None], x[:, idx], y.float())
        replay()

    return step, s


SLOPE_KEYS = ("n_free", "h", "fmax", "steps_to_relax", "steps", "converged_at", "slope", "minus_lambda", "deviation", "bound", "terms", "cv_gap",
              "cv_bound")


def slope_block(records):
    """the slope_check block from the records test 9 of tests/test_gpu_scan.py writes (scan_slope_<arch>.json in $TMDNET_RECORD_DIR)"""
    block = {"what": "tests/test_gpu_scan.py test 9: three torsion targets t - h, t, t + h branched by reset from the geometry relaxed at t; "
                     "the central difference of the converged energies against -lambda at t", "archs": {}}
    for name in sorted(os.listdir(records)):
        if name.startswith("scan_slope_") and name.endswith(".json"):
            with open(os.path.join(records, name)) as fh:
                r = json.load(fh)
            block["archs"][r["arch"]] = {k: r[k] for k in SLOPE_KEYS}
    if not block["archs"]:
        raise SystemExit(f"no scan_slope_*.json in {records}")
    return block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan.json"))
    ap.add_argument("--slope-records", default=None, metavar="DIR",
                    help="also take the slope figures tests/test_gpu_scan.py left in DIR (scan_slope_*.json) into the file's slope_check block")
    ap.add_argument("--slope-only", action="store_true", help="no timing: only refresh slope_check from --slope-records (needs no GPU)")
    a = ap.parse_args()
    if a.slope_only:
        if not a.slope_records:
            ap.error("--slope-only needs --slope-records DIR")
        result = json.load(open(a.out)) if os.path.exists(a.out) else {}
        result["slope_check"] = slope_block(a.slope_records)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
        print("wrote", a.out)
        return

    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model
    from torchmdnet_amd.scan import grid

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    K, n, fmax, drive = 10, 64, 1e-9, 1e-5
    fire = dict(dt=1e-4, dt_max=1e-3, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, max_step=1e-4)
    result = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes", "steps_per_replay": K,
              "seconds_per_block": a.seconds, "rounds": a.rounds, "fire": fire, "fmax": fmax, "drive": drive, "sizes": {}}
    torch.manual_seed(0)
    model = create_model(dict(W.C2_ARGS, static_shapes=True)).to(dev)
    z, pos, _ = W.synthetic_batch(n_mol=1, n_atoms=n)
    z, pos = z.to(dev), pos.to(dev).float().contiguous()
    cv = ("torsion", 5, 17, 29, 41)
    idx = torch.tensor(cv[1:], device=dev)
    s0 = float(torsion(torch, pos[idx][None].double())[0])
    for G in (1, 24):
        targets = (grid(-3.0, 3.0, G) if G > 1 else torch.tensor([[s0 + 1.0]], dtype=torch.float64)).to(dev)
        x0 = pos[None].repeat(G, 1, 1).contiguous()
        batch = torch.arange(G, device=dev).repeat_interleave(n)
        replay = model.capture(z.repeat(G), x0.reshape(-1, 3), batch)
        replay(x0.reshape(-1, 3))
        eager, state = eager_scan(torch, replay, (G, n), idx, targets[:, 0], fire, fmax, drive)
        scan = model.capture_scan(z, x0, [cv], targets, steps_per_replay=K, fmax=fmax, drive=drive, fire=fire)
        legs = {"a_eager": (eager, 1), "b_K10": (scan, K)}
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        scan.check()  # raises if the scan overflowed or was unusable: its timings would be of a frozen loop
        entry = {k: {"ms_per_step": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        entry["n_points"], entry["n_atoms"] = G, n
        entry["converged"] = {"eager": int(state["done"].sum()), "capture_scan": int((scan.converged_at >= 0).sum())}
        entry["displacement_max"] = {"eager": float((replay.pos.view(G, n, 3) - x0).abs().max()), "capture_scan": float((scan.pos - x0).abs().max())}
        entry["cv_minus_target_max"] = float((scan.cv[-1] - scan.target[-1]).abs().max())
        entry["ratio_b_over_a"] = entry["b_K10"]["ms_per_step"] / entry["a_eager"]["ms_per_step"]
        entry["b_K10_not_slower_than_eager"] = entry["b_K10"]["ms_per_step"] <= entry["a_eager"]["ms_per_step"]
        result["sizes"][f"{G}x{n}"] = entry
        print(f"{G}x{n}", json.dumps(entry), flush=True)
        del replay, scan, legs
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if os.path.exists(a.out):  # what this run does not measure stays: the slope figures of the tests
        with open(a.out) as fh:
            result = dict({k: v for k, v in json.load(fh).items() if k not in result}, **result)
    if a.slope_records:
        result["slope_check"] = slope_block(a.slope_records)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
