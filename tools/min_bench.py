#!/usr/bin/env python
"""A/B of the geometry minimiser: ms per FIRE step of

  (a) ``a_eager``: the loop a caller builds on ``capture()`` - one graph launch per step and FIRE as eager torch ops between the
      launches, one controller per molecule (``index_add_`` sums over ``batch``, ``torch.where`` for the branches), everything on
      the device and nothing read back;
  (b) ``b_K10``: ``capture_minimize`` with K = 10 steps per graph launch,

for 1 x 64 atoms, 256 x 64 atoms (bench.py's flagship batch) and the 192-atom periodic water box, TensorNet F = 128, L = 2.
Alternating blocks of (a) and (b) in one process, each block at least ``--seconds`` of stepping with the final synchronise inside
the clock; median and min / max over ``--rounds`` blocks.  The random-weight potential is no force field, so the steps are kept
tiny (dt, dt_max and max_step scaled down: the atoms must not travel) and fmax is far below what is reached: no molecule freezes
and both legs do the full work at every step.  Writes profiles/minimize.json.

``--cell``: the cell relaxation instead, on the 192-atom water box with TensorNet and the Equivariant Transformer, K = 10, three legs:
``c_cell_K10`` (``capture_minimize(cell=...)``), ``a_eager_cell`` (the loop a caller builds on ``capture(virial=True)``: FIRE and the
UnitCellFilter algebra as eager torch ops, nothing read back) and ``b_fixed_K10`` (the fixed-box captured loop).  Writes
profiles/minimize_cell.json.

``--lbfgs``: captured FIRE against captured L-BFGS (``capture_minimize(lbfgs=...)``) and an eager torch L-BFGS built on ``capture()``
with nothing read back (the history dot products chained through ``index_add_``), at the three sizes above: (1) evaluations to
fmax = 0.05 from the same start with ASE's defaults, (2) ms per step with alternating blocks, tiny steps and memory 10, (3) the cost
of the L-BFGS launches alone (one MIDDLE phase on forces that do not change, so every candidate has y = 0, is rejected, and the
history stays as it is) with 0, 10 and 100 pairs held.  Writes the ``bench`` section of profiles/minimize_lbfgs.json."""
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


def eager_fire(torch, replay, batch, n_mol, fire, fmax):
    """-> step(): one FIRE step of every molecule as eager torch ops on replay.pos, then one graph launch"""
    dev = replay.pos.device
    f64 = dict(dtype=torch.float64, device=dev)
    _, forces = replay()
    vel = torch.zeros_like(replay.pos)
    s = dict(dt=torch.full((n_mol,), fire["dt"], **f64), alpha=torch.full((n_mol,), fire["alpha"], **f64),
             n_pos=torch.zeros(n_mol, dtype=torch.int64, device=dev), done=torch.zeros(n_mol, dtype=torch.bool, device=dev))
    zero = torch.zeros(n_mol, **f64)

    def mol_sum(t):
        return torch.zeros(n_mol, **f64).index_add_(0, batch, t.sum(1).double())

    def step():
        vf, ff, vv = mol_sum(vel * forces), mol_sum(forces * forces), mol_sum(vel * vel)
        fmax2 = torch.zeros(n_mol, dtype=torch.float32, device=dev).index_reduce_(0, batch, (forces * forces).sum(1), "amax")
        s["done"] |= fmax2.double().sqrt() < fmax
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
        coef = (torch.stack([c_v, c_f, d], 1).to(torch.float32) * moving[:, None])[batch]
        vel.mul_(coef[:, 0:1]).addcmul_(coef[:, 1:2], forces)
        replay.pos.addcmul_(coef[:, 2:3], vel)
        replay()

    return step, s


def eager_fire_cell(torch, replay, box, fire, fmax, pressure):
    """-> step(): one FIRE step of ONE molecule and its cell (UnitCellFilter, cell_factor = N) as eager torch ops, then one launch of
    the capture(virial=True) graph; `box` is the tensor that graph reads"""
    dev = replay.pos.device
    f64 = dict(dtype=torch.float64, device=dev)
    n = replay.pos.shape[0]
    _, forces, virial = replay()
    xt, vel = replay.pos.clone(), torch.zeros_like(replay.pos)
    H0, eye = box.double().clone(), torch.eye(3, **f64)
    s = dict(dt=torch.tensor(fire["dt"], **f64), alpha=torch.tensor(fire["alpha"], **f64), n_pos=torch.zeros((), dtype=torch.int64, device=dev),
             done=torch.zeros((), dtype=torch.bool, device=dev), D=eye.clone(), VD=torch.zeros(3, 3, **f64))
    zero = torch.zeros((), **f64)
    upper = torch.triu(torch.ones(3, 3, **f64))  # the rotation gauge of capture_minimize(cell=...)

    def step():
        D32 = s["D"].float()
        ft = forces @ D32
        W = virial[0].double()
        V = torch.linalg.det(box.double()).abs()
        G = (0.5 * (W + W.T) - pressure * V * eye) @ torch.linalg.inv_ex(s["D"], check_errors=False).inverse.T * upper / n
        vf = (vel * ft).sum().double() + (s["VD"] * G).sum()
        ff = (ft * ft).sum().double() + (G * G).sum()
        vv = (vel * vel).sum().double() + (s["VD"] * s["VD"]).sum()
        fmax2 = torch.maximum((ft * ft).sum(1).max().double(), (G * G).sum(1).max())
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
        moving = (~s["done"]).double()
        c_v, c_f, d = c_v * moving, c_f * moving, d * moving
        s["VD"] = c_v * s["VD"] + c_f * G
        s["D"] = s["D"] + d * s["VD"] / n
        vel.mul_(c_v.float()).add_(ft * c_f.float())
        xt.add_(vel * d.float())
        box.copy_((H0 @ s["D"].T).float())
        torch.matmul(xt, s["D"].float().T, out=replay.pos)
        replay()

    return step, s


def main_cell(a):
    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    K, fmax, pressure = 10, 1e-9, 0.0
    fire = dict(dt=1e-4, dt_max=1e-3, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, max_step=1e-4)
    archs = {"tensornet": dict(W.C2_ARGS, static_shapes=True, max_num_neighbors=128),
             "equivariant-transformer": dict(W.C4_ARGS, static_shapes=True, max_num_neighbors=128, cutoff_upper=5.0, vector_cutoff=False)}
    result = {"device": torch.cuda.get_device_name(dev), "system": "192-atom periodic water box", "steps_per_replay": K,
              "seconds_per_block": a.seconds, "rounds": a.rounds, "fire": fire, "fmax": fmax, "pressure": pressure, "models": {}}
    z, pos, box0 = W.water_box(n_side=4)
    z, pos, batch, box0 = z.to(dev), pos.to(dev).float().contiguous(), torch.zeros_like(z).to(dev), box0.to(dev).float().contiguous()
    for name, args in archs.items():
        torch.manual_seed(0)
        model = create_model(dict(args)).to(dev)
        box_e = box0.clone()
        replay = model.capture(z, pos, batch, box_e, virial=True)
        replay(pos)
        eager, state = eager_fire_cell(torch, replay, box_e, fire, fmax, pressure)
        cell = model.capture_minimize(z, pos, batch=batch, box=box0.clone(), steps_per_replay=K, fmax=fmax, fire=fire,
                                      cell=dict(pressure=pressure))
        fixed = model.capture_minimize(z, pos, batch=batch, box=box0.clone(), steps_per_replay=K, fmax=fmax, fire=fire)
        legs = {"a_eager_cell": (eager, 1), "c_cell_K10": (cell, K), "b_fixed_K10": (fixed, K)}
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        cell.check()
        fixed.check()
        entry = {k: {"ms_per_step": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        entry["n_atoms"] = int(z.shape[0])
        entry["box_change_max"] = {"eager": float((box_e - box0).abs().max()), "capture_minimize": float((cell.box - box0).abs().max())}
        entry["ratio_cell_over_eager"] = entry["c_cell_K10"]["ms_per_step"] / entry["a_eager_cell"]["ms_per_step"]
        entry["ratio_cell_over_fixed"] = entry["c_cell_K10"]["ms_per_step"] / entry["b_fixed_K10"]["ms_per_step"]
        entry["cell_not_slower_than_eager"] = entry["c_cell_K10"]["ms_per_step"] <= entry["a_eager_cell"]["ms_per_step"]
        result["models"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del replay, cell, fixed, legs
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


def eager_lbfgs(torch, replay, batch, n_mol, lb, fmax):
    """-> step(): one L-BFGS step of every molecule as eager torch ops on replay.pos, then one graph launch.  The history is a ring
    of `memory` slots per molecule; an empty slot has rho = 0 and contributes nothing.  2 x memory dependent per-molecule reductions."""
    dev = replay.pos.device
    f64 = dict(dtype=torch.float64, device=dev)
    m = lb["memory"]
    _, forces = replay()
    n = replay.pos.shape[0]
    S, Y = torch.zeros((m, n, 3), device=dev), torch.zeros((m, n, 3), device=dev)
    rho = torch.zeros((m, n_mol), **f64)
    x_prev, f_prev = replay.pos.clone(), forces.clone()
    s = dict(done=torch.zeros(n_mol, dtype=torch.bool, device=dev), first=True)

    def mol_sum(t):
        return torch.zeros(n_mol, **f64).index_add_(0, batch, t.sum(1).double())

    def step():
        nonlocal S, Y, rho
        fmax2 = torch.zeros(n_mol, dtype=torch.float32, device=dev).index_reduce_(0, batch, (forces * forces).sum(1), "amax")
        s["done"] |= fmax2.double().sqrt() < fmax
        if not s["first"]:
            sc, yc = replay.pos - x_prev, f_prev - forces
            sy = mol_sum(sc * yc)
            acc = (sy > 0) & ~s["done"]
            a_atom = acc[batch][None, :, None]
            S = torch.where(a_atom, torch.cat([S[1:], sc[None]]), S)
            Y = torch.where(a_atom, torch.cat([Y[1:], yc[None]]), Y)
            rho = torch.where(acc[None], torch.cat([rho[1:], (1.0 / sy.clamp_min(1e-300))[None]]), rho)
        s["first"] = False
        q = -forces
        a = []
        for i in range(m - 1, -1, -1):
            a.append(rho[i] * mol_sum(S[i] * q))
            q = q - a[-1].float()[batch][:, None] * Y[i]
        a.reverse()
        z = q / lb["alpha"]
        for i in range(m):
            b = rho[i] * mol_sum(Y[i] * z)
            z = z + S[i] * (a[i] - b).float()[batch][:, None]
        longest = torch.zeros(n_mol, dtype=torch.float32, device=dev).index_reduce_(0, batch, (z * z).sum(1), "amax").double().sqrt()
        c = lb["damping"] * (lb["max_step"] / longest.clamp_min(1e-300)).clamp_max(1.0) * (~s["done"]).double()
        x_prev.copy_(replay.pos)
        f_prev.copy_(forces)
        replay.pos.addcmul_(c.float()[batch][:, None], -z)
        replay()

    return step, s


def main_lbfgs(a):
    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.minimize import MIN_MIDDLE
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    K, tiny = 10, 1e-9
    fire = dict(dt=1e-4, dt_max=1e-3, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, max_step=1e-4)
    lb = dict(memory=10, alpha=70.0, max_step=1e-4, damping=1.0)
    result = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes, random weights",
              "steps_per_replay": K, "seconds_per_block": a.seconds, "rounds": a.rounds, "fire": fire, "lbfgs_timing": lb,
              "max_steps_to_fmax": a.max_steps, "sizes": {}}
    for name in ("1x64", "256x64", "water192"):
        torch.manual_seed(0)
        if name == "water192":
            model = create_model(dict(W.C2_ARGS, static_shapes=True, max_num_neighbors=128)).to(dev)
            z, pos, box = W.water_box(n_side=4)
            batch, box = torch.zeros_like(z), box.to(dev).float().contiguous()
        else:
            model = create_model(dict(W.C2_ARGS, static_shapes=True)).to(dev)
            z, pos, batch = W.synthetic_batch(n_mol=int(name.split("x")[0]), n_atoms=64)
            box = None
        z, pos, batch = z.to(dev), pos.to(dev).float().contiguous(), batch.to(dev)
        n_mol = int(batch.max()) + 1
        entry = {"n_atoms": int(z.shape[0]), "n_mol": n_mol}
        # (1) evaluations to fmax = 0.05, ASE's defaults, the same start
        evals = {}
        for leg, kw in (("fire", dict()), ("lbfgs", dict(lbfgs={}))):
            opt = model.capture_minimize(z, pos, batch=batch, box=box, steps_per_replay=1, fmax=0.05, **kw)
            taken = opt.run(a.max_steps, check_every=10)
            opt.check()
            conv = opt.converged_at.cpu()
            done = conv >= 0
            evals[leg] = {"steps_run": taken, "converged": int(done.sum()), "of": n_mol,
                          "median_evaluations_of_converged": float(conv[done].double().median()) if bool(done.any()) else None,
                          "max_evaluations_of_converged": int(conv[done].max()) if bool(done.any()) else None,
                          "final_fmax_max": float(opt.fmax[-1].max())}
            evals[leg]["conv"] = conv
            del opt
        both = (evals["fire"]["conv"] >= 0) & (evals["lbfgs"]["conv"] >= 0)
        evals["converged_in_both"] = int(both.sum())
        if bool(both.any()):
            evals["median_evaluations_where_both_converged"] = {k: float(evals[k]["conv"][both].double().median()) for k in ("fire", "lbfgs")}
            evals["lbfgs_fewer_evaluations"] = evals["median_evaluations_where_both_converged"]["lbfgs"] < \
                evals["median_evaluations_where_both_converged"]["fire"]
        for k in ("fire", "lbfgs"):
            del evals[k]["conv"]
        entry["evaluations_to_fmax_0.05"] = evals
        # (2) ms per step: tiny steps, nothing freezes, every leg does the full work at every step
        replay = model.capture(z, pos, batch, box)
        replay(pos)
        eager, state = eager_lbfgs(torch, replay, batch, n_mol, lb, tiny)
        c_fire = model.capture_minimize(z, pos, batch=batch, box=box, steps_per_replay=K, fmax=tiny, fire=fire)
        c_lbfgs = model.capture_minimize(z, pos, batch=batch, box=box, steps_per_replay=K, fmax=tiny, lbfgs=lb)
        legs = {"eager_lbfgs": (eager, 1), "captured_fire_K10": (c_fire, K), "captured_lbfgs_K10": (c_lbfgs, K)}
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        c_fire.check()
        c_lbfgs.check()
        entry["ms_per_step"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        entry["pairs_held"] = {"captured_lbfgs": [int(c_lbfgs.pairs.min()), int(c_lbfgs.pairs.max())]}
        entry["captured_lbfgs_not_slower_than_eager"] = entry["ms_per_step"]["captured_lbfgs_K10"]["median"] <= \
            entry["ms_per_step"]["eager_lbfgs"]["median"]
        entry["ratio_lbfgs_over_fire"] = entry["ms_per_step"]["captured_lbfgs_K10"]["median"] / entry["ms_per_step"]["captured_fire_K10"]["median"]
        del replay, c_fire, c_lbfgs, legs, eager
        # (3) the L-BFGS launches alone with 0, 10 and 100 pairs held
        hist = {}
        for h in (0, 10, 100):
            mem = max(h, 1)
            opt = model.capture_minimize(z, pos, batch=batch, box=box, steps_per_replay=K, fmax=tiny, lbfgs=dict(lb, memory=mem))
            if h:
                opt(-(-3 * h // K))  # fill the history
            opt.check()
            energy = torch.zeros(n_mol, device=dev)
            middle = lambda: opt._advance(MIN_MIDDLE, opt.forces, energy, 0)
            with torch.cuda.device(dev):
                v = [_block(middle, 1, min(a.seconds, 0.5), sync) for _ in range(a.rounds)]
            held = [int(opt.pairs.min()), int(opt.pairs.max())]
            hist[str(h)] = {"ms_per_middle_phase": statistics.median(v), "min": min(v), "max": max(v), "pairs_held": held,
                            "note": "eager launches back to back, not a graph replay: an upper bound of the cost inside the graph"}
            hist[str(h)]["share_of_captured_step"] = hist[str(h)]["ms_per_middle_phase"] / entry["ms_per_step"]["captured_lbfgs_K10"]["median"]
            del opt, middle
        entry["lbfgs_launches_alone"] = hist
        result["sizes"][name] = entry
        print(name, json.dumps(entry), flush=True)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    doc["bench"] = result
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cell", action="store_true", help="the cell relaxation on the water box (profiles/minimize_cell.json)")
    ap.add_argument("--lbfgs", action="store_true", help="FIRE against L-BFGS, captured and eager (profiles/minimize_lbfgs.json)")
    ap.add_argument("--max-steps", type=int, default=300, help="--lbfgs: the most evaluations spent on reaching fmax = 0.05")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "minimize_lbfgs.json" if a.lbfgs else "minimize_cell.json" if a.cell else "minimize.json")
    if a.cell:
        return main_cell(a)
    if a.lbfgs:
        return main_lbfgs(a)

    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    K, fmax = 10, 1e-9
    fire = dict(dt=1e-4, dt_max=1e-3, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, max_step=1e-4)
    result = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes", "steps_per_replay": K,
              "seconds_per_block": a.seconds, "rounds": a.rounds, "fire": fire, "fmax": fmax, "sizes": {}}
    for name in ("1x64", "256x64", "water192"):
        torch.manual_seed(0)
        if name == "water192":
            model = create_model(dict(W.C2_ARGS, static_shapes=True, max_num_neighbors=128)).to(dev)
            z, pos, box = W.water_box(n_side=4)
            batch, box = torch.zeros_like(z), box.to(dev).float().contiguous()
        else:
            model = create_model(dict(W.C2_ARGS, static_shapes=True)).to(dev)
            z, pos, batch = W.synthetic_batch(n_mol=int(name.split("x")[0]), n_atoms=64)
            box = None
        z, pos, batch = z.to(dev), pos.to(dev).float().contiguous(), batch.to(dev)
        n_mol = int(batch.max()) + 1
        replay = model.capture(z, pos, batch, box)
        replay(pos)
        eager, state = eager_fire(torch, replay, batch, n_mol, fire, fmax)
        opt = model.capture_minimize(z, pos, batch=batch, box=box, steps_per_replay=K, fmax=fmax, fire=fire)
        legs = {"a_eager": (eager, 1), "b_K10": (opt, K)}
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        opt.check()  # raises if the minimisation overflowed: its timings would be of a frozen loop
        entry = {k: {"ms_per_step": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        entry["n_atoms"], entry["n_mol"] = int(z.shape[0]), n_mol
        entry["converged"] = {"eager": int(state["done"].sum()), "capture_minimize": int((opt.converged_at >= 0).sum())}
        entry["displacement_max"] = {"eager": float((replay.pos - pos).abs().max()), "capture_minimize": float((opt.pos - pos).abs().max())}
        entry["ratio_b_over_a"] = entry["b_K10"]["ms_per_step"] / entry["a_eager"]["ms_per_step"]
        entry["b_K10_not_slower_than_eager"] = entry["b_K10"]["ms_per_step"] <= entry["a_eager"]["ms_per_step"]
        result["sizes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del replay, opt, legs
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
