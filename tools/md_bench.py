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
potential is no force field).  Records the NPT / NVT ratio and NPT against the eager loop per size; writes profiles/md_npt.json.

``--npt-cell``: the anisotropic cell barostat, on the two systems of ``--npt`` with its thermostat and barostat parameters:

  (a) ``a_eager_cell``: the loop a caller builds on ``capture(virial=True)`` - one graph launch per step, Langevin integrator and an
      anisotropic stochastic-cell-rescaling move as eager torch ops (kinetic tensor, two fp32 matrix exponentials, a QR of the new
      box, the rotation of positions, velocities and forces), nothing read back;
  (b) ``b_K10_isotropic``: ``capture_md(thermostat=, barostat=)`` with K = 10, the isotropic loop as it was;
      ``b_K10_cell_anisotropic`` / ``b_K10_cell_semi_isotropic``: ``capture_md_cell`` with K = 10,

same alternating blocks, median and min / max.  Records what the cell barostat costs over the isotropic one (microseconds per step
and ratio) and against the eager loop; writes profiles/md_npt_cell.json.

``--constraints``: the constrained loop, on the 192-atom water box (rigid water: three coupled constraints per molecule) and on the
64-atom molecule above (its X-H bonds, ``md.hydrogen_pairs``), in a state where the atoms move so that the iterations have work to
do: dt = 2 fs, thermal velocities (300 K), and ``force_scale`` such that the random-weight model's largest initial force counts as
0.2 eV / A:

  (a) ``a_eager_shake``: the loop a caller builds on ``capture()`` - one graph launch per step, velocity Verlet, SHAKE and the
      velocity projection as eager torch ops (a fixed number of Gauss-Seidel sweeps - the largest number any cluster needed, see
      below -, the constraints of equal rank in their cluster relaxed together; nothing read back);
  (b) ``b_K10_constrained``: ``capture_md_constrained(constraints=)`` with K = 10, and ``b_K10_free``: the same without constraints.

A block is ``--block-steps`` steps from the same start (the atoms must not travel far: no force field), restarted outside the clock;
alternating blocks, median and min / max over ``--rounds`` blocks after one that warms up.  ``iteration`` records what SHAKE and
RATTLE had to do at the middle step of a block - the residual before SHAKE over its bound, and the correcting sweeps per cluster,
counted by the same Gauss-Seidel iteration in fp64 on the host from the device's state -, and ``residual_over_bound_end`` what the
unconstrained leg's positions have become.  Writes profiles/md_constraints.json.

``--remd``: temperature replica exchange, G = 8 ladders of R = 32 slots of the 64-atom molecule above (B = 256 replicas, 16 384
atoms), Langevin, K = 100 steps per replay:

  (a) ``capture_md``: the 256 replicas as plain ``capture_md`` at one temperature - the loop as it was before the exchange existed;
  (b) ``remd_X0`` / ``remd_X10`` / ``remd_X100``: ``capture_remd`` on a geometric ladder with ``exchange_every`` = 0, 10, 100.

Same alternating blocks, median and min / max; prints the acceptance matrix [G,R-1] of every leg with exchanges and records the
ratios to (a).  Writes the key ``timing`` of profiles/md_remd.json (the other keys of that file are kept).

``--bias``: collective-variable restraints and metadynamics, K = 10, NVE, on 1 x 64 and 256 x 64 atoms (the 64-atom molecule above,
one walker and 256 walkers in groups of 4):

  (a) ``capture_md``: the unbiased loop;
  (b) ``restraints``: ``capture_md_biased`` with a distance, an angle and a torsion restrained; ``metad_0`` / ``metad_1000`` /
      ``metad_10000``: the same plus two-dimensional metadynamics whose groups hold 0, 1 000 and 10 000 hills (loaded with
      ``reset(hills=)``; the pace is longer than the run, so the lists stay as they are);
  (c) ``eager_restraint`` / ``eager_metad_1000``: the loop a caller builds on ``capture()`` - one graph launch per step, velocity
      Verlet and a distance restraint (plus 1 000 one-dimensional hills per group) as eager torch ops, nothing read back.

Same alternating blocks, median and min / max; records the ratios to (a) and the slope of the cost per step in the number of hills.
Writes the key ``timing`` of profiles/md_bias.json (the other keys of that file are kept).

``--global``: the global thermostats, K = 10, one system of 64, 256 and 1 024 atoms as above:

  (a) ``a_eager_csvr``: the loop a caller builds on ``capture()`` - one graph launch per step, velocity Verlet, the kinetic energy
      by a torch reduction and the stochastic-velocity-rescaling factor from torch's own normal and gamma deviates, all on the device,
      nothing read back;
  (b) ``b_K10_langevin``: ``capture_md`` with the Langevin thermostat (the yardstick), ``b_K10_csvr`` and ``b_K10_nose_hoover``:
      ``capture_md_global`` at the same kT.

Same alternating blocks, median and min / max; records the cost of both global thermostats over the Langevin loop and CSVR against
the eager loop per size.  Writes profiles/md_global.json."""
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


def npt_cell_main(a):
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
    eye = torch.eye(3, device=dev)
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

        def a_eager_cell():  # the anisotropic move as a caller writes it in torch: fp32 matrix exponentials and a QR of the new box
            vel.add_(forces, alpha=hk)
            replay.pos.add_(vel, alpha=dt)
            replay()
            vel.add_(forces, alpha=hk)
            vel.mul_(c1).add_(torch.randn_like(vel), alpha=c2s)
            kt = (vel.t() @ vel) * (0.5 * mass_amu / fs)
            vol = torch.linalg.det(ebox).abs()
            p = (2.0 * kt + virial[0]) / vol
            d = (p - baro["pressure"] * eye) * (acoef / 3.0) + torch.sqrt(2.0 * kT * acoef / (3.0 * vol)) * torch.randn((3, 3), device=dev)
            mu, nu = torch.linalg.matrix_exp(d), torch.linalg.matrix_exp(-d.t())
            q, r = torch.linalg.qr((ebox @ mu).t())  # h mu = r^T q^T: lower triangular times a rotation
            sign = torch.sign(torch.diagonal(r))
            q = q * sign
            ebox.copy_((r * sign[:, None]).t())
            torch.matmul(replay.pos @ mu, q, out=replay.pos)
            torch.matmul(vel @ nu, q, out=vel)
            forces.copy_(forces @ q)  # the next opening kick reads them in the rotated frame

        legs = {"a_eager_cell": (a_eager_cell, 1)}
        iso = model.capture_md(z, pos, vel0, masses, dt, batch=batch, box=box.clone(), steps_per_replay=K, force_scale=fs, thermostat=th,
                               barostat=baro)
        legs["b_K10_isotropic"] = (iso, K)
        mds = [iso]
        for leg, coupling in (("b_K10_cell_anisotropic", "anisotropic"), ("b_K10_cell_semi_isotropic", "semi-isotropic")):
            md = model.capture_md_cell(z, pos, vel0, masses, dt, batch=batch, box=box.clone(), steps_per_replay=K, force_scale=fs,
                                       thermostat=th, barostat=dict(baro, coupling=coupling))
            mds.append(md)
            legs[leg] = (md, K)
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        for md in mds:
            md.check()  # raises if a trajectory overflowed or a move was unusable: its timings would be of a frozen loop
        entry = _summary(times)
        entry["n_atoms"] = n
        entry["volume_ratio_end"] = {"eager": float(torch.linalg.det(ebox).abs() / torch.linalg.det(box).abs()),
                                     "capture_md_cell": float(torch.linalg.det(mds[1].box).abs() / torch.linalg.det(box).abs())}
        iso_ms = entry["b_K10_isotropic"]["ms_per_step"]
        for leg in ("b_K10_cell_anisotropic", "b_K10_cell_semi_isotropic"):
            entry[leg]["us_per_step_over_isotropic"] = 1e3 * (entry[leg]["ms_per_step"] - iso_ms)
            entry[leg]["ratio_over_isotropic"] = entry[leg]["ms_per_step"] / iso_ms
            entry[leg]["ratio_over_eager_cell"] = entry[leg]["ms_per_step"] / entry["a_eager_cell"]["ms_per_step"]
        entry["cell_not_slower_than_eager"] = entry["b_K10_cell_anisotropic"]["ms_per_step"] <= entry["a_eager_cell"]["ms_per_step"]
        result["sizes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del replay, mds, legs
    out = a.out if a.out else os.path.join(ROOT, "profiles", "md_npt_cell.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def _count_sweeps(x, ref, rows, d2, cluster, n_clusters, tol, dt, velocity, limit=64):
    """The Gauss-Seidel iteration of csrc/tn_md_cons_math.h in fp64 torch on the host, for counting only: correcting sweeps per
    cluster until every constraint is within tolerance.  `rows`: per rank r the table rows of the r-th constraint of every cluster
    (different clusters share no atom, so relaxing a rank together IS the cluster's table order).  velocity: RATTLE on x = velocities
    at the positions `ref`; else SHAKE on x = positions with the saved positions `ref`.  -> sweeps [n_clusters] int64"""
    import torch

    sweeps = torch.zeros(n_clusters, dtype=torch.int64)
    for _ in range(limit):
        hit = torch.zeros(n_clusters, dtype=torch.bool)
        for sel, ia, ib, wa, wb in rows:
            s = ref[ia] - ref[ib]
            if velocity:
                rv = (s * (x[ia] - x[ib])).sum(1)
                bad = rv.abs() * dt > tol * d2[sel]
                g = -rv / ((wa + wb) * (s * s).sum(1))
            else:
                r = x[ia] - x[ib]
                diff = d2[sel] - (r * r).sum(1)
                bad = diff.abs() > 2.0 * tol * d2[sel]
                g = diff / (2.0 * (wa + wb) * (s * r).sum(1))
            g = torch.where(bad, g, torch.zeros_like(g))[:, None]
            x.index_add_(0, ia, g * wa[:, None] * s)
            x.index_add_(0, ib, -g * wb[:, None] * s)
            hit[cluster[sel][bad]] = True
        if not bool(hit.any()):
            break
        sweeps += hit
    return sweeps


def constraints_main(a):
    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import md as MD
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    dt, FS, K, kT, block_steps = 2.0, MD.FORCE_SCALE_EV_A_AMU_FS, 10, 0.0259, a.block_steps
    assert block_steps % K == 0
    result = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes", "steps_per_replay": K,
              "dt_fs": dt, "kT_of_the_velocities_eV": kT, "largest_initial_force_eV_per_A": 0.2, "steps_per_block": block_steps,
              "rounds": a.rounds, "sizes": {}}
    for name in ("water192", "synthetic64"):
        torch.manual_seed(0)
        if name == "water192":
            model = create_model(dict(W.C2_ARGS, static_shapes=True, max_num_neighbors=128)).to(dev)
            z, pos, box = W.water_box(n_side=4)
            pairs = MD.hydrogen_pairs(z, pos, rigid_water=True)
        else:
            model = create_model(dict(W.C2_ARGS, static_shapes=True, max_num_neighbors=64)).to(dev)
            z, pos, _ = W.synthetic_batch(n_mol=1, n_atoms=64)
            box = None
            pairs = MD.hydrogen_pairs(z, pos, cutoff=1.6)
        z, pos = z.to(dev), pos.to(dev).float().contiguous()
        box = None if box is None else box.to(dev).float().contiguous()
        n = int(z.shape[0])
        batch = torch.zeros_like(z)
        masses = torch.where(z == 1, 1.008, 12.0).float()
        # a state in which the atoms move: thermal velocities (300 K) and a 2 fs step; the random-weight model is no force field,
        # so its largest initial force counts as 0.2 eV / A (tests/test_gpu_md_constraints.py does the same)
        vel0 = (torch.sqrt(kT * FS / masses)[:, None] * torch.randn(n, 3, generator=torch.Generator().manual_seed(8)).to(dev)).float()
        replay = model.capture(z, pos, batch, box)
        _, forces = replay(pos)
        fs = FS * 0.2 / float(forces.abs().max())
        con = MD.prepare_constraints(dict(pairs=pairs), pos, batch, masses, 1)
        mds = {}
        for leg, c in (("b_K10_free", None), ("b_K10_constrained", dict(pairs=pairs))):
            mds[leg] = model.capture_md_constrained(z, pos, vel0, masses, dt, batch=batch, box=box, steps_per_replay=K, force_scale=fs,
                                                    constraints=c)
        mdc = mds["b_K10_constrained"]
        vel0p = mdc.vel.clone()  # projected onto the constraints: where every leg starts
        hk = mdc.hk[:, None]

        # ---- what the iteration has to do: its sweeps, counted on the host from the device's state in the middle of a block
        off = con["cluster_offsets"].long()
        cnt = (off[1:] - off[:-1])[:con["n_bound"]]
        cluster = torch.repeat_interleave(torch.arange(con["n_bound"]), cnt)
        rank = torch.cat([torch.arange(int(c)) for c in cnt]) if pairs.shape[0] else torch.zeros(0).long()
        table = pairs[con["order"]]
        d2 = con["constraint_d2"].double()
        w64 = 1.0 / masses.double().cpu()
        rows = []
        for r in range(int(rank.max()) + 1 if rank.numel() else 0):
            sel = (rank == r).nonzero().reshape(-1)
            rows.append((sel, table[sel, 0], table[sel, 1], w64[table[sel, 0]], w64[table[sel, 1]]))
        mdc(block_steps // K // 2)
        assert mdc.check() == block_steps // 2
        x0, v0, f0 = mdc.pos.clone(), mdc.vel.clone(), mdc.forces.clone()
        v_half = v0 + hk * f0
        x_free = x0 + dt * v_half  # after B, A: what SHAKE is given
        res, bound = MD.constraint_residuals(x_free, con["pairs"], con["lengths"], con["tol"])
        x64 = x_free.double().cpu()
        shake = _count_sweeps(x64, x0.double().cpu(), rows, d2, cluster, con["n_bound"], con["tol"], dt, False)
        x1 = x64.float().to(dev)
        _, f1 = replay(x1)
        v1 = v_half + ((x64 - x_free.double().cpu()) / dt).float().to(dev) + hk * f1
        rattle = _count_sweeps(v1.double().cpu(), x64.float().double(), rows, d2, cluster, con["n_bound"], con["tol"], dt, True)
        work = {"at_step": block_steps // 2, "residual_over_bound_before_shake": float((res / bound).max()),
                "shake_sweeps_per_cluster": {"mean": float(shake.double().mean()), "min": int(shake.min()), "max": int(shake.max())},
                "rattle_sweeps_per_cluster": {"mean": float(rattle.double().mean()), "min": int(rattle.min()), "max": int(rattle.max())}}
        sweeps = max(int(shake.max()), int(rattle.max()), 1)  # what a loop with a fixed number of sweeps needs

        # ---- the eager alternative: the constraints of rank r in their cluster form group r, relaxed together
        groups = []
        for sel, ia, ib, _, _ in rows:
            ia, ib = ia.to(dev), ib.to(dev)
            groups.append((ia, ib, con["constraint_d2"][sel].to(dev).float(), (1.0 / masses[ia])[:, None], (1.0 / masses[ib])[:, None]))
        vel = vel0p.clone()
        keep = pos.clone()

        def a_eager_shake():
            x = replay.pos
            keep.copy_(x)
            vel.addcmul_(hk, forces)
            x.add_(vel, alpha=dt)
            for _ in range(sweeps):
                for ia, ib, d2_, wa, wb in groups:
                    r, s = x[ia] - x[ib], keep[ia] - keep[ib]
                    g = ((d2_ - (r * r).sum(1)) / (2.0 * (wa + wb)[:, 0] * (s * r).sum(1)))[:, None]
                    x.index_add_(0, ia, g * wa * s)
                    x.index_add_(0, ib, -g * wb * s)
                    vel.index_add_(0, ia, g * wa * s / dt)
                    vel.index_add_(0, ib, -g * wb * s / dt)
            replay()
            vel.addcmul_(hk, forces)
            for _ in range(sweeps):
                for ia, ib, d2_, wa, wb in groups:
                    r, u = x[ia] - x[ib], vel[ia] - vel[ib]
                    k = (-(r * u).sum(1) / ((wa + wb)[:, 0] * (r * r).sum(1)))[:, None]
                    vel.index_add_(0, ia, k * wa * r)
                    vel.index_add_(0, ib, -k * wb * r)

        def restart_eager():
            vel.copy_(vel0p)
            replay(pos)

        legs = {"a_eager_shake": (a_eager_shake, 1, restart_eager)}
        for leg, md in mds.items():
            legs[leg] = (md, K, lambda md=md: md.reset(pos=pos, vel=vel0p))
        times = {k: [] for k in legs}
        ends = {}
        for rnd in range(a.rounds + 1):  # alternating blocks: every round visits every leg once; round 0 warms up
            for k, (fn, spc, restart) in legs.items():
                restart()  # every block walks the same block_steps steps from the same start, outside the clock
                sync()
                t0 = time.perf_counter()
                for _ in range(block_steps // spc):
                    fn()
                sync()
                t = time.perf_counter() - t0
                if rnd:
                    times[k].append(1e3 * t / block_steps)
                if k in mds:  # raises if the block overflowed or a cluster did not converge: it would have timed a frozen loop
                    assert mds[k].check() == block_steps
                ends[k] = (mds[k].pos if k in mds else replay.pos).clone()
        entry = _summary(times)
        entry["n_atoms"], entry["n_constraints"], entry["n_clusters"] = n, int(pairs.shape[0]), int(con["cluster_atoms"].shape[0])
        entry["iteration"] = work
        entry["eager_sweeps"] = sweeps
        entry["largest_displacement_end_A"] = float((ends["b_K10_constrained"] - pos).norm(dim=1).max())
        entry["residual_over_bound_end"] = {}
        for k, key in (("b_K10_constrained", "capture_md"), ("a_eager_shake", "eager"), ("b_K10_free", "unconstrained")):
            res, bound = MD.constraint_residuals(ends[k], con["pairs"], con["lengths"], con["tol"])
            entry["residual_over_bound_end"][key] = float((res / bound).max())
        entry["ns_per_day_constrained_at_2fs"] = 2.0 * entry["b_K10_constrained"]["ns_per_day_at_1fs"]
        entry["ratio_constrained_over_free"] = entry["b_K10_constrained"]["ms_per_step"] / entry["b_K10_free"]["ms_per_step"]
        entry["ratio_constrained_over_eager_shake"] = entry["b_K10_constrained"]["ms_per_step"] / entry["a_eager_shake"]["ms_per_step"]
        entry["b_K10_constrained_not_slower_than_eager"] = entry["b_K10_constrained"]["ms_per_step"] <= entry["a_eager_shake"]["ms_per_step"]
        result["sizes"][name] = entry
        print(name, json.dumps(entry), flush=True)
        del replay, mds, mdc, legs
    out = a.out if a.out else os.path.join(ROOT, "profiles", "md_constraints.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def remd_main(a):
    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import md as MD
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    dt, mass_amu, fs, friction, K, G, R, n = 1e-3, 12.0, MD.FORCE_SCALE_EV_A_AMU_FS, 0.01, 100, 8, 32, 64
    kT = MD.geometric_ladder(0.0259, 2.0 * 0.0259, R)
    torch.manual_seed(0)
    model = create_model(dict(W.C2_ARGS, static_shapes=True, max_num_neighbors=64)).to(dev)
    z, pos, _ = W.synthetic_batch(n_mol=1, n_atoms=n)
    z, pos = z.to(dev), pos.to(dev).float().contiguous()
    B = G * R
    masses = torch.full((n,), mass_amu, device=dev)
    pos_all = pos[None, None].repeat(G, R, 1, 1).contiguous()
    vel0 = torch.zeros_like(pos_all)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), n)
    legs, mds = {}, {}
    mds["capture_md"] = model.capture_md(z.repeat(B), pos_all.reshape(-1, 3), vel0.reshape(-1, 3), masses.repeat(B), dt, batch=batch,
                                         steps_per_replay=K, force_scale=fs, thermostat=dict(friction=friction, kT=float(kT[0]), seed=1))
    for X in (0, 10, 100):
        mds[f"remd_X{X}"] = model.capture_remd(z, pos_all, vel0, masses, dt, temperatures=kT, exchange_every=X, steps_per_replay=K,
                                               force_scale=fs, thermostat=dict(friction=friction, seed=1))
    for k, md in mds.items():
        legs[k] = (md, K)
    times = {k: [] for k in legs}
    for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
        for k, (fn, spc) in legs.items():
            times[k].append(_block(fn, spc, a.seconds, sync))
    for md in mds.values():
        md.check()  # raises if a trajectory overflowed: its timings would be of a frozen loop
    entry = _summary(times)
    base = entry["capture_md"]["ms_per_step"]
    entry["ratio_over_capture_md"] = {k: entry[k]["ms_per_step"] / base for k in entry if k.startswith("remd_")}
    entry["acceptance"] = {}
    for X in (10, 100):
        acc = mds[f"remd_X{X}"].acceptance()
        entry["acceptance"][f"remd_X{X}"] = {"attempts_per_pair": int(mds[f"remd_X{X}"].attempts.max()), "mean": float(acc.mean()),
                                             "min": float(acc.min()), "max": float(acc.max()), "matrix": acc.tolist()}
        print(f"acceptance [G,R-1], exchange_every = {X}:")
        for row in acc.tolist():
            print("  " + " ".join(f"{v:.2f}" for v in row))
    for k in legs:
        print(f"{k:12s} {entry[k]['ms_per_step']:.4f} ms/step  (min {entry[k]['min']:.4f}, max {entry[k]['max']:.4f})", flush=True)
    entry.update({"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes", "ladders": G,
                  "slots": R, "atoms_per_replica": n, "steps_per_replay": K, "seconds_per_block": a.seconds, "rounds": a.rounds,
                  "kT": kT.tolist()})
    out = a.out if a.out else os.path.join(ROOT, "profiles", "md_remd.json")
    result = {}
    if os.path.exists(out):
        with open(out) as fh:
            result = json.load(fh)
    result["timing"] = entry
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def bias_main(a):
    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import md as MD
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    dt, mass_amu, fs, K, n = 1e-3, 12.0, MD.FORCE_SCALE_EV_A_AMU_FS, 10, 64
    cvs = [("distance", 0, 1), ("angle", 1, 2, 3), ("torsion", 2, 3, 4, 5)]
    out = a.out if a.out else os.path.join(ROOT, "profiles", "md_bias.json")
    result = {}
    if os.path.exists(out):
        with open(out) as fh:
            result = json.load(fh)
    timing = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes", "steps_per_replay": K,
              "atoms_per_walker": n, "seconds_per_block": a.seconds, "rounds": a.rounds, "cvs": [list(c) for c in cvs], "sizes": {}}
    for B, Wg in ((1, 1), (256, 4)):
        torch.manual_seed(0)
        model = create_model(dict(W.C2_ARGS, static_shapes=True, max_num_neighbors=64)).to(dev)
        z1, pos1, _ = W.synthetic_batch(n_mol=1, n_atoms=n)
        z, pos = z1.to(dev).repeat(B), pos1.to(dev).float().repeat(B, 1).contiguous()
        batch = torch.repeat_interleave(torch.arange(B, device=dev), n)
        vel0 = torch.zeros_like(pos)
        masses = torch.full((B * n,), mass_amu, device=dev)
        G = B // Wg
        x1 = pos1.double()
        d0 = float((x1[0] - x1[1]).norm())
        res = [dict(cv=0, kappa=1.0, center=d0 + 0.05), dict(cv=1, kind="upper", kappa=1.0, center=1.0), dict(cv=2, kappa=0.5, center=0.3)]
        mds = {"capture_md": model.capture_md(z, pos, vel0, masses, dt, batch=batch, steps_per_replay=K, force_scale=fs)}
        mds["restraints"] = model.capture_md_biased(z, pos, vel0, masses, dt, batch=batch, steps_per_replay=K, force_scale=fs,
                                                    bias=dict(cvs=cvs, restraints=res))
        gen = torch.Generator().manual_seed(3)
        for nh in (0, 1000, 10000):
            metad = dict(cvs=[2, 0], sigma=[0.3, 0.1], height=0.01, pace=10 ** 9, kT=0.0259, bias_factor=8.0, walkers_per_group=Wg,
                         capacity=max(nh, Wg))
            md = model.capture_md_biased(z, pos, vel0, masses, dt, batch=batch, steps_per_replay=K, force_scale=fs,
                                         bias=dict(cvs=cvs, restraints=res, metad=metad))
            if nh:  # hills spread over the torsion's range and around the distance: every one of them is summed (no truncation)
                c = torch.stack([6.28 * torch.rand(G, nh, generator=gen, dtype=torch.float64) - 3.14,
                                 d0 + 0.3 * torch.randn(G, nh, generator=gen, dtype=torch.float64)], 2)
                md.reset(hills=(c, torch.full((G, nh), 1e-4, dtype=torch.float64)))
                assert md.n_hills == nh
            mds[f"metad_{nh}"] = md
        legs = {k: (md, K) for k, md in mds.items()}

        # ---- the eager alternative on capture(): a distance restraint, and 1 000 one-dimensional hills per group on the distance
        replay = model.capture(z, pos, batch)
        vel = vel0.clone()
        _, forces = replay(pos)
        ia, ib = torch.arange(B, device=dev) * n, torch.arange(B, device=dev) * n + 1
        hk = 0.5 * dt * fs / mass_amu
        hc = (d0 + 0.3 * torch.randn(G, 1000, generator=gen, dtype=torch.float64)).to(dev)
        hw = torch.full((G, 1000), 1e-4, dtype=torch.float64, device=dev)
        grp = torch.arange(B, device=dev) // Wg
        total = forces.clone()

        def eager(hills):
            def step():
                vel.add_(total, alpha=hk)
                replay.pos.add_(vel, alpha=dt)
                replay()
                x = replay.pos
                r = (x[ia] - x[ib]).double()
                s = r.norm(dim=1)
                dV = 1.0 * (s - (d0 + 0.05))
                if hills:
                    dl = s[:, None] - hc[grp]
                    dV = dV - (hw[grp] * torch.exp(-0.5 * (dl / 0.1) ** 2) * dl).sum(1) / 0.01
                f = (-(dV / s)[:, None] * r).float()
                total.copy_(forces)
                total.index_add_(0, ia, f)
                total.index_add_(0, ib, -f)
                vel.add_(total, alpha=hk)
            return step

        legs["eager_restraint"] = (eager(False), 1)
        legs["eager_metad_1000"] = (eager(True), 1)
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        for md in mds.values():
            md.check()  # raises if a trajectory froze: its timings would be of a loop that does nothing
        entry = _summary(times)
        base = entry["capture_md"]["ms_per_step"]
        entry["ratio_over_capture_md"] = {k: entry[k]["ms_per_step"] / base for k in entry if k != "capture_md"}
        entry["us_per_step_per_1000_hills"] = 1e3 * (entry["metad_10000"]["ms_per_step"] - entry["metad_0"]["ms_per_step"]) / 10.0
        entry["walkers"], entry["walkers_per_group"] = B, Wg
        timing["sizes"][f"{B}x{n}"] = entry
        for k in legs:
            print(f"{B:4d} x {n}  {k:18s} {entry[k]['ms_per_step']:.4f} ms/step  (min {entry[k]['min']:.4f}, max {entry[k]['max']:.4f})", flush=True)
        del replay, mds, legs
    result["timing"] = timing
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def global_main(a):
    import math

    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    dt, mass_amu, fs, kT, K = 1e-3, 12.0, 9.648533e-3, 0.0259, 10
    tau = 1000.0 * dt
    result = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS), static_shapes", "steps_per_replay": K,
              "seconds_per_block": a.seconds, "rounds": a.rounds, "dt_for_ns_per_day_fs": 1.0, "kT": kT, "tau": tau, "sizes": {}}
    for n in a.sizes:
        torch.manual_seed(0)
        model = create_model(dict(W.C2_ARGS, static_shapes=True, max_num_neighbors=64 if n <= 64 else 128)).to(dev)
        z, pos, batch = W.synthetic_batch(n_mol=1, n_atoms=n)
        z, pos, batch = z.to(dev), pos.to(dev), batch.to(dev)
        vel0 = torch.zeros_like(pos)
        masses = torch.full((n,), mass_amu, device=dev)
        hk = 0.5 * dt * fs / mass_amu
        ndof = 3 * n
        c = math.exp(-dt / tau)
        shape = torch.full((), 0.5 * (ndof - 1), device=dev)  # S = 2 Gamma((N - 1) / 2): chi-square with N - 1 degrees of freedom

        replay = model.capture(z, pos, batch)
        vel = vel0.clone()
        _, forces = replay(pos)

        def a_eager_csvr():
            vel.add_(forces, alpha=hk)
            replay.pos.add_(vel, alpha=dt)
            replay()
            vel.add_(forces, alpha=hk)
            ke = (vel * vel).sum() * (0.5 * mass_amu / fs)
            g = (0.5 * kT * (1.0 - c)) / ke
            r1 = torch.randn((), device=dev)
            a2 = (math.sqrt(c) + r1 * torch.sqrt(g)) ** 2 + g * 2.0 * torch._standard_gamma(shape)
            vel.mul_(torch.sqrt(a2))

        legs = {"a_eager_csvr": (a_eager_csvr, 1)}
        mds = [model.capture_md(z, pos, vel0, masses, dt, batch=batch, steps_per_replay=K, force_scale=fs,
                                thermostat=dict(friction=0.01, kT=kT, seed=1))]
        legs["b_K10_langevin"] = (mds[0], K)
        for leg, th in (("b_K10_csvr", dict(kind="csvr", kT=kT, tau=tau, seed=1)), ("b_K10_nose_hoover", dict(kind="nose-hoover", kT=kT, tau=tau))):
            md = model.capture_md_global(z, pos, vel0, masses, dt, batch=batch, steps_per_replay=K, force_scale=fs, thermostat=th)
            mds.append(md)
            legs[leg] = (md, K)
        times = {k: [] for k in legs}
        for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
            for k, (fn, spc) in legs.items():
                times[k].append(_block(fn, spc, a.seconds, sync))
        for md in mds:
            md.check()  # raises if a trajectory overflowed or a move was unusable: its timings would be of a frozen loop
        assert bool(torch.isfinite(vel).all())
        entry = _summary(times)
        entry["n_atoms"] = n
        base = entry["b_K10_langevin"]["ms_per_step"]
        entry["ratio_over_langevin"] = {k: entry[k]["ms_per_step"] / base for k in ("b_K10_csvr", "b_K10_nose_hoover")}
        entry["ratio_csvr_over_eager"] = entry["b_K10_csvr"]["ms_per_step"] / entry["a_eager_csvr"]["ms_per_step"]
        entry["b_K10_csvr_not_slower_than_eager"] = entry["b_K10_csvr"]["ms_per_step"] <= entry["a_eager_csvr"]["ms_per_step"]
        result["sizes"][str(n)] = entry
        print(n, json.dumps(entry), flush=True)
        del replay, mds, legs
    out = a.out if a.out else os.path.join(ROOT, "profiles", "md_global.json")
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
    ap.add_argument("--npt-cell", action="store_true", help="time the anisotropic cell barostat instead (profiles/md_npt_cell.json)")
    ap.add_argument("--constraints", action="store_true", help="time the constrained loop instead (profiles/md_constraints.json)")
    ap.add_argument("--remd", action="store_true", help="time temperature replica exchange instead (key 'timing' of profiles/md_remd.json)")
    ap.add_argument("--bias", action="store_true", help="time restraints and metadynamics instead (key 'timing' of profiles/md_bias.json)")
    ap.add_argument("--global", dest="global_", action="store_true", help="time the global thermostats instead (profiles/md_global.json)")
    ap.add_argument("--block-steps", type=int, default=100, help="--constraints: steps of one timed block (a multiple of 10)")
    ap.add_argument("--out", default=None, help="default: profiles/md_loop.json, with --npt profiles/md_npt.json, with --constraints "
                                                "profiles/md_constraints.json")
    a = ap.parse_args()
    if a.npt:
        return npt_main(a)
    if a.npt_cell:
        return npt_cell_main(a)
    if a.constraints:
        return constraints_main(a)
    if a.remd:
        return remd_main(a)
    if a.bias:
        return bias_main(a)
    if a.global_:
        return global_main(a)
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
