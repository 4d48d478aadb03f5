#!/usr/bin/env python
"""A/B of the Hessian assembly: ms per whole Hessian (every molecule of the batch) of

  analytic  (a) ``a_loop``: the loop a caller can write today - D calls of ``force_term_parameter_gradients(want_hv=True)`` on the
                batch, one unit seed and one column of every molecule each, the columns stacked with torch;
            (b) ``b_hessian``: ``model.hessian(method="analytic")`` - R replicas per second-order pass, one graph build;
  central   (a) ``a_loop``: a torch loop over displaced ``model(...)`` calls, two per column;
            (b) ``b_hessian``: ``model.hessian(method="central")``,

for one 64-atom molecule and for 16 of them, TensorNet F = 128, L = 2.  Alternating blocks of (a) and (b) in one process, each block
at least ``--seconds`` of whole Hessians with the final synchronise inside the clock; median and min / max over ``--rounds`` blocks.
Also records max |H_analytic - H_central| / hmax per molecule.  Writes profiles/vibrations.json."""
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


def _block(fn, seconds, sync):
    """ms per call of one block: calls until `seconds` have passed, the synchronise inside the clock"""
    calls = 0
    t0 = time.perf_counter()
    while True:
        fn()
        calls += 1
        sync()
        t = time.perf_counter() - t0
        if t >= seconds:
            return 1e3 * t / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--delta", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vibrations.json"))
    a = ap.parse_args()

    import torch

    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    n = 64
    result = {"device": torch.cuda.get_device_name(dev), "model": "TensorNet F=128 L=2 (C2_ARGS)", "seconds_per_block": a.seconds,
              "rounds": a.rounds, "delta": a.delta, "sizes": {}}
    torch.manual_seed(0)
    model = create_model(dict(W.C2_ARGS)).to(dev)
    for B in (1, 16):
        z, pos, batch = W.synthetic_batch(n_mol=B, n_atoms=n)
        z, pos, batch = z.to(dev), pos.to(dev).float().contiguous(), batch.to(dev)
        N, D = B * n, 3 * n
        rows = torch.arange(B, device=dev) * n  # first atom of every molecule

        def analytic_loop():
            H = torch.empty((B, D, D), dtype=torch.float32, device=dev)
            v = torch.zeros((N, 3), dtype=torch.float32, device=dev)
            for k in range(D):
                v.zero_()
                v[rows + k // 3, k % 3] = 1.0
                _, hv = model.force_term_parameter_gradients(z, pos, batch, None, None, B, v, want_hv=True)
                H[:, :, k] = hv.view(B, D)
            return H

        def central_loop():
            H = torch.empty((B, D, D), dtype=torch.float32, device=dev)
            for k in range(D):
                xp, xm = pos.clone(), pos.clone()
                xp[rows + k // 3, k % 3] += a.delta
                xm[rows + k // 3, k % 3] -= a.delta
                fp, fm = model(z, xp, batch)[1].detach(), model(z, xm, batch)[1].detach()
                den = (xp[rows + k // 3, k % 3] - xm[rows + k // 3, k % 3]).detach().view(B, 1)  # (the forward marks its positions)
                H[:, :, k] = -(fp - fm).view(B, D) / den
            return H

        outs, entry = {}, {"n_mol": B, "n_atoms_per_molecule": n, "columns": D}
        for method, loop in (("analytic", analytic_loop), ("central", central_loop)):
            call = lambda m=method: model.hessian(z, pos, batch, method=m, delta=a.delta)
            H, info = call()
            outs[method], ref = H, loop()
            sync()
            legs = {"a_loop": loop, "b_hessian": call}
            times = {k: [] for k in legs}
            for _ in range(a.rounds):  # alternating blocks: every round visits every leg once
                for k, fn in legs.items():
                    times[k].append(_block(fn, a.seconds, sync))
            e = {k: {"ms_per_hessian": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
            e["replicas"], e["passes"], e["engine_calls"] = info["replicas"], info["passes"], info["engine_calls"]
            e["workspace_bytes"] = info["workspace_bytes"]
            e["ratio_b_over_a"] = e["b_hessian"]["ms_per_hessian"] / e["a_loop"]["ms_per_hessian"]
            e["max_abs_b_minus_a_over_hmax"] = float(((H - ref).abs().amax((1, 2)) / ref.abs().amax((1, 2))).max())
            entry[method] = e
            print(f"{B}x{n} {method}", json.dumps(e), flush=True)
        hmax = outs["analytic"].abs().amax((1, 2))
        entry["max_abs_analytic_minus_central_over_hmax"] = float(((outs["analytic"] - outs["central"]).abs().amax((1, 2)) / hmax).max())
        result["sizes"][f"{B}x{n}"] = entry
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
