"""TEST INFRASTRUCTURE ONLY -- what the rounding-aware mode of the ET oracle (oracle/et_torch.py, ``pair_rows="bf16"``) can and
cannot tell apart, measured on the oracle alone (fp64, CPU):

  effect  relative max-norm difference of the forces between the rounded and the unrounded oracle: what a kernel that forgot to
          round its rows (or rounded only the values) would be off by;
  floor   the same difference between the rounded oracle and itself with every row element perturbed BEFORE rounding by a
          uniform relative error of +-2^-22 plus +-2^-22 of the row tensor's largest magnitude.  This stands in for the engine's
          table interpolation and fp32 rounding (about 1e-7 of the rows): a few elements round the other way, and each flip is
          a whole bf16 ulp of that element.

A bound between 4 x floor and effect / 2 passes a correct engine and fails one that rounds differently.  Systems: all nine cases
of tests/test_gpu_et.py::test_et_tile_sweeps_vs_oracle that have distance influence (the GPU test compares on every one of
them), same seeds, the first two molecules of each.  The floor is a random quantity (which elements flip): the perturbation's
seed is fixed, and other seeds move a case's floor by up to +-30 %.
tools/et_bf16_oracle_floor.py records the figures in profiles/et_bf16_oracle_floor.json; tests/test_oracle.py recomputes them."""
import torch

from oracle import et_torch as ET

# (n_mol, n_atoms, cutoff_upper, distance_influence, vector_cutoff, num_heads): test_et_tile_sweeps_vs_oracle without the "none" case
TILE_CASES = [
    (5, 64, 10.0, "both", True, 8),
    (5, 64, 10.0, "keys", False, 4),
    (5, 64, 10.0, "values", True, 16),
    (7, 32, 5.0, "both", True, 8),
    (6, 64, 4.0, "both", False, 8),
    (4, 48, 10.0, "both", True, 8),
    (3, 100, 6.0, "both", True, 8),
    (9, 40, 10.0, "both", True, 8),
    (11, 21, 10.0, "both", False, 8),
]
PERTURB = 2.0 ** -22


def case_name(case):
    n_mol, n_atoms, rc, di, vc, H = case
    return f"{n_mol}x{n_atoms}_rc{rc:g}_{di}_{'vc' if vc else 'ac'}_h{H}"


def tile_case_model(case):
    """(args, fp32 state dict on the host) of a tile-sweep case: the weights of test_et_tile_sweeps_vs_oracle (seed 5)."""
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    _, _, rc, di, vc, H = case
    args = dict(W.C4_ARGS, num_layers=2, num_heads=H, distance_influence=di, vector_cutoff=vc, cutoff_upper=rc)
    torch.manual_seed(5)
    model = create_model(dict(args))
    return args, {k: v.detach().cpu() for k, v in model.state_dict().items()}


def f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def perturbed_rounding(seed):
    """bf16_rne of x (1 + u 2^-22) + u' 2^-22 max|x| with u, u' uniform in [-1, 1]: a stand-in for rows computed in fp32."""
    gen = torch.Generator().manual_seed(seed)

    def rnd(x):
        u = 2 * torch.rand(x.shape, generator=gen, dtype=x.dtype) - 1
        w = 2 * torch.rand(x.shape, generator=gen, dtype=x.dtype) - 1
        return ET.bf16_rne(x * (1 + PERTURB * u) + PERTURB * x.abs().max() * w)

    return rnd


def rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


def measure(case, n_mol=2, seed=1):
    """{"effect", "floor"} of one case: the first ``n_mol`` molecules of its batch evaluated together, differences relative to
    the largest force component of the batch."""
    from torchmdnet_amd import workloads as W

    args, sd = tile_case_model(case)
    sd, hp = f64(sd), ET.hparams_from_args(args)
    z, pos, batch = W.synthetic_batch(n_mol=n_mol, n_atoms=case[1], first_seed=300)
    pos = pos.double()
    _, F0 = ET.energy_and_forces(sd, hp, z, pos, batch)
    _, Fr = ET.energy_and_forces(sd, hp, z, pos, batch, pair_rows="bf16")
    _, Fp = ET.energy_and_forces(sd, hp, z, pos, batch, pair_rows=perturbed_rounding(seed))
    return {"effect": rel(Fr, F0), "floor": rel(Fp, Fr)}
