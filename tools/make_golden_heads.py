"""Generate the property heads' fixtures in tests/golden/ from the UNMODIFIED reference (build machine only: needs the reference
checkout that oracle/ref_shims.py imports).

    python tools/make_golden_heads.py

  expected_{tensornet,et}_{dipolemoment,electronicspatialextent}.pt
      the reference's own golden predictions tests/expected.pkl["tensornet"][head]["pred"] + the inputs its recipe generates
      (tests/test_model.py:282-329), as expected_tensornet_scalar.pt
  heads_ref.pt, heads_et_ref.pt
      the TINY TensorNet / the TINY Equivariant Transformer with each property head (VectorOutput on the ET only), std != 1 and
      mean != 0, on a ragged batch with a one-atom molecule and a molecule id without atoms: weights
      (atomic_mass included), pred / deriv in fp32, and the fp64 weights-cast truth
"""
import os
import pickle
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "torchmd-net_amd"))

from oracle import ref_shims as R  # noqa: E402
from torchmdnet_amd import workloads as W  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
HEADS = ("DipoleMoment", "ElectronicSpatialExtent")
ET_HEADS = HEADS + ("VectorOutput",)


def sd_checksum(sd):
    return float(sum(v.double().abs().sum() for v in sd.values() if v.is_floating_point()))


def heads_batch():
    """Molecules 0 (9 atoms), 1 (one atom), 3 (14 atoms); id 2 has no atoms.  Coordinates away from the origin."""
    zs, ps, bs = [], [], []
    for m, n, seed in ((0, 9, 301), (1, 1, 302), (3, 14, 303)):
        zz, pp = W.synthetic_molecule(seed, n_atoms=n)
        zs.append(torch.from_numpy(zz) % 19 + 1)
        ps.append(torch.from_numpy(pp) + torch.tensor([7.5, -3.0, 12.0]) * (m + 1))
        bs.append(torch.full((n,), m, dtype=torch.long))
    return torch.cat(zs), torch.cat(ps).float(), torch.cat(bs)


def run(model, z, pos, batch):
    y, f = model(z, pos.clone(), batch)
    return y.detach(), f.detach()


def main():
    mm = R.reference_model_module()
    warnings.simplefilter("ignore")
    with open(os.path.join(R.REFERENCE_ROOT, "tests", "expected.pkl"), "rb") as fh:
        expected = pickle.load(fh)
    for model_name, short, head in [("tensornet", "tensornet", h) for h in HEADS] + [("equivariant-transformer", "et", h) for h in HEADS]:
        R.seed_everything(1234)
        # derivative=False, as the reference's test_forward_output for a property head: its golden vector has no deriv
        args = R.load_example_args(model_name, remove_prior=True, output_model=head, derivative=False)
        model = mm.create_model(args)
        z, pos, batch = R.create_example_batch(n_atoms=5)
        y, _ = run(model, z, pos, batch)
        exp = expected[model_name][head]
        assert (y - exp["pred"]).abs().max() < 1e-5, (model_name, head, (y - exp["pred"]).abs().max())
        torch.save(dict(args=args, z=z, pos=pos.detach(), batch=batch, pred=exp["pred"].detach(),
                        sd_checksum=sd_checksum(model.state_dict())),
                   os.path.join(OUT, f"expected_{short}_{head.lower()}.pt"))

    z, pos, batch = heads_batch()
    cases = {}
    for key, base, k, head in ([(h, W.TINY_ARGS, k, h) for k, h in enumerate(HEADS)] +
                               [("et:" + h, W.ET_TINY_ARGS, 5 + k, h) for k, h in enumerate(ET_HEADS)]):
        torch.manual_seed(11 + k)
        args = dict(base, output_model=head, derivative=True, prior_model=None)
        mean, std = torch.tensor(0.37 - 0.5 * (k % 5)), torch.tensor(1.7 + 0.4 * (k % 5))
        model = mm.create_model(dict(args), mean=mean, std=std)
        sd = {kk: v.detach().clone() for kk, v in model.state_dict().items()}
        y, f = run(model, z, pos, batch)
        m64 = mm.create_model(dict(args, precision=64), mean=mean.double(), std=std.double())
        m64.load_state_dict({kk: (v.double() if v.is_floating_point() else v) for kk, v in sd.items()})
        y64, f64 = run(m64, z, pos.double(), batch)
        cases[key] = dict(args=args, state_dict=sd, pred=y, deriv=f, pred64=y64, deriv64=f64)
    for fn, pre in (("heads_ref.pt", None), ("heads_et_ref.pt", "et:")):
        sel = {k[len(pre or ""):]: v for k, v in cases.items() if k.startswith("et:") == (pre is not None)}
        torch.save(dict(z=z, pos=pos, batch=batch, n_mol=4, empty_mol=2, single_atom_mol=1, cases=sel), os.path.join(OUT, fn))
    for fn in sorted(os.listdir(OUT)):
        if "dipole" in fn or "spatial" in fn or fn.startswith("heads_"):
            print(fn, os.path.getsize(os.path.join(OUT, fn)))


if __name__ == "__main__":
    main()
