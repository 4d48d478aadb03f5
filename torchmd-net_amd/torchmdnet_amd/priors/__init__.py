from torchmdnet_amd.priors.atomref import Atomref, BasePrior
from torchmdnet_amd.priors.d2 import D2
from torchmdnet_amd.priors.zbl import ZBL

__all__ = ["Atomref", "D2", "ZBL"]

# the pair pass (csrc/tn_prior.hip) is brute force inside a molecule: TMDNET_PRIOR_MAX_MOLECULE_ATOMS of include/tmdnet_amd.h
MAX_MOLECULE_ATOMS = 32768


def check_molecule_size(n_atoms_largest):
    """The size test of the pair pass, on the host: ``n_atoms_largest`` is the atom count of the largest molecule."""
    if int(n_atoms_largest) > MAX_MOLECULE_ATOMS:
        raise NotImplementedError(f"the ZBL / D2 pair pass is brute force inside a molecule and serves at most {MAX_MOLECULE_ATOMS} "
                                  f"atoms per molecule, got {int(n_atoms_largest)}; the cell-list variant of the pass is the follow-up")
