"""ZBL prior: the Ziegler-Biersack-Littmark screened nuclear repulsion (reference torchmdnet/priors/zbl.py:11-112), the
short-range wall of a neural potential.  Same constructor arguments, ``get_init_args()``, buffers and state-dict keys as the
reference class; a parameter container only: the pair pass of csrc/tn_prior.hip evaluates it behind the model's energy and force
call (``TorchMD_Net.energy_and_forces``), nothing is evaluated in Python."""
import numpy as np
import torch

from torchmdnet_amd.models.utils import CosineCutoff, OptimizedDistance
from torchmdnet_amd.priors.atomref import BasePrior


class ZBL(BasePrior):
    """``atomic_number[z]`` is the atomic number of species z; ``distance_scale`` / ``energy_scale`` convert the dataset's lengths
    and energies to metres and Joules; each falls back to the attribute of the same name of ``dataset``.  ``max_num_neighbors``
    is kept as an init argument only: the pass builds no pair list, so none can overflow."""

    def __init__(self, cutoff_distance, max_num_neighbors, atomic_number=None, distance_scale=None, energy_scale=None, dataset=None):
        super().__init__()
        if atomic_number is None:
            atomic_number = dataset.atomic_number
        if distance_scale is None:
            distance_scale = dataset.distance_scale
        if energy_scale is None:
            energy_scale = dataset.energy_scale
        self.register_buffer("atomic_number", torch.as_tensor(atomic_number, dtype=torch.long))
        self.distance = OptimizedDistance(0, cutoff_distance, max_num_pairs=-max_num_neighbors)  # (its `box` buffer is a state-dict key)
        self.cutoff = CosineCutoff(cutoff_upper=cutoff_distance)
        self.cutoff_distance = cutoff_distance
        self.max_num_neighbors = max_num_neighbors
        self.distance_scale = float(distance_scale)
        self.energy_scale = float(energy_scale)

    def get_init_args(self):
        return {"cutoff_distance": self.cutoff_distance, "max_num_neighbors": self.max_num_neighbors,
                "atomic_number": self.atomic_number.tolist(), "distance_scale": self.distance_scale, "energy_scale": self.energy_scale}

    def reset_parameters(self):
        pass

    def post_reduce(self, y, z, pos, batch, box=None, extra_args=None):
        raise NotImplementedError("torchmdnet_amd.priors.ZBL is a parameter container: TorchMD_Net evaluates it in the HIP pair pass")

    def engine_key(self):
        """The plain attributes the engine's copy depends on (TorchMD_Net._fingerprint; the buffer is fingerprinted as a tensor)."""
        return ("ZBL", float(self.cutoff_distance), self.distance_scale, self.energy_scale)

    def species_tables(self, max_z):
        """fp32 tables over the species 0 .. max_z - 1, tabulated in fp64: (Z, Z^0.23); NaN past the end of ``atomic_number``."""
        Z = np.full(max_z, np.nan)
        an = self.atomic_number.detach().cpu().numpy().astype(np.float64)
        Z[:min(max_z, len(an))] = an[:max_z]
        with np.errstate(invalid="ignore"):
            return Z.astype(np.float32), np.power(Z, 0.23).astype(np.float32)
