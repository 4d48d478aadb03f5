"""D2 prior: the dispersion tail of DFT-D2 (Grimme, J. Comput. Chem. 27, 1787, 2006; reference torchmdnet/priors/d2.py:11-201).
Same constructor arguments, ``get_init_args()``, buffers and state-dict keys as the reference class; a parameter container only:
the pair pass of csrc/tn_prior.hip evaluates it behind the model's energy and force call, nothing is evaluated in Python.  The
C6 / R_r table is the paper's Table 1 (data), copied as a table."""
import numpy as np
import torch

from torchmdnet_amd.models.utils import OptimizedDistance
from torchmdnet_amd.priors.atomref import BasePrior

nan = float("nan")
# C6 (J/mol nm^6) and van der Waals radius (Angstrom) of the elements H .. Xe; row 0 has no element
_C6_RR = [
    [nan, nan],
    [0.14, 1.001], [0.08, 1.012], [1.61, 0.825], [1.61, 1.408], [3.13, 1.485], [1.75, 1.452], [1.23, 1.397], [0.70, 1.342],
    [0.75, 1.287], [0.63, 1.243], [5.71, 1.144], [5.71, 1.364], [10.79, 1.639], [9.23, 1.716], [7.84, 1.705], [5.57, 1.683],
    [5.07, 1.639], [4.61, 1.595], [10.80, 1.485], [10.80, 1.474], [10.80, 1.562], [10.80, 1.562], [10.80, 1.562], [10.80, 1.562],
    [10.80, 1.562], [10.80, 1.562], [10.80, 1.562], [10.80, 1.562], [10.80, 1.562], [10.80, 1.562], [16.99, 1.650], [17.10, 1.727],
    [16.37, 1.760], [12.64, 1.771], [12.47, 1.749], [12.01, 1.727], [24.67, 1.628], [24.67, 1.606], [24.67, 1.639], [24.67, 1.639],
    [24.67, 1.639], [24.67, 1.639], [24.67, 1.639], [24.67, 1.639], [24.67, 1.639], [24.67, 1.639], [24.67, 1.639], [24.67, 1.639],
    [37.32, 1.672], [38.71, 1.804], [38.44, 1.881], [31.74, 1.892], [31.50, 1.892], [29.99, 1.881],
]


class D2(BasePrior):
    """``atomic_number[z]`` is the atomic number of species z; ``distance_scale`` / ``energy_scale`` convert the dataset's lengths
    and energies to metres and Joules (not J/mol); each falls back to the attribute of the same name of ``dataset``.  The cutoff is
    hard and the prior never sees the box, as in the reference.  ``max_num_neighbors`` is kept as an init argument only: the pass
    builds no pair list, so none can overflow."""

    C_6_R_r = torch.tensor(_C6_RR, dtype=torch.float64)
    C_6_R_r[:, 1] *= 0.1  # Angstrom -> nm

    def __init__(self, cutoff_distance, max_num_neighbors, atomic_number=None, distance_scale=None, energy_scale=None, dataset=None,
                 dtype=torch.float32):
        super().__init__()
        one = torch.tensor(1.0, dtype=dtype).item()
        self.cutoff_distance = cutoff_distance * one
        self.max_num_neighbors = int(max_num_neighbors)
        self.C_6_R_r = self.C_6_R_r.to(dtype=dtype)
        self.atomic_number = list(dataset.atomic_number if atomic_number is None else atomic_number)
        self.distance_scale = one * (dataset.distance_scale if distance_scale is None else distance_scale)
        self.energy_scale = one * (dataset.energy_scale if energy_scale is None else energy_scale)
        self.distances = OptimizedDistance(cutoff_lower=0, cutoff_upper=self.cutoff_distance, max_num_pairs=-self.max_num_neighbors)
        self.register_buffer("Z_map", torch.tensor(self.atomic_number, dtype=torch.long))
        self.register_buffer("C_6", self.C_6_R_r[:, 0])
        self.register_buffer("R_r", self.C_6_R_r[:, 1])
        self.d = 20
        self.s_6 = 1

    def reset_parameters(self):
        pass

    def get_init_args(self):
        return {"cutoff_distance": self.cutoff_distance, "max_num_neighbors": self.max_num_neighbors,
                "atomic_number": self.atomic_number, "distance_scale": self.distance_scale, "energy_scale": self.energy_scale}

    def post_reduce(self, y, z, pos, batch, box=None, extra_args=None):
        raise NotImplementedError("torchmdnet_amd.priors.D2 is a parameter container: TorchMD_Net evaluates it in the HIP pair pass")

    def engine_key(self):
        """The plain attributes the engine's copy depends on (TorchMD_Net._fingerprint; the buffers are fingerprinted as tensors)."""
        return ("D2", float(self.cutoff_distance), float(self.distance_scale), float(self.energy_scale))

    def species_tables(self, max_z):
        """fp32 tables over the species 0 .. max_z - 1, tabulated in fp64 from the buffers: (sqrt C6, R_r); NaN for a species past
        the end of ``atomic_number``, or whose element has no row in the table."""
        zmap = self.Z_map.detach().cpu().numpy()
        c6, rr = self.C_6.detach().cpu().double().numpy(), self.R_r.detach().cpu().double().numpy()
        out = np.full((2, max_z), np.nan)
        for s in range(min(max_z, len(zmap))):
            if 0 <= zmap[s] < len(c6):
                out[0, s], out[1, s] = np.sqrt(c6[zmap[s]]), rr[zmap[s]]
        return out[0].astype(np.float32), out[1].astype(np.float32)

    def check_species(self, z):
        """Refuse the species of ``z`` that have no table entry (element 0, or beyond Xe): the reference returns NaN energies or
        raises an IndexError for them.  Called on the host when a new ``z`` is staged."""
        if not z.numel():
            return
        sq, _ = self.species_tables(int(z.max()) + 1)
        bad = sorted({int(s) for s in z.detach().cpu().reshape(-1).tolist() if s < 0 or np.isnan(sq[s])})
        if bad:
            raise NotImplementedError(f"D2: species {bad} have no C6 / R_r table entry (atomic_number maps them to "
                                      f"{[self.atomic_number[s] if 0 <= s < len(self.atomic_number) else None for s in bad]}; the table "
                                      "covers H .. Xe)")
