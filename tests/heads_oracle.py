"""The TensorNet property heads restated in torch (reference output_modules.py:166-293, model.py:584-628) on top of the oracle's
representation (oracle/tensornet_torch.py): the checker for the paths the small fixtures do not reach (one large molecule, the
cell list, an unsorted batch).  Forces by autograd."""
import torch
import torch.nn.functional as Fn

from oracle import tensornet_torch as T


def head_output(sd, hp, head, z, pos, batch, n_mol, box=None):
    x = T.tensornet_representation(sd, hp, z, pos, batch, box)
    O = "output_model.output_network.layers."
    q = T.lin(Fn.silu(T.lin(x, sd, O + "0")), sd, O + "2") * sd["std"]  # [N,1]
    mass = sd["output_model.atomic_mass"].to(pos.dtype)[z].view(-1, 1)
    M = torch.zeros(n_mol, 1, dtype=pos.dtype, device=pos.device).index_add(0, batch, mass)
    mr = torch.zeros(n_mol, 3, dtype=pos.dtype, device=pos.device).index_add(0, batch, mass * pos)
    c = mr / torch.where(M > 0, M, torch.ones_like(M))
    d = pos - c[batch]
    if head == "DipoleMoment":
        mu = torch.zeros(n_mol, 3, dtype=pos.dtype, device=pos.device).index_add(0, batch, q * d) + sd["mean"]
        return torch.linalg.vector_norm(mu, dim=-1, keepdim=True)
    if head == "ElectronicSpatialExtent":
        return torch.zeros(n_mol, 1, dtype=pos.dtype, device=pos.device).index_add(0, batch, q * (d * d).sum(-1, keepdim=True)) + sd["mean"]
    raise ValueError(head)


def pred_and_forces(sd, hp, head, z, pos, batch, n_mol, box=None):
    pos = pos.detach().clone().requires_grad_(True)
    y = head_output(sd, hp, head, z, pos, batch, n_mol, box)
    (dy,) = torch.autograd.grad([y], [pos], grad_outputs=[torch.ones_like(y)])
    return y.detach(), -dy
