"""fp64 specification of the virial (helper of test_virial_host.py / test_gpu_virial.py; checker only, never imported by the product).

Autograd of the existing oracles through a per-molecule homogeneous strain, row-vector convention:
    pos -> pos (I + eps[batch]),  box -> box (I + eps)        eps [B,3,3]
    W_m = - d E_m / d eps_m |_(eps = 0)
A single box shared by all molecules is expanded to one box per molecule first (the oracles take [B,3,3] boxes), so that every
molecule is strained by its own eps together with "its" copy of the box; E_m depends on eps_m only, so one backward of sum_m E_m
gives every W_m.  The minimum-image shifts stay fixed: `torch.round` has no gradient, and the box rows it multiplies carry the
strain.  The strained box is no longer lower triangular; the oracle's minimum image reads the diagonal for the shift counts only, so
at eps = 0 nothing changes but the derivative.
"""
import torch

from oracle import et_torch as ET, tensornet_torch as T


def _module(args):
    return ET if args["model"] == "equivariant-transformer" else T


def _energy(args, sd, z, pos, batch, box, n_mol, q=None):
    mod = _module(args)
    hp = mod.hparams_from_args(args)
    if mod is ET:
        return mod.energy(sd, hp, z, pos, batch, box=box, num_systems=n_mol)
    return mod.energy(sd, hp, z, pos, batch, box=box, q=q, num_systems=n_mol)


def energy_forces_virial(args, sd, z, pos, batch, box=None, num_systems=None, q=None, dtype=torch.float64):
    """(E [B,1], F [N,3], W [B,3,3]) of the oracle in `dtype` (fp64: the specification; fp32: what the reference arithmetic alone
    reaches)."""
    n_mol = int(batch.max()) + 1 if num_systems is None else int(num_systems)
    sd = T.cast_state_dict({k: v.detach().cpu() for k, v in sd.items()}, dtype)
    z, batch = z.cpu(), batch.cpu()
    p0 = pos.detach().cpu().to(dtype).requires_grad_(True)
    eps = torch.zeros(n_mol, 3, 3, dtype=dtype, requires_grad=True)
    strain = torch.eye(3, dtype=dtype) + eps
    p = torch.einsum("na,nab->nb", p0, strain[batch])
    b = None
    if box is not None:
        b = box.detach().cpu().to(dtype)
        if b.dim() == 2:
            b = b.unsqueeze(0).expand(n_mol, 3, 3)
        b = b @ strain
    qq = None if q is None else q.detach().cpu().to(dtype)
    E = _energy(args, sd, z, p, batch, b, n_mol, qq)
    g_pos, g_eps = torch.autograd.grad(E.sum(), [p0, eps])
    return E.detach(), -g_pos, -g_eps


def energy_gradients(args, sd, z, pos, batch, box, seed, num_systems=None, dtype=torch.float64):
    """d (sum_m seed_m E_m) / d pos and / d box by plain autograd of the oracle (`box` [3,3] or [B,3,3], as given)."""
    n_mol = int(batch.max()) + 1 if num_systems is None else int(num_systems)
    sd = T.cast_state_dict({k: v.detach().cpu() for k, v in sd.items()}, dtype)
    p = pos.detach().cpu().to(dtype).requires_grad_(True)
    b = box.detach().cpu().to(dtype).requires_grad_(True)
    E = _energy(args, sd, z.cpu(), p, batch.cpu(), b, n_mol)
    g_pos, g_box = torch.autograd.grad((E.reshape(-1) * seed.detach().cpu().to(dtype).reshape(-1)).sum(), [p, b])
    return g_pos, g_box


def virial_finite_difference(args, sd, z, pos, batch, box=None, num_systems=None, h=1e-5):
    """Central differences of the fp64 oracle energy in every strain component of every molecule (tiny systems only)."""
    n_mol = int(batch.max()) + 1 if num_systems is None else int(num_systems)
    dtype = torch.float64
    sd = T.cast_state_dict({k: v.detach().cpu() for k, v in sd.items()}, dtype)
    p0 = pos.detach().cpu().to(dtype)
    b0 = None if box is None else box.detach().cpu().to(dtype)
    if b0 is not None and b0.dim() == 2:
        b0 = b0.unsqueeze(0).expand(n_mol, 3, 3)

    def e_of(eps):
        strain = torch.eye(3, dtype=dtype) + eps
        with torch.no_grad():
            return _energy(args, sd, z, torch.einsum("na,nab->nb", p0, strain[batch]), batch, None if b0 is None else b0 @ strain,
                           n_mol).reshape(-1)

    W = torch.zeros(n_mol, 3, 3, dtype=dtype)
    for a in range(3):
        for c in range(3):
            eps = torch.zeros(n_mol, 3, 3, dtype=dtype)
            eps[:, a, c] = h  # every molecule at once: E_m depends on its own strain only
            W[:, a, c] = -(e_of(eps) - e_of(-eps)) / (2 * h)
    return W
