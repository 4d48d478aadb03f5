"""-m gpu: TensorNet2 + ScalarPlusWeightedCoulomb (AceFF-2.0) through the C ABI (tmdnet_create_tn2 + the shared
entry points) against fixtures written by the UNMODIFIED reference (oracle/make_golden_tn2.py) and the torch oracle
(oracle/tn2_torch.py, pinned to those fixtures at fp64 1e-10).  Tolerance: 1e-4 relative (fp32)."""
import os

import pytest
import torch

from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu
REL = 1e-4

TN2_TINY = dict(W.TINY_ARGS, model="tensornet2", output_model="ScalarPlusWeightedCoulomb", q_dim=8, q_weights=[1.0, 0.5, 2.0])


def rel_err(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


def _model_from_sd(args, sd):
    from torchmdnet_amd.models.model import create_model

    m = create_model(dict(args))
    m.load_state_dict(sd)
    return m.to("cuda")


def _compose(u):  # [N,9,F] irreducible components -> [N,3,3,F]
    from oracle import tensornet_adjoint as A

    return A.compose(u)


@pytest.mark.parametrize("fixture", ["tn2_tiny_ref.pt", "tn2_tiny_rf_ref.pt"])
def test_tn2_vs_reference_fixture(hip_lib, golden_dir, fixture):
    g = torch.load(os.path.join(golden_dir, fixture))
    model = _model_from_sd(g["args"], g["state_dict"])
    box = None if g["box"] is None else g["box"].cuda()
    z, pos, batch, q = g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda(), g["q"].cuda()
    E, F = model(z, pos, batch, box=box, q=q)
    n, Fh, L, qd = z.shape[0], g["args"]["embedding_dimension"], g["args"]["num_layers"], g["args"]["q_dim"]
    # intermediates first: they localise a failure
    assert rel_err(_compose(model.debug_tensor("X_embed", (n, 9, Fh)).cpu()), g["inter"]["X_embed"]) < REL
    chg = model.debug_tensor("charges", (n, (L + 1) * qd)).cpu()
    for l in range(L + 1):
        assert rel_err(chg[:, l * qd:(l + 1) * qd], g["inter"][f"charges_{l}"]) < REL, f"charges_{l}"
        if l < L:
            assert rel_err(_compose(model.debug_tensor(f"X_layer{l}", (n, 9, Fh)).cpu()), g["inter"][f"X_layer{l}"]) < REL, l
    assert rel_err(E.cpu(), g["E"]) < REL
    assert rel_err(F.cpu(), g["F"]) < REL
    assert rel_err(E.cpu().double(), g["E64"]) < REL and rel_err(F.cpu().double(), g["F64"]) < REL
    E2, F2 = model(z, pos, batch, box=box, q=q)
    assert torch.equal(E, E2) and torch.equal(F, F2)  # deterministic
    # energies only, and energy.backward()
    model.derivative = False
    with torch.no_grad():
        y, _ = model(z, pos, batch, box=box, q=q)
    assert rel_err(y.cpu(), g["E"]) < REL
    pg = pos.detach().clone().requires_grad_(True)
    y, _ = model(z, pg, batch, box=box, q=q)
    y.sum().backward()
    assert rel_err(-pg.grad.cpu(), g["F"]) < REL


def test_tn2_oracle_batch_tables_static_and_properties(hip_lib):
    """a batch large enough for the radial tables and the throughput kernels, SO(3) group, no total charges, static shapes +
    graph replay, zero net force, rotation equivariance; oracle = oracle/tn2_torch.py on sampled molecules."""
    from oracle import tn2_torch as T2
    from torchmdnet_amd.models.model import create_model

    for group in ("O(3)", "SO(3)"):
        args = dict(TN2_TINY, equivariance_invariance_group=group, embedding_dimension=64, max_z=20)
        torch.manual_seed(23)
        model = create_model(dict(args), mean=torch.tensor(0.5), std=torch.tensor(2.0)).to("cuda")
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        hp = T2.hparams_from_args(args)
        z, pos, batch = W.synthetic_batch(n_mol=40, n_atoms=30, first_seed=900)
        z = z % 19 + 1
        q = torch.randint(-1, 2, (40,)).float()
        E, F = model(z.cuda(), pos.cuda(), batch.cuda(), q=q.cuda())
        assert model.engine_info("edge_table_T") >= 8192
        for m_ in (0, 17, 39):
            sel = batch == m_
            Er, Fr = T2.energy_and_forces(sd, hp, z[sel], pos[sel], torch.zeros(int(sel.sum()), dtype=torch.long), q=q[m_:m_ + 1])
            assert rel_err(E[m_].cpu(), Er) < REL, (group, m_)
            assert rel_err(F[sel.cuda()].cpu(), Fr) < REL, (group, m_)
        net = torch.zeros(40, 3).index_add(0, batch, F.cpu())
        assert net.abs().max().item() < 1e-4 * F.abs().max().item() * 30
        model.set_engine_option("edge_table_min_pairs", 10 ** 12)  # direct GEMMs for the pair blocks
        Ed, Fd = model(z.cuda(), pos.cuda(), batch.cuda(), q=q.cuda())
        assert rel_err(Ed, E) < 2e-6 and rel_err(Fd, F) < 5e-6
    # rotation (proper + improper for O(3) was covered above by the group choice; here: proper rotation of the last model)
    rot = torch.tensor([[0.9886788, -0.1102370, 0.1017945], [0.1363630, 0.9431761, -0.3030248], [-0.0626055, 0.3134752, 0.9475304]])
    Er_, Fr_ = model(z.cuda(), (pos @ rot).cuda(), batch.cuda(), q=q.cuda())
    assert rel_err(Er_, Ed) < 2e-5 and rel_err(Fr_.cpu(), Fd.cpu() @ rot) < 2e-5
    # static shapes + HIP-graph replay
    sta = create_model(dict(args, static_shapes=True))
    sta.load_state_dict(model.state_dict())
    sta = sta.to("cuda")
    zs, ps, bs = z[:90].cuda(), pos[:90].cuda(), batch[:90].cuda()
    qs = q[:3].cuda()
    replay = sta.capture(zs, ps, bs, q=qs)
    for step in range(3):
        new = ps + 0.04 * step * torch.randn(ps.shape, generator=torch.Generator().manual_seed(step)).cuda()
        Es, Fs = replay(new)
        Er, Fr = model(zs, new.clone(), bs, q=qs)
        assert rel_err(Es, Er) < 1e-5 and rel_err(Fs, Fr) < 1e-5, step


# ---- shapes the whole-model tests above leave out: molecules longer than one 64-lane round of the Coulomb kernel, an unsorted
# batch, the reaction field through the cell list (kernel by kernel: tests/test_gpu_tn2_unit.py)
TN2_SMALL = dict(W.TINY_ARGS, model="tensornet2", output_model="ScalarPlusWeightedCoulomb", num_layers=1, q_dim=4, q_weights=[1.0, 0.5],
                 max_num_neighbors=128)
RAGGED = (1, 2, 65, 130)


def _oracle64(model, args, z, pos, batch, box=None, q=None):
    """oracle/tn2_torch.py in float64 on the model's weights -> (E [B, 1], F [N, 3], charges [N, (L + 1) q_dim])"""
    from oracle import tn2_torch as T2

    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}
    p = pos.double().clone().requires_grad_(True)
    inter = {}
    y = T2.energy(sd, T2.hparams_from_args(args), z, p, batch, None if box is None else box.double(), None if q is None else q.double(),
                  inter=inter)
    (dy,) = torch.autograd.grad(y.sum(), p)
    return y.detach(), -dy, inter["charges"].detach()


def _ragged_batch():
    import numpy as np

    zs, ps = zip(*[W.synthetic_molecule(700 + m, n) for m, n in enumerate(RAGGED)])
    z, pos = torch.from_numpy(np.concatenate(zs)), torch.from_numpy(np.concatenate(ps))
    batch = torch.repeat_interleave(torch.arange(len(RAGGED)), torch.tensor(RAGGED))
    return z, pos, batch, torch.tensor([1.0, -1.0, 0.0, 2.0])


def _per_molecule(got, ref, batch, what):
    """every molecule on its own, relative to its own largest reference entry; a molecule whose reference vanishes (the force on
    a lone atom) relative to the batch's largest"""
    top = ref.abs().max().item()
    for m in range(int(batch.max()) + 1):
        sel = batch == m
        scale = ref[sel].abs().max().item()
        err = (got[sel].double() - ref[sel]).abs().max().item() / (scale if scale > 1e-6 * top else top)
        assert err < REL, (what, m, err)


def test_tn2_ragged_all_to_all_batch_and_permuted_batch(hip_lib):
    """molecules of 1, 2, 65 and 130 atoms with total charges: the Coulomb kernel's second and partial third 64-lane round, the
    equilibration with more atoms than groups; then the same atoms permuted (an unsorted `batch`: counts[3] = 1, every
    per-molecule kernel scans all atoms and filters by `batch`)."""
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(31)
    model = create_model(dict(TN2_SMALL), mean=torch.tensor(0.3), std=torch.tensor(1.5)).to("cuda")
    z, pos, batch, q = _ragged_batch()
    n, B, QC = z.shape[0], len(RAGGED), 2 * TN2_SMALL["q_dim"]
    Er, Fr, chr_ = _oracle64(model, TN2_SMALL, z, pos, batch, q=q)
    E, F = model(z.cuda(), pos.cuda(), batch.cuda(), q=q.cuda())
    assert model.graph_counts()[2] == 0
    chg = model.debug_tensor("charges", (n, QC)).cpu()
    _per_molecule(chg, chr_, batch, "charges")
    _per_molecule(E.cpu(), Er, torch.arange(B), "energy")
    _per_molecule(F.cpu(), Fr, batch, "forces")
    net = torch.zeros(B, 3).index_add(0, batch, F.cpu())
    assert net.abs().max().item() < 1e-4 * F.abs().max().item() * max(RAGGED)
    assert abs(chg[batch == 3][:, :4].sum(0) - 2.0).max().item() < 1e-4  # the charges of a molecule add up to its total charge
    # the same atoms in another order
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    assert bool((batch[perm][1:] < batch[perm][:-1]).any())
    Ep, Fp = model(z[perm].cuda(), pos[perm].cuda(), batch[perm].cuda(), q=q.cuda())
    assert model.graph_counts()[2] == 1, "the permuted batch was not taken as unsorted"
    assert rel_err(Ep, E) < 1e-5 and rel_err(Fp.cpu(), F.cpu()[perm]) < 1e-5
    _per_molecule(Ep.cpu(), Er, torch.arange(B), "energy, permuted")
    _per_molecule(Fp.cpu(), Fr[perm], batch[perm], "forces, permuted")
    _per_molecule(model.debug_tensor("charges", (n, QC)).cpu(), chr_[perm], batch[perm], "charges, permuted")


@pytest.mark.parametrize("n_mol", [1, 2])
def test_tn2_reaction_field_through_the_cell_list(hip_lib, n_mol):
    """coulomb_cutoff = 6.0 on one periodic water box whose neighbours come from the cell list.  4 x 4 x 4 waters are a box of
    12.4 A: the smallest this generator makes that is at least twice the Coulomb cutoff wide (two cells per axis).  With two
    molecules sharing the box (every other water) the cell order interleaves them: counts[3] = 1, the Coulomb kernel filters by
    the internal batch, and its forces come back to the caller's order through the permutation."""
    from torchmdnet_amd.models.model import create_model

    args = dict(TN2_SMALL, coulomb_cutoff=6.0)
    torch.manual_seed(37)
    model = create_model(dict(args)).to("cuda")
    z, pos, box = W.water_box(n_side=4, seed=3)
    n = z.shape[0]
    assert float(box[0, 0]) >= 2 * args["coulomb_cutoff"] and W.water_box(n_side=3)[2][0, 0] < 2 * args["coulomb_cutoff"]
    if n_mol == 2:  # even waters, then odd waters: `batch` is sorted for the caller, the molecules interleave in space
        water = torch.arange(n) // 3
        order = torch.cat([torch.nonzero(water % 2 == 0).flatten(), torch.nonzero(water % 2 == 1).flatten()])
        z, pos = z[order], pos[order]
        batch = (torch.arange(n) >= int((water % 2 == 0).sum())).long()
        q = torch.tensor([1.0, -1.0])
    else:
        batch, q = torch.zeros(n, dtype=torch.long), torch.tensor([1.0])
    Er, Fr, chr_ = _oracle64(model, args, z, pos, batch, box=box, q=q)
    model.cell_list_min_atoms = 1
    E, F = model(z.cuda(), pos.cuda(), batch.cuda(), box=box.cuda(), q=q.cuda())
    assert model.cell_grid(n, n_mol)[3] == 1, "the cell list did not run"
    assert model.graph_counts()[2] == (1 if n_mol == 2 else 0)
    _per_molecule(E.cpu(), Er, torch.arange(n_mol), "energy")
    _per_molecule(F.cpu(), Fr, batch, "forces")
    # and brute force gives the same
    model.cell_list_min_atoms = 10 ** 9
    Eb, Fb = model(z.cuda(), pos.cuda(), batch.cuda(), box=box.cuda(), q=q.cuda())
    assert model.cell_grid(n, n_mol)[3] == 0
    assert rel_err(E, Eb) < 1e-5 and rel_err(F, Fb) < 1e-5
