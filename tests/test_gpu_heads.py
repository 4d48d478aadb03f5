"""Property heads of TensorNet (DipoleMoment, ElectronicSpatialExtent) on the GPU: the reference's golden predictions, fixtures of
the unmodified reference (ragged batch with a one-atom molecule and an empty molecule id), and the paths those do not reach
(one large molecule, the cell list, an unsorted batch) against tests/heads_oracle.py."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HEADS = ("DipoleMoment", "ElectronicSpatialExtent")
REL = 1e-4


def rel_err(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


def _fixture(golden_dir):
    return torch.load(os.path.join(golden_dir, "heads_ref.pt"), weights_only=False)


def _model(case, **over):
    from torchmdnet_amd.models.model import create_model

    sd = case["state_dict"]
    m = create_model(dict(case["args"], **over), mean=sd["mean"], std=sd["std"])
    m.load_state_dict(sd)
    return m.to("cuda")


def _oracle(args, model, head, z, pos, batch, n_mol, box=None):
    from oracle import tensornet_torch as T
    from tests import heads_oracle as HO

    sd = {k: v.detach().to("cuda", torch.float64) if v.is_floating_point() else v.to("cuda") for k, v in model.state_dict().items()}
    hp = T.hparams_from_args(dict(args))
    y, f = HO.pred_and_forces(sd, hp, head, z.cuda(), pos.cuda().double(), batch.cuda(), n_mol,
                              None if box is None else box.cuda().double())
    return y.float().cpu(), f.float().cpu()


@pytest.mark.parametrize("head", HEADS)
def test_reference_golden_prediction(hip_lib, golden_dir, head):
    """tests/expected.pkl['tensornet'][head] of the reference (its test_forward_output)."""
    from oracle import ref_shims as R
    from torchmdnet_amd.models.model import create_model

    g = torch.load(os.path.join(golden_dir, f"expected_tensornet_{head.lower()}.pt"), weights_only=False)
    R.seed_everything(1234)
    model = create_model(dict(g["args"]))
    z, pos, batch = R.create_example_batch(n_atoms=5)
    assert torch.equal(z, g["z"]) and torch.equal(pos, g["pos"])
    pred, _ = model.to("cuda")(z.cuda(), pos.cuda(), batch.cuda())
    assert pred.shape == g["pred"].shape
    torch.testing.assert_close(pred.cpu(), g["pred"], atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("head", HEADS)
def test_fixture_pred_forces_and_edge_cases(hip_lib, golden_dir, head):
    g = _fixture(golden_dir)
    c = g["cases"][head]
    model = _model(c)
    y, f = model(g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda())
    y, f = y.cpu(), f.cpu()
    assert y.shape == (g["n_mol"], 1) and torch.isfinite(y).all() and torch.isfinite(f).all()
    assert rel_err(y, c["pred"]) < REL and rel_err(f, c["deriv"]) < REL
    # as close to the fp64 truth as the reference's own fp32 run (or within 1e-5 of it)
    for ours, ref32, ref64 in ((y, c["pred"], c["pred64"]), (f, c["deriv"], c["deriv64"])):
        assert rel_err(ours.double(), ref64) <= max(2 * rel_err(ref32.double(), ref64), 1e-5)
    mean = float(c["state_dict"]["mean"])
    empty = y[g["empty_mol"], 0].item()
    expect = abs(mean) * math.sqrt(3.0) if head == "DipoleMoment" else mean
    assert empty == pytest.approx(expect, rel=1e-6)
    one = (g["batch"] == g["single_atom_mol"]).nonzero().flatten()
    assert one.numel() == 1
    assert f[one].abs().max().item() < 1e-5
    if head == "DipoleMoment":
        assert y[g["single_atom_mol"], 0].item() == pytest.approx(abs(mean) * math.sqrt(3.0), rel=1e-5)


def _tiny_case(golden_dir, head):
    return _fixture(golden_dir)["cases"][head]


@pytest.mark.parametrize("head", HEADS)
def test_large_molecule_slices(hip_lib, golden_dir, head):
    """One 3000-atom molecule: N > 256 B, the sliced two-level reduction."""
    from torchmdnet_amd import workloads as W

    case = _tiny_case(golden_dir, head)
    model = _model(case)
    zz, pp = W.synthetic_molecule(4242, n_atoms=3000)
    z = torch.from_numpy(zz) % 19 + 1
    pos = torch.from_numpy(pp).float() + torch.tensor([40.0, -25.0, 60.0])
    batch = torch.zeros(3000, dtype=torch.long)
    y, f = model(z.cuda(), pos.cuda(), batch.cuda())
    yr, fr = _oracle(case["args"], model, head, z, pos, batch, 1)
    assert rel_err(y.cpu(), yr) < REL and rel_err(f.cpu(), fr) < REL


@pytest.mark.parametrize("head", HEADS)
def test_periodic_cell_list(hip_lib, golden_dir, head):
    """A single periodic system on the cell list (atoms renumbered internally: perm != NULL)."""
    from torchmdnet_amd import workloads as W

    case = _tiny_case(golden_dir, head)
    model = _model(case)
    model.cell_list_min_atoms = 1
    z, pos, box = W.water_box(n_side=6, spacing=3.1, seed=3)
    z = z % 19
    z[z == 0] = 1
    batch = torch.zeros(z.shape[0], dtype=torch.long)
    y, f = model(z.cuda(), pos.float().cuda(), batch.cuda(), box=box.float().cuda())
    assert model.cell_grid(z.shape[0], 1)[3] == 1, "the cell list did not run"
    yr, fr = _oracle(case["args"], model, head, z, pos.float(), batch, 1, box=box.float())
    assert rel_err(y.cpu(), yr) < REL and rel_err(f.cpu(), fr) < REL


@pytest.mark.parametrize("head", HEADS)
def test_unsorted_batch(hip_lib, golden_dir, head):
    g = _fixture(golden_dir)
    case = g["cases"][head]
    model = _model(case)
    gen = torch.Generator().manual_seed(5)
    p = torch.randperm(g["z"].shape[0], generator=gen)
    z, pos, batch = g["z"][p], g["pos"][p], g["batch"][p]
    y, f = model(z.cuda(), pos.cuda(), batch.cuda())
    yr, fr = _oracle(case["args"], model, head, z, pos, batch, g["n_mol"])
    assert rel_err(y.cpu(), yr) < REL and rel_err(f.cpu(), fr) < REL
    assert rel_err(y.cpu(), case["pred"]) < REL and rel_err(f.cpu(), case["deriv"][p]) < REL


@pytest.mark.parametrize("head", HEADS)
def test_rotation_invariance(hip_lib, golden_dir, head):
    g = _fixture(golden_dir)
    model = _model(g["cases"][head])
    if head == "DipoleMoment":  # mean is added to every component of the dipole: a fixed vector that does not rotate
        with torch.no_grad():
            model.mean.zero_()
    torch.manual_seed(3)
    Q, _ = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64))
    Q = Q.float()
    y0, f0 = model(g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda())
    y1, f1 = model(g["z"].cuda(), (g["pos"] @ Q).cuda(), g["batch"].cuda())
    assert rel_err(y1.cpu(), y0.cpu()) < REL
    assert rel_err(f1.cpu(), f0.cpu() @ Q) < REL


@pytest.mark.parametrize("head", HEADS)
def test_backward_matches_forces(hip_lib, golden_dir, head):
    g = _fixture(golden_dir)
    case = g["cases"][head]
    model = _model(case, derivative=False)
    pos = g["pos"].cuda().requires_grad_(True)
    y, _ = model(g["z"].cuda(), pos, g["batch"].cuda())
    y.sum().backward()
    assert rel_err(pos.grad.cpu(), -case["deriv"]) < REL


@pytest.mark.parametrize("head", HEADS)
def test_capture_replay(hip_lib, golden_dir, head):
    g = _fixture(golden_dir)
    model = _model(g["cases"][head], static_shapes=True)
    z, pos, batch = g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda()
    replay = model.capture(z, pos, batch, num_systems=g["n_mol"])
    moved = pos + 0.05 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(9)).cuda()
    ye, fe = model.energy_and_forces(z, moved, batch, None, None, g["n_mol"])
    yr, fr = replay(moved)
    torch.cuda.synchronize()
    assert rel_err(yr.view(-1).cpu(), ye.cpu()) < 1e-6 and rel_err(fr.cpu(), fe.cpu()) < 1e-6


def test_refusals(hip_lib, golden_dir):
    g = _fixture(golden_dir)
    model = _model(g["cases"]["DipoleMoment"])
    z, pos, batch = g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda()
    model.parameter_gradients = True
    with pytest.raises(NotImplementedError, match="has no HIP path"):
        model(z, pos, batch)
    model.parameter_gradients = False
    with pytest.raises(NotImplementedError):
        model.energy_and_forces(z, pos, batch, None, None, g["n_mol"], atom_weights=torch.ones(z.shape[0], device="cuda"))
    with pytest.raises(NotImplementedError):
        model.energy_and_forces(z, pos, batch, None, None, g["n_mol"], halo_exchange=lambda *a: None)
    y, f = model(z, pos, batch)  # the handle is still usable
    assert torch.isfinite(y).all() and torch.isfinite(f).all()


# ------------------------------------------------------------------------------------------------ Equivariant Transformer heads
ET_HEADS = HEADS + ("VectorOutput",)


def _et_fixture(golden_dir):
    return torch.load(os.path.join(golden_dir, "heads_et_ref.pt"), weights_only=False)


@pytest.mark.parametrize("head", HEADS)
def test_et_reference_golden_prediction(hip_lib, golden_dir, head):
    """tests/expected.pkl['equivariant-transformer'][head] of the reference (its test_forward_output)."""
    from oracle import ref_shims as R
    from torchmdnet_amd.models.model import create_model

    g = torch.load(os.path.join(golden_dir, f"expected_et_{head.lower()}.pt"), weights_only=False)
    R.seed_everything(1234)
    model = create_model(dict(g["args"]))
    z, pos, batch = R.create_example_batch(n_atoms=5)
    assert torch.equal(z, g["z"]) and torch.equal(pos, g["pos"])
    pred, _ = model.to("cuda")(z.cuda(), pos.cuda(), batch.cuda())
    torch.testing.assert_close(pred.cpu(), g["pred"], atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("head", ET_HEADS)
def test_et_fixture_pred_forces_and_edge_cases(hip_lib, golden_dir, head):
    g = _et_fixture(golden_dir)
    c = g["cases"][head]
    model = _model(c)
    y, f = model(g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda())
    y, f = y.cpu(), f.cpu()
    assert y.shape == (g["n_mol"], 3 if head == "VectorOutput" else 1) and y.shape == c["pred"].shape
    assert torch.isfinite(y).all() and torch.isfinite(f).all()
    assert rel_err(y, c["pred"]) < REL and rel_err(f, c["deriv"]) < REL
    for ours, ref32, ref64 in ((y, c["pred"], c["pred64"]), (f, c["deriv"], c["deriv64"])):
        assert rel_err(ours.double(), ref64) <= max(2 * rel_err(ref32.double(), ref64), 1e-5)
    mean = float(c["state_dict"]["mean"])
    expect = {"DipoleMoment": abs(mean) * math.sqrt(3.0), "ElectronicSpatialExtent": mean, "VectorOutput": mean}[head]
    assert y[g["empty_mol"]].tolist() == pytest.approx([expect] * y.shape[1], rel=1e-6)


@pytest.mark.parametrize("head", ET_HEADS)
def test_et_unsorted_batch(hip_lib, golden_dir, head):
    g = _et_fixture(golden_dir)
    c = g["cases"][head]
    model = _model(c)
    p = torch.randperm(g["z"].shape[0], generator=torch.Generator().manual_seed(5))
    y, f = model(g["z"][p].cuda(), g["pos"][p].cuda(), g["batch"][p].cuda())
    assert rel_err(y.cpu(), c["pred"]) < REL and rel_err(f.cpu(), c["deriv"][p]) < REL


def test_et_vector_equivariance(hip_lib, golden_dir):
    """The reference's tests/test_equivariance.py::test_vector_equivariance, restated: y(pos R) = y(pos) R."""
    g = _et_fixture(golden_dir)
    model = _model(g["cases"]["VectorOutput"])
    with torch.no_grad():
        model.mean.zero_()  # a mean added to every component is not a vector
    torch.manual_seed(4)
    Q, _ = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64))
    Q = Q.float()
    y0, f0 = model(g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda())
    y1, _ = model(g["z"].cuda(), (g["pos"] @ Q).cuda(), g["batch"].cuda())
    assert rel_err(y1.cpu(), y0.cpu() @ Q) < REL


@pytest.mark.parametrize("head", HEADS)
def test_et_rotation_invariance(hip_lib, golden_dir, head):
    g = _et_fixture(golden_dir)
    model = _model(g["cases"][head])
    if head == "DipoleMoment":
        with torch.no_grad():
            model.mean.zero_()
    torch.manual_seed(3)
    Q, _ = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64))
    Q = Q.float()
    y0, f0 = model(g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda())
    y1, f1 = model(g["z"].cuda(), (g["pos"] @ Q).cuda(), g["batch"].cuda())
    assert rel_err(y1.cpu(), y0.cpu()) < REL and rel_err(f1.cpu(), f0.cpu() @ Q) < REL


@pytest.mark.parametrize("head", ET_HEADS)
def test_et_backward_matches_forces(hip_lib, golden_dir, head):
    g = _et_fixture(golden_dir)
    c = g["cases"][head]
    model = _model(c, derivative=False)
    pos = g["pos"].cuda().requires_grad_(True)
    y, _ = model(g["z"].cuda(), pos, g["batch"].cuda())
    y.sum().backward()
    assert rel_err(pos.grad.cpu(), -c["deriv"]) < REL
    if head == "VectorOutput":  # a gradient that differs between the components is refused, not silently wrong
        pos.grad = None
        y, _ = model(g["z"].cuda(), pos, g["batch"].cuda())
        with pytest.raises(NotImplementedError):
            y[:, 0].sum().backward()


@pytest.mark.parametrize("head", ("DipoleMoment", "VectorOutput"))
def test_et_capture_replay(hip_lib, golden_dir, head):
    g = _et_fixture(golden_dir)
    model = _model(g["cases"][head], static_shapes=True)
    z, pos, batch = g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda()
    replay = model.capture(z, pos, batch, num_systems=g["n_mol"])
    moved = pos + 0.05 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(9)).cuda()
    ye, fe = model.energy_and_forces(z, moved, batch, None, None, g["n_mol"])
    yr, fr = replay(moved)
    torch.cuda.synchronize()
    assert rel_err(yr.reshape(-1).cpu(), ye.reshape(-1).cpu()) < 1e-6 and rel_err(fr.cpu(), fe.cpu()) < 1e-6


def test_et_refusals(hip_lib, golden_dir):
    g = _et_fixture(golden_dir)
    model = _model(g["cases"]["VectorOutput"])
    model.parameter_gradients = True
    with pytest.raises(NotImplementedError, match="has no HIP path"):
        model(g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda())


def test_mass_index_out_of_range_raises(hip_lib, golden_dir):
    """atomic_mass[z] of the reference raises IndexError for z >= 119 even where the embedding (max_z = 128) takes it."""
    from torchmdnet_amd.models.model import create_model

    args = dict(torch.load(os.path.join(golden_dir, "expected_tensornet_dipolemoment.pt"), weights_only=False)["args"], derivative=True)
    assert args["max_z"] > 120
    model = create_model(dict(args)).cuda()
    z = torch.tensor([1, 6, 120, 8], device="cuda")
    pos = torch.randn(4, 3, device="cuda")
    with pytest.raises(IndexError):
        model(z, pos, torch.zeros(4, dtype=torch.long, device="cuda"))
    z[2] = 7  # same tensor, new version: checked again
    y, f = model(z, pos, torch.zeros(4, dtype=torch.long, device="cuda"))
    assert torch.isfinite(y).all() and torch.isfinite(f).all()
