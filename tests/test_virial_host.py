"""Virial of the energy+force pass, without a GPU: the fp64 specification (tests/virial_oracle.py) against central differences, the
C ABI (new exports, revision unchanged) and the unchanged signatures of the existing Python surface."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("arch", ["tensornet", "et"])
@pytest.mark.parametrize("periodic", [False, True])
def test_strain_gradient_matches_central_differences(arch, periodic):
    """Two molecules (5 and 6 atoms); periodic: one triclinic box per molecule, small enough that the minimum image acts.  The strain
    gradient of the fp64 oracle agrees with central differences (step 1e-5: truncation ~1e-10 |E'''|, rounding ~1e-11 |E|) to 1e-7
    of max |W|, and is symmetric to rounding (rotation invariance of the energy)."""
    from tests import virial_oracle as VO
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    args = dict(W.TINY_ARGS if arch == "tensornet" else W.ET_TINY_ARGS, embedding_dimension=16, num_rbf=8)
    torch.manual_seed(3)
    model = create_model(dict(args))
    with torch.no_grad():
        model.std.fill_(1.7)
        model.mean.fill_(-0.4)
    sd = model.state_dict()
    g = torch.Generator().manual_seed(5)
    pos = torch.rand(11, 3, generator=g) * 4.0 + 20.0
    z = torch.randint(1, 9, (11,), generator=g)
    batch = torch.tensor([0] * 5 + [1] * 6)
    box = None
    if periodic:
        b0 = torch.tensor([[6.0, 0.0, 0.0], [0.8, 6.5, 0.0], [-0.5, 0.4, 7.0]])
        box = torch.stack([b0, b0 * 1.05])
    E, F, Wv = VO.energy_forces_virial(args, sd, z, pos, batch, box)
    Wfd = VO.virial_finite_difference(args, sd, z, pos, batch, box)
    scale = Wv.abs().max().item()
    assert scale > 0
    assert (Wv - Wfd).abs().max().item() / scale < 1e-7
    assert (Wv - Wv.transpose(1, 2)).abs().max().item() / scale < 1e-12
    # open molecules: W = sum_i r_i (x) F_i (translation invariance makes the origin irrelevant)
    if not periodic:
        ref = torch.zeros(2, 3, 3, dtype=torch.float64).index_add_(0, batch, pos.double().unsqueeze(2) * F.unsqueeze(1))
        assert (Wv - ref).abs().max().item() / scale < 1e-10


def test_header_and_library_export_the_virial_entries():
    from torchmdnet_amd import _C

    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert int(re.search(r"#define\s+TMDNET_ABI_VERSION\s+(\d+)", txt).group(1)) == 10  # nothing existing changed
    declared = _C.declared_symbols()
    for name in ("tmdnet_energy_forces_virial", "tmdnet_virial_workspace_bytes"):
        assert name in declared
    lib_path = os.path.join(ROOT, "torchmd-net_amd", "lib", "libtmdnet_amd.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as ge

        ge.build_hip(verbose=False)
    assert set(_C.check_symbols()) >= {"tmdnet_energy_forces_virial", "tmdnet_virial_workspace_bytes"}
    L = _C.lib()
    assert L.tmdnet_abi_version() == 10
    # the existing entry keeps its argument list; the new one is that list plus the scratch and the output
    assert len(L.tmdnet_energy_forces.argtypes) == 14
    assert len(L.tmdnet_energy_forces_virial.argtypes) == 17


def test_existing_python_surface_is_unchanged():
    from torchmdnet_amd.models.model import TorchMD_Net

    sig = inspect.signature(TorchMD_Net.energy_and_forces)
    names = list(sig.parameters)
    assert names[:11] == ["self", "z", "pos", "batch", "box", "q", "n_mol", "want_forces", "atom_weights", "halo_exchange", "cell_grid"]
    assert names[11:] == ["want_virial"] and sig.parameters["want_virial"].default is False
    assert sig.parameters["want_forces"].default is True
    assert all(sig.parameters[k].default is None for k in ("atom_weights", "halo_exchange", "cell_grid"))
    fwd = inspect.signature(TorchMD_Net.forward)
    assert list(fwd.parameters) == ["self", "z", "pos", "batch", "box", "q", "s", "extra_args", "num_systems"]
    assert all(fwd.parameters[k].default is None for k in list(fwd.parameters)[3:])
    cap = inspect.signature(TorchMD_Net.capture)
    assert list(cap.parameters) == ["self", "z", "pos", "batch", "box", "q", "num_systems", "warmup", "virial"]
    assert cap.parameters["virial"].default is False and cap.parameters["warmup"].default == 3
    efv = inspect.signature(TorchMD_Net.energy_forces_virial)
    assert list(efv.parameters) == ["self", "z", "pos", "batch", "box", "q", "num_systems"]


def test_stress_helper():
    from torchmdnet_amd.models.model import TorchMD_Net

    W = torch.arange(18, dtype=torch.float32).reshape(2, 3, 3)
    box = torch.tensor([[2.0, 0, 0], [0.5, 3.0, 0], [0.1, -0.2, 4.0]])
    s1 = TorchMD_Net.stress(W, box)
    assert torch.allclose(s1, -W / 24.0)
    s2 = TorchMD_Net.stress(W, torch.stack([box, 2 * box]))
    assert torch.allclose(s2[0], -W[0] / 24.0) and torch.allclose(s2[1], -W[1] / 192.0)


def test_operator_is_registered_with_a_fake_and_the_old_one_is_untouched():
    from torchmdnet_amd import ops  # noqa: F401

    new = torch.ops.tmdnet.energy_forces_virial.default
    assert str(new._schema) == ("tmdnet::energy_forces_virial(Tensor z, Tensor pos, Tensor batch, Tensor? box, Tensor? q, SymInt engine, "
                                "SymInt n_mol) -> (Tensor, Tensor, Tensor)")
    old = torch.ops.tmdnet.energy_forces.default
    assert str(old._schema) == ("tmdnet::energy_forces(Tensor z, Tensor pos, Tensor batch, Tensor? box, Tensor? q, SymInt engine, "
                                "SymInt n_mol, bool want_forces) -> (Tensor, Tensor)")
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        z = torch.zeros(7, dtype=torch.long, device="cuda")
        pos = torch.zeros(7, 3, device="cuda")
        e, f, w = torch.ops.tmdnet.energy_forces_virial(z, pos, z, None, None, 1, 3)
    assert e.shape == (3,) and f.shape == (7, 3) and w.shape == (3, 3, 3)
