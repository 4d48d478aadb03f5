"""Property heads (DipoleMoment, ElectronicSpatialExtent on TensorNet and the Equivariant Transformer, EquivariantVectorOutput):
model assembly, state dict, mass table, checkpoint loading and the C ABI, without a GPU."""
import os
import re
import warnings

import pytest
import torch

from oracle import ref_shims as R

HEADS = ("DipoleMoment", "ElectronicSpatialExtent")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


CASES = [("tensornet", h) for h in HEADS] + [("equivariant-transformer", h) for h in HEADS + ("VectorOutput",)]


def _example_args(model_name, head):
    """The reference's example arguments (examples/*-QM9.yaml through tests/utils.py), as recorded in the golden files."""
    short = "tensornet" if model_name == "tensornet" else "et"
    g = torch.load(os.path.join(ROOT, "tests", "golden", f"expected_{short}_dipolemoment.pt"), weights_only=False)
    return dict(g["args"], output_model=head)


@pytest.mark.parametrize("model_name,head", CASES)
def test_create_model_builds_the_head(model_name, head):
    from torchmdnet_amd.models import output_modules
    from torchmdnet_amd.models.model import create_model

    args = _example_args(model_name, head)
    model = create_model(dict(args))
    name = ("Equivariant" if model_name == "equivariant-transformer" else "") + head  # reference model.py:134
    assert type(model.output_model) is getattr(output_modules, name)
    assert model._head_kind() != 0 and not model.output_model.allow_prior_model


def test_vector_output_needs_the_equivariant_transformer():
    from torchmdnet_amd.models.model import create_model

    args = _example_args("tensornet", "VectorOutput")
    with pytest.raises(NotImplementedError):
        create_model(dict(args))


@pytest.mark.parametrize("model_name,head", CASES)
def test_state_dict_matches_the_reference(golden_dir, model_name, head):
    from torchmdnet_amd.models.model import create_model

    et = model_name != "tensornet"
    g = torch.load(os.path.join(golden_dir, "heads_et_ref.pt" if et else "heads_ref.pt"), weights_only=False)["cases"][head]
    torch.manual_seed(11 + (5 if et else 0) + (HEADS + ("VectorOutput",)).index(head))
    model = create_model(dict(g["args"]), mean=g["state_dict"]["mean"], std=g["state_dict"]["std"])
    sd = model.state_dict()
    assert set(sd) == set(g["state_dict"])
    for k, v in g["state_dict"].items():
        assert torch.equal(sd[k], v), k
    if R.reference_available():
        mm = R.reference_model_module()
        args = R.load_example_args(model_name, remove_prior=True, output_model=head, derivative=True)
        R.seed_everything(1234)
        ref = mm.create_model(dict(args)).state_dict()
        R.seed_everything(1234)
        ours = create_model(dict(args)).state_dict()
        assert set(ref) == set(ours) and all(torch.equal(ref[k], ours[k]) for k in ref)


def test_mass_table_equals_the_recorded_buffer(golden_dir):
    from torchmdnet_amd.atomic_masses import atomic_masses

    rec = torch.load(os.path.join(golden_dir, "heads_ref.pt"), weights_only=False)["cases"]["DipoleMoment"]["state_dict"]
    buf = rec["output_model.atomic_mass"]
    ours = torch.from_numpy(atomic_masses).to(buf.dtype)
    assert ours.shape == buf.shape == (119,)
    assert torch.equal(ours, buf)
    assert atomic_masses[0] == 1.0 and atomic_masses[6] == 12.011 and atomic_masses[8] == 15.999


def test_load_model_lightning_checkpoint(tmp_path, golden_dir):
    from torchmdnet_amd.models.model import load_model

    g = torch.load(os.path.join(golden_dir, "heads_ref.pt"), weights_only=False)["cases"]["DipoleMoment"]
    sd = dict(g["state_dict"])
    sd["output_model.atomic_mass"] = sd["output_model.atomic_mass"] * 1.5  # a checkpoint's own masses win
    path = str(tmp_path / "dipole.ckpt")
    torch.save(dict(hyper_parameters=dict(g["args"]), state_dict={"model." + k: v for k, v in sd.items()}), path)
    model = load_model(path)
    assert type(model.output_model).__name__ == "DipoleMoment"
    for k, v in sd.items():
        assert torch.equal(model.state_dict()[k], v), k


def test_tensornet2_dipole_is_refused_and_prior_dropped():
    from torchmdnet_amd.models.model import create_model
    from torchmdnet_amd.priors import Atomref

    args = _example_args("tensornet", "DipoleMoment")
    with pytest.raises(NotImplementedError):
        create_model(dict(args, model="tensornet2"))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        model = create_model(dict(args), prior_model=Atomref(max_z=100))
    assert model.prior_model is None
    assert any("Dropping the prior model" in str(x.message) for x in w)


def test_abi_10_and_set_output_head_symbol(hip_lib):
    from torchmdnet_amd import _C

    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert int(re.search(r"#define\s+TMDNET_ABI_VERSION\s+(\d+)", txt).group(1)) == 10
    assert "tmdnet_set_output_head" in _C.declared_symbols()
    assert hasattr(hip_lib, "tmdnet_set_output_head")
    assert hip_lib.tmdnet_abi_version() == 10


def test_set_output_head_parameter_lists(hip_lib):
    """tmdnet_set_output_head changes the handle's parameter list (host only: no GPU call)."""
    import ctypes as C

    from torchmdnet_amd import _C

    hp = _C.EtHParams(hidden_channels=32, num_layers=2, num_rbf=16, max_z=20, max_num_neighbors=32, num_heads=4,
                      neighbor_embedding=1, vector_cutoff=0, distance_influence=3, has_atomref=0, cutoff_lower=0.0, cutoff_upper=5.0)
    h = C.c_void_p()
    assert hip_lib.tmdnet_create_et(C.byref(hp), C.byref(h)) == _C.OK
    try:
        names = lambda: [hip_lib.tmdnet_param_name(h, i, None).decode() for i in range(hip_lib.tmdnet_num_params(h))]
        scalar = names()
        assert hip_lib.tmdnet_set_output_head(h, _C.HEAD_DIPOLE_MOMENT) == _C.OK
        assert set(names()) - set(scalar) == {"output_model.atomic_mass"}
        assert hip_lib.tmdnet_set_output_head(h, _C.HEAD_SPATIAL_EXTENT) == _C.OK
        mlp = "output_model.output_network.layers."
        assert set(names()) - set(scalar) == {mlp + "0.weight", mlp + "0.bias", mlp + "2.weight", mlp + "2.bias", "output_model.atomic_mass"}
        assert not any(n.startswith("output_model.output_network.0.") for n in names())
        assert hip_lib.tmdnet_set_output_head(h, _C.HEAD_VECTOR) == _C.OK
        assert set(names()) == set(scalar)
        assert hip_lib.tmdnet_set_output_head(h, 7) == _C.ERR_INVALID
    finally:
        hip_lib.tmdnet_destroy(h)
