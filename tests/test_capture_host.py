"""No GPU: what every ``capture*`` method refuses on host tensors, with the exception type and the words of each refusal
(``TorchMD_Net._capture_inputs`` is the one prelude they share).  Every call is valid but for the one fault its row names, so the row
pins the type and text of that refusal and not the order of two."""
import pytest
import torch

from torchmdnet_amd import workloads as W
from torchmdnet_amd.models.model import create_model

N, M, R = 5, 3, 2  # atoms, NEB images, REMD temperatures


def _model(**over):
    torch.manual_seed(0)
    return create_model(dict(W.TINY_ARGS, **over))


def _calls():
    """name of the method -> (the name its messages carry, call(model, **over)); ``over`` overrides keyword arguments"""
    g = torch.Generator().manual_seed(3)
    z = torch.tensor([6, 1, 1, 8, 1])
    pos, vel = torch.randn(N, 3, generator=g), torch.zeros(N, 3)
    mass = torch.full((N,), 12.0)
    images = pos[None] + 0.1 * torch.arange(M, dtype=torch.float32)[:, None, None]
    replicas = pos[None].repeat(R, 1, 1)
    bias = dict(cvs=[("distance", 0, 1)], restraints=[dict(cv=0, kind="harmonic", kappa=1.0, center=1.0)])
    remd = dict(temperatures=[0.02, 0.03], exchange_every=2, steps_per_replay=2, thermostat=dict(friction=0.1, seed=1))
    return {
        "capture": ("capture", lambda m, **kw: m.capture(z, pos, **kw)),
        "capture_md": ("capture_md", lambda m, **kw: m.capture_md(z, pos, vel, mass, 0.01, **kw)),
        "capture_md_constrained": ("capture_md", lambda m, **kw: m.capture_md_constrained(
            z, pos, vel, mass, 0.01, constraints=dict(pairs=torch.tensor([[0, 1]])), **kw)),
        "capture_md_biased": ("capture_md", lambda m, **kw: m.capture_md_biased(z, pos, vel, mass, 0.01, bias=bias, **kw)),
        "capture_remd": ("capture_remd", lambda m, **kw: m.capture_remd(z, replicas, None, mass, 0.01, **dict(remd, **kw))),
        "capture_minimize": ("capture_minimize", lambda m, **kw: m.capture_minimize(z, pos, **kw)),
        "capture_neb": ("capture_neb", lambda m, **kw: m.capture_neb(z, images, **kw)),
    }


CALLS = _calls()
LOOPS = [k for k in CALLS if k != "capture"]
TAKES_WEIGHTS = [k for k in LOOPS if k != "capture_neb"]


@pytest.fixture(scope="module")
def models():
    made = dict(dynamic=_model(), static=_model(static_shapes=True), dipole=_model(static_shapes=True, output_model="DipoleMoment"))
    yield made
    for m in made.values():  # after every refusal of this module: nothing was created on the way
        st = m._engine
        assert st.handle is None and st.graph_ws is None and st.fwd_ws is None and st.virial_ws is None and st.generation == 0


@pytest.mark.parametrize("method", list(CALLS))
def test_a_dynamic_model_is_refused(models, method):
    name, call = CALLS[method]
    with pytest.raises(RuntimeError, match=rf"{name}\(\) needs a model created with static_shapes=True"):
        call(models["dynamic"])


@pytest.mark.parametrize("method", LOOPS)
def test_a_property_head_is_refused(models, method):
    with pytest.raises(NotImplementedError, match=r"DipoleMoment.*scalar head"):
        CALLS[method][1](models["dipole"])


@pytest.mark.parametrize("method", LOOPS)
def test_a_training_model_is_refused(models, method):
    model = models["static"]
    model.parameter_gradients = True
    try:
        with pytest.raises(NotImplementedError, match="parameter_gradients=True"):
            CALLS[method][1](model)
    finally:
        model.parameter_gradients = False


@pytest.mark.parametrize("method", LOOPS)
def test_no_steps_per_replay_is_refused(models, method):
    with pytest.raises(ValueError, match="steps_per_replay"):
        CALLS[method][1](models["static"], steps_per_replay=0)


@pytest.mark.parametrize("method", TAKES_WEIGHTS)
@pytest.mark.parametrize("extra", ["atom_weights", "halo_exchange"])
def test_domain_decomposition_is_refused(models, method, extra):
    value = torch.ones(N) if extra == "atom_weights" else (lambda *a: None)
    err = ValueError if method == "capture_remd" else NotImplementedError
    with pytest.raises(err):
        CALLS[method][1](models["static"], **{extra: value})


@pytest.mark.parametrize("method", list(CALLS))
def test_host_tensors_reach_the_device_refusal(models, method):
    """an otherwise valid call (``capture`` serves every head: with the property head too): the refusal names the method"""
    name, call = CALLS[method]
    with pytest.raises(RuntimeError, match=rf"{name} runs only on an AMD GPU"):
        call(models["static"])
    if method == "capture":
        with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):
            call(models["dipole"])
