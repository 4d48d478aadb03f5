"""No GPU: ``parse_lbfgs`` and what ``capture_minimize(lbfgs=...)`` refuses on host tensors before anything is staged, with the
exception type and the words of each refusal.  Every call is valid but for the one fault its row names.  (What the shared prelude
``TorchMD_Net._capture_inputs`` refuses for every captured loop is pinned by tests/test_capture_host.py; here it is shown to hold
with ``lbfgs=`` as well.)"""
import pytest
import torch

from torchmdnet_amd import workloads as W
from torchmdnet_amd.lbfgs import LBFGS_DEFAULTS, MAX_MEMORY, parse_lbfgs
from torchmdnet_amd.models.model import create_model

N = 5
NAN, INF = float("nan"), float("inf")


def _model(**over):
    torch.manual_seed(0)
    return create_model(dict(W.TINY_ARGS, **over))


@pytest.fixture(scope="module")
def models():
    made = dict(dynamic=_model(), static=_model(static_shapes=True), dipole=_model(static_shapes=True, output_model="DipoleMoment"))
    yield made
    for m in made.values():  # after every refusal of this module: nothing was created on the way
        st = m._engine
        assert st.handle is None and st.graph_ws is None and st.fwd_ws is None and st.virial_ws is None and st.generation == 0


def _call(model, **kw):
    g = torch.Generator().manual_seed(3)
    z = torch.tensor([6, 1, 1, 8, 1])
    kw.setdefault("lbfgs", {})
    return model.capture_minimize(z, torch.randn(N, 3, generator=g), **kw)


def test_parse_lbfgs_defaults_and_overrides():
    assert LBFGS_DEFAULTS == dict(memory=100, alpha=70.0, max_step=0.2, damping=1.0)  # ASE's
    assert parse_lbfgs({}) == LBFGS_DEFAULTS and parse_lbfgs(None) == LBFGS_DEFAULTS
    got = parse_lbfgs(dict(memory=7, damping=0.5))
    assert got == dict(memory=7, alpha=70.0, max_step=0.2, damping=0.5) and isinstance(got["memory"], int)
    assert parse_lbfgs(dict(memory=MAX_MEMORY))["memory"] == MAX_MEMORY and parse_lbfgs(dict(memory=1))["memory"] == 1


@pytest.mark.parametrize("bad,words", [(dict(history=3), "unknown keys"), (dict(memory=0), "memory"), (dict(memory=-4), "memory"),
                                       (dict(memory=MAX_MEMORY + 1), "memory"), (dict(memory=2.5), "integer"), (dict(alpha=0.0), "alpha"),
                                       (dict(alpha=-70.0), "alpha"), (dict(alpha=NAN), "alpha"), (dict(alpha=INF), "alpha"),
                                       (dict(max_step=0.0), "max_step"), (dict(max_step=-0.2), "max_step"), (dict(damping=0.0), "damping"),
                                       (dict(damping=-1.0), "damping"), (dict(damping=NAN), "damping")])
def test_parse_lbfgs_refuses(bad, words):
    with pytest.raises(ValueError, match=rf"lbfgs: .*{words}"):
        parse_lbfgs(bad)


def test_bad_lbfgs_parameters_are_refused_by_capture_minimize(models):
    with pytest.raises(ValueError, match="lbfgs: unknown keys"):
        _call(models["static"], lbfgs=dict(mem=3))
    with pytest.raises(ValueError, match="lbfgs: memory"):
        _call(models["static"], lbfgs=dict(memory=0))


def test_lbfgs_with_fire_is_refused(models):
    with pytest.raises(ValueError, match="lbfgs and fire exclude each other"):
        _call(models["static"], fire=dict(dt=0.1))
    with pytest.raises(ValueError, match="lbfgs and fire exclude each other"):
        _call(models["static"], fire={})


def test_lbfgs_with_cell_is_refused(models):
    with pytest.raises(NotImplementedError, match=r"lbfgs=.*cell"):
        _call(models["static"], cell={}, box=10.0 * torch.eye(3))


def test_fmax_and_fixed_are_checked(models):
    with pytest.raises(ValueError, match="fmax must be positive"):
        _call(models["static"], fmax=0.0)
    with pytest.raises(ValueError, match="fixed must have one entry per atom"):
        _call(models["static"], fixed=torch.zeros(3))


def test_the_shared_prelude_still_refuses(models):
    with pytest.raises(RuntimeError, match=r"capture_minimize\(\) needs a model created with static_shapes=True"):
        _call(models["dynamic"])
    with pytest.raises(NotImplementedError, match=r"DipoleMoment.*scalar head"):
        _call(models["dipole"])
    with pytest.raises(ValueError, match="steps_per_replay"):
        _call(models["static"], steps_per_replay=0)
    with pytest.raises(NotImplementedError):
        _call(models["static"], atom_weights=torch.ones(N))
    with pytest.raises(NotImplementedError):
        _call(models["static"], halo_exchange=lambda *a: None)
    model = models["static"]
    model.parameter_gradients = True
    try:
        with pytest.raises(NotImplementedError, match="parameter_gradients=True"):
            _call(model)
    finally:
        model.parameter_gradients = False
    with pytest.raises(RuntimeError, match="capture_minimize runs only on an AMD GPU"):
        _call(models["static"])  # an otherwise valid call on host tensors reaches the device refusal


def test_lbfgs_none_is_the_fire_path(models):
    """the default takes the FIRE branch: its own refusals, in its own words (the cell refusal of lbfgs= does not fire)"""
    with pytest.raises(ValueError, match="fire: unknown keys"):
        _call(models["static"], lbfgs=None, fire=dict(timestep=0.1))
    with pytest.raises(RuntimeError, match="capture_minimize runs only on an AMD GPU"):
        _call(models["static"], lbfgs=None, cell={}, box=10.0 * torch.eye(3))
