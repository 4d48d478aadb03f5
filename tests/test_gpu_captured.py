"""-m gpu: what the captured loops share (torchmdnet_amd/captured.py, TorchMD_Net._capture_inputs), on every loop variant.

1. staleness: once the engine's parameter block or workspaces are re-created, a replay, a reset and a run raise instead of touching
   freed memory - and nothing is replayed
2. input lifetime: a loop captured from temporaries replays the bits of one captured from kept-alive, already-converted inputs
3. box identity: a box that moves is the caller's own tensor when it needed no conversion; the model's own box is never written"""
import pytest
import torch

from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

K = 2
SIZES = [9, 14, 5, 20, 11]  # the ragged 5-molecule system
VARIANTS = ["md", "md_constrained", "md_biased", "remd", "minimize", "minimize_cell", "neb"]
# the method a stale loop names: the constrained, the biased and the replica-exchange loop are DeviceMD objects and say capture_md
NAMES = dict(md="capture_md", md_constrained="capture_md", md_biased="capture_md", remd="capture_md", minimize="capture_minimize",
             minimize_cell="capture_minimize", neb="capture_neb")


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _model(**over):
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(4)
    return create_model(dict(W.TINY_ARGS, static_shapes=True, **over)).to("cuda")


def _system():
    """-> z, pos, batch, vel, mass, q, box [5,3,3] (device); molecule m sits 3 A further along the diagonal"""
    zs, ps, bs = [], [], []
    for m, n in enumerate(SIZES):
        z, p = W.synthetic_molecule(40 + m, n)
        zs.append(torch.from_numpy(z))
        ps.append(torch.from_numpy(p) + 3.0 * m)
        bs.append(torch.full((n,), m, dtype=torch.long))
    z, pos, batch = torch.cat(zs).cuda(), torch.cat(ps).cuda(), torch.cat(bs).cuda()
    vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    mass = torch.where(z == 1, 1.008, 12.0).float()
    box = (30.0 * torch.eye(3, device="cuda")).repeat(len(SIZES), 1, 1).contiguous()
    return z, pos, batch, vel, mass, torch.zeros(len(SIZES), device="cuda"), box


def _one_molecule(z, pos, batch, mass, m=3):
    sel = batch == m
    return z[sel], pos[sel], mass[sel]


def _capture(kind, model):
    z, pos, batch, vel, mass, q, box = _system()
    md = dict(batch=batch, q=q, steps_per_replay=K, warmup=1)
    if kind == "md":
        return model.capture_md(z, pos, vel, mass, 0.01, **md)
    if kind == "md_constrained":
        return model.capture_md_constrained(z, pos, vel, mass, 0.01, thermostat=dict(friction=0.1, kT=0.01, seed=1),
                                            constraints=dict(pairs=torch.tensor([[0, 1]])), **md)
    if kind == "md_biased":
        bias = dict(cvs=[("distance", 0, 1)], restraints=[dict(cv=0, kind="harmonic", kappa=1.0, center=1.5)])
        return model.capture_md_biased(z, pos, vel, mass, 0.01, bias=bias, **md)
    if kind == "minimize":
        return model.capture_minimize(z, pos, batch=batch, q=q, steps_per_replay=K, fmax=1e-6, warmup=1)
    if kind == "minimize_cell":
        return model.capture_minimize(z, pos, batch=batch, box=box, q=q, steps_per_replay=K, fmax=1e-6, warmup=1, cell={})
    z1, p1, m1 = _one_molecule(z, pos, batch, mass)
    shift = 0.05 * torch.randn(p1.shape, generator=torch.Generator().manual_seed(9)).cuda()
    if kind == "remd":
        return model.capture_remd(z1, torch.stack([p1, p1 + shift]), None, m1, 0.01, temperatures=[0.02, 0.03], exchange_every=K,
                                  q=q[:1], steps_per_replay=K, thermostat=dict(friction=0.1, seed=1), warmup=1)
    images = torch.stack([p1, p1 + shift, p1 + 2 * shift])  # one band of 3 images
    return model.capture_neb(z1, images, q=q[:1], steps_per_replay=K, fmax=1e-6, warmup=1)


class _NeverReplayed:
    """stands in for the graph once the engine has changed: the guard has to raise before it gets here"""

    def replay(self):
        raise AssertionError("a stale graph was replayed")


def _grow(model):
    zb, pb, bb = W.synthetic_batch(n_mol=40, n_atoms=60)
    model(zb.cuda() % 19 + 1, pb.cuda(), bb.cuda())  # a larger system: the workspaces grow


def _change_parameters(model):
    with torch.no_grad():
        model.std.mul_(2.0)
    z, pos, batch = _system()[:3]
    model(z, pos, batch)  # parameter change + eager call: the handle is re-created


# ------------------------------------------------------------------------------------------------ 1. staleness
@pytest.mark.parametrize("kind,route", [(k, _grow) for k in VARIANTS] + [("md", _change_parameters), ("minimize", _change_parameters)],
                         ids=lambda v: v if isinstance(v, str) else v.__name__.strip("_"))
def test_a_stale_loop_raises_and_replays_nothing(hip_lib, kind, route):
    model = _model()
    obj = _capture(kind, model)
    obj()
    assert obj.check() == K == obj.steps_done
    route(model)
    graph, obj.graph = obj.graph, _NeverReplayed()  # (the real graph stays alive, unreplayed, until the test ends)
    stale = rf"stale HIP graph.*{NAMES[kind]}\(\)"
    with pytest.raises(RuntimeError, match=stale):
        obj()
    with pytest.raises(RuntimeError, match=stale):
        obj.reset()
    if hasattr(obj, "run"):
        assert not bool((obj.converged_at >= 0).all())  # run() has something to do
        with pytest.raises(RuntimeError, match=stale):
            obj.run(2)
    assert obj.steps_done == K
    del graph


# ------------------------------------------------------------------------------------------------ 2. input lifetime
@pytest.mark.parametrize("kind", ["md", "minimize"])
def test_temporaries_are_staged_and_kept_alive(hip_lib, kind):
    model = _model()
    z, pos, batch, vel, mass, q, box = _system()
    n, B = z.shape[0], len(SIZES)

    def capture(z, batch, box, q):
        if kind == "md":
            return model.capture_md(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, steps_per_replay=K, warmup=1)
        return model.capture_minimize(z, pos, batch=batch, box=box, q=q, steps_per_replay=K, warmup=1)

    ref = capture(z, batch, box, q)  # kept alive, already what the engine takes
    ref()
    want = [t.clone() for t in (ref.pos, ref.forces, ref.epot)]
    assert ref.check() == K
    tmp = capture(z.int(), batch.to(torch.int32), box.double(), torch.zeros(B, dtype=torch.float64, device="cuda") + 0.0)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    junk = [torch.full((n,), 7, dtype=torch.long, device="cuda") for _ in range(3)]  # the sizes of z and batch,
    junk += [torch.full((B, 3, 3), 1e3, device="cuda"), torch.full((B,), 5.0, device="cuda")]  # of box and of q
    junk += [torch.full((n,), 3, dtype=torch.int32, device="cuda"), torch.full((B, 3, 3), 1e3, dtype=torch.float64, device="cuda")]
    tmp()
    assert tmp.check() == K
    for got, exp in zip((tmp.pos, tmp.forces, tmp.epot), want):
        assert _bits(got, exp)
    assert all(t.dtype == d for t, d in zip(tmp.inputs, (torch.long, torch.long, torch.float32, torch.float32)))
    del junk


# ------------------------------------------------------------------------------------------------ 3. box identity
BARO = dict(pressure=0.0, tau=10.0, compressibility=1e-3, kT=0.0)


def _moving_box(model, kind, box, one=False):
    z, pos, batch, vel, mass, q, _ = _system()
    if one:
        z, pos, mass = _one_molecule(z, pos, batch, mass)
        batch, vel, q = torch.zeros_like(z), vel[:z.shape[0]], q[:1]
    if kind == "barostat":
        return model.capture_md(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, steps_per_replay=K, warmup=1, barostat=BARO)
    return model.capture_minimize(z, pos, batch=batch, box=box, q=q, steps_per_replay=K, warmup=1, cell={})


@pytest.mark.parametrize("kind", ["barostat", "cell"])
def test_a_box_that_moves_is_the_callers_own(hip_lib, kind):
    box = _system()[-1]
    own = _moving_box(_model(), kind, box)
    assert own.box is box
    box64 = box.double()
    other = _moving_box(_model(), kind, box64)
    assert other.box is not box64 and other.box.dtype == torch.float32
    assert torch.equal(box64, _system()[-1].double())  # the caller's fp64 box is read, never written
    # the model's own box: the loop moves a clone
    model = _model(box_vecs=[[30.0, 0.0, 0.0], [0.0, 30.0, 0.0], [0.0, 0.0, 30.0]])
    mine = model.representation_model.distance.box
    before = mine.clone()
    loop = _moving_box(model, kind, None, one=True)
    loop(2)
    assert loop.check() == 2 * K
    assert loop.box is not mine and loop.box.data_ptr() != mine.data_ptr()
    assert model.representation_model.distance.box is mine and _bits(mine, before)
