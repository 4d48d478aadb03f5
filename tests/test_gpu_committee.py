"""-m gpu: the committee pass (csrc/tn_committee.hip), ``Ensemble.committee`` / ``capture`` / ``capture_md`` and the gate.

1. the pass alone on synthetic arrays against the float64 oracle (tests/committee_oracle.py), 4 fp32 ulps
2. ``Ensemble.committee``: three TensorNet members, and a TensorNet + Equivariant Transformer pair
3. ``Ensemble.capture``: the replay is the eager call, bit for bit
4. ``capture_md`` with copies of one member is that member's own ``capture_md``, bit for bit
5. the gate: the stop, the flags and the reset against an ungated run of the same committee
6. an overflow in a member that is not the first freezes the loop at the last completed step
7. a parameter change in a member after the capture makes the next replay raise

Bound of 1 and 2: 4 fp32 ulps of the float64 value - fp64 sums rounded once, the slack is for the order of the fp64 additions.
Every test fails on a tree without the committee: the entries and the methods do not exist."""
import copy

import numpy as np
import pytest
import torch

from tests import committee_oracle as O
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

FIELDS = ("energy", "forces", "energy_std", "forces_std", "deviation", "max_deviation", "max_atom")
GATE_SEED, GATE_KT = 8, 0.5  # initial velocities and Langevin noise of test 5 (its precondition is asserted there)


def _bits(a, b):
    if a.dtype == torch.int64:
        return a.shape == b.shape and torch.equal(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _numpy(res):
    return {k: getattr(res, k).cpu().numpy() for k in FIELDS}


def _member(seed, args=None, **over):
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(seed)
    return create_model(dict(W.TINY_ARGS if args is None else args, static_shapes=True, **over)).to("cuda")


def _system(sizes=(7, 12, 20), spread=1.0):
    zs, ps, bs = [], [], []
    for m, n in enumerate(sizes):
        z, p = W.synthetic_molecule(60 + m, n)
        zs.append(torch.from_numpy(z))
        ps.append(torch.from_numpy(p) * spread)
        bs.append(torch.full((n,), m, dtype=torch.long))
    z, pos, batch = torch.cat(zs).cuda(), torch.cat(ps).float().cuda(), torch.cat(bs).cuda()
    mass = torch.where(z == 1, 1.008, 12.0).float()
    return z, pos, batch, mass


@pytest.fixture(scope="module")
def three(hip_lib):
    """three TINY TensorNet members, seeds 1, 2, 3 (shared, never modified)"""
    return [_member(s) for s in (1, 2, 3)]


# ------------------------------------------------------------------------------------------------ 1. the pass alone
@pytest.mark.parametrize("unsorted", [False, True], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("M", [2, 3, 16])
def test_pass_against_oracle(hip_lib, M, unsorted):
    from torchmdnet_amd.committee import CommitteePass

    E, F, batch, B = O.synthetic(M, 30 + M, unsorted)
    want = O.reduce(E, F, batch, B)
    outs = [(torch.from_numpy(E[k]).cuda(), torch.from_numpy(F[k]).cuda()) for k in range(M)]
    tb = torch.from_numpy(batch).cuda()
    red = CommitteePass(M, F.shape[1], B, torch.device("cuda", torch.cuda.current_device()))
    first = red(outs, tb)
    got = _numpy(first)
    worst = O.check(got, want, batch, B)
    print("worst ulps", worst)
    assert got["max_atom"][3] == -1 and got["max_deviation"][3] == 0.0  # the molecule id without atoms
    # again over the same workspace, which nobody cleared: the words reset themselves, and the bits repeat
    ws = red.ws.clone()
    second = red(outs, tb)
    for k in FIELDS:
        assert _bits(getattr(first, k), getattr(second, k)), k
    assert torch.equal(ws, red.ws) and not bool(red.ws.any())
    # no batch vector: one molecule
    single = CommitteePass(M, F.shape[1], 1, tb.device)([(e[:1].contiguous(), f) for e, f in outs], None)
    O.check(_numpy(single), O.reduce(E[:, :1], F, None, 1), None, 1)
    # a NaN in one member: +inf, and it wins its molecule
    i = int(np.flatnonzero(batch == 4)[17])
    outs[M - 1][1][i, 1] = float("nan")
    third = red(outs, tb)
    assert third.deviation[i].item() == float("inf") and third.max_deviation[4].item() == float("inf") and third.max_atom[4].item() == i


# ------------------------------------------------------------------------------------------------ 2. Ensemble.committee
def _own(members, z, pos, batch, n_mol, q=None):
    return [m.energy_and_forces(z, pos, batch, None, q, n_mol) for m in members]


def _check_committee(ens, members, z, pos, batch, n_mol):
    res = ens.committee(z, pos, batch)
    own = _own(members, z, pos, batch, n_mol)
    E = torch.stack([e for e, _ in own]).double()
    F = torch.stack([f for _, f in own]).double()
    for name, ref in (("energy", E.mean(0)), ("energy_std", E.std(0)), ("forces", F.mean(0)), ("forces_std", F.std(0))):
        u = float(O.ulps(getattr(res, name).cpu().numpy(), ref.cpu().numpy()).max())
        print(name, "ulps vs torch float64", u)
        assert u <= 4.0, name
    want = O.reduce(E.cpu().numpy(), F.cpu().numpy(), batch.cpu().numpy(), n_mol)
    O.check(_numpy(res), want, batch.cpu().numpy(), n_mol)
    assert res._fields == FIELDS and res.energy.shape == (n_mol,) and res.max_atom.dtype == torch.int64
    assert float(res.max_deviation.min()) > 0.0  # different members disagree
    # a member inside the committee is the member alone, bit for bit: a committee of the member with itself returns its E and F
    from torchmdnet_amd.models.model import Ensemble

    for m, (e, f) in zip(members, own):
        twin = Ensemble([m, m]).committee(z, pos, batch)
        assert _bits(twin.energy, e) and _bits(twin.forces, f)
        assert not bool(twin.deviation.any()) and not bool(twin.energy_std.any()) and not bool(twin.forces_std.any())
    return res


def test_committee_of_three_tensornets(three):
    from torchmdnet_amd.models.model import Ensemble

    z, pos, batch, _ = _system()
    ens = Ensemble(three, return_std=True)
    _check_committee(ens, three, z, pos, batch, 3)
    # Ensemble.forward is what it was: the Python loop over the members and torch's fp32 mean / std
    ys, fs = zip(*[m(z, pos, batch) for m in three])
    y, f = torch.stack(ys), torch.stack(fs)
    out = ens(z, pos, batch)
    for got, ref in zip(out, (torch.mean(y, axis=0), torch.mean(f, axis=0), torch.std(y, axis=0), torch.std(f, axis=0))):
        assert _bits(got, ref)
    assert len(Ensemble(three)(z, pos, batch)) == 2


def test_committee_of_mixed_architectures(hip_lib):
    from torchmdnet_amd.models.model import Ensemble

    members = [_member(1), _member(2, W.ET_TINY_ARGS)]
    z, pos, batch, _ = _system()
    _check_committee(Ensemble(members), members, z, pos, batch, 3)


# ------------------------------------------------------------------------------------------------ 3. Ensemble.capture
def test_capture_replays_the_eager_call(three):
    from torchmdnet_amd.models.model import Ensemble

    z, pos, batch, _ = _system()
    ens = Ensemble(three)
    eager = ens.committee(z, pos, batch)
    replay = ens.capture(z, pos, batch, warmup=1)
    res = replay()
    for k in FIELDS:
        assert _bits(getattr(res, k), getattr(eager, k)), k
    for (e, f), (e0, f0) in zip(replay.member_outputs, _own(three, z, pos, batch, 3)):
        assert _bits(e, e0) and _bits(f, f0)
    moved = pos + 0.05 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(3)).cuda()
    replay.pos.copy_(moved)  # in place
    res = replay()
    eager = ens.committee(z, moved, batch)
    for k in FIELDS:
        assert _bits(getattr(res, k), getattr(eager, k)), k
    res = replay(pos)  # and through the argument
    eager = ens.committee(z, pos, batch)
    for k in FIELDS:
        assert _bits(getattr(res, k), getattr(eager, k)), k
    assert replay.graph is not None and len(replay.inputs) == 3 and replay.n_mol == 3


# ------------------------------------------------------------------------------------------------ 4. copies of one member
@pytest.mark.parametrize("thermostat", [None, dict(friction=0.1, kT=0.02, seed=5)], ids=["nve", "langevin"])
def test_md_of_identical_members_is_the_members_own_loop(three, thermostat):
    from torchmdnet_amd.models.model import Ensemble

    K = 4
    z, pos, batch, mass = _system()
    vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    single = copy.deepcopy(three[0])
    ens = Ensemble([copy.deepcopy(three[0]) for _ in range(3)])
    kw = dict(batch=batch, steps_per_replay=K, thermostat=thermostat, warmup=1)
    ref = single.capture_md(z, pos, vel, mass, 0.01, **kw)
    md = ens.capture_md(z, pos, vel, mass, 0.01, gate=dict(flag_above=0.0, stop_above=0.0), **kw)
    assert _bits(md.forces, ref.forces)
    for r in range(3):
        ref(), md()
        for name in ("pos", "vel", "forces", "epot", "ekin"):
            assert _bits(getattr(md, name), getattr(ref, name)), (r, name)
        assert not bool(md.deviation.any()) and not bool(md.energy_std.any())
    assert md.check() == ref.check() == 3 * K
    assert md.stopped is None and bool((md.flagged_at == -1).all()) and not bool(md.flagged_pos.any())
    assert not _bits(md.pos, pos)


# ------------------------------------------------------------------------------------------------ 5. the gate
def _gate_loop(three, K, gate):
    from torchmdnet_amd.models.model import Ensemble

    z, pos, batch, mass = _system()
    vel = (GATE_KT / mass.cpu()).sqrt()[:, None] * torch.randn(pos.shape, generator=torch.Generator().manual_seed(GATE_SEED))
    md = Ensemble(three).capture_md(z, pos, vel.cuda(), mass, 0.05, batch=batch, steps_per_replay=K, warmup=1, gate=gate,
                                    thermostat=dict(friction=0.2, kT=GATE_KT, seed=GATE_SEED))
    return md, pos, vel.cuda()


def test_gate_stops_and_flags_where_the_ungated_log_says(three):
    S = 12
    free, _, _ = _gate_loop(three, 1, None)
    log = []
    for s in range(1, S + 1):
        free()
        log.append(dict(D=free.deviation[0].cpu().numpy().copy(), a=free.deviation_atom[0].cpu().numpy().copy(), pos=free.pos.clone(),
                        vel=free.vel.clone(), forces=free.forces.clone()))
    assert free.check() == S and free.stopped is None
    D = np.stack([e["D"] for e in log])  # [S, B], row s - 1 is step s
    g = D.max(axis=1)
    print("g_s", g.tolist())
    records = [s for s in range(2, S + 1) if g[s - 1] > g[:s - 1].max()]
    assert records, f"the ungated run sets no new running maximum after step 1 (g = {g.tolist()}): choose GATE_SEED / GATE_KT again"
    s0 = records[-1]
    stop_above = 0.5 * (float(g[s0 - 1]) + float(g[:s0 - 1].max()))
    # flag_above: midway between two neighbouring distinct values of the per-molecule logs - of all such midpoints the one that
    # flags some molecule latest, so that a flag falls inside a replay and not at its first step whenever the log allows it
    vals = np.unique(D[:s0])
    assert len(vals) >= 2
    firsts = lambda t: [next((s for s in range(1, s0 + 1) if D[s - 1, m] > t), -1) for m in range(D.shape[1])]
    flag_above = max((0.5 * (float(lo) + float(hi)) for lo, hi in zip(vals[:-1], vals[1:])), key=lambda t: max(firsts(t)))
    first = firsts(flag_above)
    print("s0", s0, "stop_above", stop_above, "flag_above", flag_above, "first flagged", first)
    assert any(f > 0 for f in first)

    md, pos, vel = _gate_loop(three, 4, dict(flag_above=flag_above, stop_above=stop_above))

    def stopped_as_logged():
        taken = md.run(S + 4)
        assert taken == 4 * ((s0 + 3) // 4)  # whole replays, and none after the stop was read
        assert md.check() == s0  # a stop is a result: check() does not raise
        at = log[s0 - 1]
        m = int(np.argmax(at["D"]))
        assert md.stopped == (s0, m, int(at["a"][m]), float(at["D"][m]))
        for name in ("pos", "vel", "forces"):
            assert _bits(getattr(md, name), at[name]), name
        assert md.flagged_at.tolist() == first
        for m, s in enumerate(first):
            rows = (md.inputs[1] == m)
            if s > 0:
                assert _bits(md.flagged_pos[rows], log[s - 1]["pos"][rows])
                assert md.flagged_dev[m].item() == float(log[s - 1]["D"][m]) and md.flagged_atom[m].item() == int(log[s - 1]["a"][m])
            else:
                assert not bool(md.flagged_pos[rows].any()) and md.flagged_atom[m].item() == -1

    stopped_as_logged()
    keep = [t.clone() for t in (md.pos, md.vel, md.forces, md.epot, md.ekin, md.deviation, md.flagged_pos, md.flagged_at)]
    md(2)  # frozen: further replays change nothing
    assert md.check() == s0 and md.run(8) == 0
    for t, k in zip((md.pos, md.vel, md.forces, md.epot, md.ekin, md.deviation, md.flagged_pos, md.flagged_at), keep):
        assert _bits(t, k)
    # flags="keep": the loop starts over, the flags stay - nothing is flagged a second time
    md.reset(pos=pos, vel=vel)
    assert md.stopped is None and md.check() == 0 and md.flagged_at.tolist() == first
    md()
    assert md.check() == min(4, s0) and md.flagged_at.tolist() == first
    with pytest.raises(ValueError, match="'keep' or 'clear'"):
        md.reset(flags="some")
    # flags="clear": everything starts over and the same stop comes back
    md.reset(pos=pos, vel=vel, flags="clear")
    assert md.stopped is None and bool((md.flagged_at == -1).all()) and not bool(md.flagged_pos.any())
    stopped_as_logged()


# ------------------------------------------------------------------------------------------------ 6. overflow in a later member
def test_overflow_in_a_later_member_freezes_the_loop(three):
    """20 atoms spread to three times their distances: about 2 neighbours per atom inside the cutoff, so member 1's
    max_num_neighbors = 8 holds them; back at the generator's density (positions scaled by 1/3 in place, between two replays) an atom
    has about 15 and member 1's first evaluation of the second replay overflows - member 0 (64) does not."""
    from torchmdnet_amd.models.model import Ensemble

    K = 2
    z, pos, batch, mass = _system(sizes=(20,), spread=3.0)
    vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    members = [copy.deepcopy(three[0]), _member(2, max_num_neighbors=8), copy.deepcopy(three[2])]
    md = Ensemble(members).capture_md(z, pos, vel, mass, 0.01, batch=batch, steps_per_replay=K, warmup=1, gate=dict(stop_above=1e30))
    md()
    assert md.check() == K
    md.pos.mul_(1.0 / 3.0)
    names = ("pos", "vel", "forces", "epot", "ekin", "deviation", "energy_std")
    keep = [getattr(md, n).clone() for n in names]
    for _ in range(2):  # the replay that overflows, then a frozen one
        md()
        with pytest.raises(RuntimeError, match="max_num_pairs"):
            md.check()
        assert md.stopped is None
        for n, k in zip(names, keep):
            assert _bits(getattr(md, n), k), n
    # member 0 alone holds these positions: the overflow was the later member's
    E, F = members[0].energy_and_forces(z, md.pos, batch, None, None, 1)
    assert torch.isfinite(E).all() and torch.isfinite(F).all()
    with pytest.raises(RuntimeError, match="max_num_pairs"):
        members[1].energy_and_forces(z, md.pos, batch, None, None, 1)
    md.reset(pos=pos, vel=vel)
    md()
    assert md.check() == K


# ------------------------------------------------------------------------------------------------ 7. staleness
class _NeverReplayed:
    def replay(self):
        raise AssertionError("a stale graph was replayed")


def test_a_parameter_change_in_a_member_makes_the_replay_raise(three):
    from torchmdnet_amd.models.model import Ensemble

    z, pos, batch, mass = _system()
    members = [copy.deepcopy(m) for m in three[:2]]
    ens = Ensemble(members)
    md = ens.capture_md(z, pos, torch.zeros_like(pos), mass, 0.01, batch=batch, steps_per_replay=2, warmup=1)
    replay = ens.capture(z, pos, batch, warmup=1)
    md()
    assert md.check() == 2
    replay()
    with torch.no_grad():
        members[1].std.mul_(2.0)
    members[1](z, pos, batch)  # parameter change + eager call: the second member's handle is re-created
    graph, md.graph = md.graph, _NeverReplayed()  # (the real graph stays alive, unreplayed, until the test ends)
    stale = r"stale HIP graph.*Ensemble\.capture_md\(\)"
    with pytest.raises(RuntimeError, match=stale):
        md()
    with pytest.raises(RuntimeError, match=stale):
        md.reset()
    with pytest.raises(RuntimeError, match=stale):
        md.run(2)
    assert md.steps_done == 2
    with pytest.raises(RuntimeError, match=r"stale HIP graph.*Ensemble\.capture\(\)"):
        replay()
    del graph
