"""-m gpu: the observer of the device-resident MD loop (csrc/tn_observe.hip: k_obs_atoms, k_obs_rdf, k_obs_mol;
TorchMD_Net.capture_md_observed).

1. the C entry on hand-built buffers (tests/observe_cases.py), no model: counts equal the fp32 mirror exactly, frames keep the bits
   of the input, MSD and VACF within the bound of two fp64 summation orders
2. the observer does not perturb: capture_md and capture_md_observed give the same bits, per architecture
3. frames are the trajectory, and 5. (K = 8, S = 4) and (K = 4, S = 4) record the same
4. the observables from the loop's own frames, with constraints, with a global thermostat and on a batch
6. a frozen loop records nothing more   7. reset: "clear" and "keep\""""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import observe_cases as CS
from tests import observe_host_mirror as HM
from tests import observe_oracle as O
from tests.test_gpu_md_loop import FS, _bits, _model, _setup, _system
from torchmdnet_amd import md as MD
from torchmdnet_amd import observe as OBS

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the C entry
class _Loop:
    """What an Observer needs of a loop, on buffers of the test's own: an MD workspace whose step counter the test sets, no model and
    graph_ws = NULL"""

    def __init__(self, lib, pos, vel, batch, box, n_mol):
        self.L, self.pos, self.vel, self.box = lib, pos, vel, box
        self.inputs = (None, batch, box, None)
        self._model = SimpleNamespace(_engine=SimpleNamespace(handle=None, graph_ws=None))
        nb = C.c_size_t(0)
        assert lib.tmdnet_md_workspace_bytes(pos.shape[0], n_mol, C.byref(nb)) == 0
        self._ws = torch.zeros(nb.value, dtype=torch.uint8, device="cuda")

    @staticmethod
    def _s():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def completed(self, step):
        """the loop has completed `step` steps: the next observer launch sees s = step + 1"""
        assert self.L.tmdnet_md_reset(self._s(), C.c_void_p(self._ws.data_ptr()), step) == 0

    def _status(self, entry, words):
        host = (C.c_uint64 * words)()
        rc = entry(self._s(), C.c_void_p(self._ws.data_ptr()), C.cast(host, C.POINTER(C.c_uint64)))
        return rc, [int(w) for w in host]


def _case_tensors(c):
    n = len(c["z"])
    batch = c.get("batch", np.zeros(n, np.int64))
    n_mol = c.get("n_mol", 1)
    box = None if c["box"] is None else torch.from_numpy(c["box"]).cuda()
    return torch.from_numpy(c["z"]).cuda(), torch.from_numpy(c["pos"]).cuda(), torch.from_numpy(batch).cuda(), box, n_mol


@pytest.mark.parametrize("name,bins", [("five", 7), ("five", 1024), ("sixty_four", 7), ("sixty_four", 1024), ("three_hundred", 7),
                                       ("three_hundred", 1024), ("batch", 7)])
def test_c_entry_histogram_and_frames_on_hand_built_cases(hip_lib, name, bins):
    c = CS.batch_of_three() if name == "batch" else CS.case(name)
    z, pos, batch, box, n_mol = _case_tensors(c)
    vel = torch.from_numpy(CS.velocities(len(c["z"]), 3, 1)[0]).cuda()
    ob = dict(every=1, frames=dict(capacity=3, velocities=True), rdf=dict(pairs=CS.PAIRS, r_max=c["r_max"], bins=bins))
    obs = OBS.Observer(OBS.prepare_observe(ob, z, batch, box, n_mol, 1), len(c["z"]), n_mol, 1.0, "cuda")
    loop = _Loop(hip_lib, pos, vel, batch if n_mol > 1 else None, box, n_mol)
    s0 = 2 ** 32 - 3  # the counter crosses 2^32 between the second and the third sample
    loop.completed(s0)
    obs.start(loop, s0)
    for j in range(5):
        loop.completed(s0 + j)
        obs.launch(loop)
    loop.completed(s0 + 5)
    assert obs.n_samples(loop) == 5
    mode = 0 if box is None else (1 if box.dim() == 2 else 2)
    want = HM.rdf_counts(c["z"], c["pos"], c["box"], mode, _np(batch), n_mol, CS.PAIRS, c["r_max"], bins).astype(np.int64)
    _, g, counts = obs.rdf(loop)
    print(name, bins, "pairs counted per sample", want.sum(2).tolist())
    assert want.sum() > 0 and (_np(counts) == 5 * want).all()  # exactly: the cases keep their margin
    steps, fp, fv = obs.frames(loop)
    assert steps.tolist() == [s0 + 3, s0 + 4, s0 + 5] and fp.shape == (3, len(c["z"]), 3)
    assert all(_bits(fp[k], pos) and _bits(fv[k], vel) for k in range(3))
    # g against the oracle's normalisation of the oracle's own counts
    for m in range(n_mol):
        k = _np(batch) == m
        bm = None if c["box"] is None else (c["box"] if mode == 1 else c["box"][m])
        for p, (a, b) in enumerate(CS.PAIRS):
            npairs = O.pair_counts(c["z"][k], a, b)[2]
            ref = O.rdf_g(5 * O.rdf_counts(c["z"][k], c["pos"][k], bm, CS.PAIRS, c["r_max"], bins)[p], 5, npairs, c["r_max"],
                          None if bm is None else abs(np.linalg.det(bm.astype(np.float64))))
            assert np.abs(_np(g[m, p]) - ref).max() <= 1e-12 * max(ref.max(), 1.0)
    # a launch at a step that is no sample, and a launch before s0, write nothing
    keep = obs._ws.clone()
    loop.completed(s0 - 2)
    obs.launch(loop)
    assert torch.equal(obs._ws, keep)


def test_c_entry_msd_and_vacf_against_the_oracle(hip_lib):
    c = CS.batch_of_three()
    z, pos0, batch, box, n_mol = _case_tensors(c)
    n, S, ns, L, T = len(c["z"]), 2, 7, 4, 5
    vels = CS.velocities(n, 4, ns)
    rng = np.random.default_rng(6)
    walk = np.cumsum(rng.normal(0, 0.05, (ns, n, 3)), 0).astype(np.float32)
    frames = [(c["pos"] + walk[j]).astype(np.float32) for j in range(ns)]
    groups_m, groups_v = [None, 8], [1, None, 8]
    ob = dict(every=S, frames=dict(capacity=ns), msd=dict(groups=groups_m, capacity=T), vacf=dict(lags=L, groups=groups_v))
    prep = OBS.prepare_observe(ob, z, batch, box, n_mol, S)
    obs = OBS.Observer(prep, n, n_mol, 0.5, "cuda")
    pos, vel = pos0.clone(), torch.zeros_like(pos0)
    loop = _Loop(hip_lib, pos, vel, batch, box, n_mol)
    loop.completed(10)
    obs.start(loop, 10)  # origins = pos0
    for j in range(ns):
        pos.copy_(torch.from_numpy(frames[j]))
        vel.copy_(torch.from_numpy(vels[j]))
        for done in (10 + S * j, 10 + S * j + 1):  # the second launch of each pair is the sample: s = done + 1
            loop.completed(done)
            obs.launch(loop)
    loop.completed(10 + S * ns)
    assert obs.n_samples(loop) == ns
    steps, msd = obs.msd(loop)
    assert steps.tolist() == [10 + S * (j + 1) for j in range(T)] and msd.shape == (T, n_mol, 2)  # samples beyond T are not written
    want, mag = O.msd_sums(c["z"], _np(batch), n_mol, groups_m, c["pos"], frames[:T])
    sizes = _np(prep["msd_sizes"]).astype(np.float64)
    dev = np.abs(_np(msd) * sizes[None] - want)
    bound = O.sum_bound(3 * sizes[None], mag)
    print("msd: largest deviation / bound", (dev / bound).max())
    assert (dev <= bound).all() and want.min() > 0
    lag_t, cv = obs.vacf(loop)
    assert np.allclose(_np(lag_t), np.arange(L) * S * 0.5)
    acc, mag = O.vacf_sums(c["z"], _np(batch), n_mol, groups_v, vels, L)
    vs = _np(prep["vacf_sizes"]).astype(np.float64)
    cnt = np.array([O.lag_samples(ns, l) for l in range(L)], np.float64)
    dev = np.abs(_np(cv) * vs[:, :, None] * cnt[None, None, :] - acc)
    bound = O.sum_bound(3 * vs[:, :, None] * cnt[None, None, :], mag) + 4 * 2.0 ** -52 * np.abs(acc)  # (and the host's two divisions)
    print("vacf: largest deviation / bound", (dev / bound).max())
    assert (dev <= bound).all() and (acc[:, :, 1:] != 0).all()
    fr_steps, fr = obs.frames(loop)
    assert fr_steps.tolist() == [10 + S * (j + 1) for j in range(ns)] and all(_bits(fr[j], torch.from_numpy(frames[j]).cuda()) for j in range(ns))
    # lags with no sample are NaN: a fresh start, two samples, four lags
    obs.start(loop, 0)
    for done in (1, 3):
        loop.completed(done)
        obs.launch(loop)
    loop.completed(4)
    cv2 = _np(obs.vacf(loop)[1])
    assert np.isfinite(cv2[:, :, :2]).all() and np.isnan(cv2[:, :, 2:]).all() and _np(obs.msd(loop)[1]).shape[0] == 2


# ------------------------------------------------------------------------------------------------ through the model
def _observe_all(z, r_max, bins=64, S=2, F=16, T=16, L=4):
    za, zb = int(z[0]), int(z[z != z[0]][0])
    return dict(every=S, frames=dict(capacity=F, velocities=True), rdf=dict(pairs=[(None, None), (za, za), (za, zb)], r_max=r_max, bins=bins),
                msd=dict(groups=[None, za], capacity=T), vacf=dict(lags=L, groups=[None, zb]))


def _snapshot(md):
    return [t.clone() for t in (md.rdf()[2], md.msd()[1], md.vacf()[1], *md.frames()[1:])], md.frames()[0].tolist(), md.n_samples


def _same(a, b):
    return a[1] == b[1] and a[2] == b[2] and all(x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a[0], b[0]))


# ------------------------------------------------------------------------------------------------ 2. no perturbation
@pytest.mark.parametrize("arch", ["tensornet", "equivariant-transformer", "tensornet2"])
def test_the_observer_does_not_perturb_the_trajectory(hip_lib, arch):
    model, _, (z, pos, batch, box, q), vel, mass, dt = _setup(arch, "ragged")
    th = dict(friction=0.02, kT=0.025, seed=5) if arch == "tensornet" else None
    kw = dict(batch=batch, box=box, q=q, steps_per_replay=4, thermostat=th)
    plain = model.capture_md(z, pos, vel, mass, dt, **kw)
    seen = model.capture_md_observed(z, pos, vel, mass, dt, observe=_observe_all(z, 6.0), **kw)
    assert type(seen) is MD.DeviceMD
    for _ in range(3):
        plain()
        seen()
        for a, b in zip((plain.pos, plain.vel, plain.forces, plain.epot, plain.ekin), (seen.pos, seen.vel, seen.forces, seen.epot, seen.ekin)):
            assert _bits(a, b)
    assert seen.check() == plain.check() == 12 and seen.n_samples == 6 and int(seen.rdf()[2].sum()) > 0
    with pytest.raises(ValueError, match="without an observer"):
        plain.frames()


# ------------------------------------------------------------------------------------------------ 3. frames, 5. K independence
def test_frames_are_the_trajectory_and_do_not_depend_on_k(hip_lib):
    model, _, (z, pos, batch, box, q), vel, mass, dt = _setup("tensornet", "ragged")
    kw = dict(batch=batch, box=box, q=q)
    plain = model.capture_md(z, pos, vel, mass, dt, steps_per_replay=4, **kw)
    traj = []
    for _ in range(6):
        plain()
        traj.append((plain.pos.clone(), plain.vel.clone()))
    ring = model.capture_md_observed(z, pos, vel, mass, dt, steps_per_replay=4, observe=dict(every=4, frames=dict(capacity=3)), **kw)
    ring(5)
    steps, fp = ring.frames()
    assert steps.tolist() == [12, 16, 20] and all(_bits(fp[k], traj[2 + k][0]) for k in range(3))  # samples 3, 4, 5 in order
    ring()
    assert ring.frames()[0].tolist() == [16, 20, 24] and _bits(ring.frames()[1][2], traj[5][0])
    k4 = model.capture_md_observed(z, pos, vel, mass, dt, steps_per_replay=4, observe=_observe_all(z, 6.0, S=4), **kw)
    k8 = model.capture_md_observed(z, pos, vel, mass, dt, steps_per_replay=8, observe=_observe_all(z, 6.0, S=4), **kw)
    k4(6)
    k8(3)
    steps, fp, fv = k8.frames()
    assert steps.tolist() == [4, 8, 12, 16, 20, 24] and all(_bits(fp[j], traj[j][0]) for j in range(6))
    # the recorded velocity is the leapfrog one, half a kick behind the closed velocity of the plain loop
    hk = (0.5 * dt / mass.double()).float()[:, None]
    assert not _bits(fv[5], traj[5][1]) and _bits(torch.add(fv[5], torch.mul(hk, k8.forces)), traj[5][1])
    assert _same(_snapshot(k4), _snapshot(k8)) and k4.n_samples == 6
    two = model.capture_md_observed(z, pos, vel, mass, dt, steps_per_replay=8, observe=_observe_all(z, 6.0, S=2), **kw)
    two(3)
    assert two.n_samples == 12 and all(_bits(two.frames()[1][2 * j + 1], traj[j][0]) for j in range(6))


# ------------------------------------------------------------------------------------------------ 4. from the loop's own frames
def _against_own_frames(md, z, pos0, batch, box, n_mol, ob, dt):
    steps, fp, fv = md.frames()
    ns = md.n_samples
    assert ns == len(steps) and ns >= 6
    zc, bc = _np(z), _np(batch)
    frames, vels = [_np(f) for f in fp], [_np(v) for v in fv]
    prep = md._observer.prep
    _, msd = md.msd()
    want, mag = O.msd_sums(zc, bc, n_mol, ob["msd"]["groups"], _np(pos0), frames)
    sizes = _np(prep["msd_sizes"]).astype(np.float64)
    dev, bound = np.abs(_np(msd) * sizes[None] - want), O.sum_bound(3 * sizes[None], mag)
    print("msd deviation / bound", (dev / np.maximum(bound, 1e-300)).max(), "largest", want.max())
    assert (dev <= bound).all() and want.max() > 0
    L = ob["vacf"]["lags"]
    _, cv = md.vacf()
    acc, mag = O.vacf_sums(zc, bc, n_mol, ob["vacf"]["groups"], vels, L)
    vs = _np(prep["vacf_sizes"]).astype(np.float64)
    cnt = np.array([O.lag_samples(ns, l) for l in range(L)], np.float64)
    dev = np.abs(_np(cv) * vs[:, :, None] * cnt[None, None, :] - acc)
    bound = O.sum_bound(3 * vs[:, :, None] * cnt[None, None, :], mag) + 4 * 2.0 ** -52 * np.abs(acc)
    print("vacf deviation / bound", (dev / np.maximum(bound, 1e-300)).max())
    assert (dev <= bound).all()
    r = ob["rdf"]
    boxc = None if box is None else _np(box)
    mode = 0 if box is None else (1 if box.dim() == 2 else 2)
    mirror = sum(HM.rdf_counts(zc, f, boxc, mode, bc, n_mol, r["pairs"], r["r_max"], r["bins"]).astype(np.int64) for f in frames)
    counts = _np(md.rdf()[2])
    borderline = 0
    for f in frames:
        for m in range(n_mol):
            k = bc == m
            bm = None if boxc is None else (boxc if mode == 1 else boxc[m])
            _, _, rel = O.edge_margin(zc[k], f[k], bm, r["pairs"], r["r_max"], r["bins"])
            borderline += int((rel < 1e-6).sum())
    diff = int(np.abs(counts - mirror).sum())
    print("pairs counted", int(mirror[:, 0].sum()), "borderline", borderline, "sum |device - mirror|", diff)
    assert mirror[:, 0].sum() > 0
    assert borderline <= 0.005 * mirror[:, 0].sum(), "too many pairs on a bin edge for this comparison to mean anything"
    assert diff <= 2 * borderline


@pytest.mark.parametrize("mode", ["constraints", "csvr"])
def test_observables_from_the_loops_own_frames_in_the_water_box(hip_lib, mode):
    model = _model("tensornet", max_num_neighbors=128)
    z, pos, batch, box = (t.cuda() for t in _system("water192"))
    q = torch.zeros(1, device="cuda")
    mass = torch.where(z == 1, 1.008, 12.0).float()
    vel = 0.005 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    _, f0 = model.capture(z, pos, batch, box, q=q)(pos)
    fs = FS * 0.2 / float(f0.abs().max())  # (the scale of tests/test_gpu_md_constraints.py: the largest force counts as 0.2 eV / A)
    r_max = 0.45 * float(OBS.box_heights(box).min())
    ob = dict(every=2, frames=dict(capacity=8, velocities=True), rdf=dict(pairs=[(None, None), (8, 8), (1, 8)], r_max=r_max, bins=64),
              msd=dict(groups=[None, 8], capacity=8), vacf=dict(lags=4, groups=[None, 1]))
    kw = dict(constraints=dict(pairs=MD.hydrogen_pairs(z, pos, rigid_water=True))) if mode == "constraints" else \
        dict(thermostat=dict(kind="csvr", kT=0.025, tau=20.0, seed=3))
    md = model.capture_md_observed(z, pos, vel, mass, 2.0, batch=batch, box=box, q=q, steps_per_replay=4, force_scale=fs, observe=ob, **kw)
    assert type(md) is (MD.DeviceGlobalMD if mode == "csvr" else MD.DeviceMD)
    md(4)
    assert md.check() == 16
    _against_own_frames(md, z, pos, batch, box, 1, ob, 2.0)
    r, g, _ = md.rdf()
    assert g.shape == (1, 3, 64) and float(g[0, 0, :8].sum()) == 0.0 and 0.5 < float(g[0, 0, 40:].mean()) < 1.5  # no overlaps; ~1 far out


def test_observables_from_the_loops_own_frames_on_a_batch(hip_lib):
    model, _, (z, pos, batch, box, q), vel, mass, dt = _setup("tensornet", "ragged")
    ob = _observe_all(z, 5.0, bins=64, S=2, F=8, T=8, L=4)
    md = model.capture_md_observed(z, pos, vel, mass, 4 * dt, batch=batch, box=box, q=q, steps_per_replay=8, observe=ob)
    md(2)
    assert md.check() == 16
    _against_own_frames(md, z, pos, batch, box, 3, ob, 4 * dt)


# ------------------------------------------------------------------------------------------------ 6. frozen
def test_a_frozen_loop_records_nothing_more(hip_lib):
    model = _model("tensornet", max_num_neighbors=72)  # the recipe of tests/test_gpu_md_loop.py: scaled by 0.85 the box overflows
    z, pos, batch, box = (t.cuda() for t in _system("water192"))
    box = box.clone()
    box0 = box.clone()
    q = torch.zeros(1, device="cuda")
    vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    mass = torch.where(z == 1, 1.008, 12.0).float()
    ob = _observe_all(z, 0.4 * float(OBS.box_heights(box).min()), S=2, F=4)
    md = model.capture_md_observed(z, pos, vel, mass, 0.01, batch=batch, box=box, q=q, steps_per_replay=4, observe=ob)
    md()
    assert md.check() == 4 and md.n_samples == 2
    first = _snapshot(md)
    ws = md._observer._ws.clone()
    box.mul_(0.85)
    md.pos.mul_(0.85)
    md(2)
    with pytest.raises(RuntimeError, match="max_num_pairs"):
        md.check()
    assert md.steps_done == 12 and md.n_samples == 2  # the device's counter, not the host's
    assert torch.equal(md._observer._ws, ws) and _same(_snapshot(md), first)
    box.copy_(box0)
    md.reset(pos=pos, vel=vel)
    assert md.n_samples == 0 and int(md.rdf()[2].sum()) == 0 and md.frames()[1].shape[0] == 0
    md()
    assert md.check() == 4 and _same(_snapshot(md), first)  # cleared, and the same trajectory again


# ------------------------------------------------------------------------------------------------ 7. reset
def test_reset_clears_or_keeps_the_observables(hip_lib):
    model, _, (z, pos, batch, box, q), vel, mass, dt = _setup("tensornet", "ragged")
    md = model.capture_md_observed(z, pos, vel, mass, dt, batch=batch, box=box, q=q, steps_per_replay=4, observe=_observe_all(z, 6.0))
    md(2)
    two = _snapshot(md)
    md(2)
    four = _snapshot(md)
    assert two[2] == 4 and four[2] == 8 and not _same(two, four)
    md.reset(pos=pos, vel=vel)  # "clear": as a fresh capture
    assert md.n_samples == 0
    md(2)
    assert _same(_snapshot(md), two)
    with pytest.raises(ValueError, match="keep"):
        md.reset(pos=pos, observables="keep")
    with pytest.raises(ValueError, match="keep"):
        md.reset(observables="keep")  # step = 0 is not the loop's step
    with pytest.raises(ValueError, match="'clear' or 'keep'"):
        md.reset(observables="drop")
    assert _same(_snapshot(md), two)  # the refusals changed nothing
    md.reset(step=md.check(), observables="keep")
    assert md.n_samples == 4
    md(2)
    assert _same(_snapshot(md), four)  # the sums continued
    md.reset(step=100)  # a new s0: samples are counted from it
    md()
    assert md.n_samples == 2 and md.frames()[0].tolist() == [102, 104] and md.msd()[0].tolist() == [102, 104]
