"""-m gpu: the ZBL / D2 pair priors (csrc/tn_prior.hip) - the pass alone against the float64 statement tests/prior_oracle.py, end to
end against the unmodified reference (tests/golden/priors_ref.pt), additivity and the virial, every consumer of
``TorchMD_Net.energy_and_forces``, and the refusals.

Bound of the pass: element-wise |got - oracle| <= 1e-5 S for e_i, E, F and W - 1e-5 is the project's golden-vector tolerance
(tests/test_gpu_parity.py), S the sum of the ABSOLUTE pair terms behind the element (the terms cancel, so the element itself is not
the scale).  The arithmetic is about twenty fp32 roundings plus expf per pair, accumulated in fp64: about 1e-6 is expected.
Measured worst ratio over all cases (MI355X): 1.4e-6 (profiles/priors.json, key accuracy)."""
import os

import numpy as np
import pytest
import torch

from tests import prior_oracle as O

pytestmark = pytest.mark.gpu

A, EV, HARTREE = 1e-10, 1.602176634e-19, 4.3597447222071e-18
MAX_Z = 20
IDENT = [1] + list(range(1, MAX_Z))  # species s is element s (species 0: hydrogen as well - element 0 has no D2 row)
MAPPED = [1, 8, 6, 1, 7, 16, 9, 17, 35, 53, 54, 14, 15, 5, 3, 11, 12, 13, 2, 10]  # a non-identity atomic_number map


def _prior_args(cutoff, an=IDENT, es=EV):
    return dict(cutoff_distance=cutoff, max_num_neighbors=64, atomic_number=list(an), distance_scale=A, energy_scale=es)


def _oracle_dicts(zbl_args, d2_args):
    from torchmdnet_amd.priors import D2

    t = D2.C_6_R_r.double().numpy()
    zbl = d2 = None
    if zbl_args is not None:
        zbl = dict(cutoff=zbl_args["cutoff_distance"], distance_scale=zbl_args["distance_scale"], energy_scale=zbl_args["energy_scale"],
                   Z=np.asarray(zbl_args["atomic_number"], float))
    if d2_args is not None:
        an = np.asarray(d2_args["atomic_number"])
        d2 = dict(cutoff=d2_args["cutoff_distance"], distance_scale=d2_args["distance_scale"], energy_scale=d2_args["energy_scale"],
                  C6=t[an, 0], Rr=t[an, 1])
    return zbl, d2


_models = {}


def _model(zbl_args=None, d2_args=None, arch="tensornet", zero=False, **over):
    """TINY model with the given priors (cached).  zero=True: every parameter zero - the model's own E and F vanish exactly."""
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    key = (repr(zbl_args), repr(d2_args), arch, zero, tuple(sorted(over.items())))
    if key not in _models:
        torch.manual_seed(4)
        base = {"tensornet": W.TINY_ARGS, "equivariant-transformer": W.ET_TINY_ARGS}.get(arch)
        if base is None:
            base = dict(W.TINY_ARGS, model="tensornet2", output_model="ScalarPlusWeightedCoulomb", q_dim=4, q_weights=[1.0, 1.0, 1.0])
        names = [n for n, a in (("ZBL", zbl_args), ("D2", d2_args)) if a is not None]
        m = create_model(dict(base, prior_model=names or None, prior_args=[a for a in (zbl_args, d2_args) if a is not None] or None, **over))
        if zero:
            with torch.no_grad():
                for p in m.parameters():
                    p.zero_()
        _models[key] = m.to("cuda")
    return _models[key]


def _molecule(seed, n):
    from torchmdnet_amd import workloads as W

    z, p = W.synthetic_molecule(seed, n_atoms=n)
    return torch.from_numpy(z) % 19 + 1, torch.from_numpy(p).float()


def _batch(sizes, first_seed=500, ids=None):
    zs, ps, bs = [], [], []
    for k, n in enumerate(sizes):
        z, p = _molecule(first_seed + k, n)
        zs.append(z), ps.append(p + 4.0 * k), bs.append(torch.full((n,), k if ids is None else ids[k], dtype=torch.long))
    return torch.cat(zs), torch.cat(ps), torch.cat(bs)


def _pbc(golden_dir):
    p = torch.load(os.path.join(golden_dir, "tiny_pbc_ref.pt"))
    return p["z"], p["pos"].float(), p["batch"], p["box"].float()


def _case(name, golden_dir):
    """-> z, pos, batch, n_mol, box, zbl_args, d2_args (CPU tensors)"""
    box = None
    zbl_args, d2_args = _prior_args(4.0), _prior_args(7.0)
    if name.startswith("ragged"):  # 1, 2, 9, 14 and 70 atoms (the last crosses the wave width) and molecule id 3 without atoms
        z, pos, batch = _batch([1, 2, 9, 14, 70], ids=[0, 1, 2, 4, 5])
        n_mol = 6
        if name == "ragged_zbl":
            d2_args = None
        if name == "ragged_d2":
            zbl_args = None
        if name == "ragged_mapped":
            zbl_args, d2_args = _prior_args(3.5, MAPPED), _prior_args(6.0, MAPPED, HARTREE)
    elif name == "mol300":  # several LDS tiles of 256
        z, pos, batch = _batch([300], first_seed=520)
        n_mol, zbl_args, d2_args = 1, _prior_args(5.0), _prior_args(10.0)
    elif name == "unsorted":
        z, pos, batch = _batch([7, 12, 20], first_seed=530)
        perm = torch.randperm(len(z), generator=torch.Generator().manual_seed(3))
        z, pos, batch, n_mol = z[perm], pos[perm], batch[perm], 3
    elif name == "pbc1":  # one triclinic box: ZBL takes the image, D2 does not
        z, pos, batch, box = _pbc(golden_dir)
        n_mol = 1
    elif name == "pbc2":  # one box per molecule
        z, pos, batch, box = _pbc(golden_dir)
        n = len(z)
        z, pos = torch.cat([z, z.flip(0)]), torch.cat([pos, pos * 0.93 + 0.4])
        batch, box, n_mol = torch.cat([batch, batch + 1]), torch.stack([box, box * 0.93]), 2
    elif name == "contact":  # a close contact at 0.3 A
        z, pos, batch = _batch([6], first_seed=540)
        pos[1] = pos[0] + torch.tensor([0.3, 0.0, 0.0])
        n_mol = 1
    else:
        raise KeyError(name)
    # no pair within 1e-4 of a cutoff: D2's cutoff is hard, and a pair on the edge would make the fp32 and fp64 pair lists differ
    zbl, d2 = _oracle_dicts(zbl_args, d2_args)
    rng = np.random.default_rng(1)
    for _ in range(50):
        ref = O.evaluate(pos.numpy(), z.numpy(), batch.numpy(), n_mol, None if box is None else box.double().numpy(), zbl, d2)
        if ref["margin"] > 1e-4:
            break
        pos = pos + torch.from_numpy(rng.normal(size=tuple(pos.shape)) * 2e-3).float()
    assert ref["margin"] > 1e-4
    return z, pos, batch, n_mol, box, zbl_args, d2_args, ref


CASES = ["ragged", "ragged_zbl", "ragged_d2", "ragged_mapped", "mol300", "unsorted", "pbc1", "pbc2", "contact"]
_worst = {}


# ------------------------------------------------------------------------------------------------ 1. the pass alone
@pytest.mark.parametrize("name", CASES)
def test_pass_against_fp64_oracle(hip_lib, golden_dir, name):
    z, pos, batch, n_mol, box, zbl_args, d2_args, ref = _case(name, golden_dir)
    m = _model(zbl_args, d2_args)
    dev = lambda t: None if t is None else t.cuda()
    out = m.debug_pair_priors(dev(z), dev(pos), dev(batch), dev(box), num_systems=n_mol)
    again = m.debug_pair_priors(dev(z), dev(pos), dev(batch), dev(box), num_systems=n_mol)
    for a, b in zip(out, again):
        assert torch.equal(a, b), "two runs are bit-identical (no floating-point atomics, fixed order)"
    E, F, Wv, e = (t.double().cpu().numpy() for t in out)
    worst = 0.0
    for got, key in ((e, "e"), (E, "E"), (F, "F"), (Wv, "W")):
        want, S = ref[key], ref["S_" + key]
        err = np.abs(got - want)
        ratio = float((err[S > 0] / S[S > 0]).max()) if (S > 0).any() else 0.0
        print(f"[priors] {name} {key}: worst |got - oracle| / S = {ratio:.2e} (max |value| {np.abs(want).max():.3e})")
        assert (err <= 1e-5 * S).all(), (name, key, ratio)
        worst = max(worst, ratio)
    _worst[name] = worst
    print(f"[priors] {name}: worst ratio {worst:.2e}")
    assert np.abs(ref["E"]).max() > 0  # the case exercises the priors
    if name.startswith("ragged"):
        assert E[3] == 0.0 and E[0] == 0.0 and (Wv[3] == 0).all()  # no atoms; one atom
    if name == "contact":
        assert ref["E"][0] > 10.0  # eV: the wall is there
    # Newton's third law holds to the rounding of the per-atom sums
    assert np.abs(F.sum(0)).max() <= 1e-5 * ref["S_F"].sum(0).max()


def test_energy_only_and_no_virial_agree_with_the_full_pass(hip_lib, golden_dir):
    """want_forces=False adds the energy only; the pass without the virial gives the same E and F bits."""
    z, pos, batch, n_mol, box, zbl_args, d2_args, _ = _case("pbc1", golden_dir)
    m, m0 = _model(zbl_args, d2_args), _model()
    m0.load_state_dict(m.state_dict(), strict=False)
    z, pos, batch, box = z.cuda(), pos.cuda(), batch.cuda(), box.cuda()
    E, F, _, _ = m.debug_pair_priors(z, pos, batch, box, num_systems=n_mol)
    E2, F2, W2, _ = m.debug_pair_priors(z, pos, batch, box, num_systems=n_mol, want_virial=False)
    assert W2 is None and torch.equal(E, E2) and torch.equal(F, F2)
    Ee, none = m.energy_and_forces(z, pos, batch, box, None, n_mol, want_forces=False)
    E0, _ = m0.energy_and_forces(z, pos, batch, box, None, n_mol, want_forces=False)
    assert none is None and torch.equal(Ee, E0 + E)


# ------------------------------------------------------------------------------------------------ 2. end to end
@pytest.fixture(scope="module")
def fixture(golden_dir):
    return torch.load(os.path.join(golden_dir, "priors_ref.pt"), weights_only=False)


def _fixture_model(fixture, arch, setting):
    from torchmdnet_amd.models.model import create_model

    case = fixture["cases"][arch]
    pm, pa = fixture["settings"][setting]
    m = create_model(dict(case["args"], prior_model=pm, prior_args=pa), mean=case["mean"], std=case["std"])
    missing, unexpected = m.load_state_dict(case["state_dict"], strict=False)
    assert not unexpected and all(k.startswith("prior_model") for k in missing)
    if setting.startswith("Atomref"):
        with torch.no_grad():
            m.prior_model[0].atomref.weight.copy_(fixture["atomref"])
    return m.to("cuda")


@pytest.mark.parametrize("arch", ["tensornet", "equivariant-transformer"])
@pytest.mark.parametrize("setting", ["ZBL", "D2", "Atomref+ZBL+D2"])
def test_forward_against_reference_fixture(hip_lib, fixture, arch, setting):
    """The measure and bound of tests/test_gpu_parity.py::test_reference_golden_vector: element-wise, atol = rtol = 1e-5."""
    m = _fixture_model(fixture, arch, setting)
    res = fixture["cases"][arch]["results"][setting]
    y, f = m(fixture["z"].cuda(), fixture["pos"].cuda(), fixture["batch"].cuda())
    print(f"[priors] {arch} {setting}: max |y - ref| {(y.cpu() - res['y']).abs().max():.2e} of {res['y'].abs().max():.2e}, "
          f"max |f - ref| {(f.cpu() - res['f']).abs().max():.2e} of {res['f'].abs().max():.2e}")
    torch.testing.assert_close(y.cpu(), res["y"], atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(f.cpu(), res["f"], atol=1e-5, rtol=1e-5)
    if setting == "ZBL":  # and in the triclinic box
        p = fixture["pbc"]
        y, f = m(p["z"].cuda(), p["pos"].cuda(), p["batch"].cuda(), box=p["box"].cuda())
        print(f"[priors] {arch} ZBL pbc: max |y - ref| {(y.cpu() - res['y_pbc']).abs().max():.2e}, "
              f"max |f - ref| {(f.cpu() - res['f_pbc']).abs().max():.2e} of {res['f_pbc'].abs().max():.2e}")
        torch.testing.assert_close(y.cpu(), res["y_pbc"], atol=1e-5, rtol=1e-5)
        torch.testing.assert_close(f.cpu(), res["f_pbc"], atol=1e-5, rtol=1e-5)


def test_tensornet2_with_zbl_is_model_plus_pass(hip_lib):
    zbl_args = _prior_args(4.0)
    m, m0 = _model(zbl_args, None, arch="tensornet2"), _model(arch="tensornet2")
    m0.load_state_dict(m.state_dict(), strict=False)
    z, pos, batch = (t.cuda() for t in _batch([9, 14], first_seed=550))
    q = torch.tensor([0.0, 1.0], device="cuda")
    y, f = m(z, pos, batch, q=q)
    y0, f0 = m0(z, pos, batch, q=q)
    Ep, Fp, _, _ = m.debug_pair_priors(z, pos, batch)
    assert Ep.abs().min() > 0
    assert torch.equal(y.view(-1), y0.view(-1) + Ep) and torch.equal(f, f0 + Fp)  # the last bit of the fp32 addition


# ------------------------------------------------------------------------------------------------ 3. additivity and the virial
def _within_one_rounding(got, a, b):
    s = a.double() + b.double()
    ulp = torch.finfo(torch.float32).eps * s.abs()
    return bool(((got.double() - s).abs() <= ulp).all())


@pytest.mark.parametrize("arch", ["tensornet", "equivariant-transformer"])
@pytest.mark.parametrize("name", ["pbc2", "ragged"])
def test_energy_forces_virial_is_model_plus_pass(hip_lib, golden_dir, arch, name):
    z, pos, batch, n_mol, box, zbl_args, d2_args, _ = _case(name, golden_dir)
    m, m0 = _model(zbl_args, d2_args, arch=arch), _model(arch=arch)
    m0.load_state_dict(m.state_dict(), strict=False)
    dev = lambda t: None if t is None else t.cuda()
    z, pos, batch, box = dev(z), dev(pos), dev(batch), dev(box)
    E, F, Wv = m.energy_forces_virial(z, pos, batch, box, num_systems=n_mol)
    E0, F0, W0 = m0.energy_forces_virial(z, pos, batch, box, num_systems=n_mol)
    Ep, Fp, Wp, _ = m.debug_pair_priors(z, pos, batch, box, num_systems=n_mol)
    assert Wp.abs().max() > 0
    assert _within_one_rounding(E.view(-1), E0.view(-1), Ep) and _within_one_rounding(F, F0, Fp) and _within_one_rounding(Wv, W0, Wp)
    y, f = m(z, pos, batch, box=box, num_systems=n_mol)  # forward returns the same E and F bits
    assert torch.equal(y, E) and torch.equal(f, F)
    E1, F1, W1 = m0.energy_forces_virial(z, pos, batch, box, num_systems=n_mol)  # the prior-free model is what it was
    assert torch.equal(E1, E0) and torch.equal(F1, F0) and torch.equal(W1, W0)


def test_box_and_position_gradient(hip_lib, golden_dir):
    """E.backward() through tmdnet::energy_forces_virial on a zero-weight model with ZBL: pos.grad (from F) and box.grad (from W and F)
    against the oracle, 1e-4 relative max-norm each as in tests/test_gpu_virial.py.  24 atoms spread over the whole cell, so the box
    gradient is of the size of the two terms it is the difference of."""
    box = _pbc(golden_dir)[3].double().numpy()
    batch = torch.zeros(24, dtype=torch.long)
    zbl_args = _prior_args(3.9)
    zbl, _ = _oracle_dicts(zbl_args, None)
    boxf = torch.from_numpy(box).float()
    for seed in range(11, 31):  # the first geometry without a pair within 1e-4 of the cutoff
        rng = np.random.default_rng(seed)
        frac = []
        while len(frac) < 24:
            c = rng.uniform(size=3)
            d = [O.minimum_image(((c - o) @ box)[None], box)[0] for o in frac]
            if all(np.linalg.norm(v) > 0.9 for v in d):
                frac.append(c)
        pos = torch.from_numpy(np.array(frac) @ box).float()
        z = torch.from_numpy(rng.integers(1, 9, 24))
        ref = O.evaluate(pos.numpy(), z.numpy(), batch.numpy(), 1, boxf.double().numpy(), zbl, None)
        if ref["margin"] > 1e-4:
            break
    assert ref["margin"] > 1e-4
    m = _model(zbl_args, None, zero=True)
    pg, bg = pos.cuda().requires_grad_(True), boxf.cuda().requires_grad_(True)
    E, F, Wv = m.energy_forces_virial(z.cuda(), pg, batch.cuda(), bg)
    (1.7 * E).sum().backward()
    # d E / d box at fixed Cartesian positions, by central differences of the oracle
    g_box, h, b64 = np.zeros((3, 3)), 1e-6, boxf.double().numpy()
    for a in range(3):
        for c in range(3):
            if a < c:
                continue  # a lower-triangular box: the upper entries do not enter the minimum image
            d = np.zeros((3, 3))
            d[a, c] = h
            g_box[a, c] = 1.7 * (O.energy_only(pos.numpy(), z.numpy(), batch.numpy(), 1, b64 + d, zbl) -
                                 O.energy_only(pos.numpy(), z.numpy(), batch.numpy(), 1, b64 - d, zbl))[0] / (2 * h)
    rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())
    got_box = np.tril(bg.grad.double().cpu().numpy())
    errs = dict(pos_grad=rel(pg.grad.double().cpu().numpy(), -1.7 * ref["F"]), box_grad=rel(got_box, g_box))
    print(f"[priors] gradients through the operator: {errs}")
    assert errs["pos_grad"] < 1e-4 and errs["box_grad"] < 1e-4


# ------------------------------------------------------------------------------------------------ 4. every consumer
def _mol40():
    from torchmdnet_amd import workloads as W

    z, pos, batch = W.synthetic_batch(n_mol=1, n_atoms=40, first_seed=31)
    return (z % 8 + 1).cuda(), pos.cuda(), batch.cuda()


ZD = (_prior_args(4.0), _prior_args(7.0))


def test_capture_replay_is_eager(hip_lib):
    m = _model(*ZD, static_shapes=True)
    z, pos, batch = _mol40()
    replay = m.capture(z, pos, batch, virial=True)
    e, f, w = replay(pos)
    E, F, Wv = m.energy_forces_virial(z, pos, batch)
    assert torch.equal(e, E) and torch.equal(f, F) and torch.equal(w, Wv)
    e2, f2, _ = replay(pos + 0.01)
    E2, F2 = m(z, pos + 0.01, batch)
    assert torch.equal(e2, E2) and torch.equal(f2, F2) and not torch.equal(f2, F)
    F0 = _model(static_shapes=True)
    F0.load_state_dict(m.state_dict(), strict=False)
    assert not torch.equal(F0(z, pos, batch)[1], F)  # the priors are in there


def test_md_loop_sees_the_priors(hip_lib):
    m = _model(*ZD, static_shapes=True)
    z, pos, batch = _mol40()
    vel = 0.02 * torch.randn(pos.shape, generator=torch.Generator().manual_seed(8)).cuda()
    mass = torch.full((z.shape[0],), 12.0, device="cuda")
    md = m.capture_md(z, pos, vel, mass, 0.5, batch=batch, steps_per_replay=2)
    md(1)
    E, F = m(z, md.pos.clone(), batch)
    assert torch.equal(md.forces, F) and torch.equal(md.epot[-1].view(-1), E.view(-1)) and not torch.equal(md.pos, pos)


@pytest.mark.parametrize("kind", ["fire", "lbfgs"])
def test_minimisers_see_the_priors(hip_lib, kind):
    m = _model(*ZD, static_shapes=True)
    z, pos, batch = _mol40()
    kw = dict(fire={}) if kind == "fire" else dict(lbfgs=dict(memory=4))
    opt = m.capture_minimize(z, pos, batch=batch, steps_per_replay=3, **kw)
    opt(1)
    E, F = m(z, opt.pos.clone(), batch)
    assert torch.equal(opt.forces, F) and torch.equal(opt.epot[-1].view(-1), E.view(-1)) and not torch.equal(opt.pos, pos)


def test_neb_sees_the_priors(hip_lib):
    """The band keeps F_neb, not the raw forces: the energies of the last evaluation are compared, at the images it left."""
    from torchmdnet_amd.neb import interpolate

    m = _model(*ZD, static_shapes=True)
    z, pos, _ = _mol40()
    shift = torch.zeros_like(pos)
    shift[:5] = 0.3
    neb = m.capture_neb(z, interpolate(pos, pos + shift, 4), steps_per_replay=2)
    neb(1)
    zz, bb = neb.inputs[0], neb.inputs[1]
    E, _ = m(zz, neb.pos.clone(), bb)
    assert torch.equal(neb.epot[-1].reshape(-1), E.view(-1))
    m0 = _model(static_shapes=True)
    m0.load_state_dict(m.state_dict(), strict=False)
    assert not torch.equal(m0(zz, neb.pos.clone(), bb)[0], E)


def test_central_hessian_of_a_zbl_diatomic(hip_lib):
    """A C-O pair at 1.2 A along a general direction, ZBL on a zero-weight model: H = [[K, -K], [-K, K]] with
    K = u'' n n^T + (u'/r)(I - n n^T) from the oracle's analytic u' and its slope.  The bound is the error of a central difference
    of the forces at step d, computed, not fitted: the truncation (d^2 / 6 times the third derivative of the oracle's force), taken
    as the distance between the oracle's own fp64 central difference and K, plus the rounding of the two fp32 forces, each within
    the pass's bound 1e-5 |u'|, over 2 d."""
    zbl_args = _prior_args(4.0)
    zbl, _ = _oracle_dicts(zbl_args, None)
    m = _model(zbl_args, None, zero=True)
    r, delta = 1.2, 0.01
    n = np.array([0.48, -0.6, 0.64])
    pos = torch.tensor(np.stack([np.array([0.3, 0.1, -0.2]), np.array([0.3, 0.1, -0.2]) + r * n]), dtype=torch.float32)
    z = torch.tensor([6, 8])
    p64, zz, bb = pos.double().numpy(), z.numpy(), np.zeros(2, int)
    vec = p64[0] - p64[1]
    r32 = float(np.linalg.norm(vec))
    nn = np.outer(vec, vec) / r32 ** 2
    du = lambda x: float(O.zbl_u(np.longdouble(x), 6.0, 8.0, 4.0, A, EV, deriv=1))
    d1, d2 = du(r32), (du(r32 + 1e-4) - du(r32 - 1e-4)) / 2e-4  # (slope of the analytic u': its own truncation is negligible)
    K = d2 * nn + d1 / r32 * (np.eye(3) - nn)
    want = np.block([[K, -K], [-K, K]])
    fd = np.zeros((6, 6))  # the oracle's own central difference of its forces, fp64: column k = - d F / d x_k
    for k in range(6):
        d = np.zeros_like(p64)
        d[k // 3, k % 3] = delta
        fp, fm = O.evaluate(p64 + d, zz, bb, 1, None, zbl)["F"], O.evaluate(p64 - d, zz, bb, 1, None, zbl)["F"]
        fd[:, k] = -(fp - fm).reshape(-1) / (2 * delta)
    truncation = np.abs(fd - want).max()
    bound = truncation + 1e-5 * abs(d1) / delta
    H, info = m.hessian(z.cuda(), pos.cuda(), method="central", delta=delta)
    got = H[0].double().cpu().numpy()[:6, :6]
    print(f"[priors] central Hessian: max |H - analytic| = {np.abs(got - want).max():.3e}, bound {bound:.3e} "
          f"(truncation {truncation:.3e}), |H| {np.abs(want).max():.3e}")
    assert 0 < truncation < 0.01 * np.abs(want).max()
    assert np.abs(got - want).max() <= bound
    with pytest.raises(NotImplementedError, match="pair priors have no HIP path with hessian"):
        m.hessian(z.cuda(), pos.cuda(), method="analytic")


def test_changed_prior_argument_makes_the_graph_stale(hip_lib):
    from torchmdnet_amd.models.model import create_model
    from torchmdnet_amd import workloads as W

    torch.manual_seed(4)
    m = create_model(dict(W.TINY_ARGS, static_shapes=True, prior_model=["ZBL", "D2"], prior_args=[dict(ZD[0]), dict(ZD[1])])).to("cuda")
    z, pos, batch = _mol40()
    replay = m.capture(z, pos, batch)
    e, f = replay()
    e, f = e.clone(), f.clone()
    m.prior_model[0].cutoff_distance = 3.0  # a changed argument: re-uploaded by the next call
    E, F = m(z, pos, batch)
    assert not torch.equal(F, f)
    with pytest.raises(RuntimeError, match="stale HIP graph"):
        replay()


@pytest.mark.parametrize("arch", ["tensornet", "equivariant-transformer"])
def test_parameter_gradient_passes_carry_the_priors(hip_lib, arch):
    """The energies of the parameter-gradient pass do not come through ``energy_and_forces`` (TensorNet: ``_train_forward`` keeps the
    activations; ``parameter_gradients_of``: written by the reverse call): each gets the pass, so with priors they are the prior-free
    energies plus the pass's, and the parameter gradients - the priors have no parameters - are the prior-free model's, bit for bit.
    A force loss keeps exact parameter gradients and warns once that pos.grad lacks the priors' second derivative."""
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    base = dict(W.TINY_ARGS if arch == "tensornet" else W.ET_TINY_ARGS)
    models = []
    for pm, pa in ((["ZBL", "D2"], [dict(ZD[0]), dict(ZD[1])]), (None, None)):
        torch.manual_seed(6)
        m = create_model(dict(base, derivative=False, prior_model=pm, prior_args=pa)).to("cuda")
        m.parameter_gradients = True
        models.append(m)
    m, m0 = models
    z, pos, batch = (t.cuda() for t in _batch([9, 14], first_seed=560))
    Ep, _, _, _ = m.debug_pair_priors(z, pos, batch)
    ge = torch.tensor([0.7, -1.1], device="cuda")
    y, _ = m(z, pos, batch)
    y0, _ = m0(z, pos, batch)
    assert Ep.abs().min() > 1e-3 and _within_one_rounding(y.view(-1), y0.view(-1), Ep)
    (y.view(-1) * ge).sum().backward()
    (y0.view(-1) * ge).sum().backward()
    n = 0
    for (k, p), (_, p0) in zip(m.named_parameters(), m0.named_parameters()):
        if p0.grad is not None:
            assert p.grad is not None and torch.equal(p.grad, p0.grad), k
            n += 1
    assert n > 10
    E1, g1 = m.parameter_gradients_of(z, pos, batch, None, None, 2, ge)
    E0, g0 = m0.parameter_gradients_of(z, pos, batch, None, None, 2, ge)
    assert _within_one_rounding(E1, E0, Ep) and len(g1) == len(g0)
    # force matching: parameter gradients as without the priors, one warning about pos.grad
    m.derivative = m0.derivative = True
    m0.force_position_gradient = False  # the pass the model with priors takes: no H v
    R = torch.randn(pos.shape, generator=torch.Generator().manual_seed(3)).cuda()
    for mod in (m, m0):
        mod.zero_grad()
    yy, F = m(z, pos.clone(), batch)
    ((F * R).sum() + (yy.view(-1) * ge).sum()).backward()
    assert m._warned_prior_pos_grad  # (the warning is issued from the autograd thread: its flag is what is checked)
    yy0, F0 = m0(z, pos.clone(), batch)
    ((F0 * R).sum() + (yy0.view(-1) * ge).sum()).backward()
    assert not torch.equal(F, F0)
    for (k, p), (_, p0) in zip(m.named_parameters(), m0.named_parameters()):
        if p0.grad is not None:
            assert torch.equal(p.grad, p0.grad), k


# ------------------------------------------------------------------------------------------------ 5. refusals on the device
def test_refusals(hip_lib):
    from torchmdnet_amd import _C, priors

    m = _model(*ZD)
    z, pos, batch = _mol40()
    w = torch.ones(z.shape[0], device="cuda")
    with pytest.raises(NotImplementedError, match="pair priors have no HIP path with atom weights"):
        m.energy_and_forces(z, pos, batch, None, None, 1, atom_weights=w)
    with pytest.raises(NotImplementedError, match="pair priors have no HIP path with atom weights"):
        m.hessian(z, pos, method="central", atom_weights=w)
    with pytest.raises(NotImplementedError, match="pair priors have no HIP path with hessian"):
        m.hessian(z, pos, method="analytic")
    with pytest.raises(NotImplementedError, match="second derivatives"):
        m.force_term_parameter_gradients(z, pos, batch, None, None, 1, torch.ones_like(pos), want_hv=True)
    E, F = m(z, pos, batch)  # the handle stays usable
    assert torch.isfinite(E).all() and torch.isfinite(F).all()
    # the C entry answers TMDNET_ERR_INVALID for atom weights, and for more atoms than the brute-force pass serves per molecule
    st, L = m._engine, _C.lib()
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    e = torch.zeros(1, device="cuda")
    args = lambda n, aw: (st.handle, None, ws.data_ptr(), ws.numel(), n, 1, pos.data_ptr(), z.data_ptr(), batch.data_ptr(), None, 0, aw,
                          e.data_ptr(), None, None)
    assert L.tmdnet_pair_priors_add(*args(z.shape[0], w.data_ptr())) == _C.ERR_INVALID
    assert L.tmdnet_pair_priors_add(*args(priors.MAX_MOLECULE_ATOMS + 1, None)) == _C.ERR_INVALID  # (refused before anything is read)
    assert b"32768" in L.tmdnet_last_error(st.handle)
    with pytest.raises(NotImplementedError, match="32768"):
        priors.check_molecule_size(priors.MAX_MOLECULE_ATOMS + 1)  # the host-side size test: nothing that large is allocated
    # a D2 species without a table entry is refused when its z is staged
    bad = _model(None, _prior_args(7.0, [0] + list(range(1, MAX_Z))))
    with pytest.raises(NotImplementedError, match=r"species \[0\]"):
        bad(torch.zeros_like(z), pos, batch)
