"""Virial of the TensorNet and Equivariant Transformer force pass on the GPU (tmdnet_energy_forces_virial, tn_virial.hip).

Specification: tests/virial_oracle.py, fp64 autograd of the oracles through a per-molecule strain.  Error of W: max-norm relative to
max |W_ref| per call; bound 1e-4, the project's fp32 contract (BASELINE.json), which the fp32 eager oracles alone meet with two
orders of magnitude to spare (3.5e-7 .. 2.4e-6 on these cases, on the CPU).  Every case also checks E and F against the same oracle
call.  Every measured error is printed before it is asserted; with TMDNET_VIRIAL_PARITY_JSON set they are also written to that
file (the source of profiles/virial_parity.json).

Models: W.TINY_ARGS / W.ET_TINY_ARGS (F = 32, L = 2) with a non-trivial mean and std, one per architecture for the whole module; the
oracle's results are computed once per case and shared by the tests that need them."""
import atexit
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu

BOUND = 1e-4
TRICLINIC = torch.tensor([[11.0, 0.0, 0.0], [1.5, 12.0, 0.0], [-1.0, 0.7, 13.0]])
ARCHS = ("tensornet", "et")

_models, _refs, _record = {}, {}, {}


def _dump_record():
    path = os.environ.get("TMDNET_VIRIAL_PARITY_JSON")
    if path and _record:
        with open(path, "w") as fh:
            json.dump({"bound": BOUND, "error": "max |x - x_ref| / max |x_ref| against the fp64 oracle, per call", "cases": _record},
                      fh, indent=1, sort_keys=True)


atexit.register(_dump_record)


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


def _args(arch, **over):
    return dict(W.TINY_ARGS if arch == "tensornet" else W.ET_TINY_ARGS, **over)


def _model(arch, **over):
    from torchmdnet_amd.models.model import create_model

    key = (arch, tuple(sorted(over.items())))
    if key not in _models:
        torch.manual_seed(0)  # the same weights whatever `over` holds (static_shapes)
        _models[key] = create_model(_args(arch, **over), mean=torch.tensor(-0.4), std=torch.tensor(1.7)).to("cuda")
    return _models[key]


def _sd(arch, **over):
    return {k: v.detach().cpu() for k, v in _model(arch, **over).state_dict().items()}


# ------------------------------------------------------------------------------------------------ inputs
def _ragged():
    zs, ps, bs = [], [], []
    for m, n in enumerate([7, 12, 20]):
        z, p = W.synthetic_molecule(40 + m, n)
        zs.append(torch.from_numpy(z))
        ps.append(torch.from_numpy(p) + 3.0 * m)
        bs.append(torch.full((n,), m, dtype=torch.long))
    return torch.cat(zs), torch.cat(ps), torch.cat(bs), None


def _triclinic2():
    """24 atoms spread over the WHOLE cell of each molecule (uniform fractional coordinates, at least 0.9 A apart under the minimum
    image): as many pairs cross a cell face as not, so the box gradient is of the size of the two terms it is the difference of
    (a cluster in the middle of the cell would make it a small difference of large terms: ill-conditioned in fp32 for any code)."""
    rng = np.random.default_rng(50)
    boxes = torch.stack([TRICLINIC, TRICLINIC * 1.05])
    shifts = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.float64)
    zs, ps = [], []
    for m in range(2):
        b = boxes[m].double().numpy()
        frac = np.empty((0, 3))
        while frac.shape[0] < 24:
            cand = rng.uniform(0.0, 1.0, size=3)
            d = ((frac - cand)[:, None, :] + shifts[None, :, :]) @ b
            if frac.shape[0] == 0 or np.sqrt((d * d).sum(-1)).min() >= 0.9:
                frac = np.vstack([frac, cand])
        zs.append(torch.from_numpy(rng.choice(np.array([1, 6, 7, 8]), size=24)))
        ps.append(torch.from_numpy(frac @ b).float())
    batch = torch.repeat_interleave(torch.arange(2), 24)
    return torch.cat(zs), torch.cat(ps), batch, boxes


def _water(n_side, shear=False, shift=0.0):
    z, pos, box = W.water_box(n_side=n_side)
    if shear:  # same fractional coordinates in the sheared box
        frac = pos.double() @ torch.linalg.inv(box.double())
        box = box.clone()
        box[1, 0], box[2, 0], box[2, 1] = 1.3, -0.9, 0.8
        pos = (frac @ box.double()).float()
    return z, pos + shift, torch.zeros_like(z), box


def _big_open():
    z, p = W.synthetic_molecule(60, 3000)
    return torch.from_numpy(z), torch.from_numpy(p), torch.zeros(3000, dtype=torch.long), None


def _two_in_one_box():
    z, pos, box = W.water_box(n_side=10)  # 3 000 atoms in a 31 A box; 2 200 of them, dealt at random to two molecules of 1 100
    pick = torch.from_numpy(np.random.default_rng(8).permutation(3000)[:2200].copy())
    return z[pick], pos[pick], torch.repeat_interleave(torch.arange(2), 1100), box


CASES = {
    "ragged_open": _ragged,
    "triclinic_per_molecule": _triclinic2,
    "water192": lambda: _water(4),
    "water648": lambda: _water(6),
    "water1029_sheared": lambda: _water(7, shear=True),
    "open3000": _big_open,
    "two_molecules_one_box": _two_in_one_box,
}


def _inputs(case):
    return CASES[case]()


def _ref(arch, case, num_systems=None, **over):
    """fp64 oracle (E, F, W) of a case (`over`: hyper-parameters off the tiny ones), once per session."""
    from tests import virial_oracle as VO

    key = (arch, case, num_systems, tuple(sorted(over.items())))
    if key not in _refs:
        z, pos, batch, box = _inputs(case)
        _refs[key] = VO.energy_forces_virial(_args(arch, **over), _sd(arch, **over), z, pos, batch, box, num_systems=num_systems)
    return _refs[key]


def _run(model, z, pos, batch, box, **kw):
    return model.energy_forces_virial(z.cuda(), pos.cuda(), batch.cuda(), None if box is None else box.cuda(), **kw)


def _check(arch, case, tag=None, **over):
    model = _model(arch, **over)
    z, pos, batch, box = _inputs(case)
    E, F, Wv = _run(model, z, pos, batch, box)
    Er, Fr, Wr = _ref(arch, case, **over)
    assert E.shape == (Er.shape[0], 1) and F.shape == Fr.shape and Wv.shape == Wr.shape and Wv.dtype == torch.float32
    errs = {"E": rel_err(E, Er), "F": rel_err(F, Fr), "W": rel_err(Wv, Wr)}
    print(f"[virial] {arch} {tag or case}: " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    _record[f"{arch}/{tag or case}"] = errs
    assert errs["W"] < BOUND and errs["F"] < BOUND and errs["E"] < BOUND, errs
    return E, F, Wv


# ------------------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("case", ["ragged_open", "triclinic_per_molecule", "water192", "water648"])
def test_virial_vs_fp64_oracle(hip_lib, arch, case):
    """Ragged open molecules [7, 12, 20] (TensorNet: fused small schedule), two triclinic per-molecule boxes (box_mode 2), the
    192-atom periodic box (small schedule, brute force) and the 648-atom one (tn_mid.hip)."""
    _check(arch, case)


@pytest.mark.parametrize("arch", ARCHS)
def test_virial_cell_list_sheared_box(hip_lib, arch):
    """1 029 atoms in a sheared box: cell list, renumbered atoms, general schedule."""
    model = _model(arch)
    _check(arch, "water1029_sheared")
    assert model.cell_grid(1029)[3] == 1  # the cell list really ran


def test_virial_recompute_pair_rows(hip_lib):
    """The same with the sweeps interpolating the per-pair rows themselves (TensorNet option recompute_pair_rows): same
    arithmetic, so W is bit-identical to the stored-row result as E and F are.  F = 64 here: the option exists for channel counts
    that are a multiple of 64 only (it needs the merged distance gradient, message_adjoint_gd_ok; the engine answers
    TMDNET_ERR_STATE at F = 32), so this case has its own model and its own fp64 reference."""
    wide = dict(embedding_dimension=64)
    model = _model("tensornet", **wide)
    _, _, W0 = _check("tensornet", "water1029_sheared", tag="water1029_sheared_F64", **wide)
    model.set_engine_option("recompute_pair_rows", 1)
    try:
        _, _, W1 = _check("tensornet", "water1029_sheared", tag="water1029_sheared_F64+recompute_pair_rows", **wide)
    finally:
        model.set_engine_option("recompute_pair_rows", 0)
    assert torch.equal(W0, W1)


def test_virial_molecule_of_several_reduction_slices(hip_lib):
    """One open molecule of 3 000 atoms: three slices of the per-molecule reduction (1 024 atoms each at the most)."""
    _check("tensornet", "open3000")


@pytest.mark.parametrize("arch", ARCHS)
def test_virial_unsorted_batch(hip_lib, arch):
    """A permutation of the ragged case (unsorted `batch`: the engine's slow path, no atom ranges): W per molecule equals the
    sorted result, F equals it mapped back - both within the bound of the oracle and of each other (the atom numbering changes the
    summation order, nothing else)."""
    model = _model(arch)
    z, pos, batch, _ = _inputs("ragged_open")
    Es, Fs, Ws = _run(model, z, pos, batch, None)
    perm = torch.from_numpy(np.random.default_rng(2).permutation(z.shape[0]).copy())
    assert not bool((batch[perm][1:] >= batch[perm][:-1]).all())
    Eu, Fu, Wu = _run(model, z[perm], pos[perm], batch[perm], None)
    assert model._engine.counts[2] == 1  # the graph phase saw an unsorted batch
    Er, Fr, Wr = _ref(arch, "ragged_open")
    errs = {"W": rel_err(Wu, Wr), "F": rel_err(Fu, Fr[perm]), "W_vs_sorted": rel_err(Wu, Ws), "F_vs_sorted": rel_err(Fu, Fs[perm.cuda()])}
    print(f"[virial] {arch} unsorted: {errs}")
    _record[f"{arch}/ragged_open_unsorted"] = errs
    assert max(errs.values()) < BOUND, errs


@pytest.mark.parametrize("arch", ARCHS)
def test_virial_empty_molecules_are_zero(hip_lib, arch):
    """num_systems larger than batch.max() + 1: the trailing molecules have no atoms and get an exactly zero tensor."""
    model = _model(arch)
    z, pos, batch, _ = _inputs("ragged_open")
    E, F, Wv = _run(model, z, pos, batch, None, num_systems=5)
    Er, Fr, Wr = _ref(arch, "ragged_open")
    assert Wv.shape == (5, 3, 3) and E.shape == (5, 1)
    assert torch.equal(Wv[3:], torch.zeros(2, 3, 3, device="cuda"))
    assert rel_err(Wv[:3], Wr) < BOUND and rel_err(F, Fr) < BOUND


@pytest.mark.parametrize("arch", ARCHS)
def test_virial_two_molecules_interleaved_in_one_box(hip_lib, arch):
    """Two 1 100-atom molecules sharing one periodic box: the cell list renumbers them interleaved, the reduction takes the
    molecule index of the engine's order (Graph::bat_c)."""
    model = _model(arch)
    _check(arch, "two_molecules_one_box")
    assert model.cell_grid(2200, 2)[3] == 1


# ------------------------------------------------------------------------------------------------ properties (1 029 atoms)
def _random_rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return torch.from_numpy(q)


@pytest.mark.parametrize("arch", ARCHS)
def test_virial_properties(hip_lib, arch):
    model = _model(arch)
    z, pos, batch, box = _inputs("water1029_sheared")
    E, F, Wv = _run(model, z, pos, batch, box)
    scale = Wv.abs().max().item()
    # symmetric (the full tensor is returned, nothing symmetrises it)
    asym = (Wv - Wv.transpose(1, 2)).abs().max().item() / scale
    # two evaluations: bit-identical
    E2, F2, W2 = _run(model, z, pos, batch, box)
    assert torch.equal(Wv, W2) and torch.equal(E, E2) and torch.equal(F, F2)
    # E and F are those of forward, bit for bit
    Ef, Ff = model(z.cuda(), pos.cuda(), batch.cuda(), box=box.cuda())
    assert torch.equal(E, Ef) and torch.equal(F, Ff)
    # a lattice vector plus 17 A
    shift = (box[0] - 2 * box[1] + box[2] + 17.0).float()
    _, _, Wt = _run(model, z, pos + shift, batch, box)
    trans = rel_err(Wt, Wv)
    # Rotation by a random proper R, then the box back to the lower-triangular form the engine takes (LQ factorisation with a
    # positive diagonal: box R = L Q).  The positions end up rotated by Rt = R Q^T and W must be Rt^T W Rt.  The reduced form of a
    # lattice is unique, so Rt is the identity up to rounding here; the rotations that really turn the system are below.
    R = _random_rotation(4)
    qm, rm = np.linalg.qr((box.double() @ R).numpy().T)  # B^T = qm rm  ->  B = rm^T qm^T
    sgn = np.sign(np.diag(rm))
    Lb, Q = torch.from_numpy((rm.T * sgn)), torch.from_numpy((qm * sgn).T)
    assert torch.allclose(Lb @ Q, box.double() @ R, atol=1e-9) and torch.allclose(torch.triu(Lb, 1), torch.zeros(3, 3, dtype=torch.float64))
    Rt = R @ Q.T
    _, _, Wrot = _run(model, z, (pos.double() @ Rt).float(), batch, Lb.float())
    rot = rel_err(Wrot[0], Rt.T @ Wv[0].cpu().double() @ Rt)
    errs = {"asymmetry": asym, "translation": trans, "rotation_reduced_box": rot}
    print(f"[virial] {arch} properties: {errs}")
    _record[f"{arch}/properties_water1029_sheared"] = errs
    assert max(errs.values()) < BOUND, errs


@pytest.mark.parametrize("arch", ARCHS)
def test_virial_rotates_as_a_tensor(hip_lib, arch):
    """Rotations that do turn the system: a random proper rotation of the open molecules, and the quarter turn about z of the cubic
    192-atom box (it maps the lattice onto itself, so the box stays as it is): W' = R^T W R."""
    model = _model(arch)
    z, pos, batch, _ = _inputs("ragged_open")
    R = _random_rotation(9)
    _, _, W0 = _run(model, z, pos, batch, None)
    _, _, W1 = _run(model, z, (pos.double() @ R).float(), batch, None)
    e_open = rel_err(W1, R.T @ W0.cpu().double() @ R)
    z, pos, batch, box = _inputs("water192")
    R4 = torch.tensor([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    _, _, W0 = _run(model, z, pos, batch, box)
    _, _, W1 = _run(model, z, (pos.double() @ R4).float(), batch, box)
    e_box = rel_err(W1, R4.T @ W0.cpu().double() @ R4)
    print(f"[virial] {arch} rotation: open={e_open:.3e} cubic_box={e_box:.3e}")
    _record[f"{arch}/rotation"] = {"open_random": e_open, "cubic_box_quarter_turn": e_box}
    assert e_open < BOUND and e_box < BOUND


@pytest.mark.parametrize("arch", ARCHS)
def test_stress_helper_on_device(hip_lib, arch):
    model = _model(arch)
    z, pos, batch, box = _inputs("triclinic_per_molecule")
    _, _, Wv = _run(model, z, pos, batch, box)
    s = model.stress(Wv, box.cuda())
    vol = torch.linalg.det(box.double())
    assert rel_err(s, -Wv.cpu().double() / vol.view(-1, 1, 1)) < 1e-6


# ------------------------------------------------------------------------------------------------ box gradient
@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("case", ["triclinic_per_molecule", "water1029_shifted"])
def test_box_and_position_gradient(hip_lib, arch, case):
    """(E * c).sum().backward() through tmdnet::energy_forces_virial: pos.grad (from F) and box.grad (from W and F, the strain identity
    d E / d eps = X^T d E / d X + H^T d E / d H) against plain fp64 autograd of the oracle, 1e-4 relative max-norm each.  Per-molecule
    boxes (one gradient per box) and one shared box with the positions 30 A away from the origin."""
    from tests import virial_oracle as VO

    model = _model(arch)
    if case == "water1029_shifted":
        z, pos, batch, box = _water(7, shear=True, shift=30.0)
    else:
        z, pos, batch, box = _inputs(case)
    n_mol = int(batch.max()) + 1
    c = torch.from_numpy(np.random.default_rng(12).uniform(0.5, 1.5, size=n_mol)).float()
    pg = pos.cuda().requires_grad_(True)
    bg = box.cuda().requires_grad_(True)
    E, F, Wv = model.energy_forces_virial(z.cuda(), pg, batch.cuda(), bg)
    (E * c.cuda().view(-1, 1)).sum().backward()
    g_pos, g_box = VO.energy_gradients(_args(arch), _sd(arch), z, pos, batch, box, c)
    errs = {"pos_grad": rel_err(pg.grad, g_pos), "box_grad": rel_err(bg.grad, g_box)}
    print(f"[virial] {arch} {case} gradients: {errs}")
    _record[f"{arch}/gradient_{case}"] = errs
    assert bg.grad.shape == box.shape and max(errs.values()) < BOUND, errs
    # second derivatives are not implemented: a gradient of F or W raises
    E, F, Wv = model.energy_forces_virial(z.cuda(), pos.cuda().requires_grad_(True), batch.cuda(), box.cuda())
    with pytest.raises((NotImplementedError, RuntimeError)):
        Wv.sum().backward()
    with pytest.raises((NotImplementedError, RuntimeError)):
        F.sum().backward()


def test_operator_schema_and_fake(hip_lib):
    """torch.library.opcheck of the new operator (schema, fake tensors, autograd registration), as for its neighbours in
    test_gpu_branches.py (which keeps checking tmdnet::energy_forces itself)."""
    from torchmdnet_amd import ops

    model = _model("tensornet")
    z, pos, batch, box = _inputs("triclinic_per_molecule")
    if model._engine.op_key is None:
        model._engine.op_key = ops.register_engine(model)
    key = model._engine.op_key
    pg = pos.cuda().requires_grad_(True)
    bg = box.cuda().requires_grad_(True)
    torch.library.opcheck(torch.ops.tmdnet.energy_forces_virial, (z.cuda(), pg, batch.cuda(), bg, None, key, 2),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))


# ------------------------------------------------------------------------------------------------ captured graph
@pytest.mark.parametrize("arch", ARCHS)
def test_captured_graph_follows_the_box(hip_lib, arch):
    """static_shapes + capture(virial=True) on the 192-atom box; a barostat-style update between replays (box and positions scaled
    in place by 1.01): every replay's (E, F, W) equals an eager call at that geometry bit for bit."""
    model = _model(arch, static_shapes=True)
    z, pos, batch, box = (t.cuda() for t in _inputs("water192"))
    box = box.clone()
    replay = model.capture(z, pos, batch, box, virial=True)
    for step in range(3):
        box.mul_(1.01)
        replay.pos.mul_(1.01)
        E, F, Wv = replay()
        assert Wv is replay.virial and Wv.shape == (1, 3, 3)
        Ee, Fe, We = model.energy_forces_virial(z, replay.pos.clone(), batch, box.clone())
        assert torch.equal(E, Ee) and torch.equal(F, Fe) and torch.equal(Wv, We), step
    assert rel_err(box, W.water_box(n_side=4)[2] * 1.01 ** 3) < 1e-6  # the box really moved
    plain = model.capture(z, pos, batch, box)
    out = plain()
    assert len(out) == 2 and not hasattr(plain, "virial")


# ------------------------------------------------------------------------------------------------ refusals
def _c_entry(model, z, batch, n_mol):
    """tmdnet_energy_forces_virial called directly on the workspaces of the model's last evaluation."""
    from torchmdnet_amd import _C

    L, st = _C.lib(), model._engine
    n = int(z.shape[0])
    nb = C.c_size_t(0)
    assert L.tmdnet_virial_workspace_bytes(st.handle, n, n_mol, C.byref(nb)) == _C.OK
    vws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    E = torch.empty(n_mol, device="cuda")
    F = torch.empty(n, 3, device="cuda")
    Wv = torch.empty(n_mol, 3, 3, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.tmdnet_energy_forces_virial(st.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream), p(st.graph_ws), p(st.fwd_ws),
                                       st.fwd_ws.numel(), p(vws), vws.numel(), n, n_mol, st.counts[0], p(z), p(batch), None, 1, p(E),
                                       p(F), p(Wv))
    torch.cuda.synchronize()
    return rc, E, F, Wv


def test_refusals_of_the_c_entry_and_the_python_surface(hip_lib):
    """Atom weights, a halo exchange, a property head, TensorNet2 and the parameter-gradient mode: TMDNET_ERR_INVALID from the C entry,
    NotImplementedError from Python, and the handle evaluates afterwards as before.  (A TrainCtx exists only while
    tmdnet_energy_param_grads runs, so the C entry's check of it cannot be reached from outside the library: its Python
    counterpart, parameter_gradients=True, is what is tested.)"""
    from torchmdnet_amd import _C
    from torchmdnet_amd.models.model import create_model

    L = _C.lib()
    model = _model("tensornet")
    z, pos, batch, _ = (t.cuda() if t is not None else None for t in _inputs("ragged_open"))
    E0, F0, W0 = model.energy_forces_virial(z, pos, batch)
    st = model._engine
    rc, E, F, Wv = _c_entry(model, z, batch, 3)
    assert rc == _C.OK and torch.equal(Wv, W0) and torch.equal(F, F0) and torch.equal(E.view(-1, 1), E0)
    # atom weights
    w = torch.ones(z.shape[0], device="cuda")
    L.tmdnet_set_atom_weights(st.handle, C.c_void_p(w.data_ptr()))
    assert _c_entry(model, z, batch, 3)[0] == _C.ERR_INVALID
    L.tmdnet_set_atom_weights(st.handle, None)
    with pytest.raises(NotImplementedError):
        model.energy_and_forces(z, pos, batch, None, None, 3, atom_weights=w, want_virial=True)
    # halo exchange
    cb = _C.HALO_EXCHANGE_FN(lambda *a: 0)
    L.tmdnet_set_halo_exchange(st.handle, cb, None)
    assert _c_entry(model, z, batch, 3)[0] == _C.ERR_INVALID
    L.tmdnet_set_halo_exchange(st.handle, _C.HALO_EXCHANGE_FN(), None)
    with pytest.raises(NotImplementedError):
        model.energy_and_forces(z, pos, batch, None, None, 3, halo_exchange=lambda *a: None, want_virial=True)
    # parameter-gradient mode
    model.parameter_gradients = True
    try:
        with pytest.raises(NotImplementedError):
            model.energy_forces_virial(z, pos, batch)
    finally:
        model.parameter_gradients = False
    rc, E, F, Wv = _c_entry(model, z, batch, 3)
    assert rc == _C.OK and torch.equal(Wv, W0)
    E1, F1, W1 = model.energy_forces_virial(z, pos, batch)
    assert torch.equal(W1, W0) and torch.equal(F1, F0) and torch.equal(E1, E0)
    # property heads (both architectures) and TensorNet2
    others = [dict(W.TINY_ARGS, output_model="DipoleMoment"), dict(W.ET_TINY_ARGS, output_model="ElectronicSpatialExtent"),
              dict(W.TINY_ARGS, model="tensornet2", output_model="ScalarPlusWeightedCoulomb", q_dim=4, q_weights=[1.0, 0.5, 0.25],
                   cutoff_upper=4.5, max_z=12)]
    for args in others:
        torch.manual_seed(1)
        other = create_model(dict(args)).to("cuda")
        kw = dict(q=torch.zeros(3, device="cuda")) if args["model"] == "tensornet2" else {}
        Ea, Fa = other(z, pos, batch, **kw)
        assert _c_entry(other, z, batch, 3)[0] == _C.ERR_INVALID
        with pytest.raises(NotImplementedError):
            other.energy_forces_virial(z, pos, batch, **kw)
        with pytest.raises(NotImplementedError):
            other.energy_and_forces(z, pos, batch, None, kw.get("q"), 3, want_virial=True)
        Eb, Fb = other(z, pos, batch, **kw)
        assert torch.equal(Ea, Eb) and torch.equal(Fa, Fb)
