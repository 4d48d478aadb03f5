"""-m gpu: Hessians and normal-mode analysis assembled on the device (csrc/tn_vib.hip, torchmdnet_amd/vibrations.py).
1. the C entries without a model: seed + gather recover a known matrix bit for bit, the central quotient and finish equal the host
run of the same statements (tests/vib_host_mirror.py); 2. model.hessian / model.vibrations on tiny TensorNet, Equivariant Transformer
and TensorNet2 models against the fp64 specifications under oracle/ (the second-order pass for the analytic route, the first-order
pass on the same rounded displaced positions for the central route) pushed through tests/vib_oracle.py.  The measured figures go to
vibrations_*.json in the directory $TMDNET_RECORD_DIR names (default: test_records/)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import vib_host_mirror as M
from tests import vib_oracle as O
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu
REL = 1e-4  # REL of tests/test_gpu_hvp.py; also the package's stated force tolerance against the reference (README)
SIZES = [1, 2, 3, 7]
DELTA = 0.01
KINDS = ["tensornet", "et", "tensornet2"]
TN2_TINY = dict(W.TINY_ARGS, model="tensornet2", output_model="ScalarPlusWeightedCoulomb", q_dim=8, q_weights=[1.0, 0.5, 2.0])


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _ragged(sizes, seed):
    zs, ps, bs = [], [], []
    for m, n in enumerate(sizes):
        zz, pp = W.synthetic_molecule(seed + m, n_atoms=n)
        zs.append(torch.from_numpy(zz))
        ps.append(torch.from_numpy(pp))
        bs.append(torch.full((n,), m, dtype=torch.long))
    return torch.cat(zs), torch.cat(ps).float(), torch.cat(bs)


def _record(name, payload):
    out = os.environ.get("TMDNET_RECORD_DIR", "test_records")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"vibrations_{name}.json"), "w") as fh:
        json.dump(payload, fh, indent=1)


# ---- 1. the C entries -------------------------------------------------------------------------------------------------------------------
def _plan_on_device():
    batch = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    fixed = np.zeros(batch.shape, bool)
    fixed[8] = True  # one atom of the 7
    free_idx, fstart, dims = O.plan(batch, fixed)
    return batch, free_idx, fstart, dims, (_dev(batch), _dev(free_idx), _dev(fstart))


@pytest.mark.parametrize("R", [1, 4, 18, 21])
def test_seed_and_gather_recover_a_known_matrix_bit_for_bit(hip_lib, R):
    """Between tmdnet_vib_seed and tmdnet_vib_gather torch applies a known matrix per molecule, hv = H_true v (fp64 product of a
    one-hot seed: exact).  H_true comes back bit for bit for R = 1, 4, D, D + 3, the padding stays zero, and a second run has the same
    bits."""
    batch, free_idx, fstart, dims, (b_d, f_d, s_d) = _plan_on_device()
    N, B, D, n_free = len(batch), len(SIZES), int(dims.max()), len(free_idx)
    rng = np.random.default_rng(10)
    H_true = np.zeros((B, D, D), np.float32)
    for b in range(B):
        H_true[b, :dims[b], :dims[b]] = rng.normal(size=(dims[b], dims[b]))
    Ht = _dev(H_true, torch.float64)
    runs = []
    for _ in range(2):
        H = torch.zeros((B, D, D), dtype=torch.float32, device="cuda")
        v = torch.empty((R * N, 3), dtype=torch.float32, device="cuda")
        for col0 in range(0, D, R):
            assert hip_lib.tmdnet_vib_seed(None, 0, N, B, R, col0, None, _ptr(b_d), _ptr(f_d), _ptr(s_d), 0.0, _ptr(v)) == 0
            hv = torch.full((R, N, 3), 7.0, dtype=torch.float32, device="cuda")  # the fixed atom's rows hold something that must not show
            vr = v.view(R, N, 3)
            for b in range(B):
                idx = f_d[fstart[b]:fstart[b + 1]]
                d = int(dims[b])
                vb = vr[:, idx, :].reshape(R, d).double()
                hv[:, idx, :] = (vb @ Ht[b, :d, :d].T).float().reshape(R, -1, 3)
            hv = hv.reshape(R * N, 3).contiguous()
            assert hip_lib.tmdnet_vib_gather(None, 0, N, B, n_free, D, R, col0, _ptr(b_d), _ptr(f_d), _ptr(s_d), _ptr(hv), None, None, None,
                                             _ptr(H)) == 0
        torch.cuda.synchronize()
        runs.append(H.cpu().numpy())
    assert np.array_equal(runs[0], H_true)
    assert runs[0].tobytes() == runs[1].tobytes()


def test_central_gather_equals_the_host_mirror_bit_for_bit(hip_lib):
    """Displaced positions from the device, forces of a quadratic form from torch (fp64, rounded once); the same arrays through the
    host run of the header: the displaced positions and H have the same bits."""
    batch, free_idx, fstart, dims, (b_d, f_d, s_d) = _plan_on_device()
    N, B, D, n_free, R = len(batch), len(SIZES), int(dims.max()), len(free_idx), 4
    rng = np.random.default_rng(11)
    pos = (50 + 3 * rng.normal(size=(N, 3))).astype(np.float32)
    K = rng.normal(size=(3 * N, 3 * N))
    K = 0.5 * (K + K.T) * (np.repeat(batch, 3)[:, None] == np.repeat(batch, 3)[None, :])
    Kd, p_d = _dev(K), _dev(pos)
    H = torch.zeros((B, D, D), dtype=torch.float32, device="cuda")
    Hh = np.zeros((B, D, D), np.float32)
    xp, xm = (torch.empty((R * N, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    for col0 in range(0, D, R):
        for mode, x in ((1, xp), (2, xm)):
            assert hip_lib.tmdnet_vib_seed(None, mode, N, B, R, col0, _ptr(p_d), _ptr(b_d), _ptr(f_d), _ptr(s_d), DELTA, _ptr(x)) == 0
        fp = (-(xp.view(R, 3 * N).double() @ Kd)).float().view(R * N, 3).contiguous()
        fm = (-(xm.view(R, 3 * N).double() @ Kd)).float().view(R * N, 3).contiguous()
        assert hip_lib.tmdnet_vib_gather(None, 1, N, B, n_free, D, R, col0, _ptr(b_d), _ptr(f_d), _ptr(s_d), _ptr(fp), _ptr(fm), _ptr(xp),
                                         _ptr(xm), _ptr(H)) == 0
        torch.cuda.synchronize()
        xph, xmh = M.seed(M.PLUS, pos, batch, free_idx, fstart, R, col0, DELTA), M.seed(M.MINUS, pos, batch, free_idx, fstart, R, col0, DELTA)
        assert xph.tobytes() == xp.cpu().numpy().tobytes() and xmh.tobytes() == xm.cpu().numpy().tobytes()
        M.gather(M.CENTRAL, Hh, batch, free_idx, fstart, R, col0, fp.cpu().numpy(), fm.cpu().numpy(), xph, xmh)
    assert H.cpu().numpy().tobytes() == Hh.tobytes()
    for b in range(B):  # and it is the quadratic form's matrix, to the rounding of the forces over the step
        idx = (3 * free_idx[fstart[b]:fstart[b + 1], None] + np.arange(3)[None, :]).reshape(-1)
        want = K[np.ix_(idx, idx)]
        fmax = np.abs(pos.reshape(-1).astype(np.float64) @ K).max()
        assert np.abs(Hh[b, :dims[b], :dims[b]] - want).max() <= 4 * fmax * 2.0**-24 / DELTA


@pytest.mark.parametrize("project", [0, 1, 2])
def test_finish_equals_the_host_mirror(hip_lib, project):
    """The spring networks of the host tests: A within 1e-12 of the host run relative to max |A| (the device may contract an fp64
    product into the sum that consumes it), the diagnostics and the ranks equal, and a repeat bit-identical."""
    batch, fixed, pos, mass, H, mol_atoms = O.spring_network()
    free_idx, fstart, dims = O.plan(batch, fixed)
    B, D, N = H.shape[0], H.shape[1], len(batch)
    Ah, ih = M.finish(H, pos, mass, free_idx, fstart, project, mol_atoms)
    nb = C.c_size_t(0)
    assert hip_lib.tmdnet_vib_workspace_bytes(B, D, C.byref(nb)) == 0
    ws = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    t = [_dev(a) for a in (H, pos, mass, free_idx, fstart, mol_atoms.astype(np.int64))]
    outs = []
    for _ in range(2):
        A = torch.full((B, D, D), float("nan"), dtype=torch.float64, device="cuda")
        info = torch.full((B, 8), float("nan"), dtype=torch.float64, device="cuda")
        assert hip_lib.tmdnet_vib_finish(None, _ptr(ws), ws.numel(), N, B, D, project, *[_ptr(x) for x in t], _ptr(A), _ptr(info)) == 0
        torch.cuda.synchronize()
        outs.append((A.cpu().numpy(), info.cpu().numpy()))
    (A, info), (A2, info2) = outs
    assert A.tobytes() == A2.tobytes() and info.tobytes() == info2.tobytes()
    assert np.array_equal(info[:, [0, 1, 3, 4, 5, 6, 7]], ih[:, [0, 1, 3, 4, 5, 6, 7]])
    assert np.abs(info[:, 2] - ih[:, 2]).max() <= 1e-12 * ih[:, 0].max()
    for b in range(B):
        scale = np.abs(Ah[b]).max()
        assert np.abs(A[b] - Ah[b]).max() <= 1e-12 * scale, (b, np.abs(A[b] - Ah[b]).max() / scale)


# ---- 2. through the model ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(kind):
    """model, inputs and the fp64 specification's view of them; built once per architecture"""
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(41)
    z, pos, batch = _ragged(SIZES, seed=2100)
    q = None
    if kind == "tensornet":
        from oracle import tensornet_second_order as S2
        from oracle import tensornet_torch as T1

        args = dict(W.TINY_ARGS)
    elif kind == "et":
        from oracle import et_second_order as S2
        from oracle import et_torch as T1

        args = dict(W.ET_TINY_ARGS)
    else:
        from oracle import tn2_second_order as S2
        from oracle import tn2_torch as T1

        args = dict(TN2_TINY)
        q = torch.tensor([float(m % 3 - 1) for m in range(len(SIZES))])
    model = create_model(dict(args)).to("cuda")
    sd64 = {k: (t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu()) for k, t in model.state_dict().items()}
    return dict(kind=kind, model=model, args=args, sd64=sd64, hp=T1.hparams_from_args(args), z=z, pos=pos, batch=batch, q=q, box=None,
                first=T1, second=S2)


def _spec_hv(c, z, pos, batch, v, box, q):
    kw = {} if c["kind"] == "et" else dict(q=None if q is None else q.double())
    return c["second"].force_term(c["sd64"], c["hp"], z, pos.double(), batch, v, box=None if box is None else box.double(), **kw)["Hv"]


def _spec_forces(c, z, pos64, batch, box, q):
    kw = {} if c["kind"] == "et" else dict(q=None if q is None else q.double())
    return c["first"].energy_and_forces(c["sd64"], c["hp"], z, pos64, batch, box=None if box is None else box.double(), **kw)[1].detach()


def _replicated(c, R, fixed=None):
    z, batch, q = c["z"], c["batch"], c["q"]
    B = int(batch.max()) + 1
    zr = z.repeat(R)
    br = (batch[None, :] + B * torch.arange(R)[:, None]).reshape(-1)
    qr = None if q is None else q.repeat(R)
    return zr, br, qr


def _spec_hessian(c, fixed=None, chunk=24):
    """H [B, D, D] fp64 of the specification: the second-order pass on replicated batches with unit seeds, `chunk` columns at a time"""
    z, pos, batch = c["z"], c["pos"], c["batch"]
    free_idx, fstart, dims = O.plan(batch.numpy(), fixed)
    N, B, D = len(z), len(dims), int(dims.max())
    H = np.zeros((B, D, D))
    for col0 in range(0, D, chunk):
        R = min(chunk, D - col0)
        zr, br, qr = _replicated(c, R)
        v = torch.from_numpy(M.seed(M.SEED, None, batch.numpy(), free_idx, fstart, R, col0)).double()
        hv = _spec_hv(c, zr, pos.repeat(R, 1), br, v, c["box"], qr).reshape(R, N, 3).numpy()
        for r in range(R):
            for b in range(B):
                if col0 + r < dims[b]:
                    idx = free_idx[fstart[b]:fstart[b + 1]]
                    H[b, :dims[b], col0 + r] = hv[r, idx, :].reshape(-1)
    return H, (free_idx, fstart, dims)


@functools.lru_cache(maxsize=None)
def _reference(kind):
    """the specification's Hessian of a case and the analytic route's (one pass), shared by the tests that need them"""
    c = _case(kind)
    H_ref, plan = _spec_hessian(c)
    g = lambda t: None if t is None else t.cuda()
    H, info = c["model"].hessian(g(c["z"]), g(c["pos"]), g(c["batch"]), q=g(c["q"]))
    torch.cuda.synchronize()
    return H_ref, plan, H.cpu().numpy().copy(), info


def _over(err, scale):
    """err / scale; a scale of zero (the single atom: no pair, the specification's Hessian is exactly zero) admits no error at all"""
    return float(err / scale) if scale > 0 else (0.0 if err == 0 else float("inf"))


def _rel_errors(H, H_ref, dims):
    """per molecule max |dH| / hmax"""
    return [_over(np.abs(H[b, :d, :d] - H_ref[b, :d, :d]).max(), np.abs(H_ref[b, :d, :d]).max()) for b, d in enumerate(dims)]


@pytest.mark.parametrize("kind", KINDS)
def test_analytic_hessian_matches_the_specification(hip_lib, kind):
    """max |dH| < 1e-4 hmax per molecule against oracle/*_second_order.force_term(...)["Hv"], sizes [1, 2, 3, 7]; asym <= 2e-4 hmax;
    the padding is zero; one pass (R = D) with one graph build beyond the pair count's."""
    H_ref, (free_idx, fstart, dims), H, info = _reference(kind)
    errs = _rel_errors(H, H_ref, dims)
    asym = [_over(np.abs(H[b, :d, :d] - H[b, :d, :d].T).max(), np.abs(H_ref[b, :d, :d]).max()) for b, d in enumerate(dims)]
    _record(f"analytic_{kind}", dict(case=kind, sizes=SIZES, rel_error_per_molecule=errs, asym_over_hmax=asym, replicas=info["replicas"],
                                     passes=info["passes"], engine_calls=info["engine_calls"]))
    print(kind, "analytic rel errors", errs, "asym", asym)
    assert info["dims"] == [3, 6, 9, 21] and info["replicas"] == 21 and info["passes"] == 1 and info["engine_calls"] == 1
    for b, d in enumerate(dims):
        assert not H[b, d:, :].any() and not H[b, :, d:].any()
    assert max(errs) < REL, errs
    assert max(asym) <= 2 * REL, asym


@pytest.mark.parametrize("kind", KINDS)
def test_replica_counts_agree_and_a_repeat_is_bit_identical(hip_lib, kind):
    """R = 1, R = 5 and one pass agree within 1e-4 hmax (bit identity across R is not claimed: the GEMM routes depend on the row
    count); the same R twice has the same bits."""
    c = _case(kind)
    H_ref, (_, _, dims), H_all, _ = _reference(kind)
    g = lambda t: None if t is None else t.cuda()
    out = {}
    for R in (1, 5, 5):
        H, info = c["model"].hessian(g(c["z"]), g(c["pos"]), g(c["batch"]), q=g(c["q"]), replicas=R)
        torch.cuda.synchronize()
        assert info["replicas"] == R and info["passes"] == -(-21 // R) == info["engine_calls"] and info["graph_builds"] == 1
        if R in out:
            assert out[R].tobytes() == H.cpu().numpy().tobytes()
        out[R] = H.cpu().numpy()
    for a, b_ in ((out[1], out[5]), (out[1], H_all), (out[5], H_all)):
        assert max(_rel_errors(a, b_, dims)) < REL
    assert max(_rel_errors(out[1], H_ref, dims)) < REL and max(_rel_errors(out[5], H_ref, dims)) < REL


def _masses(z):
    from torchmdnet_amd.atomic_masses import atomic_masses

    return atomic_masses[z.numpy()].astype(np.float32)


@pytest.mark.parametrize("kind", KINDS)
def test_spectrum_against_the_specification(hip_lib, kind):
    """The eigenvalues of model.vibrations against those of the specification's Hessian pushed through tests/vib_oracle.py:
    |d lambda| <= D 1e-4 max |A| (Weyl, for a perturbation whose entries are bounded by REL max |A|); n_projected = 3, 5, 5 or 6, 6;
    at least that many |lambda| below the bound."""
    c = _case(kind)
    H_ref, (free_idx, fstart, dims), _, _ = _reference(kind)
    g = lambda t: None if t is None else t.cuda()
    vib = c["model"].vibrations(g(c["z"]), g(c["pos"]), g(c["batch"]), q=g(c["q"]))
    mass = _masses(c["z"])
    A_ref, info_ref = O.finish(H_ref, c["pos"].numpy(), mass, free_idx, fstart, 2)
    lam_ref = O.spectrum(A_ref, dims)
    assert vib.n_projected.tolist() == info_ref[:, 3].astype(int).tolist()
    assert vib.n_projected[0] == 3 and vib.n_projected[1] == 5 and vib.n_projected[2] in (5, 6) and vib.n_projected[3] == 6
    worst = []
    for b, d in enumerate(dims):
        bound = d * REL * np.abs(A_ref[b]).max()
        lam = vib.eigenvalues[b].numpy()
        worst.append(_over(np.abs(lam - lam_ref[b]).max(), bound))
        assert np.abs(lam - lam_ref[b]).max() <= bound, (b, worst)
        assert (np.abs(lam) <= bound).sum() >= int(vib.n_projected[b])
        assert abs(vib.amax[b].item() - np.abs(A_ref[b]).max()) <= REL * d * np.abs(A_ref[b]).max()
    _record(f"spectrum_{kind}", dict(case=kind, eigenvalue_error_over_bound=worst, n_projected=vib.n_projected.tolist(),
                                     wavenumbers=[w.tolist() for w in vib.wavenumbers()]))


@pytest.mark.parametrize("kind", KINDS)
def test_central_hessian_matches_the_first_order_specification(hip_lib, kind):
    """delta = 0.01: the same difference quotient evaluated by the fp64 first-order specification on the SAME rounded displaced
    positions (so truncation cancels): max |dH| <= 1e-4 Fmax / delta, Fmax the largest force component over the displaced
    geometries.  Central minus analytic is recorded, not asserted."""
    c = _case(kind)
    _, (free_idx, fstart, dims), H_an, _ = _reference(kind)
    g = lambda t: None if t is None else t.cuda()
    H, info = c["model"].hessian(g(c["z"]), g(c["pos"]), g(c["batch"]), q=g(c["q"]), method="central", delta=DELTA)
    torch.cuda.synchronize()
    H = H.cpu().numpy()
    N, B, D = len(c["z"]), len(dims), int(dims.max())
    R = D
    assert info["replicas"] == R and info["passes"] == 1 and info["engine_calls"] == 2
    b_np, pos = c["batch"].numpy(), c["pos"].numpy()
    xp, xm = (M.seed(mode, pos, b_np, free_idx, fstart, R, 0, DELTA) for mode in (M.PLUS, M.MINUS))
    zr, br, qr = _replicated(c, R)
    fp = _spec_forces(c, zr, torch.from_numpy(xp).double(), br, None, qr).numpy().reshape(R, N, 3)
    fm = _spec_forces(c, zr, torch.from_numpy(xm).double(), br, None, qr).numpy().reshape(R, N, 3)
    fmax = max(np.abs(fp).max(), np.abs(fm).max())
    den = (xp.astype(np.float64) - xm.astype(np.float64)).reshape(R, N, 3)
    H_ref = np.zeros((B, D, D))
    for b in range(B):
        idx = free_idx[fstart[b]:fstart[b + 1]]
        for k in range(dims[b]):
            ak, ck = O.coordinate(free_idx, fstart, b, k)
            H_ref[b, :dims[b], k] = (-(fp[k, idx, :] - fm[k, idx, :]) / den[k, ak, ck]).reshape(-1)
    err = [float(np.abs(H[b, :d, :d] - H_ref[b, :d, :d]).max()) for b, d in enumerate(dims)]
    bound = REL * fmax / DELTA
    minus_analytic = [_over(np.abs(H[b, :d, :d] - H_an[b, :d, :d]).max(), np.abs(H_an[b, :d, :d]).max()) for b, d in enumerate(dims)]
    _record(f"central_{kind}", dict(case=kind, delta=DELTA, max_abs_error_per_molecule=err, bound=bound, fmax=float(fmax),
                                    error_over_bound=max(err) / bound, central_minus_analytic_over_hmax=minus_analytic))
    print(kind, "central: err", err, "bound", bound, "central - analytic", minus_analytic)
    for b, d in enumerate(dims):
        assert not H[b, d:, :].any() and not H[b, :, d:].any()
    assert max(err) <= bound, (err, bound)


def test_periodic_box_projects_translations_only(hip_lib, golden_dir):
    """The geometry of tests/golden/tiny_pbc_ref.pt (40 atoms, triclinic box): the analytic Hessian against the specification at
    1e-4 hmax, rank 3, the spectrum within the Weyl bound."""
    from oracle import tensornet_second_order as S2
    from oracle import tensornet_torch as T
    from torchmdnet_amd.models.model import create_model

    tiny = torch.load(os.path.join(golden_dir, "tiny_ref.pt"))
    f = torch.load(os.path.join(golden_dir, "tiny_pbc_ref.pt"))
    model = create_model(dict(f["args"]))
    model.load_state_dict(tiny["state_dict"])
    model = model.to("cuda")
    c = dict(kind="tensornet", sd64=T.cast_state_dict(tiny["state_dict"], torch.float64), hp=T.hparams_from_args(f["args"]), z=f["z"],
             pos=f["pos"].float(), batch=f["batch"], q=None, box=f["box"], first=T, second=S2)
    H_ref, (free_idx, fstart, dims) = _spec_hessian(c)
    vib = model.vibrations(c["z"].cuda(), c["pos"].cuda(), c["batch"].cuda(), box=c["box"].cuda(), replicas=40)
    H = vib.hessian.cpu().numpy()
    errs = _rel_errors(H, H_ref, dims)
    A_ref, info_ref = O.finish(H_ref, c["pos"].numpy(), _masses(c["z"]), free_idx, fstart, 1)
    lam_ref = O.spectrum(A_ref, dims)[0]
    bound = dims[0] * REL * np.abs(A_ref[0]).max()
    lam = vib.eigenvalues[0].numpy()
    _record("periodic", dict(rel_error=errs, eigenvalue_error_over_bound=float(np.abs(lam - lam_ref).max() / bound), passes=vib.passes))
    assert vib.passes == 3 and vib.engine_calls == 3 and dims[0] == 120
    assert max(errs) < REL, errs
    assert vib.n_projected.tolist() == [3] and info_ref[0, 3] == 3
    assert np.abs(lam - lam_ref).max() <= bound and (np.abs(lam) <= bound).sum() >= 3


def test_fixed_atoms_give_the_sub_block_without_projection_in_fewer_passes(hip_lib):
    """Three atoms of the 7 and the single atom fixed: the partial Hessian equals the sub-block of the full one within 1e-4 hmax, no
    molecule with a fixed atom is projected, a molecule without a free atom yields an empty block, and fewer engine calls run."""
    c = _case("tensornet")
    _, (free_all, fstart_all, dims_all), H_full, info_full = _reference("tensornet")
    fixed = torch.zeros(len(c["z"]), dtype=torch.bool)
    fixed[[0, 6, 8, 11]] = True  # the single atom; atoms 0, 2 and 5 of the 7
    R = 4
    vib = c["model"].vibrations(c["z"].cuda(), c["pos"].cuda(), c["batch"].cuda(), fixed=fixed.cuda(), replicas=R)
    full = c["model"].hessian(c["z"].cuda(), c["pos"].cuda(), c["batch"].cuda(), replicas=R)[1]
    assert vib.dims == [0, 6, 9, 12] and vib.passes == 3 == vib.engine_calls and full["engine_calls"] == 6 > vib.engine_calls
    assert vib.n_projected.tolist() == [0, 5, vib.n_projected[2].item(), 0] and vib.n_projected[2] in (5, 6)
    assert vib.eigenvalues[0].numel() == 0 and vib.modes[0].shape == (0, 0)
    H = vib.hessian.cpu().numpy()
    assert H.shape == (4, 12, 12)
    keep = np.repeat(~fixed[6:13].numpy(), 3)
    sub = H_full[3][np.ix_(keep, keep)]
    hmax = np.abs(H_full[3]).max()
    assert np.abs(H[3] - sub).max() < REL * hmax
    assert np.abs(H[1, :6, :6] - H_full[1, :6, :6]).max() < REL * np.abs(H_full[1]).max() and not H[0].any()
    assert abs(vib.hmax[3].item() - np.abs(H[3]).max()) == 0.0


def test_result_object_and_refusals_on_the_device(hip_lib):
    """vibrations(...) fields have the documented shapes and units; the refusals raise before any launch (the engine-call counter
    of a later call starts from zero and the model stays usable); a property head is refused."""
    from torchmdnet_amd import vibrations as V
    from torchmdnet_amd.models.model import create_model

    c = _case("tensornet")
    z, pos, batch = c["z"].cuda(), c["pos"].cuda(), c["batch"].cuda()
    model = c["model"]
    for kw in (dict(batch=batch.flip(0)), dict(batch=batch, delta=0.0), dict(batch=batch, method="forward"),
               dict(batch=batch, fixed=torch.zeros(3, dtype=torch.bool, device="cuda")), dict(batch=batch, q=torch.zeros(2, device="cuda")),
               dict(batch=batch, masses=torch.zeros(13, device="cuda"))):
        with pytest.raises(ValueError):
            model.vibrations(z, pos, **kw)
    with pytest.raises(NotImplementedError):
        model.hessian(z, pos, batch, atom_weights=torch.ones(13, device="cuda"))
    head = create_model(dict(W.TINY_ARGS, output_model="DipoleMoment")).to("cuda")
    with pytest.raises(NotImplementedError):
        head.vibrations(z, pos, batch)
    with pytest.raises(NotImplementedError):
        head.hessian(z, pos, batch, method="central")
    masses = torch.from_numpy(_masses(c["z"])).cuda()
    vib = model.vibrations(z, pos, batch, masses=masses, method="central")
    B, D = 4, 21
    assert isinstance(vib, V.Vibrations) and vib.method == "central" and vib.engine_calls == 2
    assert vib.hessian.shape == (B, D, D) and vib.hessian.dtype == torch.float32 and vib.hessian.is_cuda
    assert [tuple(l.shape) for l in vib.eigenvalues] == [(3,), (6,), (9,), (21,)] and all(l.dtype == torch.float64 for l in vib.eigenvalues)
    assert [tuple(m.shape) for m in vib.modes] == [(3, 3), (6, 6), (9, 9), (21, 21)]
    for lam in vib.eigenvalues:
        assert bool((lam[1:] >= lam[:-1]).all())
    for t in (vib.n_projected, vib.asymmetry, vib.drift, vib.hmax, vib.amax):
        assert tuple(t.shape) == (B,)
    for b in range(B):  # the modes are orthonormal, and A v = lambda v reproduces the eigenvalues' units: omega2 = lambda * force_scale
        m = vib.modes[b]
        assert torch.allclose(m.T @ m, torch.eye(m.shape[0], dtype=torch.float64), atol=1e-10)
        assert torch.equal(vib.omega2[b], vib.eigenvalues[b] * 9.648533e-3)
        w = vib.wavenumbers()[b]
        assert torch.allclose(w.abs(), vib.eigenvalues[b].abs().sqrt() * 521.4709) and bool((torch.sign(w) == torch.sign(vib.eigenvalues[b])).all())
        d = vib.displacements()[b]
        sm = torch.from_numpy(_masses(c["z"])).double()[c["batch"] == b].repeat_interleave(3).sqrt()
        assert torch.allclose(d * sm[:, None], m)
    assert tuple(vib.zero_point_energy().shape) == (B,) and bool((vib.zero_point_energy() >= 0).all())
    assert len(vib.n_negative()) == B
    # no projection on request: the rank is zero; the acoustic sum adds n entries, each good to REL hmax, of an exact sum of zero
    raw = model.vibrations(z, pos, batch, masses=masses, project=False)
    assert raw.n_projected.tolist() == [0, 0, 0, 0]
    assert bool((raw.drift <= torch.tensor(SIZES, dtype=torch.float64) * REL * raw.hmax).all()), (raw.drift, raw.hmax)
