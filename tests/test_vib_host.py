"""No GPU: the arithmetic of the Hessian assembly and normal-mode preparation (csrc/tn_vib_math.h, compiled host-only by
tests/vib_host_mirror.py) against tests/vib_oracle.py - the scheme in fp64 numpy, written from the equations.  1. the index maps of
seed and gather, 2. the central difference quotient, 3. finish on spring networks with known Hessians, 4. the result object, the
refusals, the additive ABI and the signatures, 5. the sanitizers on a stand-alone program."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import vib_host_mirror as M
from tests import vib_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIB_ENTRIES = (("tmdnet_vib_workspace_bytes", 3), ("tmdnet_vib_seed", 12), ("tmdnet_vib_gather", 16), ("tmdnet_vib_finish", 15))
SIZES = [1, 2, 3, 7]
FIXED_ATOM = 8  # one atom of the 7


def _batch():
    batch = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    fixed = np.zeros(batch.shape, bool)
    fixed[FIXED_ATOM] = True
    return batch, fixed


# ---- 1. index maps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 4, 18, 21])
def test_every_valid_entry_is_written_exactly_once(R):
    """Sizes [1, 2, 3, 7], one atom of the 7 fixed, D = 18; R = 1, 4, D, D + 3.  hv carries a code of (replica, atom, component), so
    H[b][i, k] names the row it was read from; the write counts are 1 on every valid (b, i, k) and 0 elsewhere; the fixed atom's
    values appear nowhere; SEED holds exactly one 1.0 per seeded molecule and replica, at the carried coordinate."""
    batch, fixed = _batch()
    free_idx, fstart, dims = O.plan(batch, fixed)
    N, B, D = len(batch), len(SIZES), int(dims.max())
    assert D == 18 and list(dims) == [3, 6, 9, 18]
    H = np.zeros((B, D, D), np.float32)
    writes = np.zeros((B, D, D), np.int32)
    for col0 in range(0, D, R):
        v = M.seed(M.SEED, None, batch, free_idx, fstart, R, col0).reshape(R, N, 3)
        for r in range(R):
            for b in range(B):
                rows = v[r][batch == b]
                k = col0 + r
                if k < dims[b]:
                    atom, comp = O.coordinate(free_idx, fstart, b, k)
                    want = np.zeros((N, 3), np.float32)
                    want[atom, comp] = 1.0
                    assert np.array_equal(rows, want[batch == b])
                else:
                    assert not rows.any()  # fewer columns than k, or the padding of the last pass: unseeded
        code = (1 + np.arange(R * N * 3, dtype=np.float32)).reshape(R * N, 3)  # exact in fp32
        M.gather(M.ANALYTIC, H, batch, free_idx, fstart, R, col0, code, writes=writes)
    for b in range(B):
        d = dims[b]
        assert (writes[b, :d, :d] == 1).all()
        writes[b, :d, :d] = 0
        for i in range(d):
            atom, comp = O.coordinate(free_idx, fstart, b, i)
            for k in range(d):
                r = k % R
                assert H[b, i, k] == 1 + 3 * (r * N + atom) + comp
        H[b, :d, :d] = 0
    assert not writes.any() and not H.any()  # the padding is never touched


def test_displacement_is_one_rounded_addition_and_leaves_the_rest_alone():
    batch, fixed = _batch()
    free_idx, fstart, dims = O.plan(batch, fixed)
    N = len(batch)
    rng = np.random.default_rng(1)
    pos = (100 + rng.normal(size=(N, 3))).astype(np.float32)
    delta = np.float32(0.01)
    R, col0 = 4, 4
    for mode, sign in ((M.PLUS, 1), (M.MINUS, -1)):
        x = M.seed(mode, pos, batch, free_idx, fstart, R, col0, float(delta)).reshape(R, N, 3)
        for r in range(R):
            want = pos.copy()
            for b in range(len(SIZES)):
                if col0 + r < dims[b]:
                    atom, comp = O.coordinate(free_idx, fstart, b, col0 + r)
                    want[atom, comp] = np.float32(pos[atom, comp] + np.float32(sign) * delta)
            assert np.array_equal(x[r], want)
            assert np.array_equal(x[r][FIXED_ATOM], pos[FIXED_ATOM])


# ---- 2. the central difference quotient ---------------------------------------------------------------------------------------------------
def _forces(x, K, c):
    """F = -dE/dx of E = x^T K x / 2 + c sum x^3 over one replica's 3 N coordinates, fp64 at the fp32 positions, rounded once"""
    x = x.astype(np.float64)
    return (-(x @ K) - 3.0 * c * x * x).astype(np.float32)


def test_central_quotient_equals_the_oracle_on_the_same_rounded_positions():
    """Forces of an energy with known third derivatives; molecule-diagonal K so that replicas of other molecules' columns do not mix.
    The header's entry equals the oracle's within 1 fp32 ulp (both round one fp64 quotient: measured 0)."""
    batch, fixed = _batch()
    free_idx, fstart, dims = O.plan(batch, fixed)
    N, B, D, R = len(batch), len(SIZES), int(dims.max()), 4
    rng = np.random.default_rng(2)
    pos = rng.normal(size=(N, 3)).astype(np.float32) * 2
    K = rng.normal(size=(3 * N, 3 * N))
    K = 0.5 * (K + K.T) * (np.repeat(batch, 3)[:, None] == np.repeat(batch, 3)[None, :])
    H = np.zeros((B, D, D), np.float32)
    ref = np.zeros((B, D, D), np.float32)
    for col0 in range(0, D, R):
        xp = M.seed(M.PLUS, pos, batch, free_idx, fstart, R, col0, 0.01)
        xm = M.seed(M.MINUS, pos, batch, free_idx, fstart, R, col0, 0.01)
        fp = np.concatenate([_forces(xp.reshape(R, -1)[r], K, 0.3) for r in range(R)]).reshape(-1, 3)
        fm = np.concatenate([_forces(xm.reshape(R, -1)[r], K, 0.3) for r in range(R)]).reshape(-1, 3)
        M.gather(M.CENTRAL, H, batch, free_idx, fstart, R, col0, fp, fm, xp, xm)
        for r in range(R):
            for b in range(B):
                k = col0 + r
                if k >= dims[b]:
                    continue
                ak, ck = O.coordinate(free_idx, fstart, b, k)
                for i in range(dims[b]):
                    ai, ci = O.coordinate(free_idx, fstart, b, i)
                    ref[b, i, k] = O.central_entry(fp[r * N + ai, ci], fm[r * N + ai, ci], xp[r * N + ak, ck], xm[r * N + ak, ck])
    ulp = np.spacing(np.abs(ref).astype(np.float32))
    assert (np.abs(H.astype(np.float64) - ref.astype(np.float64)) <= ulp).all()
    # and the quotient is the Hessian K + 6 c diag(x) up to truncation (none for this cubic) and the forces' rounding
    for b in range(B):
        idx = np.concatenate([3 * free_idx[fstart[b]:fstart[b + 1], None] + np.arange(3)[None, :]]).reshape(-1)
        want = K[np.ix_(idx, idx)] + np.diag(6 * 0.3 * pos.reshape(-1)[idx].astype(np.float64))
        scale = np.abs(_forces(pos.reshape(-1), K, 0.3)).max() * 2.0**-24 / 0.01  # one rounding of a force over delta
        assert np.abs(H[b, :dims[b], :dims[b]] - want).max() <= 4 * scale + 1e-6 * np.abs(want).max()


def test_the_denominator_is_the_actual_difference_of_the_rounded_positions():
    """|x| ~ 100: delta = 0.01 is not representable on the grid of x (ulp 7.6e-6), so x+ - x- differs from 2 delta in the fourth
    digit.  With F = -k x exact in fp32 (k a power of two) the quotient over the actual difference gives k EXACTLY; over 2 delta it
    would be wrong by up to 4e-4 k."""
    batch = np.zeros(5, np.int64)
    free_idx, fstart, dims = O.plan(batch)
    rng = np.random.default_rng(3)
    pos = (100 + 10 * rng.random(size=(5, 3))).astype(np.float32)
    k = np.float32(0.5)
    D = 15
    H = np.zeros((1, D, D), np.float32)
    xp = M.seed(M.PLUS, pos, batch, free_idx, fstart, D, 0, 0.01)
    xm = M.seed(M.MINUS, pos, batch, free_idx, fstart, D, 0, 0.01)
    M.gather(M.CENTRAL, H, batch, free_idx, fstart, D, 0, -k * xp, -k * xm, xp, xm)
    assert np.array_equal(H[0], k * np.eye(D, dtype=np.float32))
    moved = (xp.astype(np.float64) - xm.astype(np.float64)).reshape(D, -1)[np.arange(D), np.arange(D)]
    naive = k * moved / (2 * 0.01)
    assert np.abs(naive - k).max() > 1e-5 * k  # the test can tell the two denominators apart


# ---- 3. finish -----------------------------------------------------------------------------------------------------------------------------
def test_finish_equals_the_oracle_with_the_documented_ranks():
    batch, fixed, pos, mass, H, mol_atoms = O.spring_network()
    free_idx, fstart, dims = O.plan(batch, fixed)
    for project, ranks in ((2, [6, 5, 5, 3, 0]), (1, [3, 3, 3, 3, 0]), (0, [0, 0, 0, 0, 0])):  # free, with a box, not asked for
        A, info = M.finish(H, pos, mass, free_idx, fstart, project, mol_atoms)
        Ar, inf_r = O.finish(H, pos, mass, free_idx, fstart, project, mol_atoms)
        assert info[:, 3].tolist() == ranks and inf_r[:, 3].tolist() == ranks
        assert info[:, 5].tolist() == list(dims) and info[:, 4].tolist() == [project] * 4 + [0]
        for b in range(len(dims)):
            scale = max(np.abs(Ar[b]).max(), 1e-300)
            assert np.abs(A[b] - Ar[b]).max() <= 1e-12 * scale, (project, b, np.abs(A[b] - Ar[b]).max() / scale)
            d = dims[b]
            assert not A[b, d:, :].any() and not A[b, :, d:].any()  # zero in its padding
        assert np.array_equal(info[:, 0], inf_r[:, 0]) and (info[:, 1] == 0).all()  # hmax; a symmetric input has no asymmetry
        assert np.abs(info[:, 2] - inf_r[:, 2]).max() <= 1e-14 * info[:, 0].max()
    # the projected matrix annihilates the projected vectors, and the count of projected modes is the recorded rank - a chain of
    # central springs has zero-stiffness bends, so zero eigenvalues are NOT counted
    A, info = M.finish(H, pos, mass, free_idx, fstart, 2, mol_atoms)
    lam = O.spectrum(A, dims)
    tol = 1e-10 * np.abs(A).max()
    assert (np.abs(lam[0]) < tol).sum() == 6 and (np.abs(lam[3]) < tol).sum() == 3
    assert (np.abs(lam[1]) < tol).sum() > 5  # 9 coordinates, rank 5, two stretches: the two bends of the collinear chain are soft too
    assert (lam[0] > -tol).all()
    # without mol_atoms (no atom is fixed by the caller's word) the last molecule is projected like the first
    assert M.finish(H, pos, mass, free_idx, fstart, 2, None)[1][4, 3] == 6


def test_diatomic_frequency_is_the_reduced_mass_formula():
    """an axis-aligned diatomic, k = 2: H = k e e^T blocks are exact in fp32, so the one nonzero eigenvalue is k (1/m1 + 1/m2) to 1e-12"""
    batch = np.zeros(2, np.int64)
    free_idx, fstart, dims = O.plan(batch)
    pos = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.5]], np.float32)
    mass = np.array([1.0, 16.0], np.float32)
    H = O.spring_hessian(pos.astype(np.float64), [(0, 1)], [2.0]).astype(np.float32)[None]
    A, info = M.finish(H, pos, mass, free_idx, fstart, 2)
    lam = O.spectrum(A, dims)[0]
    want = 2.0 * (1 / 1.0 + 1 / 16.0)
    assert info[0, 3] == 5 and abs(lam[-1] - want) <= 1e-12 * want and np.abs(lam[:-1]).max() <= 1e-12 * want


def test_planted_asymmetry_and_acoustic_sum_are_reported_exactly():
    """an axis-aligned lattice network with power-of-two springs: every entry is exact, the acoustic sum is exactly zero; a planted
    0.25 on one off-diagonal entry is the asymmetry and the drift, exactly"""
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0]], np.float32)
    bonds = [(0, 1), (0, 2), (0, 3), (1, 4), (2, 4)]
    H = O.spring_hessian(pos.astype(np.float64), bonds, [1.0, 2.0, 0.5, 4.0, 1.0]).astype(np.float32)[None]
    batch = np.zeros(5, np.int64)
    free_idx, fstart, dims = O.plan(batch)
    mass = np.ones(5, np.float32)
    _, info = M.finish(H, pos, mass, free_idx, fstart, 2)
    assert info[0, 0] == np.abs(H).max() and info[0, 1] == 0.0 and info[0, 2] == 0.0
    H[0, 2, 7] += 0.25
    A, info = M.finish(H, pos, mass, free_idx, fstart, 2)
    assert info[0, 1] == 0.25 and info[0, 2] == 0.25
    Ar, _ = O.finish(H, pos, mass, free_idx, fstart, 2)
    assert np.abs(A - Ar).max() <= 1e-12 * np.abs(Ar).max()  # S = (H + H^T) / 2 enters A


# ---- 4. the result object, the refusals, the ABI ---------------------------------------------------------------------------------------
def test_wavenumber_constant():
    from torchmdnet_amd import vibrations as V

    assert abs(O.wavenumber_factor() - V.WAVENUMBER) < 5e-5  # 521.4709 to the digits given
    assert O.WAVENUMBER == V.WAVENUMBER
    # force_scale: 1 eV / (A^2 amu) in fs^-2
    assert abs(1.602176634e-19 / (1e-20 * 1.66053906660e-27) * 1e-30 - 9.648533e-3) < 1e-9


def _hand_made(lams, n_projected):
    import torch

    from torchmdnet_amd import vibrations as V

    dims = [len(l) for l in lams]
    D = max(dims)
    A = torch.zeros(len(lams), D, D, dtype=torch.float64)
    for b, l in enumerate(lams):
        A[b, :len(l), :len(l)] = torch.diag(torch.tensor(l, dtype=torch.float64))
    n_free = [d // 3 for d in dims]
    fstart = torch.tensor(np.concatenate([[0], np.cumsum(n_free)]), dtype=torch.long)
    info = dict(method="analytic", replicas=1, passes=D, engine_calls=D, dims=dims, free_idx=torch.arange(sum(n_free)), fstart=fstart)
    rows = torch.zeros(len(lams), 8, dtype=torch.float64)
    rows[:, 3] = torch.tensor(n_projected, dtype=torch.float64)
    return V.Vibrations(torch.zeros(len(lams), D, D), info, A, rows, torch.full((sum(n_free),), 4.0), 9.648533e-3)


def test_result_object_on_a_hand_made_spectrum():
    import torch

    from torchmdnet_amd import vibrations as V

    vib = _hand_made([[4.0, 1e-9, -1e-9, 0.0, 9.0, -0.25], [1.0, 0.0, 0.0]], [3, 2])
    assert [l.tolist() for l in vib.eigenvalues] == [[-0.25, -1e-9, 0.0, 1e-9, 4.0, 9.0], [0.0, 0.0, 1.0]]
    assert vib.default_tolerance() == [6 * 1e-4 * 9.0, 3 * 1e-4 * 1.0]
    assert vib.n_negative() == [1, 0] and vib.n_negative(tol=0.5) == [0, 0] and vib.n_negative(tol=0.0) == [2, 0]
    w = vib.wavenumbers()[0]
    assert torch.allclose(w[[0, 4, 5]], torch.tensor([-0.5, 2.0, 3.0], dtype=torch.float64) * V.WAVENUMBER)
    # the three eigenvalues of smallest magnitude are the projected ones; of the rest, 4 and 9 are positive
    zpe = vib.zero_point_energy()
    fs = 9.648533e-3
    assert abs(zpe[0].item() - 0.5 * V.HBAR_EV_FS * (np.sqrt(4 * fs) + np.sqrt(9 * fs))) < 1e-15
    assert abs(zpe[1].item() - 0.5 * V.HBAR_EV_FS * np.sqrt(fs)) < 1e-15
    assert torch.equal(vib.omega2[0], vib.eigenvalues[0] * fs)
    disp = vib.displacements()
    assert torch.allclose(disp[0], vib.modes[0] / 2.0) and vib.n_projected.tolist() == [3, 2]  # every mass is 4


def test_refusals_come_before_anything_is_staged():
    """host tensors throughout: every refusal is raised before the first check that the inputs live on a GPU"""
    import torch

    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    model = create_model(dict(W.TINY_ARGS))
    z = torch.tensor([1, 6, 8, 1, 1])
    pos = torch.randn(5, 3)
    batch = torch.tensor([0, 0, 0, 1, 1])
    ok = dict(z=z, pos=pos, batch=batch)
    for kw in (dict(ok, batch=torch.tensor([0, 1, 0, 1, 1])), dict(ok, batch=torch.tensor([1, 1, 1, 0, 0])), dict(ok, delta=0.0),
               dict(ok, delta=-0.01), dict(ok, delta=float("nan")), dict(ok, method="forward"), dict(ok, fixed=torch.zeros(4, dtype=torch.bool)),
               dict(ok, q=torch.zeros(3)), dict(ok, replicas=0), dict(ok, batch=torch.zeros(4, dtype=torch.long))):
        with pytest.raises(ValueError):
            model.hessian(**kw)
        with pytest.raises(ValueError):
            model.vibrations(**kw)
    for masses in (torch.ones(4), torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0]), torch.tensor([1.0, float("inf"), 1.0, 1.0, 1.0]),
                   torch.tensor([1.0, float("nan"), 1.0, 1.0, 1.0]), torch.tensor([1.0, -2.0, 1.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            model.vibrations(**ok, masses=masses)
    with pytest.raises(NotImplementedError):
        model.hessian(**ok, method="analytic", atom_weights=torch.ones(5))
    # a mass that is unusable on a FIXED atom is nobody's business: the request passes the checks and stops at the device check
    fixed = torch.tensor([False, True, False, False, False])
    with pytest.raises(RuntimeError, match="AMD GPU"):
        model.vibrations(**ok, masses=torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0]), fixed=fixed)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        model.hessian(**ok)
    head = create_model(dict(W.TINY_ARGS, output_model="DipoleMoment"))
    for call in (head.hessian, head.vibrations):
        with pytest.raises(NotImplementedError):
            call(**ok)
        with pytest.raises(NotImplementedError):
            call(**ok, method="central")


def test_header_and_bindings_are_additive():
    txt = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    assert re.search(r"#define\s+TMDNET_ABI_VERSION\s+10\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from torchmdnet_amd import _C

    src = open(_C.__file__).read()
    for name, n_args in VIB_ENTRIES:
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == n_args, name
        assert name in _C.declared_symbols() and name + ".argtypes" in src
    for name, n_args in (("tmdnet_loss_param_grads", 15), ("tmdnet_energy_forces", 14), ("tmdnet_neb_advance", 34)):  # untouched
        args = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
        assert len(args.split(",")) == n_args, name
    for name, value in (("SEED", 0), ("PLUS", 1), ("MINUS", 2), ("ANALYTIC", 0), ("CENTRAL", 1), ("PROJECT_NONE", 0), ("PROJECT_TRANS", 1),
                        ("PROJECT_TRANS_ROT", 2), ("INFO", 8)):
        assert re.search(r"#define\s+TMDNET_VIB_" + name + r"\s+" + str(value) + r"\b", txt) and getattr(_C, "VIB_" + name) == value


def test_library_exports_the_entries(hip_lib):
    import ctypes as C

    assert hip_lib.tmdnet_abi_version() == 10
    for name, n_args in VIB_ENTRIES:
        assert len(getattr(hip_lib, name).argtypes) == n_args, name
    nb = C.c_size_t(0)
    assert hip_lib.tmdnet_vib_workspace_bytes(16, 192, C.byref(nb)) == 0 and nb.value == 16 * (12 * 192 + 36) * 8
    assert hip_lib.tmdnet_vib_workspace_bytes(0, 0, C.byref(nb)) == 0 and nb.value == 0
    for bad in ((-1, 3), (1, 4), (1, -3)):
        assert hip_lib.tmdnet_vib_workspace_bytes(*bad, C.byref(nb)) != 0
    # argument checks happen before anything is enqueued: no device is needed to be refused
    p = C.c_void_p(256)
    assert hip_lib.tmdnet_vib_seed(None, 3, 4, 1, 1, 0, p, p, p, p, 0.01, p) == 1  # unknown mode
    assert hip_lib.tmdnet_vib_seed(None, 1, 4, 1, 1, 0, p, p, p, p, 0.0, p) == 1  # delta
    assert hip_lib.tmdnet_vib_seed(None, 1, 4, 1, 0, 0, p, p, p, p, 0.01, p) == 1  # no replica
    assert hip_lib.tmdnet_vib_seed(None, 0, 4, 1, 1, 0, None, p, p, p, 0.0, None) == 1  # no output
    assert hip_lib.tmdnet_vib_gather(None, 2, 4, 1, 4, 12, 1, 0, p, p, p, p, p, p, p, p) == 1  # unknown mode
    assert hip_lib.tmdnet_vib_gather(None, 1, 4, 1, 4, 12, 1, 0, p, p, p, p, None, p, p, p) == 1  # central without F-
    assert hip_lib.tmdnet_vib_gather(None, 0, 4, 1, 4, 15, 1, 0, p, p, p, p, None, None, None, p) == 1  # dim beyond 3 n_atoms
    assert hip_lib.tmdnet_vib_gather(None, 0, 4, 1, 4, 12, 70000, 0, p, p, p, p, None, None, None, p) == 1  # the grid's rows
    assert hip_lib.tmdnet_vib_finish(None, p, 8, 4, 1, 12, 2, p, p, p, p, p, None, p, p) == 4  # workspace too small
    assert hip_lib.tmdnet_vib_finish(None, p, 1 << 20, 4, 1, 12, 3, p, p, p, p, p, None, p, p) == 1  # unknown projection


def test_method_and_module_signatures():
    from torchmdnet_amd import vibrations as V
    from torchmdnet_amd.models.model import TorchMD_Net

    h = inspect.signature(TorchMD_Net.hessian).parameters
    assert list(h)[1:11] == ["z", "pos", "batch", "box", "q", "method", "delta", "fixed", "replicas", "max_workspace_bytes"]
    assert h["method"].default == "analytic" and h["delta"].default == 0.01 and h["replicas"].default is None
    assert h["max_workspace_bytes"].default == 8 << 30
    v = inspect.signature(TorchMD_Net.vibrations).parameters
    assert list(v)[1:] == ["z", "pos", "batch", "box", "q", "masses", "project", "force_scale", "hessian_kw"]
    assert v["project"].default is True and v["force_scale"].default == 9.648533e-3 and v["masses"].default is None
    for name in ("displacements", "wavenumbers", "n_negative", "zero_point_energy", "omega2"):
        assert hasattr(V.Vibrations, name)
    assert V.METHODS == ("analytic", "central")


# ---- 5. the sanitizers -----------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path):
    """tests/vib_host.hip with its own main, host code only (-Xarch_host -fsanitize=address,undefined): every entry of the mirror on
    heap arrays of exact size.  A report makes the program exit non-zero (-fno-sanitize-recover)."""
    exe = str(tmp_path / "vib_host_san")
    subprocess.check_call([M.hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DVIB_HOST_MAIN", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", M.SOURCE, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "bad 0" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
