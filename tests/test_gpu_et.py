"""gpu: Equivariant Transformer energy+force path (BASELINE configs[3]) through the C ABI
(tmdnet_create_et + the shared entry points) against the reference's golden vector, fixtures produced by the
unmodified reference, and the oracle (oracle/et_torch.py, oracle/et_adjoint.py).  Tolerance: 1e-4 relative (fp32).
The attention sweeps kernel by kernel, every output and slot array against float64: tests/test_gpu_et_unit.py."""
import json
import os

import pytest
import torch

from oracle import ref_shims as R
from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu
REL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# bf16 pair rows against the fp64 oracle that rounds the same rows (oracle/et_torch.py, pair_rows="bf16"): the rounding itself is in
# the reference, what is left are the few elements whose rounding flips.  The bound is recorded in profiles/et_bf16_oracle_floor.json
# (tools/et_bf16_oracle_floor.py; CPU measurement of the oracle): at least 4 x the noise floor of fp32-accurate rows, at most half of
# what unrounded rows would be off by (tests/test_et_bf16_oracle.py holds both conditions).
with open(os.path.join(ROOT, "profiles", "et_bf16_oracle_floor.json")) as _fh:
    BF16_ORACLE_REL = json.load(_fh)["bound"]
SAME_ROWS_REL = 1e-5  # bf16-row kernels against the fp32-row kernels fed the same rounded values: two schedules of one fp32 arithmetic


def rel_err(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


def _three_models(args, sd=None, seed=None, min_pairs=None):
    """fp32 rows, bf16 storage, bf16 values in fp32 storage: the same weights.  -> (exact, stored, values), host state dict"""
    from torchmdnet_amd.models.model import create_model

    models = []
    for storage in ("fp32", "bf16", "bf16-values"):
        if seed is not None:
            torch.manual_seed(seed)
        m = create_model(dict(args, pair_storage=storage))
        if sd is None:
            sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        m.load_state_dict(sd)
        m = m.to("cuda")
        if min_pairs is not None:
            m.set_engine_option("edge_table_min_pairs", min_pairs)
        models.append(m)
    assert [m.engine_info("pair_rows_bf16") for m in models] == [0.0, 1.0, 2.0]
    return models, sd


def _f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _per_molecule(what, E, F, Eref, Fref, batch, n_mol, bound, small=0, e_batch=False):
    """relative max-norm of E and F per molecule; molecules of fewer than `small` atoms relative to the whole batch.  `e_batch`: the
    energies as one vector over the batch (max |dE| / max |E|, as `rel_err(E, Eo)` elsewhere in this file) - against the
    rounding-aware oracle, whose remaining difference is a handful of flipped roundings of absolute size: a molecule whose atomic
    energies nearly cancel (|E_mol| a twentieth of its neighbours') has no error scale of its own.  Prints the worst figures before
    it asserts."""
    batch = batch.cpu()
    E, F, Eref, Fref = E.detach().cpu().reshape(-1).double(), F.detach().cpu().double(), Eref.cpu().reshape(-1).double(), Fref.cpu().double()
    errs = []
    for m in range(n_mol):
        sel = batch == m
        whole = int(sel.sum()) < small
        fden = (Fref if whole else Fref[sel]).abs().max().item()
        eden = (Eref if whole or e_batch else Eref[m:m + 1]).abs().max().item()
        errs.append((abs(E[m].item() - Eref[m].item()) / max(eden, 1e-12), (F[sel] - Fref[sel]).abs().max().item() / max(fden, 1e-12)))
    print(f"{what}: worst E {max(e for e, _ in errs):.3e} F {max(f for _, f in errs):.3e} (bound {bound:.1e}, {n_mol} molecules)")
    for m, (e, f) in enumerate(errs):
        assert e < bound and f < bound, (what, m, e, f)
    return errs


def _oracle_bf16(sd64, hp, z, pos, batch, n_mol, box=None):
    """the rounding-aware fp64 oracle on every molecule of the batch -> E [n_mol], F [N, 3]"""
    from oracle import et_torch as ET

    E, F = torch.zeros(n_mol, dtype=torch.float64), torch.zeros(pos.shape[0], 3, dtype=torch.float64)
    for m in range(n_mol):
        sel = batch == m
        Eo, Fo = ET.energy_and_forces(sd64, hp, z[sel], pos[sel].double(), torch.zeros(int(sel.sum()), dtype=torch.long), box=box,
                                      pair_rows="bf16")
        E[m], F[sel] = Eo.reshape(()), Fo
    return E, F


def _tile_meta(model):
    return model.debug_tensor("tile_meta", (2,)).view(torch.int32).cpu().tolist()  # [tiles open?, number of tiles]


def _model_from_sd(args, sd):
    from torchmdnet_amd.models.model import create_model

    m = create_model(dict(args))
    m.load_state_dict(sd)
    return m.to("cuda")


def test_et_reference_golden_vector(hip_lib, golden_dir):
    from torchmdnet_amd.models.model import create_model

    g = torch.load(os.path.join(golden_dir, "expected_et_scalar.pt"))
    R.seed_everything(1234)
    model = create_model(dict(g["args"])).to("cuda")
    z, pos, batch = R.create_example_batch(n_atoms=5)
    E, F = model(z.cuda(), pos.cuda(), batch.cuda())
    torch.testing.assert_close(E.cpu(), g["pred"], atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(F.cpu(), g["deriv"], atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("fixture", ["et_tiny_ref.pt", "et_tiny_vc_ref.pt"])
def test_et_tiny_vs_reference_fixture(hip_lib, golden_dir, fixture):
    """ragged molecules, both cutoff placements / distance-influence branches; intermediates of the residual stream
    and of the reverse pass (hand-derived adjoints of oracle/et_adjoint.py)."""
    from oracle import et_adjoint as EA
    from oracle import et_torch as ET

    g = torch.load(os.path.join(golden_dir, fixture))
    model = _model_from_sd(g["args"], g["state_dict"])
    z, pos, batch = g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda()
    E, F = model(z, pos, batch)
    hp = ET.hparams_from_args(g["args"])
    N, Fd, L = z.shape[0], hp["hidden_channels"], hp["num_layers"]
    _, _, cache = EA.energy_forces(g["state_dict"], hp, g["z"], g["pos"], g["batch"], want_cache=True)
    assert rel_err(model.debug_tensor("x_embed", (N, Fd)).cpu(), cache["x_embed"]) < REL
    for l in range(L):
        assert rel_err(model.debug_tensor(f"x_layer{l}", (N, Fd)).cpu(), cache[f"x_layer{l}"]) < REL, l
        assert rel_err(model.debug_tensor(f"vec_layer{l}", (N, 3, Fd)).cpu(), cache[f"vec_layer{l}"]) < REL, l
    assert rel_err(model.debug_tensor("x_out", (N, Fd)).cpu(), g["inter"]["x_out"]) < REL
    assert rel_err(model.debug_tensor("g_x", (N, Fd)).cpu(), cache["g_x_layer0"]) < REL
    assert rel_err(model.debug_tensor("g_vec", (N, 3, Fd)).cpu(), cache["g_vec_layer0"]) < REL
    assert rel_err(E.cpu(), g["E"]) < REL
    assert rel_err(F.cpu(), g["F"]) < REL


def test_et_c4_vs_reference_fixture(hip_lib, golden_dir):
    """BASELINE configs[3]: examples/ET-SPICE.yaml hyper-parameters (F=128, L=5, 8 heads, K=64, rc=10, vector cutoff),
    weights from seed 0, 3 molecules of S-mol64 evaluated by the unmodified reference."""
    from torchmdnet_amd.models.model import create_model

    g = torch.load(os.path.join(golden_dir, "et_c4_ref.pt"))
    torch.manual_seed(0)
    model = create_model(dict(W.C4_ARGS)).to("cuda")
    z, pos, batch = W.synthetic_batch(n_mol=g["n_mol"])
    E, F = model(z.cuda(), pos.cuda(), batch.cuda())
    assert rel_err(E.cpu(), g["E"]) < REL
    assert rel_err(F.cpu(), g["F"]) < REL


def test_et_batch_properties(hip_lib):
    """64 molecules x 64 atoms on the C4 model: oracle on two sampled molecules, bit-identical repeat, zero net force
    per molecule, invariance to permuting molecules and to a rigid translation."""
    from oracle import et_torch as ET
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(0)
    model = create_model(dict(W.C4_ARGS)).to("cuda")
    n_mol = 64
    z, pos, batch = W.synthetic_batch(n_mol=n_mol)
    zc, pc, bc = z.cuda(), pos.cuda(), batch.cuda()
    E, F = model(zc, pc, bc)
    E2, F2 = model(zc, pc.clone(), bc)
    assert torch.equal(E, E2) and torch.equal(F, F2)
    net = torch.zeros(n_mol, 3, device="cuda").index_add(0, bc, F)
    assert net.abs().max().item() < 1e-3 * F.abs().max().item()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    hp = ET.hparams_from_args(W.C4_ARGS)
    for m in (3, 41):
        sel = batch == m
        Eo, Fo = ET.energy_and_forces(sd, hp, z[sel], pos[sel], torch.zeros(int(sel.sum()), dtype=torch.long))
        assert rel_err(E[m].cpu().reshape(1, 1), Eo) < REL
        assert rel_err(F[sel.cuda()].cpu(), Fo) < REL
    perm = torch.randperm(n_mol, generator=torch.Generator().manual_seed(1))
    order = torch.cat([torch.nonzero(batch == int(m)).flatten() for m in perm])
    newb = torch.repeat_interleave(torch.arange(n_mol), 64)
    Ep, Fp = model(z[order].cuda(), (pos[order] + torch.tensor([3.0, -2.0, 1.0])).cuda(), newb.cuda())
    assert rel_err(Ep.cpu(), E.cpu()[perm]) < 1e-5
    assert rel_err(Fp.cpu(), F.cpu()[order]) < 1e-4


def test_et_static_shapes_and_graph_replay(hip_lib, golden_dir):
    """static_shapes=True (no read-back, capacity-sized launches) equals the dynamic path, and a captured HIP graph
    replays with new positions (the MD use of the ET path)."""
    g = torch.load(os.path.join(golden_dir, "et_tiny_ref.pt"))
    dyn = _model_from_sd(g["args"], g["state_dict"])
    sta = _model_from_sd(dict(g["args"], static_shapes=True), g["state_dict"])
    z, pos, batch = g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda()
    Ed, Fd = dyn(z, pos, batch)
    Es, Fs = sta(z, pos, batch)
    torch.testing.assert_close(Es, Ed, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(Fs, Fd, atol=1e-5, rtol=1e-5)
    replay = sta.capture(z, pos, batch)
    E1, F1 = replay()
    assert rel_err(E1.cpu(), g["E"]) < REL and rel_err(F1.cpu(), g["F"]) < REL
    torch.manual_seed(0)
    pos2 = pos + 0.05 * torch.randn_like(pos)
    E2, F2 = replay(pos2)
    E2, F2 = E2.clone(), F2.clone()
    Er, Fr = dyn(z, pos2, batch)
    assert rel_err(E2, Er) < 1e-5 and rel_err(F2, Fr) < 1e-5


def test_et_periodic_box_vs_oracle(hip_lib, golden_dir):
    """triclinic minimum image through the shared neighbour phase; oracle = oracle/et_torch.py with the same box."""
    from oracle import et_torch as ET

    g = torch.load(os.path.join(golden_dir, "et_tiny_vc_ref.pt"))
    model = _model_from_sd(g["args"], g["state_dict"])
    zz, pp = W.synthetic_molecule(55, n_atoms=40, density=0.03)
    z, pos = torch.from_numpy(zz) % 19 + 1, torch.from_numpy(pp)
    box = torch.tensor([[11.0, 0.0, 0.0], [0.4, 11.5, 0.0], [0.3, -0.6, 10.6]])
    batch = torch.zeros(40, dtype=torch.long)
    E, F = model(z.cuda(), pos.cuda(), batch.cuda(), box=box.cuda())
    Eo, Fo = ET.energy_and_forces(g["state_dict"], ET.hparams_from_args(g["args"]), z, pos, batch, box=box)
    assert rel_err(E.cpu(), Eo) < REL and rel_err(F.cpu(), Fo) < REL


@pytest.mark.parametrize("F,H,K,di,ne,vc", [(64, 2, 20, "none", False, False), (64, 8, 16, "values", True, True),
                                            (256, 4, 32, "both", True, False)])
def test_et_shape_sweep_vs_oracle(hip_lib, F, H, K, di, ne, vc):
    """head sizes 8 / 32 / 64 lanes, no / values-only distance influence, without neighbour embedding, K not a multiple of
    16 (fp32-MFMA fallback of the pair GEMMs), a batch for the throughput kernels and a tiny one; oracle = et_torch."""
    from oracle import et_torch as ET
    from torchmdnet_amd.models.model import create_model

    args = dict(W.C4_ARGS, embedding_dimension=F, num_heads=H, num_rbf=K, num_layers=2, distance_influence=di,
                neighbor_embedding=ne, vector_cutoff=vc, cutoff_upper=5.0, max_z=20, max_num_neighbors=64)
    torch.manual_seed(12)
    model = create_model(dict(args)).to("cuda")
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    hp = ET.hparams_from_args(args)
    for n_mol, n_atoms in ((40, 40), (2, 9)):
        z, pos, batch = W.synthetic_batch(n_mol=n_mol, n_atoms=n_atoms, first_seed=700)
        z = z % 19 + 1
        E, Fo = model(z.cuda(), pos.cuda(), batch.cuda())
        sel = batch < 2
        Eo, Fr = ET.energy_and_forces(sd, hp, z[sel], pos[sel], batch[sel])
        assert rel_err(E[:2].cpu(), Eo) < REL, (F, H, K, n_mol)
        assert rel_err(Fo[sel.cuda()].cpu(), Fr) < REL, (F, H, K, n_mol)


TILE_CASES = [
    (5, 64, 10.0, "both", True, 8),     # dense closed tiles: slot order, the pair rows exchanged through the LDS mailbox
    (5, 64, 10.0, "keys", False, 4),    # ... one projection only (no exchange), attention cutoff, heads of 32 channels
    (5, 64, 10.0, "values", True, 16),  # ... heads of 8 channels
    (5, 64, 10.0, "none", False, 8),    # ... no filter rows at all
    (7, 32, 5.0, "both", True, 8),      # two molecules per tile, sparse rows: list order; the last tile is half empty
    (6, 64, 4.0, "both", False, 8),     # closed tiles with short rows (list order), attention cutoff
    (4, 48, 10.0, "both", True, 8),     # molecules straddle the tiles: the flag sends the step to the row sweeps
    (3, 100, 6.0, "both", True, 8),     # rows longer than a tile
    (9, 40, 10.0, "both", True, 8),     # one 40-atom molecule per tile (tiles = runs of whole molecules <= 64 rows), slot order off
    (11, 21, 10.0, "both", False, 8),   # three molecules per tile, dense inside a molecule, list order
]
# closed tiles filled between 25 % and 70 %: the tile sweeps with bf16 rows (and with bf16 values), the row sweeps with fp32 rows -
# the only tile kernels that see sparse tiles (directed edges incl. self loops / (tiles x 64 x 64): 0.26, 0.39, 0.30)
SPARSE_TILE_CASES = {(7, 32, 5.0), (9, 40, 10.0), (11, 21, 10.0)}


@pytest.mark.parametrize("n_mol,n_atoms,rc,di,vc,H", TILE_CASES)
def test_et_tile_sweeps_vs_oracle(hip_lib, n_mol, n_atoms, rc, di, vc, H):
    """The tile generation of the attention sweeps (tn_et_g16.hip: a workgroup = 64 rows x 32 channels, node rows in LDS, slot or
    list order, the pair rows fetched once and exchanged) and the device-side choice between it and the row sweeps, against
    oracle/et_torch.py on the first, a middle and the last molecule; fp32 and bf16 pair rows; bit-identical repeats.  With
    distance influence: the bf16-row kernels against the fp32-row kernels on the same rounded values (same choice of sweep
    generation, 1e-5 per molecule) and against the rounding-aware fp64 oracle on every molecule (BF16_ORACLE_REL)."""
    from oracle import et_torch as ET

    args = dict(W.C4_ARGS, num_layers=2, num_heads=H, distance_influence=di, vector_cutoff=vc, cutoff_upper=rc)
    if di == "none":
        from torchmdnet_amd.models.model import create_model

        torch.manual_seed(5)
        model = create_model(dict(args)).to("cuda")
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    else:
        (model, stored, values), sd = _three_models(args, seed=5)
    hp = ET.hparams_from_args(args)
    z, pos, batch = W.synthetic_batch(n_mol=n_mol, n_atoms=n_atoms, first_seed=300)
    zc, pc, bc = z.cuda(), pos.cuda(), batch.cuda()
    E, F = model(zc, pc, bc)
    E2, F2 = model(zc, pc.clone(), bc)
    assert torch.equal(E, E2) and torch.equal(F, F2)
    for m in sorted({0, n_mol // 2, n_mol - 1}):
        sel = batch == m
        Eo, Fo = ET.energy_and_forces(sd, hp, z[sel], pos[sel], torch.zeros(int(sel.sum()), dtype=torch.long))
        assert rel_err(E[m].cpu().reshape(1, 1), Eo) < REL, (m, "E")
        assert rel_err(F[sel.cuda()].cpu(), Fo) < REL, (m, "F")
    if di != "none":  # bf16 storage of the pair rows: the same kernels with the other row type
        meta0 = _tile_meta(model)
        Eb, Fb = stored(zc, pc, bc)
        meta1 = _tile_meta(stored)
        assert rel_err(Eb.cpu(), E.cpu()) < 2e-2 and rel_err(Fb.cpu(), F.cpu()) < 2e-2
        assert torch.isfinite(Fb).all()
        assert not torch.equal(Fb, F)  # the rows really are rounded
        Ev, Fv = values(zc, pc, bc)
        Ev2, Fv2 = values(zc, pc.clone(), bc)
        assert torch.equal(Ev, Ev2) and torch.equal(Fv, Fv2)
        assert _tile_meta(values) == meta1  # the same sweep generation for the same input
        fill = stored.graph_counts()[1] / (meta1[1] * 64.0 * 64.0)
        print(f"tile_meta fp32 {meta0} bf16 {meta1} fill {fill:.3f}")
        if (n_mol, n_atoms, rc) in SPARSE_TILE_CASES:
            assert meta1[0] == 0 and 0.25 <= fill < 0.70 and meta0[0] == 1, (meta0, meta1, fill)
        _per_molecule("bf16 rows vs bf16 values", Eb, Fb, Ev, Fv, batch, n_mol, SAME_ROWS_REL)
        Eo, Fo = _oracle_bf16(_f64(sd), hp, z, pos, batch, n_mol)
        _per_molecule("bf16 rows vs rounding-aware oracle", Eb, Fb, Eo, Fo, batch, n_mol, BF16_ORACLE_REL, e_batch=True)


def test_et_tile_sweeps_ragged_batch_vs_oracle(hip_lib):
    """Molecules of different sizes (1 .. 64 atoms, two of 70: those open the tiles and send the step to the row sweeps) in one
    batch: the tiles are packed from whole molecules on the device; every molecule against oracle/et_torch.py."""
    import numpy as np
    from oracle import et_torch as ET

    args = dict(W.C4_ARGS, num_layers=2)
    (model, stored, values), sd = _three_models(args, seed=9)
    hp = ET.hparams_from_args(args)
    rng = np.random.default_rng(3)
    # (sizes, what the device decides): dense closed tiles -> tile sweeps; closed but half empty -> row sweeps (the fill rule of
    # k_et_tile_pack); molecules of more than 64 atoms -> open -> row sweeps
    for sizes, want_tiles in (([64, 30, 34, 64, 20, 44, 64], True), ([64, 1, 17, 40, 33, 31, 2, 64, 5, 59, 64, 12], False),
                              ([20, 70, 8, 70, 3], False)):
        zs, ps, bs = [], [], []
        for m, n in enumerate(sizes):
            z, pos, _ = W.synthetic_batch(n_mol=1, n_atoms=n, first_seed=500 + m)
            zs.append(z); ps.append(pos); bs.append(torch.full((n,), m, dtype=torch.long))
        z, pos, batch = torch.cat(zs), torch.cat(ps), torch.cat(bs)
        E, F = model(z.cuda(), pos.cuda(), batch.cuda())
        meta = _tile_meta(model)
        assert (meta[0] == 0) == want_tiles and (not want_tiles or 0 < meta[1] <= len(sizes)), (sizes, meta)
        for m in range(len(sizes)):
            sel = batch == m
            Eo, Fo = ET.energy_and_forces(sd, hp, z[sel], pos[sel], torch.zeros(int(sel.sum()), dtype=torch.long))
            assert abs(E[m].item() - Eo.item()) < 1e-4 * max(1.0, abs(Eo.item())), (sizes, m)
            assert (F[sel.cuda()].cpu() - Fo).abs().max().item() < 1e-4 * max(1.0, Fo.abs().max().item()), (sizes, m)
        # bf16 rows: the bf16-row kernels against the fp32-row kernels on the same rounded values, and against the oracle that
        # rounds the same rows.  The oracle's noise floor was measured on molecules of 21 .. 100 atoms: smaller ones (a handful of
        # pairs, where one flipped rounding does not average out) are taken relative to the largest force of the batch
        Eb, Fb = stored(z.cuda(), pos.cuda(), batch.cuda())
        Ev, Fv = values(z.cuda(), pos.cuda(), batch.cuda())
        assert _tile_meta(values) == _tile_meta(stored), sizes
        Ev2, Fv2 = values(z.cuda(), pos.cuda(), batch.cuda())
        assert torch.equal(Ev, Ev2) and torch.equal(Fv, Fv2), sizes
        print(sizes, "tile_meta fp32", meta, "bf16", _tile_meta(stored))
        _per_molecule("ragged: bf16 rows vs bf16 values", Eb, Fb, Ev, Fv, batch, len(sizes), SAME_ROWS_REL, small=21)
        Eo, Fo = _oracle_bf16(_f64(sd), hp, z, pos, batch, len(sizes))
        _per_molecule("ragged: bf16 rows vs rounding-aware oracle", Eb, Fb, Eo, Fo, batch, len(sizes), BF16_ORACLE_REL, small=21, e_batch=True)


def test_et_tile_sweeps_replay_from_a_captured_graph(hip_lib):
    """The tile generation is chosen on the device (no read-back), so a captured step keeps working when the positions - and with
    them the neighbour lists inside the closed tiles - change between replays: three 64-atom molecules, static shapes."""
    from torchmdnet_amd.models.model import create_model

    args = dict(W.C4_ARGS, num_layers=2)
    torch.manual_seed(4)
    dyn = create_model(dict(args)).to("cuda")
    sta = create_model(dict(args, static_shapes=True)).to("cuda")
    sta.load_state_dict(dyn.state_dict())
    z, pos, batch = (t.cuda() for t in W.synthetic_batch(n_mol=3, n_atoms=64, first_seed=40))
    replay = sta.capture(z, pos, batch)
    E0, F0 = replay()
    Ed, Fd = dyn(z, pos, batch)
    assert rel_err(E0, Ed) < 1e-5 and rel_err(F0, Fd) < 1e-5
    assert dyn.debug_tensor("tile_meta", (2,)).view(torch.int32).cpu().tolist() == [0, 3]  # closed, three tiles
    torch.manual_seed(1)
    for scale in (0.05, 0.3):
        pos2 = pos + scale * torch.randn_like(pos)
        E2, F2 = replay(pos2)
        E2, F2 = E2.clone(), F2.clone()
        Er, Fr = dyn(z, pos2, batch)
        assert rel_err(E2, Er) < 1e-5 and rel_err(F2, Fr) < 1e-5, scale


def test_et_randomised_small_systems_vs_oracle(hip_lib, golden_dir):
    """single atoms, isolated atoms (only the self loop: vec stays zero -> the norm's zero-row mask), ragged sizes, unsorted
    batch vectors, periodic boxes; oracle = oracle/et_torch.py."""
    import numpy as np
    from oracle import et_torch as ET

    for fixture in ("et_tiny_ref.pt", "et_tiny_vc_ref.pt"):
        g = torch.load(os.path.join(golden_dir, fixture))
        model = _model_from_sd(g["args"], g["state_dict"])
        hp = ET.hparams_from_args(g["args"])
        rng = np.random.default_rng(7)
        for case in range(10):
            n_mol = int(rng.integers(1, 5))
            sizes = [int(rng.integers(1, 12)) for _ in range(n_mol)]
            spread = float(rng.choice([1.5, 3.0, 9.0]))
            pos = np.concatenate([rng.uniform(0, spread * max(s, 2) ** (1 / 3), size=(s, 3)) for s in sizes]).astype(np.float32)
            z = rng.integers(1, 20, size=sum(sizes))
            batch = np.repeat(np.arange(n_mol), sizes)
            box = torch.tensor([[12.0, 0, 0], [0.5, 12.5, 0], [-0.4, 0.7, 13.0]]) if case % 3 == 1 else None
            if case % 4 == 3 and n_mol > 1:
                perm = rng.permutation(len(z))
                pos, z, batch = pos[perm], z[perm], batch[perm]
            zt, pt, bt = torch.from_numpy(z), torch.from_numpy(pos), torch.from_numpy(batch)
            E, F = model(zt.cuda(), pt.cuda(), bt.cuda(), box=None if box is None else box.cuda())
            for m in range(n_mol):
                sel = bt == m
                Eo, Fo = ET.energy_and_forces(g["state_dict"], hp, zt[sel], pt[sel], torch.zeros(int(sel.sum()), dtype=torch.long), box=box)
                assert abs(E[m].item() - Eo.item()) < 1e-4 * max(1.0, abs(Eo.item())), (fixture, case, m)
                assert (F[sel.cuda()].cpu() - Fo).abs().max().item() < 1e-4 * max(1.0, Fo.abs().max().item()), (fixture, case, m)


def test_et_energy_only_and_backward(hip_lib, golden_dir):
    """derivative=False: energies alone (the pair GEMMs then carry no tangents), and energy.backward() filling pos.grad the way
    the ASE calculator uses the model (calculators.py:311-316)."""
    g = torch.load(os.path.join(golden_dir, "et_tiny_ref.pt"))
    model = _model_from_sd(dict(g["args"], derivative=False), g["state_dict"])
    z, batch = g["z"].cuda(), g["batch"].cuda()
    with torch.no_grad():
        E0, empty = model(z, g["pos"].cuda(), batch)
    assert empty.numel() == 0 and rel_err(E0.cpu(), g["E"]) < REL
    pos = g["pos"].cuda().clone().requires_grad_(True)
    E1, _ = model(z, pos, batch)
    E1.sum().backward()
    assert rel_err(-pos.grad.cpu(), g["F"]) < REL and rel_err(E1.detach().cpu(), g["E"]) < REL


@pytest.mark.parametrize("fixture", ["et_tiny_ref.pt", "et_tiny_vc_ref.pt"])
def test_et_radial_tables_equal_direct_evaluation(hip_lib, golden_dir, fixture):
    """The distance filters of every attention layer and of the neighbour embedding are functions of the pair distance alone:
    tabulated at parameter upload (fp64 build, verified at the interval midpoints) and interpolated per pair instead of the
    pair-row GEMMs (csrc/tn_edge_table.hip).  Same numbers as the direct path to fp32 rounding."""
    g = torch.load(os.path.join(golden_dir, fixture))
    model = _model_from_sd(g["args"], g["state_dict"])
    z, pos, batch = g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda()
    assert model.engine_info("edge_table_T") >= 8192
    assert model.engine_info("edge_table_err_value") < 5e-7 and model.engine_info("edge_table_err_slope") < 2e-6
    model.set_engine_option("edge_table_min_pairs", 10 ** 12)
    Ed, Fd = model(z, pos, batch)
    model.set_engine_option("edge_table_min_pairs", 0)
    Et, Ft = model(z, pos, batch)
    assert rel_err(Et, Ed) < 2e-6 and rel_err(Ft, Fd) < 2e-6
    assert rel_err(Et.cpu(), g["E"]) < REL and rel_err(Ft.cpu(), g["F"]) < REL


BF16_REL = 2.0 ** -8  # = 3.9e-3, one bf16 ulp: stated bound of the reduced-precision STORAGE mode vs the fp32 oracle (measured on the
# C4 model, 64 x 64 atoms: E 3.8e-4, F 2.1e-3 vs the oracle, F 1.8e-3 vs the fp32-exact engine; profiles/r03_notes.md)


def test_et_pair_rows_bf16_vs_fp32_oracle(hip_lib):
    """BASELINE configs[3] says bf16; the reference has no bf16 mode (models/utils.py:715: 16 -> float16), so SURVEY a13's
    rule applies: compare with the fp32 oracle at a bf16-appropriate, STATED tolerance.  `pair_storage="bf16"` keeps the
    per-pair filter rows (dkv, tkv: reference torchmd_et.py:375-415) as bf16 between the table interpolation and the
    attention sweeps; arithmetic stays fp32.  C4 model, 64 x 64 atoms: vs the oracle on two molecules and vs the fp32-exact
    engine on the whole batch; deterministic; without the tables (short pair list) the call keeps fp32 rows."""
    import json

    from oracle import et_torch as ET
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(0)
    exact = create_model(dict(W.C4_ARGS)).to("cuda")
    model = create_model(dict(W.C4_ARGS, pair_storage="bf16"))
    model.load_state_dict(exact.state_dict())
    model = model.to("cuda")
    n_mol = 64
    z, pos, batch = W.synthetic_batch(n_mol=n_mol)
    zc, pc, bc = z.cuda(), pos.cuda(), batch.cuda()
    E, F = model(zc, pc, bc)
    assert model.engine_info("pair_rows_bf16") == 1.0 and model.engine_info("edge_table_T") >= 8192
    E2, F2 = model(zc, pc.clone(), bc)
    assert torch.equal(E, E2) and torch.equal(F, F2)
    Ex, Fx = exact(zc, pc.clone(), bc)
    err_e, err_f = rel_err(E, Ex), rel_err(F, Fx)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "et_bf16_error.json"), "w") as fh:
        json.dump({"E_vs_fp32_engine": err_e, "F_vs_fp32_engine": err_f}, fh)
    assert 0.0 < err_f < BF16_REL and err_e < BF16_REL, (err_e, err_f)  # > 0: the rows really are rounded
    sd = {k: v.detach().cpu() for k, v in exact.state_dict().items()}
    hp = ET.hparams_from_args(W.C4_ARGS)
    worst = [err_e, err_f]
    for m in (3, 41):
        sel = batch == m
        Eo, Fo = ET.energy_and_forces(sd, hp, z[sel], pos[sel], torch.zeros(int(sel.sum()), dtype=torch.long))
        worst.append(rel_err(E[m].cpu().reshape(1, 1), Eo))
        worst.append(rel_err(F[sel.cuda()].cpu(), Fo))
    assert max(worst) < BF16_REL, worst
    with open(os.path.join(out, "et_bf16_error.json"), "w") as fh:
        json.dump({"E_vs_fp32_engine": err_e, "F_vs_fp32_engine": err_f, "E_F_vs_oracle_mol3_mol41": worst[2:], "bound": BF16_REL}, fh)
    net = torch.zeros(n_mol, 3, device="cuda").index_add(0, bc, F)
    assert net.abs().max().item() < 1e-3 * F.abs().max().item()  # pair-symmetric storage: Newton's third law survives rounding
    # a pair list below `edge_table_min_pairs` runs the value + tangent GEMMs: fp32 rows, bit-equal to the exact engine
    sel = batch < 1
    model.set_engine_option("edge_table_min_pairs", 10 ** 9)
    exact.set_engine_option("edge_table_min_pairs", 10 ** 9)
    Es, Fs = model(zc[sel.cuda()], pc[sel.cuda()].clone(), bc[sel.cuda()])
    Et, Ft = exact(zc[sel.cuda()], pc[sel.cuda()].clone(), bc[sel.cuda()])
    assert torch.equal(Es, Et) and torch.equal(Fs, Ft)


def test_et_pair_rows_bf16_tiny_direct_interpolation_and_replay(hip_lib, golden_dir):
    """the one-launch interpolation (short pair lists) and static shapes + HIP-graph replay in the bf16 storage mode"""
    from torchmdnet_amd.models.model import create_model

    g = torch.load(os.path.join(golden_dir, "et_tiny_ref.pt"))
    model = create_model(dict(g["args"], pair_storage="bf16", static_shapes=True))
    model.load_state_dict(g["state_dict"])
    model = model.to("cuda")
    model.set_engine_option("edge_table_min_pairs", 0)
    z, pos, batch = g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda()
    E, F = model(z, pos, batch)
    assert rel_err(E.cpu(), g["E"]) < BF16_REL and rel_err(F.cpu(), g["F"]) < 3 * BF16_REL
    assert not torch.equal(F.cpu(), g["F"])
    replay = model.capture(z, pos, batch)
    E1, F1 = replay()
    assert torch.equal(E1.reshape(-1), E.reshape(-1)) and torch.equal(F1, F)


# ---- the bf16 pair rows, rounding taken out of the comparison -----------------------------------------------------------------
def _pair_rows(model, name, layer, Wd):
    """[P + 1, Wd] int32 bit patterns of a layer's stored rows of the last call (bf16 storage: the 16 bits in the upper half)"""
    P = model.graph_counts()[0]
    if model.pair_storage == "bf16":
        raw = model.debug_tensor(f"{name}{layer}", (P + 1, Wd // 2)).view(torch.int16).reshape(P + 1, Wd)
        return raw.to(torch.int32) << 16
    return model.debug_tensor(f"{name}{layer}", (P + 1, Wd)).view(torch.int32)


def _assert_rows_exact(models, L, Wd, names, what):
    exact, stored, values = models
    for l in range(L):
        for name in names:
            r0, r1, r2 = (_pair_rows(m, name, l, Wd) for m in models)
            want = r0.view(torch.float32).bfloat16().float().view(torch.int32)  # round to nearest even, the self-pair row P included
            assert torch.equal(r2, want), (what, name, l, int((r2 != want).sum()))
            assert torch.equal(r1, r2), (what, name, l, int((r1 != r2).sum()))
            assert not torch.equal(r2, r0), (what, name, l)  # and the fp32 rows are not bf16 values to begin with


ROW_CASES = {  # name: (model arguments, molecules, atoms, interpolation kernel)
    "direct_both_L2": (dict(W.ET_TINY_ARGS, distance_influence="both"), 2, 13, "direct"),
    "direct_keys_L2": (dict(W.ET_TINY_ARGS, distance_influence="keys"), 2, 13, "direct"),
    "direct_values_L2": (dict(W.ET_TINY_ARGS, distance_influence="values"), 2, 13, "direct"),
    "direct_both_L5": (dict(W.C4_ARGS), 1, 64, "direct"),         # 4 tables + 1 table per launch
    "bucketed_both_L5": (dict(W.C4_ARGS), 10, 64, "bucketed"),    # the smallest batch of 64-atom molecules above 16384 pairs
    "bucketed_keys_L2": (dict(W.C4_ARGS, num_layers=2, distance_influence="keys"), 10, 64, "bucketed"),
    "bucketed_values_L2": (dict(W.C4_ARGS, num_layers=2, embedding_dimension=64, distance_influence="values"), 10, 64, "bucketed"),
}


@pytest.mark.parametrize("case", sorted(ROW_CASES))
def test_et_pair_rows_bf16_are_the_rounded_fp32_rows_bit_for_bit(hip_lib, case):
    """The rows the table interpolation stores (both kernels of tn_edge_table.hip, both launch splits, row lengths F, 3F, 4F): with
    `pair_storage="bf16-values"` exactly the fp32 mode's rows rounded to the nearest even bf16, with "bf16" the upper halves of
    those - value and tangent rows of every layer, every pair and the self-pair row.  An energy-only call writes no tangent rows."""
    args, n_mol, n_atoms, kernel = ROW_CASES[case]
    models, _ = _three_models(args, seed=21, min_pairs=0)
    F, L = args["embedding_dimension"], args["num_layers"]
    Wd = {"keys": 1, "values": 3, "both": 4}[args["distance_influence"]] * F
    z, pos, batch = W.synthetic_batch(n_mol=n_mol, n_atoms=n_atoms, first_seed=900)
    z = z % 19 + 1
    zc, pc, bc = z.cuda(), pos.cuda(), batch.cuda()
    for m in models:
        m(zc, pc, bc)
    P = models[0].graph_counts()[0]
    assert [m.graph_counts()[0] for m in models] == [P] * 3 and (P + 1 > 16384) == (kernel == "bucketed"), P
    _assert_rows_exact(models, L, Wd, ("dkv", "tkv"), case)
    for m in models:
        m.energy_and_forces(zc, pc, bc, None, None, n_mol, want_forces=False)
        with pytest.raises(RuntimeError, match="tangent"):
            m.debug_tensor("tkv0", (P + 1, Wd // (2 if m.pair_storage == "bf16" else 1)))
    _assert_rows_exact(models, L, Wd, ("dkv",), case + " (energies only)")
    with pytest.raises(RuntimeError, match="layer out of range"):
        models[0].debug_tensor(f"dkv{L}", (P + 1, Wd))
    with pytest.raises(RuntimeError, match="wrong size"):
        models[1].debug_tensor("dkv0", (P + 1, Wd))


def test_et_pair_rows_debug_tensor_refused_without_distance_influence(hip_lib):
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(2)
    model = create_model(dict(W.ET_TINY_ARGS, distance_influence="none")).to("cuda")
    z, pos, batch = W.synthetic_batch(n_mol=2, n_atoms=9, first_seed=900)
    model((z % 19 + 1).cuda(), pos.cuda(), batch.cuda())
    for name in ("dkv0", "tkv0"):
        with pytest.raises(RuntimeError, match="no pair rows"):
            model.debug_tensor(name, (1,))


def test_et_pair_rows_bf16_periodic_box_same_rows_and_oracle(hip_lib, golden_dir):
    """the triclinic system of test_et_periodic_box_vs_oracle with bf16 rows (tables forced on: 40 atoms)"""
    from oracle import et_torch as ET

    g = torch.load(os.path.join(golden_dir, "et_tiny_vc_ref.pt"))
    (exact, stored, values), sd = _three_models(g["args"], sd=g["state_dict"], min_pairs=0)
    zz, pp = W.synthetic_molecule(55, n_atoms=40, density=0.03)
    z, pos = torch.from_numpy(zz) % 19 + 1, torch.from_numpy(pp)
    box = torch.tensor([[11.0, 0.0, 0.0], [0.4, 11.5, 0.0], [0.3, -0.6, 10.6]])
    batch = torch.zeros(40, dtype=torch.long)
    out = [m(z.cuda(), pos.cuda(), batch.cuda(), box=box.cuda()) for m in (exact, stored, values)]
    (E, F), (Eb, Fb), (Ev, Fv) = out
    assert not torch.equal(Fb, F)
    Ev2, Fv2 = values(z.cuda(), pos.cuda().clone(), batch.cuda(), box=box.cuda())
    assert torch.equal(Ev, Ev2) and torch.equal(Fv, Fv2)
    _per_molecule("periodic: bf16 rows vs bf16 values", Eb, Fb, Ev, Fv, batch, 1, SAME_ROWS_REL)
    Eo, Fo = ET.energy_and_forces(_f64(sd), ET.hparams_from_args(g["args"]), z, pos.double(), batch, box=box.double(), pair_rows="bf16")
    _per_molecule("periodic: bf16 rows vs rounding-aware oracle", Eb, Fb, Eo, Fo, batch, 1, BF16_ORACLE_REL, e_batch=True)


def test_et_pair_rows_bf16_replay_equals_bf16_values(hip_lib, golden_dir):
    """the graph replay of the tiny bf16 test (static shapes, one-launch interpolation) against the same step with bf16 values in
    fp32 rows, captured as well; replays bit-identical in both"""
    g = torch.load(os.path.join(golden_dir, "et_tiny_ref.pt"))
    (_, stored, values), _ = _three_models(dict(g["args"], static_shapes=True), sd=g["state_dict"], min_pairs=0)
    z, pos, batch = g["z"].cuda(), g["pos"].cuda(), g["batch"].cuda()
    n_mol = int(g["batch"].max()) + 1
    outs = []
    for m in (stored, values):
        E, F = m(z, pos, batch)
        replay = m.capture(z, pos, batch)
        E1, F1 = replay()
        assert torch.equal(E1.reshape(-1), E.reshape(-1)) and torch.equal(F1, F)
        E1, F1 = E1.clone(), F1.clone()
        E2, F2 = replay()
        assert torch.equal(E2, E1) and torch.equal(F2, F1)
        outs.append((E1.reshape(-1), F1))
    _per_molecule("replay: bf16 rows vs bf16 values", outs[0][0], outs[0][1], outs[1][0], outs[1][1], g["batch"], n_mol, SAME_ROWS_REL)
