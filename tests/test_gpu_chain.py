"""-m gpu: the per-atom chain kernels (csrc/tn_chain.hip) against the launches they replace (same library, same weights, option
"chain_min_atoms" = huge) and against the oracle.  The readout chain runs LayerNorm -> Lin, silu -> O1 -> head -> O1^T . silu' ->
Lin^T -> LayerNorm adjoint -> adjoint of the invariants for a tile of 32 atoms in one launch (reference tensornet.py:398-402,
models/utils.py:552-580, output_modules.py:43-73 and their autograd adjoints).  Both schedules evaluate the same sums in a
different order: they agree to rounding (the bounds of tests/test_gpu_embed_rb.py for that situation); the oracle bound is the
standing 1e-4.

Shapes: C2 hyper-parameters, N just above the 1 024 atoms of the small-system schedules: a multiple of the 32-atom tile, a last
tile of 19 rows with molecules straddling tiles, and a ragged batch (1 .. 90 atoms per molecule) with total charges.

The embedding's gate MLP (LayerNorm -> L1, silu -> L2, silu; tensornet.py:586-593) and its adjoint are two more chains of the
same kind.  All three are on by default from 4 096 atoms.
CHAINS: the bits of option "chain_mask" / info "chain_last": 1 readout, 2 gate forward, 4 gate adjoint."""
import pytest
import torch

from torchmdnet_amd import workloads as W

pytestmark = pytest.mark.gpu
REL = 1e-4
CHAINS = 7
F = 128


def rel_err(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


def _pair(args, seed=0):
    """the same weights twice: chains on for every N of the general schedule, and chains off"""
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(seed)
    on = create_model(dict(args)).to("cuda")
    off = create_model(dict(args))
    off.load_state_dict(on.state_dict())
    off = off.to("cuda")
    on.set_engine_option("chain_min_atoms", 0)
    off.set_engine_option("chain_min_atoms", 10 ** 12)
    return on, off


def _ragged():
    """the generator of test_radial_basis_embedding_vs_oracle_charges_ragged: molecules of 1 .. 90 atoms, total charges"""
    sizes = [90, 1, 33, 64, 2, 17] * 6  # 1242 atoms
    zs, ps, bs = [], [], []
    for m, n in enumerate(sizes):
        zz, pp = W.synthetic_molecule(7000 + m, n_atoms=n)
        zs.append(torch.from_numpy(zz))
        ps.append(torch.from_numpy(pp))
        bs.append(torch.full((n,), m, dtype=torch.long))
    q = torch.tensor([float(m % 3 - 1) for m in range(len(sizes))])
    return torch.cat(zs), torch.cat(ps), torch.cat(bs), q


def _batch(shape):
    if shape == "33x32":
        return W.synthetic_batch(n_mol=33, n_atoms=32, first_seed=500) + (None,)
    if shape == "27x41":
        return W.synthetic_batch(n_mol=27, n_atoms=41, first_seed=600) + (None,)
    return _ragged()


SHAPES = ("33x32", "27x41", "ragged")


@pytest.fixture(scope="module")
def models(hip_lib):
    return _pair(dict(W.C2_ARGS), seed=11)


@pytest.fixture(scope="module")
def runs(models):
    """every shape once through both models: E, F, chain_last and the two debug tensors; shared by the tests, not modified"""
    on, off = models
    out = {}
    for shape in SHAPES:
        z, pos, batch, q = _batch(shape)
        zc, bc = z.cuda(), batch.cuda()
        qc = q.cuda() if q is not None else None
        n = z.shape[0]
        rec = {"in": (z, pos, batch, q)}
        for key, model in (("on", on), ("off", off)):
            E, Fo = model(zc, pos.cuda(), bc, q=qc)
            rec[key] = dict(E=E.detach().clone(), F=Fo.detach().clone(), last=model.engine_info("chain_last"),
                            x=model.debug_tensor("x", (n, F)).clone(), G=model.debug_tensor("G_embed", (n, 9, F)).clone())
        E2, F2 = on(zc, pos.cuda(), bc, q=qc)
        rec["again"] = (E2.detach().clone(), F2.detach().clone())
        out[shape] = rec
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_equals_unfused_launches(runs, shape):
    a, b = runs[shape]["on"], runs[shape]["off"]
    eE, eF = rel_err(a["E"], b["E"]), rel_err(a["F"], b["F"])
    ex, eG = rel_err(a["x"], b["x"]), rel_err(a["G"], b["G"])
    print(f"{shape}: E {eE:.2e} F {eF:.2e} x {ex:.2e} G {eG:.2e}")
    assert eE < 5e-6 and eF < 2e-5, (eE, eF)
    assert ex < 5e-6 and eG < 5e-6, (ex, eG)


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_info_key(runs, models, shape):
    assert runs[shape]["on"]["last"] == CHAINS and runs[shape]["off"]["last"] == 0
    assert models[0].engine_info("chain_mask") == CHAINS and models[0].engine_info("chain_min_atoms") == 0
    assert models[1].engine_info("chain_mask") == CHAINS and models[1].engine_info("chain_min_atoms") == 10 ** 12


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_deterministic(runs, shape):
    E2, F2 = runs[shape]["again"]
    assert torch.equal(runs[shape]["on"]["E"], E2) and torch.equal(runs[shape]["on"]["F"], F2)


def test_chain_vs_oracle(runs, models):
    """every molecule of the 27 x 41 batch (last tile of 19 rows, molecules straddle the tiles) against the torch oracle"""
    from oracle import tensornet_torch as T

    z, pos, batch, _ = runs["27x41"]["in"]
    sd = {k: v.detach().cpu() for k, v in models[0].state_dict().items()}
    Er, Fr = T.energy_and_forces(sd, T.hparams_from_args(dict(W.C2_ARGS)), z, pos, batch)
    eE, eF = rel_err(runs["27x41"]["on"]["E"].cpu(), Er), rel_err(runs["27x41"]["on"]["F"].cpu(), Fr)
    print(f"oracle: E {eE:.2e} F {eF:.2e}")
    assert eE < REL and eF < REL, (eE, eF)


@pytest.mark.parametrize("mask", [1, 2, 4])
def test_chain_mask_bits(hip_lib, runs, mask):
    """one chain at a time between unfused neighbours (a producer / consumer mismatch shows here)"""
    on, _ = _pair(dict(W.C2_ARGS), seed=11)
    on.set_engine_option("chain_mask", mask)
    assert on.engine_info("chain_mask") == mask
    for shape in ("27x41", "ragged"):
        z, pos, batch, q = runs[shape]["in"]
        E, Fo = on(z.cuda(), pos.cuda(), batch.cuda(), q=q.cuda() if q is not None else None)
        assert on.engine_info("chain_last") == (mask & CHAINS)
        b = runs[shape]["off"]
        if mask & CHAINS:
            assert rel_err(E, b["E"]) < 5e-6 and rel_err(Fo, b["F"]) < 2e-5, (rel_err(E, b["E"]), rel_err(Fo, b["F"]))
        else:
            assert torch.equal(E, b["E"]) and torch.equal(Fo, b["F"])


def test_chain_fallbacks(hip_lib, runs):
    """a property head and an energy-only call keep the unfused launches: no chain reported, same bits as the twin without chains"""
    z, pos, batch, _ = runs["33x32"]["in"]
    zc, bc = z.cuda(), batch.cuda()
    on, off = _pair(dict(W.C2_ARGS, output_model="DipoleMoment"), seed=5)
    y1, f1 = on(zc, pos.cuda(), bc)
    assert on.engine_info("chain_last") == 0
    y2, f2 = off(zc, pos.cuda(), bc)
    assert torch.equal(y1, y2) and torch.equal(f1, f2)
    on, off = _pair(dict(W.C2_ARGS, derivative=False), seed=11)
    with torch.no_grad():
        e1, _ = on(zc, pos.cuda(), bc)
        assert on.engine_info("chain_last") == 0
        e2, _ = off(zc, pos.cuda(), bc)
    assert torch.equal(e1, e2)


def test_chain_graph_replay(hip_lib, runs):
    """static shapes: one capture + replay of the step with the three chains equals the eager call"""
    from torchmdnet_amd.models.model import create_model

    z, pos, batch, _ = runs["33x32"]["in"]
    zc, pc, bc = z.cuda(), pos.cuda(), batch.cuda()
    torch.manual_seed(11)
    sta = create_model(dict(W.C2_ARGS, static_shapes=True)).to("cuda")
    sta.set_engine_option("chain_min_atoms", 0)
    E, Fo = sta(zc, pc, bc)
    assert sta.engine_info("chain_last") == CHAINS
    E, Fo = E.detach().clone(), Fo.detach().clone()
    replay = sta.capture(zc, pc, bc)
    E1, F1 = replay()
    assert sta.engine_info("chain_last") == CHAINS
    assert torch.equal(E1, E) and torch.equal(F1, Fo)
