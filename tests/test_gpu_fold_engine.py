"""The group-product adjoint folded into the reverse tile sweep (option "fold_node_adjoint"), through the engine, C2 model.

128 molecules of 64 atoms are the smallest batch that takes the tile route at F = 128; every molecule fills one aligned 64-row
tile, so the graph build reports closed tiles and the reverse sweeps run folded.  With the first molecule cut to 63 atoms and
the second grown to 65 (same atoms), molecules straddle the tile boundaries and the parent pair of launches runs.  A graph
built through the static entry has no read-back and never folds."""
import pytest
import torch

pytestmark = pytest.mark.gpu

REL = 1e-4       # the project's bound against the oracle
REL_FOLD = 2e-5  # forces with the fold against without it, max-norm relative (profiles/chain_fusion_notes.md)


def rel_err(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-12)


@pytest.fixture(scope="module")
def setup():
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    torch.manual_seed(0)
    model = create_model(dict(W.C2_ARGS)).cuda()
    z, pos, batch = W.synthetic_batch(n_mol=128)
    return model, z, pos, batch


def run(model, z, pos, batch, fold):
    model.set_engine_option("fold_node_adjoint", 1.0 if fold else 0.0)
    E, F = model(z.cuda(), pos.cuda(), batch.cuda())
    torch.cuda.synchronize()
    return E.clone(), F.clone(), int(model.engine_info("message_adjoint_fold_last")), int(model.engine_info("message_adjoint_route_last"))


def test_closed_tiles_fold(setup):
    from oracle import tensornet_torch as T
    from torchmdnet_amd import _C
    from torchmdnet_amd import workloads as W

    model, z, pos, batch = setup
    assert int(model.engine_info("fold_node_adjoint")) in (0, 1)
    E0, F0, fold0, route0 = run(model, z, pos, batch, False)
    E1, F1, fold1, route1 = run(model, z, pos, batch, True)
    assert (fold0, route0) == (0, _C.MSG_GD_TILE)
    assert (fold1, route1) == (1, _C.MSG_GD_TILE)
    assert model._engine.counts[2] == 0  # what Python exposes of the read-back keeps its meaning: (pairs, edges, unsorted)
    assert len(model._engine.counts) == 3
    assert torch.equal(E0, E1), "the forward pass is untouched"
    e = rel_err(F1, F0)
    print("forces, fold on against off: %.3g (bit-identical: %s)" % (e, torch.equal(F0, F1)))
    assert e <= REL_FOLD
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    hp = T.hparams_from_args(W.C2_ARGS)
    for m in (0, 127):
        sl = slice(64 * m, 64 * (m + 1))
        Er, Fr = T.energy_and_forces(sd, hp, z[sl], pos[sl].double(), torch.zeros(64, dtype=torch.long))
        assert abs(E1[m].item() - Er.item()) / max(abs(Er.item()), 1e-12) < REL, m
        assert rel_err(F1[sl].cpu().double(), Fr) < REL, m
    E2, F2, _, _ = run(model, z, pos, batch, True)
    assert torch.equal(E1, E2) and torch.equal(F1, F2)


def test_straddling_molecules_keep_the_pair_of_launches(setup):
    from torchmdnet_amd import _C

    model, z, pos, _ = setup
    sizes = [63, 65] + [64] * 126
    batch = torch.repeat_interleave(torch.arange(128), torch.tensor(sizes))
    E0, F0, fold0, _ = run(model, z, pos, batch, False)
    E1, F1, fold1, route1 = run(model, z, pos, batch, True)
    assert fold0 == 0 and fold1 == 0 and route1 == _C.MSG_GD_TILE
    assert torch.equal(E0, E1) and torch.equal(F0, F1)
    assert bool(torch.isfinite(F1).all())


def test_static_graph_never_folds(setup):
    from torchmdnet_amd import workloads as W
    from torchmdnet_amd.models.model import create_model

    _, z, pos, batch = setup
    torch.manual_seed(0)
    model = create_model(dict(W.C2_ARGS, static_shapes=True)).cuda()
    _, F, fold, _ = run(model, z, pos, batch, True)
    assert fold == 0 and bool(torch.isfinite(F).all())
