"""The slots of the reverse tile sweeps (csrc/tn_message_pair.hip: adjoint_tile_body).  A tile whose non-self entries carry one
contiguous range of pair ids, two entries per id, keeps its slots (pair, direction) in LDS during the walk and writes the range
[2 pmin, 2 pmax + 2) of its channel chunk's slot array once, coalesced; every other tile stores each slot from the edge loop.
Both kernels that share the body run here through tmdnet_debug_message_fold (folded: k_message_adjoint_rows8_fold; unfolded:
k_message_bwd_node, then k_message_adjoint_rows8) at F = 32 and 128, in the three modes of the group product.

Graphs (closed tiles throughout, complete molecules unless noted):
  complete64   2016 pairs: the LDS slot buffer exactly full                       (tests/message_fold_cases.py)
  singles64    64 one-atom molecules: no non-self entry, nothing staged, nothing written out
  mols3_61_64  3 + 61 atoms, then 64: the second tile's range starts at pair id 1833, an odd id - the head of its write-out is
               8-byte but not 16-byte aligned
  partial      64 (band) + 37 atoms: a partial last tile                           (tests/message_fold_cases.py)
  permuted64   complete64 with its 2016 pair ids sent through a fixed injection into 0 .. 2599: the ids span more than 2016
               and 584 pair rows in between belong to no edge - the range condition fails and the direct stores run

Per case and mode: slots (the whole arrays) and gPn bit-identical between the two kernels; both within the bound of the float64
oracle (tests/message_oracle.py through tests/message_fold_cases.py); the sentinel's bits intact in every slot no entry of the
graph owns, in the floats past 2 P and in the slot array beyond the kernel's count; every owned slot finite.

Bounds: profiles/message_fold_floor.json for the two graphs it lists; for the others the same rule on the case's own inputs -
max(2e-6, 4 x the float32 rounding floor of the reference against itself in float64), never above 1e-5 (kernel_unit_cases.bound_of),
the floor computed here on the CPU."""
import math

import pytest
import torch

from tests import kernel_unit_cases as K
from tests import message_fold_cases as M
from tests import message_oracle as O
from tests.message_unit_cases import FWD_MODES

pytestmark = pytest.mark.gpu

P_WIDE = 2600  # pair rows of permuted64 (2016 of them used)
OWN_GRAPHS = {"singles64": [1] * 64, "mols3_61_64": [3, 61, 64], "permuted64": [64]}
LISTED = ("complete64", "partial")  # graphs of message_fold_cases with their bounds in profiles/message_fold_floor.json
CASES = [(g, F) for g in ("complete64", "singles64", "mols3_61_64", "partial", "permuted64") for F in M.FS]


def own_graph(name):
    """complete molecules of the listed sizes in the form of message_fold_cases.build_graph; permuted64: pair ids through a fixed
    injection into 0 .. P_WIDE - 1, the self pair at P_WIDE"""
    rows, cols, batch = [], [], []
    base = 0
    for m, n in enumerate(OWN_GRAPHS[name]):
        i, j = torch.nonzero(torch.ones(n, n, dtype=torch.bool), as_tuple=True)
        rows.append(i + base)
        cols.append(j + base)
        batch += [m] * n
        base += n
    rows, cols = torch.cat(rows), torch.cat(cols)
    N = base
    assert bool((rows // 64 == cols // 64).all())
    lower = rows > cols
    used = int(lower.sum())
    ids = torch.arange(used)
    P = used
    if name == "permuted64":
        P = P_WIDE
        ids = torch.randperm(P_WIDE, generator=torch.Generator().manual_seed(64))[:used]
        assert int(ids.max() - ids.min()) + 1 > 2016
    pid = torch.full((N * N,), -1, dtype=torch.int64)
    pid[(rows * N + cols)[lower]] = ids
    epair = torch.where(rows == cols, torch.tensor(P), pid[torch.maximum(rows, cols) * N + torch.minimum(rows, cols)])
    esign = torch.where(rows == cols, 0.0, torch.where(cols < rows, 1.0, -1.0)).float()
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.bincount(rows, minlength=N).cumsum(0)
    return dict(N=N, P=P, rowptr=rowptr, rows=rows, col=cols, epair=epair, esign=esign, batch=torch.tensor(batch), B=len(OWN_GRAPHS[name]))


def own_inputs(name, g, F):
    """scaled as message_fold_cases.make_inputs scales them"""
    N, P = g["N"], g["P"]
    gen = torch.Generator().manual_seed(9000011 * (1 + sorted(OWN_GRAPHS).index(name)) + F)
    rn = lambda *s: torch.randn(*s, generator=gen)
    sw = (N / g["col"].numel()) ** 0.5
    return dict(w=rn(P + 1, 3, F) * sw, dw=rn(P + 1, 3, F) * sw, Pn=rn(N, 9, F) * 0.5, Mi=rn(N, 9, F) * 0.5, gCh=rn(N, 9, F),
                q_mol=rn(g["B"]), kap_atom=1 + 0.3 * rn(N))


def owned_slots(g):
    """indices 2 p + dir of the slots some entry of the graph owns, ascending"""
    ns = g["rows"] != g["col"]
    return torch.unique(2 * g["epair"][ns] + (g["col"][ns] > g["rows"][ns]).long())


def errors(got_gPn, got_slots, ref, own):
    """the figures of message_fold_cases.errors, the slots on the owned ones only (the reference holds zeros elsewhere)"""
    rs, sc = ref["slots"]
    return {"gPn": O.per_atom_rel_err(got_gPn, ref["gPn"]), "slots": O.slot_rel_err(got_slots[:, own], rs[:, own], sc[:, own])}


@pytest.fixture(scope="module")
def listed_bounds():
    return M.load_bounds()["cases"]


@pytest.mark.parametrize("case", CASES, ids=[M.case_id(c) for c in CASES])
def test_slots_and_gPn_of_both_reverse_sweeps(hip_lib, listed_bounds, case):
    gname, F = case
    if gname in LISTED:
        g, d = M.build_graph(gname), M.make_inputs(gname, F)
    else:
        g = own_graph(gname)
        d = own_inputs(gname, g, F)
    N, P, cnt = g["N"], g["P"], F // M.GROUP
    own_cpu = owned_slots(g)
    if gname in LISTED:
        ent = listed_bounds[M.case_id(case)]
        bound = {mode: {k: ent[mode][k]["bound"] for k in ("gPn", "slots")} for mode in FWD_MODES}
    else:  # the rule of the listed bounds on this case's inputs (CPU)
        d64c = {k: v.double() for k, v in d.items()}
        bound = {}
        for mode in FWD_MODES:
            r32, r64 = M.reference(g, d, mode), M.reference(g, d64c, mode)
            fl = errors(r32["gPn"], r32["slots"][0], r64, own_cpu)
            bound[mode] = {k: K.bound_of(v) for k, v in fl.items()}
    dev = "cuda"
    gd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}
    dd = {k: v.to(dev).contiguous() for k, v in d.items()}
    d64 = {k: v.double() for k, v in dd.items()}
    own = own_cpu.to(dev)
    csr = dict(rowptr=gd["rowptr"].int(), col=gd["col"].int(), epair=gd["epair"].int(), esign=gd["esign"].contiguous(),
               counts=torch.tensor([P, g["col"].numel(), 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev))
    unowned = torch.ones(2 * P + 2 + M.SLOT_PAD, dtype=torch.bool, device=dev)
    unowned[own] = False
    for mode in FWD_MODES:
        ref = M.reference(gd, d64, mode)
        fo, un = M.fresh_outputs(g, F, dev), M.fresh_outputs(g, F, dev)
        assert M.launch(hip_lib, gd, csr, dd, F, mode, fo, True) == 0
        assert M.launch(hip_lib, gd, csr, dd, F, mode, un, False) == 0
        for tag, o in (("folded", fo), ("unfolded", un)):
            e = errors(o["gPn"][:N], o["slots"][:cnt, :2 * P], ref, own)
            print(M.case_id(case), mode, tag, {k: f"{v:.3g}" for k, v in e.items()}, bound[mode])
            assert bool(torch.isfinite(o["slots"][:cnt][:, own]).all()), (case, mode, tag, "an owned slot was not written")
            for k, v in e.items():
                assert 2e-6 <= bound[mode][k] <= 1e-5
                assert math.isfinite(v) and v < bound[mode][k], (case, mode, tag, k, v, bound[mode][k])
            assert bool((K.bits(o["slots"][:cnt][:, unowned]) == K.SENTINEL).all()), (case, mode, tag, "a slot no entry owns, or past 2 P, was written")
            assert bool((K.bits(o["slots"][cnt:]) == K.SENTINEL).all()), (case, mode, tag, "a slot array beyond the kernel's count was written")
            assert bool((K.bits(o["gPn"][N:]) == K.SENTINEL).all()), (case, mode, tag, "rows behind N were written")
        assert bool(torch.equal(K.bits(fo["slots"]), K.bits(un["slots"]))), (case, mode, "the slots of the two kernels differ")
        assert bool(torch.equal(K.bits(fo["gPn"]), K.bits(un["gPn"]))), (case, mode, "gPn of the two kernels differs")
