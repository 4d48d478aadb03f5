"""Keeps tests/message_oracle.py and tests/message_unit_cases.py honest without a device.

* the adjoint, the distance-gradient halves and the tangent the oracle states equal torch.autograd of the forward statement they
  belong to, in float64, to 1e-12; the group product is tied to the plain 3x3 algebra;
* the graph builder gives the engine's form (symmetric, ascending columns, one self edge with pair id P per row, esign by col < row);
* the constants restated in the cases module are the ones in the .hip sources;
* the case list AS A WHOLE contains at least one 64-row tile of every class of the tile kernels' block-uniform branches and of
  the balanced walk's boundaries, so tests/test_gpu_message.py cannot silently stop covering one when a case is edited;
* profiles/message_unit_floor.json has a bound by the project's rule for every output of every case.
The GPU test (tests/test_gpu_message.py) compares the kernels with these statements."""
import os
import re

import pytest
import torch

from oracle.tensornet_adjoint import compose
from tests import kernel_unit_cases as K
from tests import message_oracle as O
from tests import message_unit_cases as M

TOL = 1e-12
F = 64  # two channel groups of 32, one of 64
CSRC = os.path.join(M.ROOT, "torchmd-net_amd", "csrc")


def _rn(*s, seed=0):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.fixture(scope="module", params=["ladder", "star64"])
def graph(request):
    g = dict(M.build_graph(request.param))
    if request.param == "ladder":  # the first 10 molecules are enough here
        n = 55
        keep = g["rows"] < n
        pid = torch.unique(g["epair"][keep & (g["rows"] != g["col"])])
        assert torch.equal(pid, torch.arange(pid.numel()))  # pairs are numbered in the order of (i, j)
        P = pid.numel()
        g.update(N=n, P=P, rows=g["rows"][keep], col=g["col"][keep], esign=g["esign"][keep], rowptr=g["rowptr"][:n + 1],
                 epair=torch.where(g["rows"][keep] == g["col"][keep], torch.tensor(P), g["epair"][keep]), batch=g["batch"][:n], B=10)
    return g


def test_graph_builder_gives_the_engines_form():
    for name in M.GRAPHS:
        g = M.build_graph(name)
        N, P, rows, col, ep = g["N"], g["P"], g["rows"], g["col"], g["epair"]
        assert N == sum(n for n, _ in M.GRAPHS[name]) and g["rowptr"][-1] == col.numel() == 2 * P + N
        assert torch.equal(rows, torch.repeat_interleave(torch.arange(N), g["rowptr"][1:] - g["rowptr"][:-1]))
        key = rows * N + col
        assert bool((key[1:] > key[:-1]).all())  # columns ascend within a row, no duplicates
        assert torch.equal(torch.sort(col * N + rows).values, key)  # symmetric
        self_e = rows == col
        assert int(self_e.sum()) == N and bool((ep[self_e] == P).all()) and bool((g["esign"][self_e] == 0).all())
        assert bool((ep[~self_e] < P).all()) and torch.equal(torch.bincount(ep[~self_e], minlength=P), torch.full((P,), 2))
        assert torch.equal(g["esign"][~self_e], torch.where(col < rows, 1.0, -1.0)[~self_e])
        lo = (~self_e) & (col < rows)  # both entries of a pair carry its id
        back = dict(zip((col[lo] * N + rows[lo]).tolist(), ep[lo].tolist()))
        up = (~self_e) & (col > rows)
        assert [back[k] for k in (rows[up] * N + col[up]).tolist()] == ep[up].tolist()
        assert bool((g["batch"][rows] == g["batch"][col]).all())


def test_group_product_is_the_3x3_statement():
    Y, Mi, kap = _rn(5, 9, 3, seed=1), _rn(5, 9, 3, seed=2), _rn(5, seed=3)
    Yf, Mf = compose(Y), compose(Mi)
    for o3 in (1, 0):
        Cm = kap[:, None, None, None] * (torch.einsum("nabf,nbcf->nacf", Yf, Mf) + torch.einsum("nabf,nbcf->nacf", Mf, Yf)) if o3 else \
            2 * torch.einsum("nabf,nbcf->nacf", Yf, Mf)
        want = Cm / ((Cm ** 2).sum((1, 2)) + 1)[:, None, None]
        assert O.per_atom_rel_err(compose(O.group_product(Y, Mi, kap, o3)), want) < TOL
    q, batch = _rn(2, seed=4), torch.tensor([0, 0, 1, 1, 1])
    assert torch.equal(O.kappa(q, batch, 5, Y), 1 + 0.1 * q[batch]) and torch.equal(O.kappa(kap, None, 5, Y), kap)
    assert torch.equal(O.kappa(None, None, 5, Y), torch.ones(5, dtype=torch.float64))


def test_gather_is_the_row_sum(graph):
    g = graph
    w, src = _rn(g["P"] + 1, 3, F, seed=5), _rn(g["N"], 9, F, seed=6)
    Mi = O.gather(g, w, src)
    for i in (0, g["N"] // 2, g["N"] - 1):
        acc = torch.zeros(9, F, dtype=torch.float64)
        for e in range(int(g["rowptr"][i]), int(g["rowptr"][i + 1])):
            for c in range(9):
                acc[c] += w[g["epair"][e], O.TYPE_OF[c]] * src[g["col"][e], c]
        assert float((Mi[i] - acc).abs().max()) < TOL * float(acc.abs().max())


def test_adjoint_is_the_gradient_of_the_message_sum(graph):
    g = graph
    w, gMi = _rn(g["P"] + 1, 3, F, seed=7), _rn(g["N"], 9, F, seed=8)
    src = _rn(g["N"], 9, F, seed=9).requires_grad_()
    (auto,) = torch.autograd.grad((gMi * O.gather(g, w, src)).sum(), src)
    assert O.per_atom_rel_err(O.adjoint(g, w, gMi), auto) < TOL


@pytest.mark.parametrize("group", [64, 32])
def test_pair_halves_sum_to_the_distance_gradient(graph, group):
    """h(i <- j) + h(j <- i), summed over the channel groups, is d <gMi, Mi(w0 + d dw)> / d d[p] for a scalar d per pair."""
    g = graph
    P = g["P"]
    w0, dw = _rn(P + 1, 3, F, seed=10), _rn(P + 1, 3, F, seed=11)
    gMi, Pn = _rn(g["N"], 9, F, seed=12), _rn(g["N"], 9, F, seed=13)
    d = torch.zeros(P + 1, dtype=torch.float64, requires_grad=True)
    (auto,) = torch.autograd.grad((gMi * O.gather(g, w0 + d[:, None, None] * dw, Pn)).sum(), d)
    slots, scale = O.pair_halves(g, dw, gMi, Pn, group)
    assert slots.shape == (F // group, 2 * P) and bool((scale > 0).all())
    both = slots.sum(0).reshape(P, 2).sum(1)
    assert float((both - auto[:P]).abs().max()) < TOL * float(scale.sum(0).max())
    # and each half on its own, entry by entry: slot 2 p + 0 belongs to the row with col < row
    for e in (1, g["col"].numel() // 2, g["col"].numel() - 2):
        i, j, p = int(g["rows"][e]), int(g["col"][e]), int(g["epair"][e])
        if i == j:
            continue
        t = (dw[p][O.TYPE_OF] * gMi[j] * Pn[i]).sum(0).reshape(F // group, group).sum(1)
        assert float((slots[:, 2 * p + (0 if j < i else 1)] - t).abs().max()) < TOL * float(scale.max())
        assert (g["esign"][e] > 0) == (j < i)


def test_dual_tangent_is_the_forward_mode_derivative(graph):
    g = graph
    w, w_t = _rn(g["P"] + 1, 3, F, seed=14), _rn(g["P"] + 1, 3, F, seed=15)
    src, src_t = _rn(g["N"], 9, F, seed=16), _rn(g["N"], 9, F, seed=17)
    val, tan = torch.autograd.functional.jvp(lambda a, b: O.gather(g, a, b), (w, src), (w_t, src_t))
    v, t = O.dual(g, w, w_t, src, src_t)
    assert O.per_atom_rel_err(v, val) < TOL and O.per_atom_rel_err(t, tan) < TOL


def test_constants_restated_in_the_cases_are_the_sources():
    pair = open(os.path.join(CSRC, "tn_message_pair.hip")).read()
    kern = open(os.path.join(CSRC, "tn_kernels.hip")).read()
    const = lambda text, name: int(re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text).group(1))
    assert (const(pair, "MP_TA"), const(pair, "MP_W"), const(pair, "MP_E"), const(pair, "MP_FC"), const(pair, "MP_U")) == \
        (M.MP_TA, M.MP_W, M.MP_E, M.MP_FC, M.MP_U)
    assert const(kern, "kEG") == M.KEG
    assert re.search(r"k_message_rows8<8, 4>\), dim3\(tiles \* nchunks\), dim3\(512\)", pair) and M.LPR == 8  # eight lanes own a row
    assert K.SENTINEL == 0x7FC0BEEF and K.TAIL == 64


def test_case_list_covers_every_tile_class():
    found, blocks = M.census_of_case_list()
    missing = [k for k, v in found.items() if not v]
    assert not missing, f"no tile of class {missing} in message_unit_cases.TILE_GRAPHS"
    # the named graphs still are what the classes were written for
    where = lambda k: {gname for gname, _ in found[k]}
    assert "one_atom" in where("one_live_row") and "chain65" in where("one_live_row")
    assert {"chain63", "chain65"} <= where("partial_tile_dead_rows_help")
    assert "complete64" in where("both_limits_met_exactly") and "complete64" in where("equal_rows_no_helper")
    assert {"complete65", "complete100", "mixed"} <= where("unstaged_global_slice")
    assert "complete65" in where("window_one_past_the_limit")
    assert {"complete100", "mixed"} <= where("global_slice_rows_longer_than_8_lpr")
    assert "chain130" in where("unstaged_lds_slice") and "star64" in where("full_tile_long_rows_hand_tails")
    assert "tiny90" in where("window_of_dozens_of_molecules")
    t = M.tile_census(*[M.build_graph("chain130")[k] for k in ("rowptr", "col", "N")])[0]
    assert t["wn"] == 84 and 2400 < t["nE"] < 2800
    t = M.tile_census(*[M.build_graph("complete65")[k] for k in ("rowptr", "col", "N")])[0]
    assert (t["wn"], t["nE"]) == (65, 4160)
    # xcd_chunk's remainder path: a block count that is no multiple of 8, in the launch that holds every class at once
    assert all(blocks[("mixed", Fv)] % 8 for Fv in (32, 96)) and any(b % 8 == 0 and b > 8 for b in blocks.values())
    # every tile graph at two channel counts or more, fewer than a dozen graphs, every unroll tail in the ladder
    assert all(len(Fs) >= 2 and set(Fs) <= {32, 96, 128, 256} for Fs in M.TILE_GRAPHS.values()) and len(M.TILE_GRAPHS) < 12
    g = M.build_graph("ladder")
    assert set((g["rowptr"][1:] - g["rowptr"][:-1]).tolist()) == set(range(1, 27)) and g["N"] == 351


def test_floor_file_has_a_bound_by_the_rule_for_every_case():
    doc = M.load_bounds()["cases"]
    assert set(doc) == {M.case_id(c) for c in M.all_cases()}
    for case in M.all_cases():
        ent = doc[M.case_id(case)]
        assert set(ent) == set(M.outputs_of(case[0]))
        for k, v in ent.items():
            assert v["bound"] == K.bound_of(v["floor"]) and K.BOUND_MIN <= v["bound"] <= K.BOUND_CAP


def test_floor_file_matches_a_recomputed_floor():
    """one small case recomputed: the file belongs to these inputs"""
    case = ("gd_tile", "chain65", 32)
    ent = M.load_bounds()["cases"][M.case_id(case)]
    for k, e in M.floor_of(case).items():
        assert 0.5 * ent[k]["floor"] <= e <= 2 * ent[k]["floor"], (k, e, ent[k]["floor"])  # (summation order of the host's torch)
