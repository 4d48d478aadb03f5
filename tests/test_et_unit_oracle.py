"""not-gpu: the float64 statements the ET kernel-level unit tests compare with (tests/et_unit_oracle.py) and their case list
(tests/et_unit_cases.py).  Every hand-written adjoint against autograd of the forward statement (1e-12 in float64); the forward
statement against the edge sweep of oracle/et_adjoint.py on the molecules of the reference fixtures; the census of the tile
classes over the case list; the size of the attention pre-activations of the ordinary cases; the constants restated from the
kernels against the sources; profiles/et_unit_floor.json against the case list and the bound rule."""
import os
import re

import pytest
import torch

from tests import et_unit_cases as U
from tests import et_unit_oracle as O
from tests import kernel_unit_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _f64(d):
    return {k: (v.double() if torch.is_tensor(v) else v) for k, v in d.items()}


@pytest.mark.parametrize("gname,F,hd", [("edge47", 8, 4), ("chain", 6, 2), ("ladder", 8, 8), ("one_atom", 4, 2)])
@pytest.mark.parametrize("combo", U.COMBOS8, ids=lambda c: "k%dv%dc%d" % c)
def test_attention_adjoint_is_autograd_of_the_forward_statement(gname, F, hd, combo):
    """g_qkv, g_vec, and PER CHANNEL the edge's d / d d(pair) and d / d rhat - the quantities whose partial sums the slot arrays
    hold - equal autograd of sum(g_xagg xagg + g_vagg vagg); the slot arrays are those channels' sums, each edge in its own slot."""
    g = U.build_graph(gname)
    d, lay = U.make_inputs(gname, F, hd, combo)
    d = _f64(d)
    E = g["E"]
    qkv, vec = d["qkv"].clone().requires_grad_(), d["vec"].clone().requires_grad_()
    delta = torch.zeros(E, F, dtype=torch.float64, requires_grad=True)
    t0 = O.edge_terms(g, d, lay)
    rhat_c = t0["rhat"][:, :, None].expand(E, 3, F).clone().requires_grad_()
    xagg, vagg = O.attn_forward(g, dict(d, qkv=qkv, vec=vec), lay, delta, rhat_c)
    x0, v0 = O.attn_forward(g, d, lay)
    assert torch.equal(x0, xagg.detach()) and torch.equal(v0, vagg.detach())  # delta = 0 and rhat per channel change nothing
    L = (d["g_xagg"] * xagg).sum() + (d["g_vagg"] * vagg).sum()
    a_qkv, a_vec, a_delta, a_rhat = torch.autograd.grad(L, [qkv, vec, delta, rhat_c])
    adj = O.attn_adjoint(g, d, lay)
    for n, name in enumerate(("g_q", "g_k", "g_vx", "g_v1", "g_v2")):
        assert rel(adj["g_qkv"][:, n * F:(n + 1) * F], a_qkv[:, n * F:(n + 1) * F]) < TOL, name
    assert rel(adj["g_vec"], a_vec) < TOL
    assert rel(adj["gd_c"], a_delta) < TOL and rel(adj["gr_c"], a_rhat) < TOL
    assert bool((adj["gd_abs"] >= adj["gd_c"].abs() - 1e-300).all())
    # slot arrays: one per `group` channels; slot 2 p + dir belongs to exactly one entry, the self edges to none
    sl = O.slot_index(g)
    own = sl >= 0
    assert int(own.sum()) == 2 * g["P"] and sorted(sl[own].tolist()) == list(range(2 * g["P"]))
    assert bool((g["esign"][own] != 0).all()) and bool((g["rows"][~own] == g["col"][~own]).all())
    assert bool(((sl[own] % 2 == 0) == (g["col"][own] < g["rows"][own])).all())  # dir 0: the row atom is the pair's first (j < i)
    for group in (32, 64, 2):
        if group == 2 and F % 2:
            continue
        gd2, gds, gr2, grs = O.slot_sums(g, adj, lay, group)
        W = -(-F // group)
        assert gd2.shape == (W, 2 * g["P"]) and gr2.shape == (W, 2 * g["P"], 3)
        for w in range(W):
            ch = slice(w * group, min(F, (w + 1) * group))
            assert g["P"] == 0 or rel(gd2[w][sl[own]], a_delta[own][:, ch].sum(1)) < TOL
            assert g["P"] == 0 or rel(gr2[w][sl[own]], a_rhat[own][:, :, ch].sum(2)) < TOL
        assert bool((gds >= gd2.abs() - 1e-300).all()) and bool((grs >= gr2.abs() - 1e-300).all())
    # the pair combine is the sum the geometry pass wants: d / d d(p) of both directions, d / d prhat = -d / d rhat(i <- j) + ...
    nw = 3
    gd2, _, gr2, _ = O.slot_sums(g, adj, lay, -(-F // nw))
    extra = torch.randn(2 * (g["P"] + 1), dtype=torch.float64)
    gd, gds, grh, grs = O.pair_combine(gd2, gr2, extra, g["P"])
    for p in range(min(g["P"], 7)):
        e_lo = [e for e in range(E) if int(g["epair"][e]) == p]
        assert len(e_lo) == 2
        assert abs(float(gd[p]) - float(extra[2 * p] + a_delta[e_lo].sum())) < 1e-11 * float(gds[p])
        want = sum(float(g["esign"][e]) * -a_rhat[e].sum(1) for e in e_lo)  # rhat(i <- j) = -esign prhat
        assert float((grh[p] - want).abs().max()) < 1e-11 * float(grs[p].max())


@pytest.mark.parametrize("combo", [(1, 1, 0), (1, 0, 1), (0, 1, 1), (0, 1, 0)], ids=lambda c: "k%dv%dc%d" % c)
def test_filter_row_adjoints_are_autograd(combo):
    """TRAIN_FILTER: the two directions' slots of a pair add up to d L / d dkv[p], the atoms' self rows to d L / d dkv[P];
    TRAIN_GPRE: times silu'(pre) when dkv = silu(pre)."""
    gname, F, hd = "edge47", 8, 4
    g = U.build_graph(gname)
    d, lay = U.make_inputs(gname, F, hd, combo)
    d = _f64(d)
    pre = torch.randn(g["P"] + 1, lay["Wd"], dtype=torch.float64, requires_grad=True)
    dkv = O.silu(pre)
    xagg, vagg = O.attn_forward(g, dict(d, dkv=dkv), lay)
    L = (d["g_xagg"] * xagg).sum() + (d["g_vagg"] * vagg).sum()
    a_dkv, a_pre = torch.autograd.grad(L, [dkv, pre])
    slots, self_rows = O.train_filter(g, dict(d, dkv=dkv.detach()), lay)
    assert not torch.isnan(slots).any() and not torch.isnan(self_rows).any()  # these layouts use every column
    assert rel(slots[0] + slots[1], a_dkv[:g["P"]]) < TOL and rel(self_rows.sum(0), a_dkv[g["P"]]) < TOL
    assert rel(O.train_gpre(slots, self_rows.sum(0), pre.detach()), a_pre) < TOL


def test_neighbour_embedding_adjoints_are_autograd():
    gname, F = "ladder", 6
    g = U.build_graph(gname)
    d = {k: (v.double() if v.is_floating_point() else v) for k, v in U.other_inputs(gname, F).items()}
    N, P = g["N"], g["P"]
    en = d["embN"][d["z"]].clone().requires_grad_()
    Wn = d["Wn"].clone().requires_grad_()
    delta = torch.zeros(P + 1, dtype=torch.float64, requires_grad=True)
    xcat = O.nbr_embed(g, d["z"], d["emb"], en, Wn + d["dWn"] * delta[:, None])
    assert torch.equal(xcat[:, :F], d["emb"][d["z"]])
    # plain statement of the sum, entry by entry
    want = torch.zeros(N, F, dtype=torch.float64)
    for e in range(g["E"]):
        i, j = int(g["rows"][e]), int(g["col"][e])
        if i != j:
            want[i] += d["Wn"][int(g["epair"][e])] * d["embN"][d["z"][j]]
    assert rel(xcat[:, F:].detach(), want) < TOL
    g_nbr = d["g_xcat"][:, F:]
    a_en, a_Wn, a_delta = torch.autograd.grad((g_nbr * xcat[:, F:]).sum(), [en, Wn, delta])
    v, s = O.nbr_embed_bwd(g, en.detach(), g_nbr, d["dWn"])
    assert rel(v, a_delta[:P]) < TOL and float(a_delta[P]) == 0.0 and bool((s >= v.abs()).all())
    slots, gEN = O.train_nbr(g, en.detach(), d["Wn"], g_nbr)
    assert rel(slots[0] + slots[1], a_Wn[:P]) < TOL and rel(gEN, a_en) < TOL


@pytest.mark.parametrize("fixture", ["et_tiny_ref.pt", "et_tiny_vc_ref.pt"])
def test_forward_statement_is_the_edge_sweep_of_the_et_specification(golden_dir, fixture):
    """xagg and vagg of every layer of oracle/et_adjoint.py (pinned to the unmodified reference in tests/test_oracle.py), from its
    own operands re-laid as the kernels want them: symmetric CSR with the row atom as target, per-pair rows, prhat per pair."""
    from oracle import et_adjoint as EA
    from oracle import et_torch as ET
    from oracle import tensornet_torch as T

    gold = torch.load(os.path.join(golden_dir, fixture))
    hp = ET.hparams_from_args(gold["args"])
    sd = T.cast_state_dict(gold["state_dict"], torch.float64)
    _, _, cache = EA.energy_forces(sd, hp, gold["z"], gold["pos"].double(), gold["batch"], want_cache=True)
    F, hd = hp["hidden_channels"], hp["hidden_channels"] // hp["num_heads"]
    N = gold["z"].shape[0]
    for l in range(hp["num_layers"]):
        c = cache[f"attn_layer{l}"]
        order = torch.argsort(c["tgt"] * N + c["src"])
        rows, col = c["tgt"][order], c["src"][order]
        lower = rows > col
        P = int(lower.sum())
        pid = torch.full((N * N,), -1, dtype=torch.int64)
        pid[(rows * N + col)[lower]] = torch.arange(P)
        epair = torch.where(rows == col, torch.tensor(P), pid[torch.maximum(rows, col) * N + torch.minimum(rows, col)])
        esign = torch.where(rows == col, 0.0, torch.where(col < rows, 1.0, -1.0))
        g = dict(N=N, P=P, E=int(rows.numel()), rows=rows, col=col, epair=epair, esign=esign)
        first = torch.zeros(P + 1, dtype=torch.int64)  # an entry of every pair (the self pair: any self edge)
        first[epair] = torch.arange(rows.numel())
        per_pair = lambda t: t[order][first]
        has_dk, has_dv = c["dk"] is not None, c["dv"] is not None
        parts = ([per_pair(c["dk"])] if has_dk else []) + ([per_pair(t) for t in c["dv"]] if has_dv else [])
        lay = U.layout_of(F, hd, (int(has_dk), int(has_dv), int(hp["vector_cutoff"])))
        low = torch.nonzero(lower)[:, 0]  # the entry (i <- j), i > j, of every pair: rhat(i <- j) = -prhat
        d = dict(qkv=torch.cat([c["q"], c["k"], c["vx"], c["v1"], c["v2"]], 1), vec=c["vec"], C=per_pair(c["C"]),
                 dkv=torch.cat(parts, 1) if parts else None, prhat=-c["rhat"][order][low][torch.argsort(epair[low])])
        xagg, vagg = O.attn_forward(g, d, lay)
        assert rel(xagg, c["xagg"]) < TOL, (fixture, l)
        if float(c["vagg"].abs().max()) > 0:
            assert rel(vagg, c["vagg"]) < TOL, (fixture, l)


def test_case_list_contains_every_tile_class():
    """Each class is computed from the graphs by the kernels' own rules (tile packing, slot order from a longest row of 48 on);
    the case list as a whole has a tile of every class, every tile graph runs with both row types, the slot-order graphs with
    and without the mailbox and with tkv below dkv, and every (keys, values, cutoff) combination at one tile and one row shape."""
    found = U.census_of_case_list()
    missing = [k for k, v in found.items() if not v]
    assert not missing, missing
    cases = U.all_cases()
    assert len({U.case_id(c) for c in cases}) == len(cases)
    tile = [c for c in cases if c.kernel == U.TILE]
    for gname in U.TILE_GRAPHS:
        assert {c.bf16 for c in tile if c.graph == gname} == {0, 1}, gname
        assert {c.combo for c in tile if c.graph == gname} >= set(U.COMBOS3), gname
    assert {(c.F, c.hd) for c in tile} >= set(U.TILE_SHAPES)
    assert {(c.F, c.hd) for c in cases if c.kernel == U.ROW_PIPELINED} == set(U.PIPE_SHAPES)
    assert {(c.F, c.hd) for c in cases if c.kernel == U.ROW_GENERIC and c.variant != "extreme"} == set(U.GENERIC_SHAPES)
    for sel in (U.TILE, U.ROW_PIPELINED, U.ROW_GENERIC):
        assert any({c.combo for c in cases if c.kernel == sel and (c.F, c.hd) == s and c.bf16 == 0} == set(U.COMBOS8)
                   for s in U.TILE_SHAPES + U.PIPE_SHAPES + U.GENERIC_SHAPES), sel
        assert sum(1 for c in cases if c.kernel == sel and c.variant == "extreme") == 1
        assert any(c.bf16 for c in cases if c.kernel == sel)
    for gname in U.SLOT_GRAPHS:
        assert any(t["slot"] for t in U.tile_census(U.build_graph(gname))), gname
        assert {c.variant for c in tile if c.graph == gname and c.combo == (1, 1, 0) and not c.bf16} >= {"", "nomb", "tkvlow"}, gname
    # the mailbox: taken by both sweeps, by the reverse sweep alone (one projection), dropped (bf16 rows, switched off, tkv low)
    mb = {U.mailbox_runs(c) for c in tile}
    assert mb == {(True, True), (False, True), (True, False), (False, False)}
    assert U.mailbox_runs(U.Case(U.TILE, "full64", 64, 16, (1, 1, 0), 0, "tkvlow")) == (True, False)
    # list and slot order in ONE launch, with a partial last tile
    t = U.tile_census(U.build_graph("full64x3+37"))
    assert [x["slot"] for x in t] == [True, True, True, False] and t[-1]["partial"]
    # greedy packing: 1 + 2 + 5 + 20 + 36 | 30 + 34 | 64 | 63 + 1
    assert [x["mols"] for x in U.tile_census(U.build_graph("packed"))] == [[1, 2, 5, 20, 36], [30, 34], [64], [63, 1]]
    # the fill rule met exactly: 1024 entries = 0.25 x 4096, so bf16 rows take the tile and one atom fewer does not
    g32, g31 = U.build_graph("fill_edge32"), U.build_graph("fill_edge31")
    assert g32["E"] == 1024 and U.tile_prep_statement(g32, U.MIN_FILL_BF16)[0] == 0 and U.tile_prep_statement(g31, U.MIN_FILL_BF16)[0] == 1
    assert U.tile_prep_statement(g32, U.MIN_FILL_F32)[0] == 1 and U.tile_prep_statement(U.build_graph("open70"), 0.0)[0] == 1
    # the row kernels meet every unroll tail: rows of 1 .. 26 entries, and a system of one atom
    lad = U.build_graph("ladder")
    assert set((lad["rowptr"][1:] - lad["rowptr"][:-1]).tolist()) == set(range(1, 27)) and U.build_graph("one_atom")["N"] == 1
    # every graph is in the engine's form: symmetric, columns ascending, one self edge per row
    for gname in U.GRAPHS:
        g = U.build_graph(gname)
        key = (g["rows"] * g["N"] + g["col"]).tolist()
        assert key == sorted(set(key)) and set(key) == set((g["col"] * g["N"] + g["rows"]).tolist())
        assert int((g["rows"] == g["col"]).sum()) == g["N"]
        assert bool((g["pair_i"] > g["pair_j"]).all()) and bool((g["batch"][g["rows"]] == g["batch"][g["col"]]).all())


def test_ordinary_cases_keep_the_preactivations_small():
    """|a| <= 4 in every case but the extremes: the bounds are rounding bounds, and silu's curvature is not to be confused with it"""
    seen = {}
    for c in U.all_cases():
        if c.variant == "extreme":
            continue
        key = (c.graph, c.F, c.hd, c.combo, c.bf16)
        if key not in seen:
            seen[key] = U.max_preactivation(*key)
        assert seen[key] <= 4.0, (U.case_id(c), seen[key])
    for c in U.all_cases():
        if c.variant == "extreme":
            g = U.build_graph(c.graph)
            d, lay = U.make_inputs(c.graph, c.F, c.hd, c.combo, c.bf16, True)
            a = O.edge_terms(g, _f64(d), lay)["a"]
            assert set(a.unique().tolist()) == set(U.EXTREMES), U.case_id(c)  # exactly these values, every one of them


def test_constants_restated_from_the_kernels():
    src = open(os.path.join(ROOT, "torchmd-net_amd", "csrc", "tn_et_g16.hip")).read()
    assert int(re.search(r"constexpr int G16_ROWS = (\d+);", src).group(1)) == U.G16_ROWS
    assert int(re.search(r'getenv\("TMDNET_ET_G16_SLOT_MIN"\)\) : (\d+);', src).group(1)) == U.SLOT_MIN
    assert int(re.search(r'getenv\("TMDNET_ET_G16_SYNC"\)\) : (\d+);', src).group(1)) == U.SYNC_EVERY
    m = re.search(r"\(pair_bf16 \? ([0-9.]+)f : ([0-9.]+)f\)", src)
    assert (float(m.group(1)), float(m.group(2))) == (U.MIN_FILL_BF16, U.MIN_FILL_F32)
    assert "pair (24 bits)" in src and "P1 - 1 <= 0xFFFFFF" in src and U.PAIR_ID_BITS == 24
    assert U.sweep_waves(96) == 3 and U.sweep_waves(40) == 1 and U.sweep_waves(64) == 2
    from torchmdnet_amd import _C
    assert (U.OP_QUERY, U.OP_TILE_PREP, U.OP_ATTN_FWD, U.OP_ATTN_BWD, U.OP_PAIR_COMBINE, U.OP_NBR_EMBED, U.OP_NBR_EMBED_BWD, U.OP_TRAIN_NBR,
            U.OP_TRAIN_FILTER, U.OP_TRAIN_GPRE) == (_C.ET_OP_QUERY, _C.ET_OP_TILE_PREP, _C.ET_OP_ATTN_FWD, _C.ET_OP_ATTN_BWD, _C.ET_OP_PAIR_COMBINE,
                                                    _C.ET_OP_NBR_EMBED, _C.ET_OP_NBR_EMBED_BWD, _C.ET_OP_TRAIN_NBR, _C.ET_OP_TRAIN_FILTER,
                                                    _C.ET_OP_TRAIN_GPRE)
    assert (U.AUTO, U.ROW_GENERIC, U.ROW_PIPELINED, U.TILE) == (_C.ET_AUTO, _C.ET_ROW_GENERIC, _C.ET_ROW_PIPELINED, _C.ET_TILE)
    hdr = open(os.path.join(ROOT, "include", "tmdnet_amd.h")).read()
    for name in ("OP_QUERY", "OP_TILE_PREP", "OP_ATTN_FWD", "OP_ATTN_BWD", "OP_PAIR_COMBINE", "OP_NBR_EMBED", "OP_NBR_EMBED_BWD",
                 "OP_TRAIN_NBR", "OP_TRAIN_FILTER", "OP_TRAIN_GPRE", "AUTO", "ROW_GENERIC", "ROW_PIPELINED", "TILE"):
        assert int(re.search(r"#define\s+TMDNET_ET_%s\s+(\d+)" % name, hdr).group(1)) == getattr(_C, "ET_" + name), name


def test_floor_file_matches_the_case_list_and_the_rule():
    """profiles/et_unit_floor.json (tools/et_unit_floor.py) has an entry per case and output, bound = bound_of(floor + the analytic
    term of the hardware sigmoid, zero unless the tool's docstring derives one); a sample of floors is recomputed here."""
    doc = U.load_bounds()["cases"]
    ids = [U.case_id(c) for c in U.all_cases()] + [U.other_id(gn, F) for gn in U.OTHER_GRAPHS for F in U.OTHER_F] + \
        [U.filter_id(fc) for fc in U.FILTER_CASES]
    assert sorted(doc) == sorted(ids)
    for cid, ent in doc.items():
        for k, v in ent.items():
            assert v["bound"] == K.bound_of(v["floor"]) and 2e-6 <= v["bound"] <= 1e-5, (cid, k)
    for c in U.all_cases()[::37]:
        fl = U.floor_of(c)
        assert set(fl) == set(U.FWD_OUTPUTS + U.BWD_OUTPUTS) == set(doc[U.case_id(c)])
        for k, v in fl.items():
            assert abs(v - doc[U.case_id(c)][k]["floor"]) <= 0.5 * v + 1e-9, (U.case_id(c), k, v)  # (float32 sums: thread count may move the last bits)
