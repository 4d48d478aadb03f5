"""TEST INFRASTRUCTURE ONLY -- the cases of the kernel-level unit tests of the Equivariant Transformer's edge sweeps
(tmdnet_debug_et): hand-built graphs, seeded inputs, launches and the figures the tests assert on.  One statement serves three
users: tests/test_gpu_et_unit.py (asserts), tools/et_unit_floor.py (the fp32 rounding floor of the reference on these very inputs
without a device, and the errors observed on the device, into profiles/et_unit_floor.json, from which the test reads its bounds)
and tests/test_et_unit_oracle.py (the class census of the tiles over the case list, no device).
"""
import ctypes as C
import json
import os
from collections import namedtuple

import numpy as np
import torch

from tests import et_unit_oracle as O
from tests import message_unit_cases as M
from tests.kernel_unit_cases import SENTINEL, TAIL, bits, sentinel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR_JSON = os.path.join(ROOT, "profiles", "et_unit_floor.json")
# restated from csrc/tn_et_g16.hip (tests/test_et_unit_oracle.py parses the source and compares)
G16_ROWS, SLOT_MIN, SYNC_EVERY, MIN_FILL_F32, MIN_FILL_BF16, PAIR_ID_BITS = 64, 48, 4, 0.70, 0.25, 24
# ops and selectors of tmdnet_debug_et (the values of torchmdnet_amd._C, restated so that this module imports without the library)
(OP_QUERY, OP_TILE_PREP, OP_ATTN_FWD, OP_ATTN_BWD, OP_PAIR_COMBINE, OP_NBR_EMBED, OP_NBR_EMBED_BWD, OP_TRAIN_NBR, OP_TRAIN_FILTER,
 OP_TRAIN_GPRE) = range(10)
AUTO, ROW_GENERIC, ROW_PIPELINED, TILE = range(4)
KERNEL_NAMES = {AUTO: "auto", ROW_GENERIC: "row", ROW_PIPELINED: "rowp", TILE: "tile"}

# graph name -> [(atoms, rule)] per molecule; rule: "complete", ("band", b): |a - b| <= b, ("hub", L): atom 0 has exactly L entries
# (itself and atoms 1 .. L - 1), the others a band of 3 with the pairs (a, a + 2), a even, taken out (rows with gaps), and the last
# atom has nothing but its self edge
GRAPHS = {
    "full64": [(64, "complete")],
    "full64x3+37": [(64, "complete")] * 3 + [(37, "complete")],
    "edge48": [(64, ("hub", 48))],
    "edge47": [(64, ("hub", 47))],
    "packed": [(n, "complete") for n in (1, 2, 5, 20, 36, 30, 34, 64, 63, 1)],
    "chain": [(40, ("band", 1))],
    "fill_edge32": [(32, "complete")],
    "fill_edge31": [(31, "complete")],
    "open70": [(70, "complete")],
    "ladder": list(M.GRAPHS["ladder"]),
    "one_atom": [(1, "complete")],
}
TILE_GRAPHS = ("full64", "full64x3+37", "edge48", "edge47", "packed", "chain", "fill_edge32")
SLOT_GRAPHS = ("full64", "full64x3+37", "edge48", "packed")  # graphs with a tile that walks in slot order
ROW_GRAPHS = ("ladder", "packed", "open70", "one_atom")
TILE_SHAPES = [(32, 2), (32, 32), (64, 4), (64, 8), (64, 16), (96, 32), (128, 16)]
PIPE_SHAPES = [(64, 4), (64, 16), (128, 16)]
GENERIC_SHAPES = [(40, 8), (48, 16), (64, 64), (96, 32)]
ALL_SHAPES_TILE_GRAPHS = ("full64x3+37", "edge48")  # every tile shape runs on these two; (64, 16) and (32, 2) on the others
# (keys, values, vector cutoff): the three distinct layouts with the cutoff alternating, and all eight
COMBOS3 = [(1, 1, 0), (1, 0, 1), (0, 1, 0)]
COMBOS8 = [(k, v, c) for k in (0, 1) for v in (0, 1) for c in (0, 1)]
EXTREMES = [30.0, -30.0, 88.0, -88.0, 1e4, -1e4, 0.5]  # pre-activations of the extremes cases (and one ordinary value)

# kernel: selector; variant: "" | "nomb" (mailbox off) | "tkvlow" (tkv allocated below dkv) | "extreme" | "slotall" (slot order whatever
# the longest row: slot_min = 1) | "listall" (list order always: slot_min = 0) | "sync0" / "sync2" (list order's barrier interval)
Case = namedtuple("Case", "kernel graph F hd combo bf16 variant")


def all_cases():
    out = []
    for gname in TILE_GRAPHS:
        shapes = TILE_SHAPES if gname in ALL_SHAPES_TILE_GRAPHS else [(64, 16), (32, 2)]
        for (F, hd) in shapes:
            combos = COMBOS8 if (gname == "full64x3+37" and (F, hd) == (64, 16)) else COMBOS3
            out += [Case(TILE, gname, F, hd, cb, bf, "") for cb in combos for bf in (0, 1)]
    for gname in SLOT_GRAPHS:  # the mailbox needs fp32 rows and both projections
        out += [Case(TILE, gname, 64, 16, (1, 1, 0), 0, v) for v in ("nomb", "tkvlow")]
    out.append(Case(TILE, "full64x3+37", 128, 16, (1, 1, 1), 0, "nomb"))
    out.append(Case(TILE, "open70", 64, 16, (1, 1, 0), 0, ""))  # open tiles: the tile kernels write nothing
    # the walks off their thresholds: slot order (and the mailbox) on sparse and partial tiles, list order on full ones, and the
    # list walk without and with a barrier every other step
    out += [Case(TILE, "chain", 64, 16, (1, 1, 0), 0, "slotall"), Case(TILE, "edge47", 64, 16, (1, 1, 0), 0, "slotall"),
            Case(TILE, "edge47", 64, 16, (1, 0, 1), 1, "slotall"), Case(TILE, "full64x3+37", 64, 16, (0, 1, 0), 0, "slotall"),
            Case(TILE, "full64", 64, 16, (1, 1, 0), 0, "listall"), Case(TILE, "packed", 64, 16, (1, 1, 0), 1, "listall"),
            Case(TILE, "full64x3+37", 64, 16, (1, 1, 0), 0, "sync0"), Case(TILE, "chain", 32, 2, (1, 1, 0), 0, "sync2")]
    for sel, shapes in ((ROW_PIPELINED, PIPE_SHAPES), (ROW_GENERIC, GENERIC_SHAPES)):
        for gname in ROW_GRAPHS:
            for (F, hd) in shapes:
                combos = COMBOS8 if (gname == "ladder" and (F, hd) in ((64, 16), (48, 16))) else COMBOS3
                if gname in ("open70", "one_atom"):  # rows of 70 entries, and a row of one: one layout per shape
                    combos = COMBOS3[:1]
                out += [Case(sel, gname, F, hd, cb, 0, "") for cb in combos]
                if gname == "ladder":  # the bf16-row walk of the row kernels
                    out += [Case(sel, gname, F, hd, cb, 1, "") for cb in COMBOS3]
    out += [Case(TILE, "full64", 64, 4, (1, 1, 0), 0, "extreme"), Case(ROW_PIPELINED, "ladder", 64, 4, (1, 1, 0), 0, "extreme"),
            Case(ROW_GENERIC, "ladder", 40, 8, (1, 1, 0), 0, "extreme")]
    return out


def case_id(c):
    return "%s-%s-F%d-hd%d-k%dv%dc%d-%s%s" % (KERNEL_NAMES[c.kernel], c.graph, c.F, c.hd, *c.combo, "bf16" if c.bf16 else "fp32",
                                             "-" + c.variant if c.variant else "")


FWD_OUTPUTS = ["xagg", "vagg0", "vagg1", "vagg2"]
BWD_OUTPUTS = ["g_q", "g_k", "g_vx", "g_v1", "g_v2", "g_vec", "gd2", "gr2"]


# ====================================================================================== graphs
_graph_cache = {}


def _adjacency(n, rule):
    a = torch.arange(n)
    if rule == "complete":
        return torch.ones(n, n, dtype=torch.bool)
    if rule[0] == "band":
        return (a[:, None] - a[None, :]).abs() <= rule[1]
    assert rule[0] == "hub"
    L = rule[1]
    adj = (a[:, None] - a[None, :]).abs() <= 3
    lo, hi = torch.minimum(a[:, None], a[None, :]), torch.maximum(a[:, None], a[None, :])
    adj &= ~((hi - lo == 2) & (lo % 2 == 0))
    hub = ((lo == 0) & (hi < L))
    adj = (adj & (lo != 0)) | hub
    adj[n - 1, :] = False
    adj[:, n - 1] = False
    adj |= torch.eye(n, dtype=torch.bool)
    return adj


def build_graph(name):
    """the CSR of GRAPHS[name] in the engine's form (int64 tensors on the CPU): rows / col / epair / esign per entry, rowptr,
    pair_i > pair_j per pair, the molecule index of every atom"""
    if name in _graph_cache:
        return _graph_cache[name]
    rows, cols, batch = [], [], []
    base = 0
    for m, (n, rule) in enumerate(GRAPHS[name]):
        i, j = torch.nonzero(_adjacency(n, rule), as_tuple=True)  # sorted by (row, column)
        rows.append(i + base)
        cols.append(j + base)
        batch += [m] * n
        base += n
    rows, cols = torch.cat(rows), torch.cat(cols)
    N = base
    lower = rows > cols
    P = int(lower.sum())
    pid = torch.full((N * N,), -1, dtype=torch.int64)
    pid[(rows * N + cols)[lower]] = torch.arange(P)  # pair (i, j), i > j, numbered in the order of (i, j)
    epair = torch.where(rows == cols, torch.tensor(P), pid[torch.maximum(rows, cols) * N + torch.minimum(rows, cols)])
    assert int(epair.min()) >= 0
    esign = torch.where(rows == cols, 0.0, torch.where(cols < rows, 1.0, -1.0)).float()
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.bincount(rows, minlength=N).cumsum(0)
    g = dict(N=N, P=P, E=int(rows.numel()), rowptr=rowptr, rows=rows, col=cols, epair=epair, esign=esign, batch=torch.tensor(batch),
             B=len(GRAPHS[name]), pair_i=rows[lower], pair_j=cols[lower])
    _graph_cache[name] = g
    return g


# ====================================================================================== the tile prep and the launchers, restated
def max_tiles_of(N, B):
    return max(1, min(B, 2 * ((N + G16_ROWS - 1) // G16_ROWS) + 1))


def tile_prep_statement(g, min_fill):
    """(open, tiles, tile_start) as k_et_tile_pack and k_et_tile_open decide them: tiles are runs of whole molecules packed greedily
    into at most 64 rows; open when a molecule has more than 64 atoms, when a row has a neighbour outside its tile, or when there
    are fewer than min_fill x tiles x 4096 entries - compared in float32, as the kernel does."""
    N, batch = g["N"], g["batch"].numpy()
    starts = np.zeros(N + 1, dtype=bool)
    starts[0] = starts[N] = True
    starts[1:N] = batch[1:] != batch[:-1]
    ts, s0, is_open = [], 0, False
    while s0 < N:
        cand = [r for r in range(s0 + 1, min(s0 + G16_ROWS, N) + 1) if starts[r]]
        if cand:
            nxt = cand[-1]
        else:
            nxt, is_open = min(s0 + G16_ROWS, N), True
        ts.append(s0)
        s0 = nxt
    ts.append(N)
    n = len(ts) - 1
    if n > max_tiles_of(N, g["B"]):
        is_open = True
    if np.float32(g["E"]) < np.float32(min_fill) * np.float32(n) * np.float32(G16_ROWS * G16_ROWS):
        is_open = True
    if not is_open:
        rp, col = g["rowptr"].numpy(), g["col"].numpy()
        for t in range(n):
            for r in range(ts[t], ts[t + 1]):
                if rp[r + 1] > rp[r] and (col[rp[r]] < ts[t] or col[rp[r + 1] - 1] >= ts[t + 1]):
                    is_open = True
    return int(is_open), n, ts


def g16_shape_ok(N, P1, F, hd, Wd):
    lim = 1 << 31
    return (F % 32 == 0 and F <= 1024 and hd in (2, 4, 8, 16, 32) and N * 5 * F * 4 < lim and P1 * Wd * 4 < lim and (2 * P1 + N) * 32 < lim
            and P1 - 1 < (1 << PAIR_ID_BITS))


def pipelined_ok(F, hd):
    return F % 64 == 0 and F <= 1024 and hd <= 16


def sweep_waves(F):
    return F // 32 if F % 32 == 0 else (F + 63) // 64


def auto_route(g, F, hd, Wd, bf16):
    """the generation launch_et_attn_fwd / launch_et_attn_bwd end up running, and the meta they leave"""
    is_open, n, _ = tile_prep_statement(g, MIN_FILL_BF16 if bf16 else MIN_FILL_F32)
    if g16_shape_ok(g["N"], g["P"] + 1, F, hd, Wd) and not is_open:
        return TILE, (is_open, n)
    return (ROW_PIPELINED if pipelined_ok(F, hd) else ROW_GENERIC), (is_open, n)


def tile_census(g):
    """what each tile of the packing does in the tile kernels, by the rules in the kernels: a dict per tile"""
    is_open, n, ts = tile_prep_statement(g, 0.0)
    rp, col, batch = g["rowptr"].tolist(), g["col"].tolist(), g["batch"].tolist()
    out = []
    for t in range(n):
        r0, r1 = ts[t], ts[t + 1]
        lens = [rp[r + 1] - rp[r] for r in range(r0, r1)]
        longest = max(lens)
        slot = longest >= SLOT_MIN
        mols = [batch[r0:r1].count(m) for m in sorted(set(batch[r0:r1]))]
        out.append(dict(open=bool(is_open), rows=r1 - r0, longest=longest, slot=slot, partial=r1 - r0 < G16_ROWS, mols=mols,
                        gap_rows=sum(1 for k, r in enumerate(range(r0, r1)) if 1 < lens[k] and col[rp[r + 1] - 1] - col[rp[r]] + 1 > lens[k]),
                        self_only_rows=sum(1 for L in lens if L == 1), short_rows=sum(1 for L in lens if L < longest),
                        list_steps=None if slot else longest, edges=rp[r1] - rp[r0]))
    return out


# the tile classes the case list as a whole must contain (tests/test_et_unit_oracle.py); t = a tile of tile_census
TILE_CLASSES = {
    "slot_order_full_tile": lambda t: t["slot"] and t["rows"] == 64 and t["longest"] == 64 and t["short_rows"] == 0,
    "slot_order_longest_row_exactly_at_threshold": lambda t: t["slot"] and t["longest"] == SLOT_MIN,
    "list_order_longest_row_one_below_threshold": lambda t: not t["slot"] and t["longest"] == SLOT_MIN - 1,
    "slot_order_rows_with_gaps": lambda t: t["slot"] and t["gap_rows"] > 0,
    "slot_order_row_with_only_its_self_edge": lambda t: t["slot"] and t["self_only_rows"] > 0,
    "list_order_rows_with_gaps": lambda t: not t["slot"] and t["gap_rows"] > 0,
    "list_order_odd_step_count": lambda t: not t["slot"] and t["list_steps"] % 2 == 1,
    "list_order_even_step_count": lambda t: not t["slot"] and t["list_steps"] % 2 == 0,
    "list_order_partial_last_tile": lambda t: not t["slot"] and t["partial"],
    "list_order_fill_far_below_threshold": lambda t: not t["slot"] and t["edges"] < 0.05 * 4096,
    "several_molecules_in_a_tile": lambda t: len(t["mols"]) >= 5,
    "tile_of_63_plus_1": lambda t: t["mols"] == [63, 1],
    "open_tiles": lambda t: t["open"],
}


def census_of_case_list():
    """class -> [(graph, tile index)] over the graphs of the TILE cases; also which (graph, row type) pairs are mailbox eligible"""
    found = {k: [] for k in TILE_CLASSES}
    graphs = sorted({c.graph for c in all_cases() if c.kernel == TILE})
    for gname in graphs:
        for n, t in enumerate(tile_census(build_graph(gname))):
            for k, pred in TILE_CLASSES.items():
                if pred(t):
                    found[k].append((gname, n))
    return found


def mailbox_runs(c):
    """does a tile of this TILE case take the exchange: slot order, fp32 rows, both projections, not switched off (the reverse
    sweep with any projections, and tkv not below dkv)"""
    slot = c.variant == "slotall" or (c.variant != "listall" and any(t["slot"] for t in tile_census(build_graph(c.graph))))
    fwd = slot and not c.bf16 and c.combo[0] and c.combo[1] and c.variant != "nomb"
    bwd = slot and not c.bf16 and c.variant not in ("nomb", "tkvlow")
    return fwd, bwd


# ====================================================================================== inputs
def layout_of(F, hd, combo):
    k, v, vc = combo
    return dict(F=F, hd=hd, dk_off=0 if k else -1, dv_off=(F if k else 0) if v else -1, vc=vc, Wd=(F if k else 0) + (3 * F if v else 0))


def make_inputs(gname, F, hd, combo, bf16=0, extreme=False):
    """fp32 operands on the CPU.  q and k scaled and signed so that the attention pre-activations stay within a few units, of both
    signs; dkv in (0.2, 1.2), its
    tangent ~ N(0, 1); C, dC in (0, 1); prhat random unit vectors.  bf16: the pair rows are rounded to bf16 first, so the reference
    receives the very values the kernel widens.  extreme: q, k and the key filter are chosen so that a = EXTREMES[(atom + head) % 7]
    exactly."""
    g = build_graph(gname)
    N, P = g["N"], g["P"]
    lay = layout_of(F, hd, combo)
    Wd = lay["Wd"]
    gen = torch.Generator().manual_seed(1000003 * sorted(GRAPHS).index(gname) + 1009 * F + 31 * hd + COMBOS8.index(tuple(combo)) + 7 * bf16)
    rn = lambda *s: torch.randn(*s, generator=gen)
    ru = lambda *s: torch.rand(*s, generator=gen)
    qkv = rn(N, 5 * F)
    # q > 0 and k of one sign per (atom, head): the products of a head do not cancel, so a pre-activation near zero is not a badly
    # conditioned sum (its rounding would otherwise dominate the one-term distance slots of a model without projections)
    # (scale: |a| a few tenths on average whatever the head width, so that a wide head - one or two per atom, all their channels
    # sharing the factor silu'(a) - does not sit on the root of silu' at -1.278, where that factor is a difference of equals)
    qkv[:, :F] = qkv[:, :F].abs() * min(0.3 / hd ** 0.5, 0.6 / hd)
    sign = lambda: torch.where(ru(N, F // hd) < 0.5, -1.0, 1.0).repeat_interleave(hd, dim=1)
    qkv[:, F:2 * F] = qkv[:, F:2 * F].abs() * sign()
    qkv[:, 2 * F:3 * F] = qkv[:, 2 * F:3 * F].abs() * sign()  # likewise vx against g_xagg: the other sum over a head's channels
    d = dict(qkv=qkv, vec=rn(N, 3, F) * 0.5, C=ru(P + 1) * 0.98 + 0.01, dC=ru(P + 1) * 0.98 + 0.01,
             prhat=torch.nn.functional.normalize(rn(max(P, 1), 3), dim=1), g_xagg=rn(N, F).abs() * sign(), g_vagg=rn(N, 3, F), g_vec_old=rn(N, 3, F))
    d["dkv"] = ru(P + 1, Wd) + 0.2 if Wd else None
    d["tkv"] = rn(P + 1, Wd) if Wd else None
    if extreme:
        assert combo[0] and hd & (hd - 1) == 0
        ext = torch.tensor(EXTREMES)
        head = torch.arange(F) // hd
        d["qkv"][:, :F] = ext[(torch.arange(N)[:, None] + head[None, :]) % len(EXTREMES)]
        d["qkv"][:, F:2 * F] = 1.0 / hd
        d["dkv"][:, :F] = 1.0
    if bf16 and Wd:
        d["dkv"], d["tkv"] = d["dkv"].bfloat16().float(), d["tkv"].bfloat16().float()
    return d, lay


def max_preactivation(gname, F, hd, combo, bf16=0):
    g = build_graph(gname)
    d, lay = make_inputs(gname, F, hd, combo, bf16)
    return float(O.edge_terms(g, {k: (v.double() if torch.is_tensor(v) else v) for k, v in d.items()}, lay)["a"].abs().max())


def attn_reference(g, d, lay, group):
    """name -> expected tensor, or (value, scale) for the slot arrays, in the dtype of d"""
    F = lay["F"]
    xagg, vagg = O.attn_forward(g, d, lay)
    adj = O.attn_adjoint(g, d, lay)
    gd2, gds, gr2, grs = O.slot_sums(g, adj, lay, group)
    ref = {"xagg": xagg, "vagg0": vagg[:, 0], "vagg1": vagg[:, 1], "vagg2": vagg[:, 2], "g_vec": d["g_vec_old"] + adj["g_vec"],
           "gd2": (gd2, gds), "gr2": (gr2, grs)}
    for n, k in enumerate(("g_q", "g_k", "g_vx", "g_v1", "g_v2")):
        ref[k] = adj["g_qkv"][:, n * F:(n + 1) * F]
    return ref


def errors(got, ref):
    return {k: (O.scaled_err(got[k], r[0], r[1]) if isinstance(r, tuple) else O.per_row_rel_err(got[k], r)) for k, r in ref.items() if k in got}


def slot_group(c):
    return 32 if c.kernel == TILE else 64


def floor_of(c):
    """rounding floor per output: the statements in float32 against themselves in float64 on the case's own inputs (CPU)"""
    g = build_graph(c.graph)
    d, lay = make_inputs(c.graph, c.F, c.hd, c.combo, c.bf16, c.variant == "extreme")
    lo = attn_reference(g, d, lay, slot_group(c))
    hi = attn_reference(g, {k: (v.double() if torch.is_tensor(v) else v) for k, v in d.items()}, lay, slot_group(c))
    return errors({k: (v[0] if isinstance(v, tuple) else v) for k, v in lo.items()}, hi)


FLOOR_UNIT = 1e-9  # profiles/et_unit_floor.json keeps floors and observed errors as integers in this unit


def load_bounds():
    """{"cases": {id: {output: dict(floor, bound, observed_gpu)}}} from the file's one line per case, "floor" and "observed_gpu"
    lists in the order of "outputs" (or of the case's own "names"); the bound is kernel_unit_cases.bound_of of the floor kept"""
    from tests.kernel_unit_cases import bound_of

    with open(FLOOR_JSON) as fh:
        doc = json.load(fh)
    cases = {}
    for cid, ent in doc["cases"].items():
        names = ent.get("names", doc["outputs"])
        obs = ent.get("observed_gpu") or [None] * len(names)
        cases[cid] = {k: dict(floor=f * FLOOR_UNIT, bound=bound_of(f * FLOOR_UNIT), observed_gpu=None if o is None else o * FLOOR_UNIT)
                      for k, f, o in zip(names, ent["floor"], obs)}
    return dict(doc, cases=cases)


def floor_kept(e):
    """a floor as the file keeps it: rounded UP to a whole unit (at least one)"""
    return max(1, int(-(-e // FLOOR_UNIT))) * FLOOR_UNIT


def save_bounds(doc, path):
    std = FWD_OUTPUTS + BWD_OUTPUTS
    lines = []
    for cid in sorted(doc["cases"]):
        ent = doc["cases"][cid]
        names = std if set(ent) == set(std) else list(ent)
        row = {} if names is std else {"names": names}
        row["floor"] = [round(ent[k]["floor"] / FLOOR_UNIT) for k in names]
        if any(ent[k]["observed_gpu"] is not None for k in names):
            row["observed_gpu"] = [None if ent[k]["observed_gpu"] is None else round(ent[k]["observed_gpu"] / FLOOR_UNIT) for k in names]
        lines.append(" %s: %s" % (json.dumps(cid), json.dumps(row, separators=(",", ":"))))
    head = {"rule": doc["rule"], "unit": FLOOR_UNIT, "outputs": std}
    with open(path, "w") as fh:
        fh.write("%s,\n\"cases\": {\n%s\n}}\n" % (json.dumps(head, indent=0)[:-2], ",\n".join(lines)))


# ====================================================================================== launches
_dev_cache = {}


def _ptr(t):
    return None if t is None else t.data_ptr()


def device_graph(gname, device="cuda"):
    key = ("graph", gname)
    if key not in _dev_cache:
        g = build_graph(gname)
        gd = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in g.items()}
        cnt = [g["P"], g["E"], 0, 0, 0, 0, 0, 0]
        pad1 = lambda t: torch.cat([t, torch.zeros(1, dtype=t.dtype)]).int().to(device)  # (never empty: a NULL pointer is rejected)
        csr = dict(rowptr=gd["rowptr"].int(), col=gd["col"].int(), epair=gd["epair"].int(), esign=gd["esign"].contiguous(),
                   counts=torch.tensor(cnt, dtype=torch.int32, device=device), pair_i=pad1(g["pair_i"]), pair_j=pad1(g["pair_j"]),
                   counts_overflow=torch.tensor(cnt[:2] + [1] + cnt[3:], dtype=torch.int32, device=device), batch=gd["batch"].long().contiguous())
        _dev_cache[key] = (gd, csr)
    return _dev_cache[key]


def device_case(c, device="cuda"):
    """the device copy of a case's graph and inputs and its float64 reference (evaluated on the device once, left unchanged)"""
    key = (c.graph, c.F, c.hd, c.combo, c.bf16, c.variant == "extreme")
    if key not in _dev_cache:
        for k in [k for k in _dev_cache if k[0] != "graph"]:
            if len(_dev_cache) > 8:
                del _dev_cache[k]
        gd, csr = device_graph(c.graph, device)
        d, lay = make_inputs(c.graph, c.F, c.hd, c.combo, c.bf16, c.variant == "extreme")
        dd = {k: (v.to(device).contiguous() if torch.is_tensor(v) else v) for k, v in d.items()}
        _dev_cache[key] = (gd, csr, dd, lay, {k: (v.double() if torch.is_tensor(v) else v) for k, v in dd.items()}, {})
    return _dev_cache[key]


def pair_rows_on_device(dd, bf16, tkv_low=False):
    """(dkv, tkv) as the kernel reads them: fp32 or bf16 (exact: the inputs are representable); tkv_low: one allocation with tkv in
    front of dkv, the case in which the reverse tile sweep must drop its mailbox by itself"""
    if dd["dkv"] is None:
        return None, None
    dt = torch.bfloat16 if bf16 else torch.float32
    if not tkv_low:
        return dd["dkv"].to(dt).contiguous(), dd["tkv"].to(dt).contiguous()
    n = dd["dkv"].numel()
    n_al = (n + 63) // 64 * 64
    buf = torch.empty(2 * n_al, dtype=dt, device=dd["dkv"].device)
    buf[:n] = dd["tkv"].to(dt).reshape(-1)
    buf[n_al:n_al + n] = dd["dkv"].to(dt).reshape(-1)
    return buf[n_al:n_al + n].view_as(dd["dkv"]), buf[:n].view_as(dd["tkv"])


def et_args(g, csr, lay, op, kernel, bf16=0, counts="counts"):
    from torchmdnet_amd import _C

    x = _C.EtUnitArgs()
    x.op, x.kernel = op, kernel
    x.N, x.B, x.P, x.E, x.F, x.hd, x.Wd = g["N"], g["B"], g["P"], g["E"], lay["F"], lay["hd"], lay["Wd"]
    x.dk_off, x.dv_off, x.vector_cutoff, x.pair_bf16 = lay["dk_off"], lay["dv_off"], lay["vc"], bf16
    x.skip_prep, x.slot_min, x.mailbox, x.sync_every, x.nw, x.min_fill = 0, -1, -1, -1, 0, -1.0
    for k in ("rowptr", "col", "epair", "esign", "pair_i", "pair_j", "batch"):
        setattr(x, k, _ptr(csr[k]))
    x.counts = _ptr(csr[counts])
    return x


SLOT_PAD = 6  # floats of every slot array behind the self pair's two


def prep_buffers(g, device):
    return dict(meta=torch.full((2,), -1, dtype=torch.int32, device=device), tile_start=torch.full((g["N"] + 8,), -1, dtype=torch.int32, device=device),
                erec=sentinel((g["E"] + TAIL, 8), device))


def fresh_outputs(g, dd, lay, device):
    """outputs with 64 sentinel rows behind row N; g_vec starts from the case's random old contents; one slot array more than the
    caller sums, each with the self pair's two slots and a pad behind the pairs'"""
    N, F = g["N"], lay["F"]
    nw, stride = sweep_waves(F), 2 * (g["P"] + 1) + SLOT_PAD
    out = dict(xagg=sentinel((N + TAIL, F), device), vagg=sentinel((N + TAIL, 3, F), device), g_qkv=sentinel((N + TAIL, 5 * F), device),
               g_vec=sentinel((N + TAIL, 3, F), device), gd2=sentinel((nw + 1, stride), device), gr2=sentinel((nw + 1, stride, 3), device))
    out["g_vec"][:N] = dd["g_vec_old"]
    return out


def launch(lib, x, dd, rows, out, prep, edit=None):
    """one call of tmdnet_debug_et with the operands of an attention case -> (rc, route); edit(x) runs just before the call"""
    x.C, x.dC, x.qkv, x.vec, x.prhat = (_ptr(dd[k]) for k in ("C", "dC", "qkv", "vec", "prhat"))
    x.dkv, x.tkv = _ptr(rows[0]), _ptr(rows[1])
    x.g_xagg, x.g_vagg = _ptr(dd["g_xagg"]), _ptr(dd["g_vagg"])
    x.meta, x.tile_start, x.erec = (_ptr(prep[k]) for k in ("meta", "tile_start", "erec"))
    for k in ("xagg", "vagg", "g_qkv", "g_vec", "gd2", "gr2"):
        setattr(x, k, _ptr(out[k]))
    x.slot_stride = out["gd2"].shape[1]
    if edit:
        edit(x)
    route = C.c_int32(-7)
    rc = lib.tmdnet_debug_et(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(x), C.byref(route))
    torch.cuda.synchronize()
    return rc, route.value


def split_outputs(out, N, F, count, P):
    got = {"xagg": out["xagg"][:N], "g_vec": out["g_vec"][:N], "gd2": out["gd2"][:count, :2 * P], "gr2": out["gr2"][:count, :2 * P]}
    for a in range(3):
        got["vagg%d" % a] = out["vagg"][:N, a]
    for n, k in enumerate(("g_q", "g_k", "g_vx", "g_v1", "g_v2")):
        got[k] = out["g_qkv"][:N, n * F:(n + 1) * F]
    return got


def run_case(lib, c, device="cuda"):
    """Launch both attention ops of a case (each twice, once with the overflow flag set, the tile kernel once with meta[0] = 1)
    -> dict(err={output: figure}, finite, route_ok, tail_ok, unowned_ok, zeroed_ok, deterministic, overflow_ok, flag_ok, max_a)."""
    gd, csr, dd, lay, d64, refs = device_case(c, device)
    group = slot_group(c)
    if group not in refs:
        refs[group] = attn_reference(gd, d64, lay, group)
    ref = refs[group]
    N, P, F = gd["N"], gd["P"], lay["F"]
    rows = pair_rows_on_device(dd, c.bf16, c.variant == "tkvlow")
    nw = sweep_waves(F)
    count = nw if c.kernel == TILE else (F + 63) // 64  # arrays the kernel fills with sums; the row kernels zero the others
    writes = not (c.kernel == TILE and tile_prep_statement(build_graph(c.graph), 0.0)[0])  # open tiles: the tile kernels return
    res = dict(err={}, finite=True, route_ok=True, tail_ok=True, unowned_ok=True, zeroed_ok=True, deterministic=True, overflow_ok=True, flag_ok=True)
    init = fresh_outputs(gd, dd, lay, device)

    def args(op, counts="counts"):
        x = et_args(gd, csr, lay, op, c.kernel, c.bf16, counts)
        if c.kernel == TILE:
            x.min_fill = 0.0  # the fill rule is a performance choice of the prep: TILE_PREP and AUTO test it
            x.mailbox = 0 if c.variant == "nomb" else -1
            x.slot_min = {"slotall": 1, "listall": 0}.get(c.variant, -1)
            x.sync_every = {"sync0": 0, "sync2": 2}.get(c.variant, -1)
        return x

    for op, names in ((OP_ATTN_FWD, FWD_OUTPUTS), (OP_ATTN_BWD, BWD_OUTPUTS)):
        runs = []
        for _ in range(2):
            out = fresh_outputs(gd, dd, lay, device)
            rc, route = launch(lib, args(op), dd, rows, out, prep_buffers(gd, device))
            assert rc == 0, f"tmdnet_debug_et returned {rc}"
            res["route_ok"] &= route == (c.kernel if writes else 0)
            runs.append(out)
        a, b = runs
        mine = ("xagg", "vagg") if op == OP_ATTN_FWD else ("g_qkv", "g_vec", "gd2", "gr2")
        res["deterministic"] &= all(bool(torch.equal(bits(a[k]), bits(b[k]))) for k in a)
        res["unowned_ok"] &= all(bool(torch.equal(bits(a[k]), bits(init[k]))) for k in a if k not in mine)  # the other op's outputs
        if not writes:
            res["unowned_ok"] &= all(bool(torch.equal(bits(a[k]), bits(init[k]))) for k in a)
            continue
        got = split_outputs(a, N, F, count, P)
        for k in names:
            r = ref[k]
            res["err"].update(errors({k: got[k]}, {k: r}))
            res["finite"] &= bool(torch.isfinite(got[k]).all())
        res["tail_ok"] &= all(bool((bits(a[k][N:]) == SENTINEL).all()) for k in mine if k in ("xagg", "vagg", "g_qkv", "g_vec"))
        if op == OP_ATTN_BWD:
            for k in ("gd2", "gr2"):
                # the self pair's slots and the pad of every array, and every array beyond the caller's count, bit-unchanged
                res["unowned_ok"] &= bool((bits(a[k][:, 2 * P:]) == SENTINEL).all()) and bool((bits(a[k][nw:]) == SENTINEL).all())
                res["zeroed_ok"] &= bool((bits(a[k][count:nw, :2 * P]) == 0).all())  # (+0.0 exactly)
        # pair overflow (counts[2] != 0): the adjacency is not to be trusted, every kernel returns without a write
        out = fresh_outputs(gd, dd, lay, device)
        rc, _ = launch(lib, args(op, "counts_overflow"), dd, rows, out, prep_buffers(gd, device))
        assert rc == 0
        res["overflow_ok"] &= all(bool(torch.equal(bits(out[k]), bits(init[k]))) for k in out)
        if c.kernel == TILE:  # the flag of the prep set by hand: the tile kernels leave the step to the row sweeps
            prep = prep_buffers(gd, device)
            x = args(OP_TILE_PREP)
            rc, _ = launch(lib, x, dd, rows, out, prep)
            assert rc == 0 and prep["meta"].tolist() == [0, tile_prep_statement(build_graph(c.graph), 0.0)[1]]
            prep["meta"][0] = 1
            x = args(op)
            x.skip_prep = 1
            rc, route = launch(lib, x, dd, rows, out, prep)
            assert rc == 0
            res["flag_ok"] &= route == 0 and all(bool(torch.equal(bits(out[k]), bits(init[k]))) for k in out)
    return res


# ====================================================================================== the other ops
OTHER_GRAPHS = ("ladder", "packed")
OTHER_F = (40, 64)
MAX_Z = 12


def other_inputs(gname, F):
    """fp32 operands of the neighbour-embedding ops, the pair combine and g_pre on the CPU (seeded)"""
    g = build_graph(gname)
    N, P = g["N"], g["P"]
    gen = torch.Generator().manual_seed(77003 * sorted(GRAPHS).index(gname) + F)
    rn = lambda *s: torch.randn(*s, generator=gen)
    nw = sweep_waves(F)
    stride = 2 * (P + 1) + SLOT_PAD
    Wd = 4 * F
    return dict(z=torch.randint(0, MAX_Z, (N,), generator=gen), emb=rn(MAX_Z, F), embN=rn(MAX_Z, F), Wn=rn(P + 1, F) * 0.3, dWn=rn(P + 1, F),
                g_xcat=rn(N, 2 * F), gd2_old=rn(stride), gd2=rn(nw, stride), gr2=rn(nw, stride, 3), gd_extra=rn(2 * (P + 1)),
                slots=rn(2, P + 1, Wd), self_sum=rn(Wd), pre=rn(P + 1, Wd) * 2)


def other_reference(g, d, F):
    """op name -> {output: tensor or (value, scale)} in the dtype of d"""
    P = g["P"]
    en = d["embN"][d["z"]]
    g_nbr = d["g_xcat"][:, F:]
    v, s = O.nbr_embed_bwd(g, en, g_nbr, d["dWn"])
    slots, gEN = O.train_nbr(g, en, d["Wn"], g_nbr)
    gd, gds, grh, grs = O.pair_combine(d["gd2"], d["gr2"], d["gd_extra"], P)
    return {
        "nbr_embed": {"xcat": O.nbr_embed(g, d["z"], d["emb"], en, d["Wn"])},
        "nbr_embed_bwd": {"gd2": (d["gd2_old"][0:2 * P:2] + v, d["gd2_old"][0:2 * P:2].abs() + s)},
        "train_nbr": {"slots0": slots[0], "slots1": slots[1], "gEN": gEN},
        "pair_combine": {"gd": (gd, gds), "g_rhat": (grh, grs)},
        "train_gpre": {"g_pre": O.train_gpre(d["slots"][:, :P], d["self_sum"], d["pre"])},
    }


def other_floor(gname, F):
    g, d = build_graph(gname), other_inputs(gname, F)
    lo = other_reference(g, d, F)
    hi = other_reference(g, {k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}, F)
    return {op: errors({k: (v[0] if isinstance(v, tuple) else v) for k, v in lo[op].items()}, hi[op]) for op in hi}


def other_id(gname, F):
    return "other-%s-F%d" % (gname, F)


def run_other(lib, gname, F, device="cuda"):
    """every other op on (graph, F), each launched twice and once with the overflow flag
    -> dict(err={op: {output: figure}}, tail_ok, unowned_ok, deterministic, overflow_ok)"""
    gd, csr = device_graph(gname, device)
    N, P = gd["N"], gd["P"]
    d = {k: v.to(device).contiguous() for k, v in other_inputs(gname, F).items()}
    ref = other_reference(gd, {k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}, F)
    Wd = d["pre"].shape[1]
    lay = dict(F=F, hd=8, dk_off=0, dv_off=F, vc=0, Wd=Wd)
    res = dict(err={}, tail_ok=True, unowned_ok=True, deterministic=True, overflow_ok=True)

    def call(op, out, counts="counts"):
        x = et_args(gd, csr, lay, op, 0, 0, counts)
        for k in ("z", "emb", "embN", "Wn", "dWn", "g_xcat", "gd_extra", "self_sum", "pre"):
            setattr(x, k, _ptr(d[k]))
        x.nw, x.slot_stride = d["gd2"].shape[0], d["gd2"].shape[1]
        x.gd2, x.gr2 = _ptr(d["gd2"]), _ptr(d["gr2"])
        x.dir_stride = (P + 1) * (F if op == OP_TRAIN_NBR else Wd)
        x.slots = _ptr(d["slots"])
        for k, v in out.items():
            setattr(x, k, _ptr(v))
        rc = lib.tmdnet_debug_et(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(x), None)
        torch.cuda.synchronize()
        assert rc == 0, (op, rc)

    def fresh(op):
        if op == OP_NBR_EMBED:
            return dict(xcat=sentinel((N + TAIL, 2 * F), device))
        if op == OP_NBR_EMBED_BWD:
            o = sentinel((2 * (P + 1) + SLOT_PAD,), device)
            o[:2 * P:2] = d["gd2_old"][:2 * P:2]
            return dict(gd2=o)
        if op == OP_TRAIN_NBR:
            return dict(slots=sentinel((2, P + 1, F), device), gEN=sentinel((N + TAIL, F), device))
        if op == OP_PAIR_COMBINE:
            return dict(gd=sentinel((P + TAIL,), device), g_rhat=sentinel((P + TAIL, 3), device))
        return dict(g_pre=sentinel((P + 1 + TAIL, Wd), device))

    def view(op, o):
        if op == OP_NBR_EMBED:
            return {"xcat": o["xcat"][:N]}, [o["xcat"][N:]]
        if op == OP_NBR_EMBED_BWD:
            return {"gd2": o["gd2"][0:2 * P:2]}, [o["gd2"][1:2 * P:2], o["gd2"][2 * P:]]
        if op == OP_TRAIN_NBR:
            return {"slots0": o["slots"][0, :P], "slots1": o["slots"][1, :P], "gEN": o["gEN"][:N]}, [o["slots"][:, P:], o["gEN"][N:]]
        if op == OP_PAIR_COMBINE:
            return {"gd": o["gd"][:P], "g_rhat": o["g_rhat"][:P]}, [o["gd"][P:], o["g_rhat"][P:]]
        return {"g_pre": o["g_pre"][:P + 1]}, [o["g_pre"][P + 1:]]

    for op, name in ((OP_NBR_EMBED, "nbr_embed"), (OP_NBR_EMBED_BWD, "nbr_embed_bwd"), (OP_TRAIN_NBR, "train_nbr"),
                     (OP_PAIR_COMBINE, "pair_combine"), (OP_TRAIN_GPRE, "train_gpre")):
        a, b, init = fresh(op), fresh(op), fresh(op)
        call(op, a)
        call(op, b)
        got, untouched = view(op, a)
        res["err"][name] = errors(got, ref[name])
        res["tail_ok"] &= all(bool((bits(t) == SENTINEL).all()) for t in untouched)
        res["deterministic"] &= all(bool(torch.equal(bits(a[k]), bits(b[k]))) for k in a)
        if op != OP_TRAIN_GPRE:  # (k_et_train_gpre reads the pair count alone)
            o = fresh(op)
            call(op, o, "counts_overflow")
            res["overflow_ok"] &= all(bool(torch.equal(bits(o[k]), bits(init[k]))) for k in o)
    return res


FILTER_CASES = [(gname, F, hd, cb) for gname in OTHER_GRAPHS for (F, hd, cb) in ((40, 8, (1, 1, 0)), (64, 16, (1, 0, 1)), (64, 16, (0, 1, 0)), (96, 32, (1, 1, 1)))]


def filter_id(fc):
    return "filter-%s-F%d-hd%d-k%dv%dc%d" % (fc[0], fc[1], fc[2], *fc[3])


def filter_reference(g, d, lay):
    slots, self_rows = O.train_filter(g, d, lay)
    return {"slots0": slots[0], "slots1": slots[1], "self_rows": self_rows}


def filter_floor(fc):
    g = build_graph(fc[0])
    d, lay = make_inputs(*fc)
    lo = filter_reference(g, d, lay)
    hi = filter_reference(g, {k: (v.double() if torch.is_tensor(v) else v) for k, v in d.items()}, lay)
    return {k: O.per_row_rel_err(lo[k], hi[k]) for k in hi}


def run_filter(lib, fc, device="cuda"):
    """TRAIN_FILTER on the inputs of the attention case (fp32 rows) -> dict(err, unowned_ok, deterministic, overflow_ok)"""
    c = Case(ROW_GENERIC, fc[0], fc[1], fc[2], fc[3], 0, "")
    gd, csr, dd, lay, d64, refs = device_case(c, device)
    if "filter" not in refs:
        refs["filter"] = filter_reference(gd, d64, lay)
    ref = refs["filter"]
    N, P, Wd = gd["N"], gd["P"], lay["Wd"]
    rows = pair_rows_on_device(dd, 0)

    def call(counts="counts"):
        out = dict(slots=sentinel((2, P + 1, Wd), device), self_rows=sentinel((N + TAIL, Wd), device))
        x = et_args(gd, csr, lay, OP_TRAIN_FILTER, 0, 0, counts)
        x.dir_stride = (P + 1) * Wd
        x.slots, x.self_rows = _ptr(out["slots"]), _ptr(out["self_rows"])
        rc, _ = launch(lib, x, dd, rows, fresh_outputs(gd, dd, lay, device), prep_buffers(gd, device))
        assert rc == 0, rc
        return out

    a, b, o = call(), call(), call("counts_overflow")
    got = {"slots0": a["slots"][0, :P], "slots1": a["slots"][1, :P], "self_rows": a["self_rows"][:N]}
    return dict(err={k: O.per_row_rel_err(got[k], ref[k]) for k in ref},
                unowned_ok=bool((bits(a["slots"][:, P:]) == SENTINEL).all()) and bool((bits(a["self_rows"][N:]) == SENTINEL).all()),
                deterministic=all(bool(torch.equal(bits(a[k]), bits(b[k]))) for k in a),
                overflow_ok=all(bool((bits(v) == SENTINEL).all()) for v in o.values()))
