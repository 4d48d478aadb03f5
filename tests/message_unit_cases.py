"""TEST INFRASTRUCTURE ONLY -- the cases of the kernel-level unit tests of TensorNet's neighbour sweeps (tmdnet_debug_message):
hand-built graphs, seeded inputs, launches and the figures the tests assert on.  One statement serves three users:
tests/test_gpu_message.py (asserts), tools/message_unit_floor.py (the fp32 rounding floor of the reference on these very inputs
without a device, and the errors observed on the device, into profiles/message_unit_floor.json, from which the test reads its
bounds) and tests/test_message_oracle.py (the branch census of the tile kernels over the case list, no device).
"""
import ctypes as C
import json
import os

import torch

from tests import message_oracle as O
from tests.kernel_unit_cases import SENTINEL, TAIL, bits, sentinel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR_JSON = os.path.join(ROOT, "profiles", "message_unit_floor.json")
# restated from csrc/tn_message_pair.hip and csrc/tn_kernels.hip (tests/test_message_oracle.py parses the sources and compares)
MP_TA, MP_W, MP_E, MP_FC, MP_U, LPR, KEG = 64, 64, 4096, 32, 2, 8, 8

MIXED = [3, 1, 100, 2, 7, 64, 1, 1, 30]
# graph name -> [(atoms, rule)] per molecule; rule: "complete", ("band", b): |a - b| <= b, ("hubs", h): a < h or b < h
GRAPHS = {
    "one_atom": [(1, "complete")],
    "chain63": [(63, ("band", 5))],
    "chain64": [(64, ("band", 5))],
    "chain65": [(65, ("band", 5))],
    "complete64": [(64, "complete")],
    "complete65": [(65, "complete")],
    "complete100": [(100, "complete")],
    "chain130": [(130, ("band", 20))],
    "star64": [(64, ("hubs", 8))],
    "tiny90": [((1, 2, 3, 2)[k % 4], "complete") for k in range(90)],  # every 64-row tile starts a molecule
    "mixed": [(n, "complete") for n in MIXED],
    "ladder": [(n, "complete") for n in range(1, 27)],
}
TILE_GRAPHS = {  # graph -> F values of the tile kernels
    "one_atom": (32, 96), "chain63": (32, 128), "chain64": (32, 128), "chain65": (32, 128), "complete64": (32, 256),
    "complete65": (96, 128), "complete100": (32, 256), "chain130": (32, 96), "star64": (32, 128), "tiny90": (96, 256),
    "mixed": (32, 96, 256),
}
ROW_GRAPHS = ("ladder", "mixed")
ROW_F = {"fwd_row": (24, 96, 256), "adj_row": (24, 96, 256), "dual": (24, 96, 256), "dual_acc": (24, 96, 256),
         "fwd_split": (64, 128), "adj_split": (64, 128), "gd_split": (64, 128), "gd_row": (64, 192)}
# kernel name -> (op, selector) of tmdnet_debug_message, slot group width (0: no slots)
KERNELS = {
    "fwd_row": (0, 1, 0), "fwd_split": (0, 2, 0), "fwd_tile": (0, 3, 0), "adj_row": (1, 4, 0), "adj_split": (1, 5, 0),
    "gd_row": (2, 6, 64), "gd_split": (2, 7, 64), "gd_tile": (2, 8, 32), "dual": (3, 9, 0), "dual_acc": (3, 10, 0),
}
FWD_MODES = ("o3_mol", "o3_atom", "so3")  # O(3) with per-molecule q, O(3) with per-atom kap, SO(3)


def all_cases():
    """[(kernel, graph, F)]"""
    out = [(k, gname, F) for gname, Fs in TILE_GRAPHS.items() for F in Fs for k in ("fwd_tile", "gd_tile")]
    # grouped by (graph, F): the device copy and the fp64 references of a (graph, F) are built once (_device_case)
    for gname in ROW_GRAPHS:
        for F in sorted({F for Fs in ROW_F.values() for F in Fs}):
            out += [(k, gname, F) for k, Fs in ROW_F.items() if F in Fs]
    return out


def case_id(case):
    return "%s-%s-F%d" % case


def outputs_of(kernel):
    if kernel.startswith("fwd"):
        return ["Mi"] + ["Ch_" + m for m in FWD_MODES]
    if kernel.startswith("adj"):
        return ["gPn"]
    if kernel.startswith("gd"):
        return ["gPn", "slots"]
    return ["out", "out_t"]


# ====================================================================================== graphs
_graph_cache = {}


def build_graph(name):
    """the CSR of GRAPHS[name] in the engine's form (int64 tensors on the CPU), plus the molecule index of every atom"""
    if name in _graph_cache:
        return _graph_cache[name]
    rows, cols, batch = [], [], []
    base = 0
    for m, (n, rule) in enumerate(GRAPHS[name]):
        a = torch.arange(n)
        if rule == "complete":
            adj = torch.ones(n, n, dtype=torch.bool)
        elif rule[0] == "band":
            adj = (a[:, None] - a[None, :]).abs() <= rule[1]
        else:
            assert rule[0] == "hubs"
            adj = (a[:, None] < rule[1]) | (a[None, :] < rule[1]) | (a[:, None] == a[None, :])
        i, j = torch.nonzero(adj, as_tuple=True)  # sorted by (row, column)
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
    g = dict(N=N, P=P, rowptr=rowptr, rows=rows, col=cols, epair=epair, esign=esign, batch=torch.tensor(batch), B=len(GRAPHS[name]))
    _graph_cache[name] = g
    return g


def tile_census(rowptr, col, N):
    """what each 64-row tile of k_message_rows8 / k_message_adjoint_rows8 does, by the rules in the kernels: a dict per tile"""
    rowptr, col = torch.as_tensor(rowptr).tolist(), torch.as_tensor(col).tolist()
    out = []
    for r0 in range(0, N, MP_TA):
        r1 = min(N, r0 + MP_TA)
        lens = [rowptr[r0 + t + 1] - rowptr[r0 + t] if r0 + t < r1 else 0 for t in range(MP_TA)]
        nE = rowptr[r1] - rowptr[r0]
        live = [t for t in range(r1 - r0) if lens[t] > 0]
        lo = min(col[rowptr[r0 + t]] for t in live) if live else 1
        hi = max(col[rowptr[r0 + t + 1] - 1] for t in live) if live else 0
        wn = hi - lo + 1
        order = sorted(range(MP_TA), key=lambda t: (-lens[t], t))  # rank 0 = longest, ties by row
        helpers, dead_helpers = 0, 0
        if nE <= MP_E:
            for rank in range(MP_TA // 2, MP_TA):
                t, partner = order[rank], order[MP_TA - 1 - rank]
                if ((lens[partner] - lens[t]) // 2) & ~(MP_U - 1) > 0:
                    helpers += 1
                    dead_helpers += 1 if r0 + t >= r1 else 0
        mols = len({(col[rowptr[r0 + t]], col[rowptr[r0 + t + 1] - 1]) for t in live})
        out.append(dict(nE=nE, wn=wn, staged=bool(live) and wn <= MP_W, csr_lds=nE <= MP_E, helpers=helpers, dead=MP_TA - (r1 - r0),
                        dead_helpers=dead_helpers, live=r1 - r0, max_len=max(lens), min_live_len=min(lens[t] for t in live),
                        windows=mols))
    return out


# the tile classes the case list as a whole must contain (tests/test_message_oracle.py)
TILE_CLASSES = {
    "one_live_row": lambda t: t["live"] == 1,
    "staged_lds_slice": lambda t: t["staged"] and t["csr_lds"],
    "partial_tile_dead_rows_help": lambda t: t["dead"] > 0 and t["dead_helpers"] > 0,
    "both_limits_met_exactly": lambda t: t["wn"] == MP_W and t["nE"] == MP_E and t["staged"] and t["csr_lds"],
    "window_one_past_the_limit": lambda t: t["wn"] == MP_W + 1 and not t["staged"],
    "unstaged_global_slice": lambda t: not t["staged"] and not t["csr_lds"],
    "unstaged_lds_slice": lambda t: not t["staged"] and t["csr_lds"],
    "global_slice_rows_longer_than_8_lpr": lambda t: not t["csr_lds"] and t["max_len"] > 8 * LPR,
    "full_tile_long_rows_hand_tails": lambda t: t["dead"] == 0 and t["helpers"] == 8 and t["max_len"] == 64,
    "equal_rows_no_helper": lambda t: t["dead"] == 0 and t["csr_lds"] and t["helpers"] == 0 and t["max_len"] == t["min_live_len"],
    "window_of_dozens_of_molecules": lambda t: t["staged"] and t["windows"] >= 24,
}


def census_of_case_list():
    """class -> [(graph, tile index)] over the tile-kernel graphs; and the block counts (tiles x chunks) of every tile case"""
    found = {k: [] for k in TILE_CLASSES}
    blocks = {}
    for gname, Fs in TILE_GRAPHS.items():
        g = build_graph(gname)
        tiles = tile_census(g["rowptr"], g["col"], g["N"])
        for k, pred in TILE_CLASSES.items():
            found[k] += [(gname, n) for n, t in enumerate(tiles) if pred(t)]
        for F in Fs:
            blocks[(gname, F)] = len(tiles) * (F // MP_FC)
    return found, blocks


# ====================================================================================== inputs
def make_inputs(gname, F):
    """fp32 operands on the CPU: w, dw, w_t ~ N(0, 1 / mean row length) with P + 1 rows, src, Pn, src_t ~ N(0, 0.25),
    gMi ~ N(0, 1), a charge per molecule, a kappa per atom, and the old contents of the accumulating outputs."""
    g = build_graph(gname)
    N, P = g["N"], g["P"]
    gen = torch.Generator().manual_seed(1000003 * sorted(GRAPHS).index(gname) + F)
    rn = lambda *s: torch.randn(*s, generator=gen)
    sw = (N / g["col"].numel()) ** 0.5
    d = dict(w=rn(P + 1, 3, F) * sw, dw=rn(P + 1, 3, F) * sw, w_t=rn(P + 1, 3, F) * sw, src=rn(N, 9, F) * 0.5, Pn=rn(N, 9, F) * 0.5,
             src_t=rn(N, 9, F) * 0.5, gMi=rn(N, 9, F), q_mol=rn(g["B"]), kap_atom=1 + 0.3 * rn(N), old=rn(N, 9, F), old_t=rn(N, 9, F))
    return d


def reference(kernel, g, d):
    """output name -> expected tensor in the dtype of d (graph index tensors on d's device); slots -> (value, scale)"""
    if kernel.startswith("fwd"):
        Mi = O.gather(g, d["w"], d["src"])
        ref = {"Mi": Mi}
        for mode in FWD_MODES:
            q, batch, o3 = fwd_mode_args(mode, g, d)
            ref["Ch_" + mode] = O.group_product(d["src"], Mi, O.kappa(q, batch, g["N"], Mi), o3)
        return ref
    if kernel.startswith("adj"):
        return {"gPn": d["old"] + O.adjoint(g, d["w"], d["gMi"])}
    if kernel.startswith("gd"):
        return {"gPn": d["old"] + O.adjoint(g, d["w"], d["gMi"]), "slots": O.pair_halves(g, d["dw"], d["gMi"], d["Pn"], KERNELS[kernel][2])}
    v, t = O.dual(g, d["w"], d["w_t"], d["src"], d["src_t"])
    return {"out": d["old"] + v, "out_t": d["old_t"] + t} if kernel == "dual_acc" else {"out": v, "out_t": t}


def fwd_mode_args(mode, g, d):
    if mode == "o3_mol":
        return d["q_mol"], g["batch"], 1
    if mode == "o3_atom":
        return d["kap_atom"], None, 1
    return d["q_mol"], g["batch"], 0  # SO(3): kappa is not used


def worse(prev, e):
    """the larger of two error figures; a NaN (an output left at the sentinel, or a NaN the kernel made) wins over any number"""
    if prev is None or prev != prev:
        return e if prev is None else prev
    return e if not (e <= prev) else prev


def _errors(kernel, got, ref):
    out = {}
    for k, r in ref.items():
        out[k] = O.slot_rel_err(got[k][0], r[0], r[1]) if k == "slots" else O.per_atom_rel_err(got[k], r)
    return out


def floor_of(case):
    """rounding floor per output: the statements in float32 against themselves in float64 on the case's own inputs (CPU)"""
    kernel, gname, F = case
    g, d = build_graph(gname), make_inputs(gname, F)
    lo = reference(kernel, g, d)
    hi = reference(kernel, g, {k: v.double() for k, v in d.items()})
    return _errors(kernel, lo, hi)


def load_bounds():
    with open(FLOOR_JSON) as fh:
        return json.load(fh)


# ====================================================================================== launches
_dev_cache = {}


def _device_case(gname, F, device):
    key = (gname, F)
    if key not in _dev_cache:
        _dev_cache.clear()  # one (graph, F) at a time: the cases arrive grouped
        g = build_graph(gname)
        gd = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in g.items()}
        d = {k: v.to(device).contiguous() for k, v in make_inputs(gname, F).items()}
        csr = dict(rowptr=gd["rowptr"].int(), col=gd["col"].int(), epair=gd["epair"].int(), esign=gd["esign"].contiguous(),
                   counts=torch.tensor([g["P"], g["col"].numel(), 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=device),
                   counts_overflow=torch.tensor([g["P"], g["col"].numel(), 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=device))
        _dev_cache[key] = (gd, d, csr, {k: v.double() for k, v in d.items()}, {})
    return _dev_cache[key]


def _ptr(t):
    return None if t is None else t.data_ptr()


def message_args(kernel, g, csr, F, small_mols=1):
    from torchmdnet_amd import _C

    x = _C.MessageArgs()
    x.op, x.kernel = KERNELS[kernel][0], KERNELS[kernel][1]
    x.N, x.F, x.P, x.small_mols, x.o3, x.balance, x.accumulate = g["N"], F, g["P"], small_mols, 1, -1, int(kernel == "dual_acc")
    x.rowptr, x.col, x.epair, x.esign, x.counts = (_ptr(csr[k]) for k in ("rowptr", "col", "epair", "esign", "counts"))
    return x


SLOT_PAD = 6  # floats of every slot array behind the self pair's two


def fresh_outputs(kernel, g, d, F, device):
    """outputs with 64 sentinel rows behind row N; accumulating outputs start from the case's random old contents; the slot
    arrays (one more than the tile kernel's count) are all sentinel"""
    N = g["N"]
    out = {"out": sentinel((N + TAIL, 9, F), device), "out2": sentinel((N + TAIL, 9, F), device)}
    if kernel.startswith(("adj", "gd")) or kernel == "dual_acc":
        out["out"][:N] = d["old"]
    if kernel == "dual_acc":
        out["out2"][:N] = d["old_t"]
    if kernel.startswith("gd"):
        out["slots"] = sentinel((F // 32 + 1, 2 * g["P"] + 2 + SLOT_PAD), device)
    return out


def launch(lib, kernel, x, d, out, mode=None, g=None, balance=-1):
    """one call of tmdnet_debug_message -> (rc, route, slot arrays)"""
    x.out, x.out2 = _ptr(out["out"]), _ptr(out["out2"])
    x.w, x.q, x.batch, x.balance = _ptr(d["w"]), None, None, balance
    if kernel.startswith("fwd"):
        q, batch, o3 = fwd_mode_args(mode, g, d)
        x.src, x.q, x.batch, x.o3 = _ptr(d["src"]), _ptr(q), _ptr(batch), o3
    elif kernel.startswith("adj"):
        x.src = _ptr(d["gMi"])
    elif kernel.startswith("gd"):
        x.src, x.src2, x.w2 = _ptr(d["gMi"]), _ptr(d["Pn"]), _ptr(d["dw"])
        x.slots, x.slot_stride = _ptr(out["slots"]), out["slots"].shape[1]
    else:
        x.src, x.src2, x.w2 = _ptr(d["src"]), _ptr(d["src_t"]), _ptr(d["w_t"])
    route, ns = C.c_int32(-1), C.c_int32(-1)
    rc = lib.tmdnet_debug_message(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(x), C.byref(route), C.byref(ns))
    torch.cuda.synchronize()
    return rc, route.value, ns.value


def run_case(lib, case, device="cuda"):
    """Launch one case (every forward mode, both balance settings of the forward tile kernel; each launch twice, and once with
    the overflow flag set) -> dict(err={output: figure}, finite, route_ok, slot_arrays_ok, tail_ok, unowned_ok, deterministic, overflow_ok)."""
    kernel, gname, F = case
    g, d, csr, d64, refs = _device_case(gname, F, device)
    rkey = "fwd" if kernel.startswith("fwd") else ("adj" if kernel.startswith("adj") else kernel)
    if rkey not in refs:  # fp64 on the device, once per (graph, F, statement), left unchanged
        refs[rkey] = reference(kernel, g, d64)
    ref = refs[rkey]
    N, P = g["N"], g["P"]
    group = KERNELS[kernel][2]
    res = dict(err={}, finite=True, route_ok=True, slot_arrays_ok=True, tail_ok=True, unowned_ok=True, deterministic=True, overflow_ok=True)
    x = message_args(kernel, g, csr, F)
    modes = FWD_MODES if kernel.startswith("fwd") else (None,)
    balances = (0, 1) if kernel == "fwd_tile" else (-1,)
    names = {"fwd": ("Mi", "Ch_%s"), "adj": ("gPn", None), "gd": ("gPn", None), "dual": ("out", "out_t")}[kernel.split("_")[0]]
    for mode in modes:
        for bal in balances:
            runs = []
            for _ in range(2):
                out = fresh_outputs(kernel, g, d, F, device)
                rc, route, ns = launch(lib, kernel, x, d, out, mode, g, bal)
                assert rc == 0, f"tmdnet_debug_message returned {rc}"
                res["route_ok"] &= route == KERNELS[kernel][1]
                res["slot_arrays_ok"] &= ns == (F // group if group else 0)
                runs.append(out)
            a, b = runs
            got = {names[0]: a["out"][:N]}
            if names[1]:
                got[names[1] % mode if "%" in names[1] else names[1]] = a["out2"][:N]
            else:
                res["unowned_ok"] &= bool((bits(a["out2"]) == SENTINEL).all())  # the second output is not this sweep's
            if group:
                cnt = F // group
                got["slots"] = a["slots"][:cnt, :2 * P]
                res["unowned_ok"] &= bool((bits(a["slots"][:cnt, 2 * P:]) == SENTINEL).all()) and bool((bits(a["slots"][cnt:]) == SENTINEL).all())
            for k, v in got.items():
                r = ref[k]
                e = O.slot_rel_err(v, r[0], r[1]) if k == "slots" else O.per_atom_rel_err(v, r)
                res["err"][k] = worse(res["err"].get(k), e)
                res["finite"] &= bool(torch.isfinite(v).all())
            res["tail_ok"] &= bool((bits(a["out"][N:]) == SENTINEL).all()) and bool((bits(a["out2"][N:]) == SENTINEL).all())
            res["deterministic"] &= all(bool(torch.equal(bits(a[k]), bits(b[k]))) for k in a)
    # pair overflow (counts[2] != 0): the adjacency is not to be trusted, every kernel returns without a write
    x.counts = _ptr(csr["counts_overflow"])
    out = {k: sentinel(tuple(v.shape), device) for k, v in fresh_outputs(kernel, g, d, F, device).items()}
    rc, _, _ = launch(lib, kernel, x, d, out, modes[0], g, balances[-1])
    assert rc == 0
    res["overflow_ok"] = all(bool((bits(v) == SENTINEL).all()) for v in out.values())
    return res
