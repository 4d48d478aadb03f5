"""TEST INFRASTRUCTURE ONLY -- the cases of the unit test of the reverse tile sweep with the group-product adjoint folded into its
prologue (csrc/tn_message_pair.hip: k_message_adjoint_rows8_fold, through tmdnet_debug_message_fold): hand-built graphs whose
tiles are all closed, seeded inputs, the float64 / float32 reference, launches and the figures the test asserts on.  One
statement serves tests/test_gpu_message_fold.py (asserts) and tools/message_fold_floor.py (the fp32 rounding floor of the
reference on these very inputs without a device, and the errors observed on the device, into profiles/message_fold_floor.json).

Reference, in the precision of its inputs: gM, gY = autograd gradients of sum(gCh * group_product(Pn, Mi, kap, o3)) with respect
to Mi and Pn (tests/message_oracle.py), gPn = gY + adjoint(g, w, gM), slots = pair_halves(g, dw, gM, Pn, 32)."""
import ctypes as C
import json
import os

import torch

from tests import message_oracle as O
from tests.kernel_unit_cases import SENTINEL, TAIL, bits, sentinel
from tests.message_unit_cases import FWD_MODES, SLOT_PAD, fwd_mode_args, worse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR_JSON = os.path.join(ROOT, "profiles", "message_fold_floor.json")
GROUP = 32  # channels per slot array of the tile kernels

# graph name -> [(atoms, rule)] per molecule; rule: "complete", ("band", b): |a - b| <= b, ("hubs", h): a < h or b < h.
# No molecule straddles a multiple of 64 rows: every tile is closed.
GRAPHS = {
    "complete64": [(64, "complete")],                                     # nE = 4096 = MP_E exactly, equal rows, no helper
    "partial": [(64, ("band", 9)), (37, "complete")],                     # 64 + 37: a partial last tile, its dead rows help
    "molecules": [(20, "complete"), (44, ("band", 6)), (64, "complete"),  # several molecules per tile,
                  (1, "complete"), (63, "complete")],                     # a one-atom molecule that helps the rows of 63
    "star": [(64, ("hubs", 1))],                                          # one row of 64 entries, the others of 2: parked sums
}
FS = (32, 128)


def all_cases():
    """[(graph, F)]; every case runs the three modes of the group product"""
    return [(gname, F) for gname in GRAPHS for F in FS]


def case_id(case):
    return "%s-F%d" % case


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
            adj = (a[:, None] < rule[1]) | (a[None, :] < rule[1]) | (a[:, None] == a[None, :])
        i, j = torch.nonzero(adj, as_tuple=True)  # sorted by (row, column)
        rows.append(i + base)
        cols.append(j + base)
        batch += [m] * n
        base += n
    rows, cols = torch.cat(rows), torch.cat(cols)
    N = base
    assert bool((rows // 64 == cols // 64).all()), "the tiles of a fold case must be closed"
    lower = rows > cols
    P = int(lower.sum())
    pid = torch.full((N * N,), -1, dtype=torch.int64)
    pid[(rows * N + cols)[lower]] = torch.arange(P)
    epair = torch.where(rows == cols, torch.tensor(P), pid[torch.maximum(rows, cols) * N + torch.minimum(rows, cols)])
    esign = torch.where(rows == cols, 0.0, torch.where(cols < rows, 1.0, -1.0)).float()
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.bincount(rows, minlength=N).cumsum(0)
    g = dict(N=N, P=P, rowptr=rowptr, rows=rows, col=cols, epair=epair, esign=esign, batch=torch.tensor(batch), B=len(GRAPHS[name]))
    _graph_cache[name] = g
    return g


def make_inputs(gname, F):
    """fp32 operands on the CPU, scaled as tests/message_unit_cases.make_inputs scales them: w, dw ~ N(0, 1 / mean row length)
    with P + 1 rows, Pn, Mi ~ N(0, 0.25), gCh ~ N(0, 1), a charge per molecule, a kappa per atom."""
    g = build_graph(gname)
    N, P = g["N"], g["P"]
    gen = torch.Generator().manual_seed(7000003 * sorted(GRAPHS).index(gname) + F)
    rn = lambda *s: torch.randn(*s, generator=gen)
    sw = (N / g["col"].numel()) ** 0.5
    return dict(w=rn(P + 1, 3, F) * sw, dw=rn(P + 1, 3, F) * sw, Pn=rn(N, 9, F) * 0.5, Mi=rn(N, 9, F) * 0.5, gCh=rn(N, 9, F),
                q_mol=rn(g["B"]), kap_atom=1 + 0.3 * rn(N))


def reference(g, d, mode):
    """{"gPn": tensor, "slots": (value, scale)} in the dtype of d (graph index tensors on d's device)"""
    q, batch, o3 = fwd_mode_args(mode, g, d)
    Y, Mm = d["Pn"].clone().requires_grad_(True), d["Mi"].clone().requires_grad_(True)
    Ch = O.group_product(Y, Mm, O.kappa(q, batch, g["N"], Y), o3)
    gY, gM = torch.autograd.grad((Ch * d["gCh"]).sum(), (Y, Mm))
    return {"gPn": gY + O.adjoint(g, d["w"], gM), "slots": O.pair_halves(g, d["dw"], gM, d["Pn"], GROUP)}


def errors(got, ref):
    return {"gPn": O.per_atom_rel_err(got["gPn"], ref["gPn"]), "slots": O.slot_rel_err(got["slots"][0], ref["slots"][0], ref["slots"][1])}


def floor_of(case):
    """mode -> rounding floor per output: the reference in float32 against itself in float64 on the case's own inputs (CPU)"""
    gname, F = case
    g, d = build_graph(gname), make_inputs(gname, F)
    d64 = {k: v.double() for k, v in d.items()}
    return {mode: errors(reference(g, d, mode), reference(g, d64, mode)) for mode in FWD_MODES}


def load_bounds():
    with open(FLOOR_JSON) as fh:
        return json.load(fh)


def _ptr(t):
    return None if t is None else t.data_ptr()


def launch(lib, g, csr, d, F, mode, out, folded, counts="counts"):
    """one call of tmdnet_debug_message_fold -> rc"""
    from torchmdnet_amd import _C

    q, batch, o3 = fwd_mode_args(mode, g, d)
    x = _C.MessageFoldArgs()
    x.N, x.F, x.P, x.o3, x.folded = g["N"], F, g["P"], o3, int(folded)
    x.rowptr, x.col, x.epair, x.esign, x.counts = (_ptr(csr[k]) for k in ("rowptr", "col", "epair", "esign", counts))
    x.w, x.dw, x.gCh, x.Pn, x.Mi, x.q, x.batch = (_ptr(t) for t in (d["w"], d["dw"], d["gCh"], d["Pn"], d["Mi"], q, batch))
    x.gMi, x.gPn, x.slots, x.slot_stride = _ptr(out["gMi"]), _ptr(out["gPn"]), _ptr(out["slots"]), out["slots"].shape[1]
    rc = lib.tmdnet_debug_message_fold(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(x))
    torch.cuda.synchronize()
    return rc


def fresh_outputs(g, F, device):
    """all sentinel: gPn and gMi with 64 rows behind row N, one slot array more than the kernel writes"""
    N = g["N"]
    return {"gPn": sentinel((N + TAIL, 9, F), device), "gMi": sentinel((N + TAIL, 9, F), device),
            "slots": sentinel((F // GROUP + 1, 2 * g["P"] + 2 + SLOT_PAD), device)}


def run_case(lib, case, device="cuda"):
    """Launch one case in the three modes: folded twice, the parent sequence once, folded once with the overflow flag set.
    -> dict(err={mode: {output: figure}}, vs_parent={mode: figure}, gPn_bit_identical={mode: bool}, and the flags below)."""
    gname, F = case
    g = build_graph(gname)
    gd = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in g.items()}
    d = {k: v.to(device).contiguous() for k, v in make_inputs(gname, F).items()}
    d64 = {k: v.double() for k, v in d.items()}
    N, P, cnt = g["N"], g["P"], F // GROUP
    csr = dict(rowptr=gd["rowptr"].int(), col=gd["col"].int(), epair=gd["epair"].int(), esign=gd["esign"].contiguous(),
               counts=torch.tensor([P, g["col"].numel(), 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=device),
               counts_overflow=torch.tensor([P, g["col"].numel(), 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=device))
    res = dict(err={}, vs_parent={}, gPn_bit_identical={}, finite=True, slots_equal_parent=True, tail_ok=True, unowned_ok=True,
               deterministic=True, overflow_ok=True, gMi_untouched=True)
    for mode in FWD_MODES:
        ref = reference(gd, d64, mode)  # fp64 on the device, once per mode
        a, b, par = (fresh_outputs(g, F, device) for _ in range(3))
        assert launch(lib, gd, csr, d, F, mode, a, True) == 0
        assert launch(lib, gd, csr, d, F, mode, b, True) == 0
        assert launch(lib, gd, csr, d, F, mode, par, False) == 0
        got = {"gPn": a["gPn"][:N], "slots": (a["slots"][:cnt, :2 * P],)}
        res["err"][mode] = errors(got, ref)
        res["finite"] &= bool(torch.isfinite(got["gPn"]).all()) and bool(torch.isfinite(got["slots"][0]).all())
        res["vs_parent"][mode] = O.per_atom_rel_err(a["gPn"][:N], par["gPn"][:N].double())
        res["gPn_bit_identical"][mode] = bool(torch.equal(bits(a["gPn"][:N]), bits(par["gPn"][:N])))
        res["slots_equal_parent"] &= bool(torch.equal(bits(a["slots"]), bits(par["slots"])))
        res["tail_ok"] &= bool((bits(a["gPn"][N:]) == SENTINEL).all())
        res["unowned_ok"] &= bool((bits(a["slots"][:cnt, 2 * P:]) == SENTINEL).all()) and bool((bits(a["slots"][cnt:]) == SENTINEL).all())
        res["deterministic"] &= all(bool(torch.equal(bits(a[k]), bits(b[k]))) for k in a)
        res["gMi_untouched"] &= bool((bits(a["gMi"]) == SENTINEL).all())
    out = fresh_outputs(g, F, device)
    assert launch(lib, gd, csr, d, F, FWD_MODES[0], out, True, counts="counts_overflow") == 0
    res["overflow_ok"] = all(bool((bits(v) == SENTINEL).all()) for v in out.values())
    res["worst"] = {}
    for mode in FWD_MODES:
        for k, e in res["err"][mode].items():
            res["worst"][k] = worse(res["worst"].get(k), e)
    return res
