"""The Equivariant Transformer's edge sweeps and their adjoints in isolation, through tmdnet_debug_et, on hand-built graphs, against
the float64 statements of tests/et_unit_oracle.py (kept honest by autograd in tests/test_et_unit_oracle.py).

Every kernel generation the launchers can pick runs by explicit selection: the tile sweeps k_et_attn_fwd_g16 / k_et_attn_bwd_g16
(slot order and list order, with the LDS mailbox, with it switched off, and with tkv allocated below dkv so that the launcher drops
it; slot order forced onto sparse and partial tiles, list order onto full ones, the list walk with no barrier and with one every
other step), the pipelined row sweeps k_et_attn_*_p and the generic ones k_et_attn_fwd / k_et_attn_bwd.  The graphs are built to land on
the block-uniform branches that random molecules miss: a longest row of exactly 48 and of 47 entries (the slot-order threshold),
slot-order rows with gaps and a row with nothing but its self edge, list order with an odd step count, a partial last tile next to
full ones in one launch, greedy packing of several molecules per tile and a tile of 63 + 1 atoms, a fill of exactly 0.25 x 4096
entries, open tiles, and for the row kernels a ladder of complete molecules of 1 .. 26 atoms (every unroll tail) and a system of one
atom.  Head widths 2 .. 64, F from 32 to 128 (40 and 48 for the generic kernels), the (keys, values, vector-cutoff) combinations,
fp32 and bf16 pair rows (bf16 inputs are exactly representable, so the reference receives the very values the kernel widens).
tests/test_et_unit_oracle.py asserts, without a device, that the case list contains every class.

Per case, for ATTN_FWD and ATTN_BWD: xagg, the three components of vagg, the five blocks of g_qkv and g_vec PER ATOM (each block
normalised by that atom's own maximum; g_vec starts from random contents); every slot array of gd2 and gr2 on its own against the
float64 partial sum of its channels, every slot normalised by the sum of the absolute values of its terms; the 64 sentinel rows
behind row N, the self pair's slots, every slot beyond the pair list and every array beyond the caller's count bit-unchanged; the
arrays the row kernels must zero exactly zero; two launches bit-identical; nothing written with counts[2] set; the tile kernels
write nothing with meta[0] = 1; *route_out is the generation that wrote.  One extremes case per generation: pre-activations of
exactly +-30, +-88 and +-1e4, outputs finite, same comparison.

Bounds: profiles/et_unit_floor.json, max(2e-6, 4 x the float32 rounding floor of the reference itself on the case's inputs), never
above 1e-5 (tools/et_unit_floor.py; the errors observed on the MI355X are recorded beside them)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import et_unit_cases as U
from tests import kernel_unit_cases as K

pytestmark = pytest.mark.gpu

CASES = U.all_cases()


@pytest.fixture(scope="module")
def bounds():
    return U.load_bounds()["cases"]


def _check(ent, err, who):
    for k, e in err.items():
        b = ent[k]["bound"]
        assert b == K.bound_of(ent[k]["floor"]) and 2e-6 <= b <= 1e-5
        assert math.isfinite(e) and e < b, (who, k, e, b)


@pytest.mark.parametrize("case", CASES, ids=[U.case_id(c) for c in CASES])
def test_et_attention_kernel_vs_fp64(hip_lib, bounds, case):
    r = U.run_case(hip_lib, case)
    ent = bounds[U.case_id(case)]
    print(U.case_id(case), {k: f"{e:.3g}" for k, e in r["err"].items()}, {k: ent[k]["bound"] for k in r["err"]})
    if case.graph == "open70" and case.kernel == U.TILE:
        assert r["err"] == {}  # open tiles: nothing to compare, nothing written (unowned_ok), route 0 (route_ok)
    else:
        assert set(r["err"]) == set(U.FWD_OUTPUTS + U.BWD_OUTPUTS)
    assert r["finite"], (case, "an output row or a slot the kernel owns was left at the NaN sentinel, or is not finite")
    _check(ent, r["err"], case)
    assert r["route_ok"], (case, "*route_out is not the generation that wrote")
    assert r["tail_ok"], (case, "rows behind N were written")
    assert r["unowned_ok"], (case, "the self pair's slots, a slot behind the pair list, an array beyond the count or an output of the other op was written")
    assert r["zeroed_ok"], (case, "a slot array the row kernels must zero is not exactly zero")
    assert r["deterministic"], (case, "two launches differ")
    assert r["overflow_ok"], (case, "written although the pair-overflow flag is set")
    assert r["flag_ok"], (case, "the tile kernel wrote although meta[0] = 1")


PREP = [(g, bf, mf) for g in U.GRAPHS for bf in (0, 1) for mf in (-1.0, 0.0)] + \
    [("fill_edge32", 0, 0.25), ("fill_edge32", 0, float(np.nextafter(np.float32(0.25), np.float32(1)))), ("fill_edge31", 1, 961 / 4096),
     ("packed", 0, 11848 / 16384), ("packed", 0, float(np.nextafter(np.float32(11848 / 16384), np.float32(1))))]


@pytest.mark.parametrize("gname,bf16,min_fill", PREP, ids=["%d-%s-%s-fill%.4g" % (n, g, "bf16" if b else "fp32", m) for n, (g, b, m) in enumerate(PREP)])
def test_tile_prep(hip_lib, gname, bf16, min_fill):
    """meta and tile_start against the numpy statement of the greedy packing and of the open and fill rules (the fill comparison in
    float32, as the kernel makes it); erec bit for bit from its inputs, zeros for the direction of a self edge, nothing behind E."""
    gd, csr = U.device_graph(gname)
    g = U.build_graph(gname)
    d, lay = U.make_inputs(gname, 32, 2, (0, 0, 0))
    dd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}
    eff = min_fill if min_fill >= 0 else (U.MIN_FILL_BF16 if bf16 else U.MIN_FILL_F32)
    is_open, n, ts = U.tile_prep_statement(g, eff)
    out = U.fresh_outputs(gd, dd, lay, "cuda")
    for counts in ("counts", "counts_overflow"):
        prep = U.prep_buffers(gd, "cuda")
        x = U.et_args(gd, csr, lay, U.OP_TILE_PREP, 0, bf16, counts)
        x.min_fill = min_fill
        rc, route = U.launch(hip_lib, x, dd, (None, None), out, prep)
        assert rc == 0 and route == 0
        if counts == "counts_overflow":  # the step fails anyway: open, no tiles, no records
            assert prep["meta"].tolist() == [1, 0] and bool((K.bits(prep["erec"]) == K.SENTINEL).all())
            continue
        assert prep["meta"].tolist() == [is_open, n], (prep["meta"].tolist(), is_open, n)
        assert prep["tile_start"][:n + 1].tolist() == ts and bool((prep["tile_start"][n + 1:] == -1).all())
        E, P = g["E"], g["P"]
        rec = prep["erec"]
        assert bool((K.bits(rec[E:]) == K.SENTINEL).all())
        p = gd["epair"]
        prh = torch.cat([dd["prhat"][:P], torch.zeros(1, 3, device="cuda")])[p] * (gd["esign"] != 0)[:, None]
        want = torch.cat([gd["col"].int().view(torch.float32)[:, None], p.int().view(torch.float32)[:, None], gd["esign"][:, None],
                          dd["C"][p][:, None], dd["dC"][p][:, None], prh], 1)
        assert torch.equal(K.bits(rec[:E].contiguous()), K.bits(want.contiguous()))
    assert all(bool((K.bits(v[gd["N"]:] if k not in ("gd2", "gr2") else v) == K.SENTINEL).all()) for k, v in out.items())


AUTO_CASES = [
    # graph, F, hd, combo, bf16 -> the generation the launchers end up with
    ("full64", 64, 16, (1, 1, 0), 0, U.TILE),
    ("full64", 96, 32, (1, 0, 1), 0, U.TILE),
    ("packed", 64, 16, (1, 1, 0), 0, U.TILE),          # 11848 entries >= 0.70 x 4 x 4096
    ("full64x3+37", 128, 16, (0, 1, 1), 1, U.TILE),
    ("fill_edge32", 64, 16, (1, 1, 0), 1, U.TILE),      # 1024 = 0.25 x 4096 exactly: not below
    ("fill_edge31", 64, 16, (1, 1, 0), 1, U.ROW_PIPELINED),
    ("fill_edge32", 64, 16, (1, 1, 0), 0, U.ROW_PIPELINED),  # fp32 rows want 0.70
    ("open70", 64, 16, (1, 1, 0), 0, U.ROW_PIPELINED),
    ("open70", 96, 32, (0, 1, 0), 0, U.ROW_GENERIC),
    ("ladder", 40, 8, (1, 1, 0), 0, U.ROW_GENERIC),     # F % 32: no tile kernel whatever the flag says
    ("ladder", 64, 64, (1, 0, 1), 0, U.ROW_GENERIC),
    ("one_atom", 64, 4, (1, 1, 0), 0, U.ROW_PIPELINED),
]


@pytest.mark.parametrize("gname,F,hd,combo,bf16,want", AUTO_CASES, ids=["%s-F%d-hd%d-%s" % (a[0], a[1], a[2], "bf16" if a[4] else "fp32") for a in AUTO_CASES])
def test_auto_is_what_the_engine_enqueues(hip_lib, gname, F, hd, combo, bf16, want):
    """TMDNET_ET_AUTO = tile prep + launch_et_attn_fwd / launch_et_attn_bwd: *route_out and meta as the numpy statement of the prep
    and the launchers' predicates predict, and the outputs bit for bit those of the explicitly selected kernel."""
    c = U.Case(want, gname, F, hd, combo, bf16, "")
    gd, csr, dd, lay, _, _ = U.device_case(c)
    route_want, meta_want = U.auto_route(U.build_graph(gname), F, hd, lay["Wd"], bf16)
    assert route_want == want
    rows = U.pair_rows_on_device(dd, bf16)
    for op in (U.OP_ATTN_FWD, U.OP_ATTN_BWD):
        outs = []
        for sel in (U.AUTO, want):
            out, prep = U.fresh_outputs(gd, dd, lay, "cuda"), U.prep_buffers(gd, "cuda")
            rc, route = U.launch(hip_lib, U.et_args(gd, csr, lay, op, sel, bf16), dd, rows, out, prep)
            assert rc == 0 and route == want, (op, sel, rc, route)
            if sel == U.AUTO or sel == U.TILE:
                assert tuple(prep["meta"].tolist()) == meta_want
            else:
                assert prep["meta"].tolist() == [-1, -1]  # the row kernels by selection need no prep and run none
            outs.append(out)
        assert all(torch.equal(K.bits(outs[0][k]), K.bits(outs[1][k])) for k in outs[0]), (op, "AUTO differs from the selected kernel")
        mine = ("xagg", "vagg") if op == U.OP_ATTN_FWD else ("g_qkv", "g_vec")
        assert all(bool(torch.isfinite(outs[0][k][:gd["N"]]).all()) for k in mine)


def test_et_rejects_what_is_outside_the_contract(hip_lib):
    """TMDNET_ERR_INVALID and no launch: every output still holds the sentinel, *route_out is untouched."""
    from torchmdnet_amd import _C

    c = U.Case(U.TILE, "full64", 64, 16, (1, 1, 0), 0, "")
    gd, csr, dd, lay, _, _ = U.device_case(c)
    rows = U.pair_rows_on_device(dd, 0)
    rows_bf = U.pair_rows_on_device(dd, 1)
    out = {k: K.sentinel(tuple(v.shape), "cuda") for k, v in U.fresh_outputs(gd, dd, lay, "cuda").items()}
    prep = U.prep_buffers(gd, "cuda")
    extra = dict(slots=K.sentinel((2, gd["P"] + 1, lay["Wd"]), "cuda"), self_rows=K.sentinel((gd["N"], lay["Wd"]), "cuda"))

    def call(op, sel, edit, bf16=0):
        x = U.et_args(gd, csr, lay, op, sel, bf16)
        x.dir_stride = (gd["P"] + 1) * lay["Wd"]
        x.slots, x.self_rows = extra["slots"].data_ptr(), extra["self_rows"].data_ptr()
        return U.launch(hip_lib, x, dd, rows_bf if bf16 else rows, out, prep, edit)

    def rejected(op, sel, edit, bf16=0):
        rc, route = call(op, sel, edit, bf16)
        assert rc == _C.ERR_INVALID and route == -7, (op, sel, rc, route)

    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip_lib.tmdnet_debug_et(s, None, None) == _C.ERR_INVALID
    sels = (U.AUTO, U.ROW_GENERIC, U.ROW_PIPELINED, U.TILE)
    for op in (U.OP_ATTN_FWD, U.OP_ATTN_BWD):
        for sel in sels:
            for field, bad in (("N", 0), ("N", -3), ("P", -1), ("F", 0), ("F", 1088), ("hd", 0), ("hd", 3), ("hd", 128), ("Wd", 4 * 64 - 1),
                               ("dk_off", 8), ("dk_off", -2), ("dv_off", 0), ("dv_off", 2 * 64), ("pair_bf16", 2)):
                rejected(op, sel, lambda x, f=field, v=bad: setattr(x, f, v))
            for field in ("rowptr", "col", "epair", "esign", "counts", "prhat", "C", "dC", "qkv", "vec", "dkv"):
                rejected(op, sel, lambda x, f=field: setattr(x, f, None))
            for field in (("xagg", "vagg") if op == U.OP_ATTN_FWD else ("g_xagg", "g_vagg", "g_qkv", "g_vec", "gd2", "gr2", "tkv")):
                rejected(op, sel, lambda x, f=field: setattr(x, f, None))
        for sel in (-1, 4, 99):
            rejected(op, sel, lambda x: None)
        rejected(U.OP_ATTN_BWD, U.TILE, lambda x: setattr(x, "slot_stride", 2 * (gd["P"] + 1) - 1))
        # a row kernel outside its contract: the pipelined sweeps want F % 64 == 0 and hd <= 16
        for F, hd in ((32, 16), (96, 16), (64, 32), (64, 64)):
            rejected(op, U.ROW_PIPELINED, lambda x, F=F, hd=hd: (setattr(x, "F", F), setattr(x, "hd", hd), setattr(x, "dv_off", F)))
        # the tile kernels: F % 32, a head of 1 or of 64 channels, the prep's arrays, B, E, alignment
        for F, hd in ((48, 16), (40, 8), (64, 64), (64, 1)):
            rejected(op, U.TILE, lambda x, F=F, hd=hd: (setattr(x, "F", F), setattr(x, "hd", hd), setattr(x, "dv_off", F)))
        for sel in (U.AUTO, U.TILE):
            for field in ("meta", "tile_start", "erec"):
                rejected(op, sel, lambda x, f=field: setattr(x, f, None))
            rejected(op, sel, lambda x: setattr(x, "B", 0))
            rejected(op, sel, lambda x: setattr(x, "E", -1))
            rejected(op, sel, lambda x: setattr(x, "qkv", x.qkv + 8))
    rejected(U.OP_TILE_PREP, 0, lambda x: setattr(x, "B", 0))
    rejected(U.OP_TILE_PREP, 0, lambda x: setattr(x, "meta", None))
    rejected(U.OP_TILE_PREP, 0, lambda x: setattr(x, "erec", None))
    rejected(-1, 0, lambda x: None)
    rejected(10, 0, lambda x: None)
    # TRAIN_FILTER reads dkv as fp32: never with bf16 rows; and it needs a projection to write for
    rc, _ = call(U.OP_TRAIN_FILTER, 0, lambda x: None)
    assert rc == _C.OK
    extra["slots"].copy_(K.sentinel(tuple(extra["slots"].shape), "cuda"))
    extra["self_rows"].copy_(K.sentinel(tuple(extra["self_rows"].shape), "cuda"))
    rejected(U.OP_TRAIN_FILTER, 0, lambda x: None, bf16=1)
    rejected(U.OP_TRAIN_FILTER, 0, lambda x: (setattr(x, "dk_off", -1), setattr(x, "dv_off", -1)))
    rejected(U.OP_TRAIN_FILTER, 0, lambda x: setattr(x, "slots", None))
    rejected(U.OP_TRAIN_FILTER, 0, lambda x: setattr(x, "self_rows", None))
    rejected(U.OP_TRAIN_FILTER, 0, lambda x: setattr(x, "dir_stride", (gd["P"] + 1) * lay["Wd"] - 1))
    for op, fields in ((U.OP_PAIR_COMBINE, ("gd2", "gr2", "gd_extra", "gd", "g_rhat")), (U.OP_NBR_EMBED, ("z", "emb", "embN", "Wn", "xcat")),
                       (U.OP_NBR_EMBED_BWD, ("pair_i", "z", "embN", "g_xcat", "dWn")), (U.OP_TRAIN_NBR, ("z", "embN", "Wn", "g_xcat", "gEN")),
                       (U.OP_TRAIN_GPRE, ("self_sum", "pre", "g_pre"))):
        rejected(op, 0, lambda x: None)  # (none of these operands is bound here: each op misses at least one)
    torch.cuda.synchronize()
    assert all(bool((K.bits(t) == K.SENTINEL).all()) for t in list(out.values()) + list(extra.values())), "a rejected call launched"
    assert prep["meta"].tolist() == [-1, -1]
    # and the same arguments, within the contract, run
    rc, route = call(U.OP_ATTN_FWD, U.TILE, lambda x: setattr(x, "min_fill", 0.0))
    assert (rc, route) == (_C.OK, U.TILE) and bool(torch.isfinite(out["xagg"][:gd["N"]]).all())


OTHER = [(g, F) for g in U.OTHER_GRAPHS for F in U.OTHER_F]


@pytest.mark.parametrize("gname,F", OTHER, ids=[U.other_id(g, F) for g, F in OTHER])
def test_pair_combine_and_neighbour_embedding_ops_vs_fp64(hip_lib, bounds, gname, F):
    """PAIR_COMBINE, NBR_EMBED, NBR_EMBED_BWD, TRAIN_NBR and TRAIN_GPRE against their statements: rows per atom or pair, sums over
    slots against the sum of the absolute values of their terms; rows behind the end untouched, two launches identical, nothing
    written with the overflow flag set."""
    r = U.run_other(hip_lib, gname, F)
    ent = bounds[U.other_id(gname, F)]
    flat = {f"{op}.{k}": e for op, d in r["err"].items() for k, e in d.items()}
    print(U.other_id(gname, F), {k: f"{e:.3g}" for k, e in flat.items()})
    assert set(flat) == set(ent)
    _check(ent, flat, (gname, F))
    assert r["tail_ok"] and r["deterministic"] and r["overflow_ok"], r


@pytest.mark.parametrize("fc", U.FILTER_CASES, ids=[U.filter_id(fc) for fc in U.FILTER_CASES])
def test_filter_row_adjoint_vs_fp64(hip_lib, bounds, fc):
    """TRAIN_FILTER: the per-direction rows of every pair and the self rows of every atom, per row, against float64"""
    r = U.run_filter(hip_lib, fc)
    ent = bounds[U.filter_id(fc)]
    print(U.filter_id(fc), {k: f"{e:.3g}" for k, e in r["err"].items()})
    assert set(r["err"]) == set(ent)
    _check(ent, r["err"], fc)
    assert r["unowned_ok"] and r["deterministic"] and r["overflow_ok"], r
