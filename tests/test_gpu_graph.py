"""-m gpu: the neighbour graph that tmdnet_build_graph[_static] leaves in its workspace, read back array by array through
tmdnet_debug_graph and compared with the float64 specification tests/graph_oracle.py on the cases of tests/graph_unit_cases.py
(tests/test_graph_oracle.py shows without a device that the specification agrees with oracle/neighbors_numpy.py, that no case has
a borderline decision and that the list reaches every branch of the graph kernels).

Integer arrays, flags, the renumbering and the grid are compared EXACTLY.  The minimum image is the reference's sequential
z -> y -> x rounding, which is not the nearest image in the strongly skewed boxes used here: the engine is kept as the reference has
it.  Of a build that fails on an out-of-range molecule index only the flags are pinned (the row counts of such a build are
unspecified: the wave kernels empty the offending rows, the thread-per-atom kernels every row).

Float arrays against float64, with u = 2^-24 and S = |pos_i|inf + |pos_j|inf + sum |box entries| of the pair: one fp32 subtraction
and at most three fused shifts give |pdelta - spec| <= 4 u S, pd twice that, prhat 4 u per component.  The prhat bound does not
survive the error that pdelta is allowed: the same fp32 statement in numpy (graph_oracle.fp32_statement) already misses it in
every periodic case (up to 44 x 4 u for atoms three box lengths outside), so where that floor exceeds the derived bound the test
allows 4 x the floor of the case, and nowhere else.  Observed on the MI355X (profiles/graph_unit.json, floors and errors per case):
all three arrays carry the bits of the fp32 statement in every case; pdelta reaches 0.23, pd 0.19 of its derived bound."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # before the library is loaded, as in every GPU test module: both then share the HIP runtime that torch brings

from tests import graph_oracle as O
from tests import graph_unit_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
OK, ERR_INVALID, ERR_OVERFLOW, ERR_STATE = 0, 1, 3, 5
REPORT = {}


@pytest.fixture(scope="module")
def eng(hip_lib):
    e = G.Engine()
    yield e
    e.close()
    _report()


def _report():
    """the largest observed error and fp32 floor of every float array, as multiples of the derived bound (written to the file named
    by GRAPH_UNIT_REPORT when set: profiles/graph_unit.json is such a run on the MI355X)"""
    if not REPORT:
        return
    summary = {k: {q: max(rec[k][q] for rec in REPORT.values()) for q in ("observed_over_derived", "floor_over_derived")}
               for k in ("pdelta", "pd", "prhat")}
    print("[graph_unit] summary", json.dumps(summary))
    if os.environ.get("GRAPH_UNIT_REPORT"):
        with open(os.environ["GRAPH_UNIT_REPORT"], "w") as fh:
            json.dump({"unit": "u = 2^-24; derived bounds: pdelta 4 u S, pd 8 u S, prhat 4 u (tests/test_gpu_graph.py)",
                       "summary": summary, "cases": REPORT}, fh, indent=1, sort_keys=True)


def _is_sentinel(a):
    return bool(np.all(a.view(np.uint8) == G.SENTINEL))


def _invariants(a, n, filled):
    """what the sweeps rely on, asserted on the device's own arrays alone"""
    P, E = int(a["counts"][0]), int(a["counts"][1])
    assert np.array_equal(a["rowptr"], np.concatenate([[0], np.cumsum(a["ntot"])])) and a["rowptr"][n] == E
    assert np.array_equal(a["pairptr"], np.concatenate([[0], np.cumsum(a["nlow"])])) and a["pairptr"][n] == P
    if not filled:
        return
    col, ep, sg = a["col"][:E], a["epair"][:E], a["esign"][:E]
    row = np.repeat(np.arange(n), a["ntot"])
    start = np.zeros(E, dtype=bool)
    start[a["rowptr"][:n][a["ntot"] > 0]] = True
    assert np.all((np.diff(col) > 0) | start[1:]), "columns must ascend strictly inside a row"
    rank = np.arange(E) - a["rowptr"][:n][row]
    assert np.array_equal(col < row, rank < a["nlow"][row]), "the lower neighbours come first"
    assert np.array_equal(sg, np.sign(row - col).astype(np.float32)), "esign is +1 / 0 / -1 by orientation"
    assert np.all(ep[col == row] == P) and np.all(ep[col != row] < P) and np.all(ep >= 0)
    lower, upper = col < row, col > row
    assert np.array_equal(a["pair_i"][ep[lower]], row[lower]) and np.array_equal(a["pair_j"][ep[lower]], col[lower])
    assert np.array_equal(a["pair_i"][ep[upper]], col[upper]) and np.array_equal(a["pair_j"][ep[upper]], row[upper])
    assert np.array_equal(np.bincount(ep, minlength=P + 1)[:P], np.full(P, 2)), "every pair id is used by exactly two edges"
    assert np.array_equal(ep[lower], np.arange(P)), "lower edges in row order are the pair list"
    assert a["pd"][P] == 0.0, "pd[P] is the self pair"


def _check_perm(a, n):
    perm, key = a["perm"].astype(np.int64), a["cell_key_sorted"]
    assert np.array_equal(np.sort(perm), np.arange(n)), "perm is a bijection"
    assert np.all(np.diff(key) >= 0) and np.all((np.diff(key) > 0) | (np.diff(perm) > 0)), "a stable sort by cell id"


def _check_floats(name, tag, a, s):
    P = int(s["counts"][0])
    if not P:
        return
    S = s["scale"]
    f_d, f_pd, f_rh = O.fp32_statement(s)
    got = {"pdelta": a["pdelta"][: 3 * P].reshape(P, 3).astype(np.float64), "pd": a["pd"][:P].astype(np.float64),
           "prhat": a["prhat"][: 3 * P].reshape(P, 3).astype(np.float64)}
    ref = {"pdelta": s["pdelta"], "pd": s["pd"][:P], "prhat": s["prhat"]}
    floor = {"pdelta": f_d.astype(np.float64), "pd": f_pd[:P].astype(np.float64), "prhat": f_rh.astype(np.float64)}
    bound = {"pdelta": (4 * U * S)[:, None], "pd": 8 * U * S, "prhat": np.full((P, 1), 4 * U)}
    rec = {}
    for k in ("pdelta", "pd", "prhat"):
        err, flo = np.abs(got[k] - ref[k]), np.abs(floor[k] - ref[k])
        allowed = bound[k] if np.all(flo <= bound[k]) else np.maximum(bound[k], 4 * flo.max())
        rec[k] = dict(observed_over_derived=float((err / bound[k]).max()), floor_over_derived=float((flo / bound[k]).max()),
                      observed_max=float(err.max()), floor_max=float(flo.max()), bit_equal_to_fp32_statement=bool(np.array_equal(got[k], floor[k])))
        print(f"[graph_unit] {name} {tag} {k}: {rec[k]}")
        assert np.all(err <= allowed), (name, tag, k, rec[k])
    REPORT[f"{name}/{tag}"] = rec


def _compare(name, tag, c, r, s, static):
    a = r["arrays"]
    cnt, exp = a["counts"][:6], s["counts"]
    bad_batch, bad_z, over = bool(exp[5]), bool(exp[4]), bool(exp[2])
    want_rc = ERR_INVALID if (bad_batch or bad_z) else (ERR_OVERFLOW if over else OK)
    assert r["rc_counts"] == want_rc and r["rc"] == (OK if static else want_rc), (name, tag, r["rc"], r["rc_counts"])
    assert _is_sentinel(r["tail"]), "bytes behind tmdnet_graph_workspace_bytes were written"
    assert np.array_equal(r["counts_query"][:6], cnt) and (static or np.array_equal(r["counts_host"][:6], cnt))
    filled = not over if static else want_rc == OK
    if bad_batch:
        assert np.array_equal(cnt[[2, 3, 5]], exp[[2, 3, 5]]), (name, tag, cnt)
    else:
        assert np.array_equal(cnt, exp), (name, tag, cnt, exp)
        _invariants(a, c.n, filled)
        for k in ("nlow", "ntot", "rowptr", "pairptr", "mstart", "mend", "perm", "cell_key_sorted", "bat_c", "z_c", "cgrid"):
            if k in s:
                assert np.array_equal(a[k], s[k]), (name, tag, k)
    if s["route_cell"]:
        assert r["grid"] == tuple(int(v) for v in s["cgrid"][:3]) + (1,), (name, r["grid"])
        _check_perm(a, c.n)
        if c.z is not None:
            assert np.array_equal(a["z_c"], np.clip(c.z, 0, G.MAX_Z - 1)[a["perm"]]), "z_c == z[perm]"
        assert np.allclose(a["boxd"][:9].reshape(3, 3), s["boxd"], rtol=1e-6, atol=0)
    else:
        assert r["grid"] == (0, 0, 0, 0)
    P, E = int(cnt[0]), int(cnt[1])
    if not filled:  # overflow or a refused input: the fill and link phases must not have run
        for k in G.FILL_ARRAYS:
            assert _is_sentinel(a[k]), (name, tag, k, "written although the build did not go through")
        return
    for k in ("col", "epair", "esign", "pair_i", "pair_j"):
        m = E if k in ("col", "epair", "esign") else P
        assert np.array_equal(a[k][:m], s[k]), (name, tag, k)
        assert _is_sentinel(a[k][m:]), (name, tag, k, "written past its end")
    assert _is_sentinel(a["pd"][P + 1:]) and _is_sentinel(a["pdelta"][3 * P:]) and _is_sentinel(a["prhat"][3 * P:])
    _check_floats(name, tag, a, s)


def _same(a, b, skip=()):
    return [k for k in a if k not in skip and not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]


@pytest.mark.parametrize("name", list(G.CASES))
def test_graph_equals_specification(eng, name):
    c = G.CASES[name]
    s = G.spec_of(c)
    racy = ("mstart", "mend") if (not s["route_cell"] and s["counts"][3]) else ()  # unsorted batch: ranges unused, written by many
    dyn = eng.build(c, static=False)
    _compare(name, "dynamic", c, dyn, s, False)
    again = eng.build(c, static=False)
    assert not _same(dyn["arrays"], again["arrays"], racy), "two builds differ"
    if c.static:
        st = eng.build(c, static=True)
        _compare(name, "static", c, st, s, True)
        skip = racy + (G.FILL_ARRAYS if (dyn["rc"] != OK) != bool(s["counts"][2]) else ())  # a refused z: only the static build fills
        assert not _same(dyn["arrays"], st["arrays"], skip), "static and dynamic builds differ"


@pytest.mark.parametrize("name", [n for n in G.CELL if G.CASES[n].weights is None])
def test_cell_and_brute_routes_agree_bit_for_bit(eng, name):
    """the stated purpose of pair_geometry: same pairs after mapping through perm, identical pdelta / pd bits"""
    c = G.CASES[name]
    cell, brute = eng.build(c)["arrays"], eng.build(c, cell=None)["arrays"]
    P = int(cell["counts"][0])
    assert P == int(brute["counts"][0]) and P > 0
    hi, lo, sign, o = O.pair_set_original(dict(pair_i=cell["pair_i"][:P], pair_j=cell["pair_j"][:P]), cell["perm"])
    assert np.array_equal(hi, brute["pair_i"][:P]) and np.array_equal(lo, brute["pair_j"][:P])  # brute: already (i, j) sorted
    # an orientation flipped by the renumbering negates the difference before the image is chosen; rounding to nearest is symmetric
    # in the sign, so every later step is negated exactly: equal values (a zero may change its sign bit), identical distances
    d_c = cell["pdelta"][: 3 * P].reshape(P, 3)[o] * sign[:, None].astype(np.float32)
    assert np.array_equal(d_c, brute["pdelta"][: 3 * P].reshape(P, 3))
    assert np.array_equal(cell["pd"][:P][o].view(np.uint32), brute["pd"][:P].view(np.uint32))


def test_ghost_pairs_are_left_out(eng):
    c = G.CASES["cell_ghosts"]
    a = eng.build(c)["arrays"]
    P = int(a["counts"][0])
    w = c.weights[a["perm"]]
    assert np.all((w[a["pair_i"][:P]] != 0) | (w[a["pair_j"][:P]] != 0))
    full = int(eng.build(G.CASES["cell_auto"])["arrays"]["counts"][0])
    assert 0 < P < full


@pytest.mark.parametrize("switch", ["TMDNET_SCALAR_GRAPH", "TMDNET_NO_GRAPH_SMALL"])
def test_developer_switch_kernels_build_the_same_bits(eng, tmp_path, switch):
    """the thread-per-atom specification kernels and the general kernels in place of the one-launch small-system kernel, each in a
    fresh interpreter (the switches are read once per process), against the in-process result, bit for bit"""
    path = str(tmp_path / "graph.npz")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "graph_unit_cases.py"), path], env=dict(os.environ, **{switch: "1"}),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "GRAPH_DUMP_OK" in out.stdout, (switch, out.stdout[-500:], out.stderr[-1500:])
    child = np.load(path)
    for name in G.SWITCH_CASES:
        c, s = G.CASES[name], G.spec_of(G.CASES[name], None)
        for static in ([False, True] if c.static else [False]):
            r = eng.build(c, static=static, cell=None)
            assert np.array_equal(child[f"{name}/{int(static)}/rc"], [r["rc"], r["rc_counts"]])
            for k, v in r["arrays"].items():
                w = child[f"{name}/{int(static)}/{k}"]
                if s["counts"][5]:  # a refused molecule index: the flags only (module docstring)
                    assert k != "counts" or np.array_equal(v[[2, 3, 5]], w[[2, 3, 5]])
                elif not (s["counts"][3] and k in ("mstart", "mend")):
                    assert np.array_equal(v.view(np.uint8), w.view(np.uint8)), (switch, name, static, k)


def test_accessor_contract(eng):
    import ctypes as C

    c = G.CASES["small_64"]
    r = eng.build(c)
    h, L, ws = eng.handle(c), eng.L, r["ws"]
    out = torch.full((4 * (c.n + 1),), G.SENTINEL, dtype=torch.uint8, device="cuda")
    call = lambda w, n, b, name, nbytes: L.tmdnet_debug_graph(h, eng.stream(), C.c_void_p(w.data_ptr()), n, b, name, C.c_void_p(out.data_ptr()), nbytes)  # noqa: E731
    assert call(ws, c.n, 1, b"rowptr", 4 * (c.n + 1)) == OK
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.int32), r["arrays"]["rowptr"])
    out.fill_(G.SENTINEL)
    assert call(ws, c.n, 1, b"no_such_array", 4 * c.n) == ERR_INVALID and b"unknown graph array" in L.tmdnet_last_error(h)
    assert call(ws, c.n, 1, b"rowptr", 4 * c.n) == ERR_INVALID and b"size mismatch" in L.tmdnet_last_error(h)
    assert call(ws, c.n + 1, 1, b"nlow", 4 * (c.n + 1)) == ERR_INVALID  # not the atom count of the last build on this workspace
    other = eng.handle(dataclasses.replace(c, mnn=c.mnn - 1))  # a handle that never built a graph on this workspace
    assert L.tmdnet_debug_graph(other, eng.stream(), C.c_void_p(ws.data_ptr()), c.n, 1, b"rowptr", C.c_void_p(out.data_ptr()),
                                4 * (c.n + 1)) == ERR_STATE
    assert L.tmdnet_debug_graph(h, eng.stream(), C.c_void_p(ws.data_ptr()), c.n, 1, None, C.c_void_p(out.data_ptr()), 4) == ERR_INVALID
    torch.cuda.synchronize()
    assert _is_sentinel(out.cpu().numpy()), "a refused call wrote something"
