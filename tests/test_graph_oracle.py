"""not-gpu: the float64 specification of the neighbour graph (tests/graph_oracle.py) and the case list of the graph unit tests
(tests/graph_unit_cases.py), checked without a device: on EVERY case the specification has the pair set, vectors and distances of
oracle/neighbors_numpy.py (the reference's own executable statement), no case has a borderline decision (squared cutoffs, roundf
ties, cell faces, grid sizes - the allowed share is zero, so tests/test_gpu_graph.py compares integers exactly), and the list as a
whole reaches every branch of the graph kernels (csrc/tn_graph_wave.hip, tn_kernels.hip, tn_cell.hip) listed in the census below."""
import numpy as np
import pytest

from oracle import neighbors_numpy as NN
from tests import graph_oracle as O
from tests import graph_unit_cases as G


def _reference_pairs(c):
    """pairs of oracle/neighbors_numpy.py in the caller's numbering, (hi, lo) sorted, delta = pos[hi] - pos[lo] (+ image)"""
    valid = np.flatnonzero((c.batch >= 0) & (c.batch < c.n_mol))
    idx = valid[np.argsort(c.batch[valid], kind="stable")]
    pos = c.pos.astype(np.float64)[idx]
    box = None if c.box is None else c.box.astype(np.float64)
    nb, d, dist = NN.reference_neighbors(pos, c.batch[idx], False, False, float(np.float32(c.up)), box, float(np.float32(c.lo)))
    a, b = idx[nb[0]], idx[nb[1]]
    sign = np.where(a > b, 1.0, -1.0)
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    o = np.lexsort((lo, hi))
    return hi[o], lo[o], (d * sign[:, None])[o], dist[o]


@pytest.mark.parametrize("name", list(G.CASES))
def test_specification_agrees_with_the_reference_statement(name):
    c = G.CASES[name]
    hi_r, lo_r, d_r, dist_r = _reference_pairs(c)
    for cell in ([None] if c.cell is None else [None, c.cell]):
        s = G.spec_of(c, cell)
        if c.weights is not None and cell is not None:  # ghost-ghost pairs are left out
            keep = ~((c.weights[hi_r] == 0) & (c.weights[lo_r] == 0))
            hi_r, lo_r, d_r, dist_r = hi_r[keep], lo_r[keep], d_r[keep], dist_r[keep]
        hi, lo, sign, o = O.pair_set_original(s, s.get("perm"))
        assert np.array_equal(hi, hi_r) and np.array_equal(lo, lo_r), (name, cell, len(hi), len(hi_r))
        assert np.abs(s["pdelta"][o] * sign[:, None] - d_r).max(initial=0.0) < 1e-12
        assert np.abs(s["pd"][:-1][o] - dist_r).max(initial=0.0) < 1e-12 and s["pd"][-1] == 0.0
        # the structure the sweeps rely on, of the specification itself
        P, E = int(s["counts"][0]), int(s["counts"][1])
        assert s["rowptr"][-1] == E == len(s["col"]) and s["pairptr"][-1] == P == len(s["pair_i"])
        assert np.all(s["pair_i"] > s["pair_j"]) and np.array_equal(np.bincount(s["epair"], minlength=P + 1)[:P], np.full(P, 2))
        unit = np.linalg.norm(s["prhat"], axis=1)
        assert np.all((np.abs(unit - 1.0) < 1e-12) | ((unit == 0) & (s["pd"][:-1] == 0)))


@pytest.mark.parametrize("name", list(G.CASES))
def test_no_case_has_a_borderline_decision(name):
    c = G.CASES[name]
    for cell in ([None] if c.cell is None else [None, c.cell]):
        m = G.spec_of(c, cell)["margins"]
        if c.borderline_ok:  # the exactly representable case: ON the cutoff in float64 and in fp32 alike
            assert m["exact_cut"] > 0 and m["cut"] > 1e-2 and np.all(c.pos == np.round(c.pos))
            continue
        assert m["exact_cut"] == 0 and not m["offenders"], (name, m)
        assert m["cut"] > O.TOL_CUT and m["round"] > O.TOL_ROUND and m["cell"] > O.TOL_CELL and m["grid"] > 1e-3, (name, m)
        assert (m["on_face"] > 0) == (name == "cell_faces" and cell is not None)


def test_exact_case_pins_both_cutoffs():
    up, lo = G.spec_of(G.CASES["exact_upper"]), G.spec_of(G.CASES["exact_lower"])
    pairs = lambda s: set(zip(s["pair_i"].tolist(), s["pair_j"].tolist()))  # noqa: E731
    assert (1, 0) not in pairs(up) and (3, 0) not in pairs(up) and (2, 0) in pairs(up)  # d == up is out
    assert (1, 0) in pairs(lo) and (3, 0) in pairs(lo) and (5, 1) in pairs(lo) and (2, 0) not in pairs(lo)  # d == lo is in


def test_case_list_reaches_every_branch():
    """host-side census: what each kernel branch needs, found in the specification of at least one case"""
    C, S = G.CASES, {n: G.spec_of(c) for n, c in G.CASES.items()}
    brute = [C[n] for n in G.BRUTE]
    seen = set()
    for c in brute:
        s = S[c.name]
        sizes = np.bincount(c.batch[(c.batch >= 0) & (c.batch < c.n_mol)], minlength=c.n_mol)
        used = np.flatnonzero(sizes)
        if "mstart" in s and np.any(s["mstart"][used] % 64):
            seen.add("range off a multiple of 64")
        if np.any(sizes == 1):
            seen.add("one-atom molecule")
        if c.name == "ladder_1_to_70":
            assert set(sizes % 64) == set(range(64))  # every tail of the 64-lane candidate loop
            seen.add("every tail")
        if s["ntot"].max(initial=0) > 64 and c.n_mol == 1:
            seen.add("two ballot passes")
        if int(s["counts"][0]) and s["pd"][:-1].min() == 0:
            seen.add("coincident")
        if len(used) and np.any(sizes[: used[-1]] == 0) and sizes[-1] == 0:
            seen.add("empty molecules")
        if s["counts"][3] and not s["counts"][5]:
            seen.add("unsorted N<=256" if c.n <= 256 else "unsorted")
        seen.add(f"box mode {c.box_mode}")
        if c.box_mode == 1 and abs(c.box[1, 0]) >= 0.44 * c.box[0, 0] and abs(c.box[2, 1]) >= 0.44 * c.box[1, 1] and abs(c.box[2, 0]) >= 0.39 * c.box[0, 0]:
            seen.add("large skew")
            if c.pos.min() < -2 * c.box[0, 0] and c.pos.max() > 2 * c.box[0, 0]:
                seen.add("outside the box")
        if c.lo > 0:
            seen.add("lower cutoff")
        if c.n > 8192:
            seen.add("scan tile carry")
        if c.static and c.n_mol == 1 and c.z is None:
            seen.add(f"static N={c.n}")
        if c.static and c.n == 256 and c.n_mol == 4:
            seen.add("static 256 as four molecules")
        if c.static and c.n <= 256 and c.n_mol > 256:
            seen.add("mol_lds false")
        if c.static and c.n <= 256 and s["ecap"] > 16384:
            seen.add("col_lds false")
        if c.z is not None and s["counts"][4]:
            seen.add("z out of range N<=256" if c.n <= 256 else "z out of range")
        if c.z is not None and not s["counts"][4]:
            seen.add("z")
        if s["counts"][5]:
            seen.add("batch out of range")
        if s["counts"][1] == s["ecap"]:
            assert not s["counts"][2]
            seen.add("E == ecap")
        if s["counts"][1] == s["ecap"] + 1:
            assert s["counts"][2]
            seen.add("E == ecap + 1")
    need = {"range off a multiple of 64", "one-atom molecule", "every tail", "two ballot passes", "coincident", "empty molecules", "unsorted",
            "unsorted N<=256", "box mode 0", "box mode 1", "box mode 2", "large skew", "outside the box", "lower cutoff", "scan tile carry",
            "static 256 as four molecules", "mol_lds false", "col_lds false", "z", "z out of range", "z out of range N<=256",
            "batch out of range", "E == ecap", "E == ecap + 1"} | {f"static N={n}" for n in (1, 63, 64, 65, 255, 257)}
    assert need <= seen, sorted(need - seen)
    seen = set()
    for n in G.CELL:
        c, s = C[n], S[n]
        assert s["route_cell"], n
        g = tuple(int(v) for v in s["cgrid"][:3])
        seen.add(("auto" if c.cell == "auto" else "explicit", g))
        if s["cgrid"][3] > 1024:
            seen.add("more than 1024 cells")
        if np.bincount(s["cell_key_sorted"]).max() > 64:
            seen.add("more than 64 atoms in a cell")
        if c.cell == "auto" and c.box is not None and g[0] < int(c.box[0, 0] / c.up) and g[0] == O.grid_cap(c.n):
            seen.add("ncap clamp")
        if c.box is not None and abs(c.box[1, 0]) >= 0.44 * c.box[0, 0]:
            seen.add("skew")
        if s["margins"]["on_face"] and np.any((c.pos < 0) & (c.pos > -1e-6)):
            seen.add("faces and a hair below zero")
        if c.box is not None and c.pos.min() < -2 * c.box[0, 0]:
            seen.add("outside the box")
        if c.n_mol > 1 and s["counts"][3] == 1 and "bat_c" in s:
            seen.add("several molecules")
        if c.box_mode == 0:
            seen.add("no box")
        if c.z is not None:
            seen.add("z")
        if c.weights is not None and 0 < (c.weights == 0).sum() < c.n:
            seen.add("ghosts")
        if min(g) < 3 and int(s["counts"][0]) > 0:
            seen.add("axis with fewer than three cells")
    need = {("explicit", g) for g in ((1, 1, 1), (1, 2, 3), (2, 2, 2), (3, 3, 3), (4, 5, 3), (11, 11, 11))} | {
        ("auto", (4, 5, 3)), ("auto", (11, 11, 11)), "more than 1024 cells", "more than 64 atoms in a cell", "ncap clamp", "skew",
        "faces and a hair below zero", "outside the box", "several molecules", "no box", "z", "ghosts", "axis with fewer than three cells"}
    assert need <= seen, sorted(map(str, need - seen))
    # small systems: only the scan case (8193 atoms) and the full molecule ladder (1 + 2 + ... + 70 = 2485 atoms) are above 700 atoms
    assert max(c.n for c in C.values() if c.name != "scan_8193" and c.name != "ladder_1_to_70") <= 700


def test_accessor_is_declared_and_bound():
    from torchmdnet_amd import _C

    assert "tmdnet_debug_graph" in _C.declared_symbols()
    assert int(__import__("re").search(r"TMDNET_ABI_VERSION\s+(\d+)", open(_C.HEADER_PATH).read()).group(1)) == 10  # additive
