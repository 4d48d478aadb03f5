"""The workspace layouts of the captured loops are ABI: Python reads some of them at fixed byte offsets (DeviceCellMD.matrices,
DeviceBiasedMD._hill_store, DeviceGlobalMD._stage_thermostat, the L-BFGS class through tmdnet_lbfgs_layout), so every size entry
must keep returning what it returned when tests/golden/loop_layouts.json was recorded (output of this project's own library,
before the layouts moved onto the Carver of csrc/tn_loop.h).  No GPU: the size entries are host code.

`python -m tests.test_loop_layouts` rewrites the table from the library in the tree (only when an entry changes on purpose)."""
import ctypes as C
import itertools
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_layouts.json")

ATOMS = (0, 1, 1024, 1025, 300000)
MOLS = (1, 3, 300)  # 1 024 B is below, between and above the atom counts: one slice, several, and the cap of 256


def _nb():
    return list(itertools.product(ATOMS, MOLS)) + [(3 * 1024, 3), (3 * 1024 + 1, 3), (0, 0), (10 ** 6, 1), (2 ** 29 - 1, 1)]


def cases():
    """(entry, arguments) of every size entry of the loops, each with its extra arguments at their extremes"""
    out = []
    for n, b in _nb():
        for entry in ("md", "md_barostat_cell", "committee", "min", "min_cell"):
            out.append((entry, (n, b)))
        for memory in (1, 7, 512):
            out.append(("lbfgs", (n, b, memory)))
            out.append(("lbfgs_layout", (n, b, memory)))
    for b in (0,) + MOLS + (2 ** 27 - 1,):
        out.append(("md_barostat", (b,)))
        for chain in (0, 1, 8):
            out.append(("md_thermostat", (b, chain)))
    for n, clusters, cons in ((0, 0, 0), (1025, 1, 12), (300000, 100000, 1200000)):
        out.append(("md_constraints", (n, clusters, cons)))
    for b, ladder in ((2, 2), (300, 2), (300, 300), (300, 3), (2 ** 27 - 2, 2)):
        out.append(("md_exchange", (b, ladder)))
    for b, n_cv, dm, w, cap in ((1, 1, 0, 1, 0), (3, 8, 0, 1, 0), (3, 1, 1, 1, 1), (300, 8, 2, 1, 1000), (300, 8, 2, 300, 300),
                                (300, 2, 1, 3, 10 ** 6), (1, 2, 2, 1, 2 ** 40)):
        out.append(("md_bias", (b, n_cv, dm, w, cap)))
    for n in ATOMS:
        for m, g in ((3, 1), (7, 3), (16, 300)):
            if n * m * g <= (2 ** 31 - 1) // 4:
                out.append(("neb", (n, m, g)))
    # the optimisers added since: one unit (a dimer, a path, a scan point, a walker) is the molecule; rows of 3 floats stay below 2^31
    for n, b in _nb():
        if b >= 1 and n * b <= (2 ** 31 - 1) // 16:
            out.append(("dimer", (n, b)))
            for capacity in (1, 4096):  # irc: its frames stay below 2^36 rows
                if n * b * capacity <= 2 ** 36:
                    out.append(("irc", (n, b, capacity)))
            if n >= 1:
                out.append(("scan", (n, b)))
        if b >= 1 and 1 <= n <= (2 ** 31 - 1) // 4:
            for capacity in (1, 64):  # hop: the rows of its ring stay below 2^31 floats
                if n * capacity <= (2 ** 31 - 1) // 4:
                    out.append(("hop", (n, b, capacity)))
    return out


_SIZE_ENTRIES = {
    "md": "tmdnet_md_workspace_bytes",
    "md_barostat": "tmdnet_md_barostat_workspace_bytes",
    "md_barostat_cell": "tmdnet_md_barostat_cell_workspace_bytes",
    "md_thermostat": "tmdnet_md_thermostat_workspace_bytes",
    "md_constraints": "tmdnet_md_constraints_workspace_bytes",
    "md_exchange": "tmdnet_md_exchange_workspace_bytes",
    "md_bias": "tmdnet_md_bias_workspace_bytes",
    "committee": "tmdnet_committee_workspace_bytes",
    "min": "tmdnet_min_workspace_bytes",
    "min_cell": "tmdnet_min_workspace_bytes_cell",
    "lbfgs": "tmdnet_lbfgs_workspace_bytes",
    "neb": "tmdnet_neb_workspace_bytes",
    "dimer": "tmdnet_dimer_workspace_bytes",
    "irc": "tmdnet_irc_workspace_bytes",
    "scan": "tmdnet_scan_workspace_bytes",
    "hop": "tmdnet_hop_workspace_bytes",
}


def evaluate(lib, entry, args):
    """what the library answers: the byte count, or the 17 offsets of tmdnet_lbfgs_layout"""
    if entry == "lbfgs_layout":
        off = (C.c_int64 * 17)()
        assert lib.tmdnet_lbfgs_layout(*args, off) == 0, (entry, args)
        return list(off)
    size = C.c_size_t(0)
    assert getattr(lib, _SIZE_ENTRIES[entry])(*args, C.byref(size)) == 0, (entry, args)
    return size.value


def table(lib):
    return [{"entry": e, "args": list(a), "value": evaluate(lib, e, a)} for e, a in cases()]


def test_every_size_entry_answers_what_it_answered(hip_lib):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert [(g["entry"], tuple(g["args"])) for g in golden] == cases()  # the table covers exactly the cases above
    for g in golden:
        assert evaluate(hip_lib, g["entry"], tuple(g["args"])) == g["value"], (g["entry"], g["args"])


def test_the_table_covers_every_entry_and_the_edges():
    c = cases()
    assert {e for e, _ in c} == set(_SIZE_ENTRIES) | {"lbfgs_layout"}
    md = {a for e, a in c if e == "md"}
    for n in ATOMS:
        for b in MOLS:
            assert (n, b) in md
    assert any(n <= 1024 * b for n, b in md) and any(n > 1024 * b for n, b in md)


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge

    ge.build_hip(verbose=False)
    from torchmdnet_amd import _C

    with open(GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(row) for row in table(_C.lib())) + "\n]\n")
    print("wrote", GOLDEN)
