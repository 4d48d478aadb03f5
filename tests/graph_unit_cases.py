"""TEST INFRASTRUCTURE ONLY -- the cases of the neighbour-graph unit tests (tests/test_gpu_graph.py on the device,
tests/test_graph_oracle.py without one), their specification (tests/graph_oracle.py, cached per case) and the few lines that
build a graph through the C entry points and read it back with tmdnet_debug_graph.

Every case is generated from a fixed seed and then NUDGED until, in float64, no candidate pair lies within relative 1e-5 of a
squared cutoff and no scaled difference within 1e-4 of a half-integer (graph_oracle.TOL_*): the integer arrays of a correct engine
then equal the specification exactly.  Atoms placed on purpose (cell faces, coincident atoms, exactly representable distances)
are `fixed` and never nudged.  `python tests/graph_unit_cases.py OUT.npz` builds the brute-force cases on the device and dumps
the arrays: the child interpreters of the developer-switch test run it."""
import functools
import os
import sys
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

if __name__ == "__main__":
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "torchmd-net_amd"), os.path.join(_ROOT, "tests")]
try:
    from tests import graph_oracle as O
except ImportError:  # run as a script from tests/
    import graph_oracle as O

MAX_Z = 20
FILL_ARRAYS = ("col", "epair", "esign", "pair_i", "pair_j", "pd", "pdelta", "prhat")  # written by the fill and link phases only
DTYPES = dict(counts=np.int32, mstart=np.int32, mend=np.int32, nlow=np.int32, ntot=np.int32, rowptr=np.int32, pairptr=np.int32,
              col=np.int32, epair=np.int32, esign=np.float32, pair_i=np.int32, pair_j=np.int32, pd=np.float32, pdelta=np.float32,
              prhat=np.float32, perm=np.int32, z_c=np.int64, bat_c=np.int64, cgrid=np.int32, boxd=np.float32,
              cell_key_sorted=np.int32, cell_start=np.int32)
SENTINEL = 0xA5


@dataclass
class Case:
    name: str
    pos: np.ndarray
    batch: np.ndarray
    n_mol: int
    up: float = 4.0
    lo: float = 0.0
    mnn: int = 128
    box: Optional[np.ndarray] = None
    box_mode: int = 0
    z: Optional[np.ndarray] = None
    cell: object = None          # None: brute force; "auto": device grid; (nx, ny, nz): explicit grid
    weights: Optional[np.ndarray] = None  # ghost weights (a no-op halo exchange is set for the build)
    static: bool = True          # also built by tmdnet_build_graph_static (and compared bit for bit with the dynamic build)
    borderline_ok: bool = False  # the exactly representable case: pairs ON a cutoff on purpose
    fixed: np.ndarray = field(default=None, repr=False)

    @property
    def n(self):
        return len(self.pos)


def spec_of(c: Case, cell="case"):
    return _spec(c.name, None if cell is None else (c.cell if cell == "case" else cell))


@functools.lru_cache(maxsize=None)
def _spec(name, cell):
    c = CASES[name]
    return O.build(c.pos, c.batch, c.n_mol, c.lo, c.up, c.mnn, c.box, c.box_mode, c.z, MAX_Z, cell,
                   c.weights if cell is not None else None)


# ------------------------------------------------------------------------------------------------ generation
def _nudge(c: Case, seed):
    """move the atoms of borderline pairs (never the fixed ones) until the specification reports none"""
    rng = np.random.default_rng(seed + 7919)
    fixed = np.zeros(c.n, dtype=bool) if c.fixed is None else c.fixed
    for _ in range(200):
        s = O.build(c.pos, c.batch, c.n_mol, c.lo, c.up, c.mnn, c.box, c.box_mode, None, MAX_Z, None)
        off = np.array(sorted(s["margins"]["offenders"]), dtype=np.int64)
        if c.cell is not None and not len(off):  # the cell route: no atom within TOL_CELL of an interior cell face either
            s = O.build(c.pos, c.batch, c.n_mol, c.lo, c.up, c.mnn, c.box, c.box_mode, None, MAX_Z, c.cell)
            if s["route_cell"]:
                grid, boxd = s["cgrid"].astype(np.int64), s["boxd"]
                p = c.pos.astype(np.float64)
                bad = np.zeros(c.n, dtype=bool)
                for i in range(c.n):
                    m = O.new_margins()
                    O.cell_keys(p[i:i + 1], boxd, grid, m)
                    bad[i] = m["cell"] < O.TOL_CELL
                off = np.flatnonzero(bad & ~fixed)
        off = off[~fixed[off]] if len(off) else off
        if not len(off):
            return c
        c.pos[off] += rng.uniform(-0.02, 0.02, size=(len(off), 3)).astype(np.float32)
    raise AssertionError(f"case {c.name}: could not be nudged away from the borderline")


def _blob(rng, n, density=0.1, centre=(0.0, 0.0, 0.0)):
    edge = (n / density) ** (1.0 / 3.0)
    return (rng.uniform(-0.5, 0.5, size=(n, 3)) * edge + np.asarray(centre)).astype(np.float32)


def _in_box(rng, n, box):
    return (rng.uniform(0.0, 1.0, size=(n, 3)) @ np.asarray(box, dtype=np.float64)).astype(np.float32)


def _mols(rng, sizes, density=0.1, spread=30.0):
    pos = [_blob(rng, k, density, rng.uniform(-spread, spread, size=3)) for k in sizes]
    return np.concatenate(pos), np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)


ORTHO = np.diag([9.0, 10.0, 11.0]).astype(np.float32)
SKEW = np.array([[10.0, 0, 0], [4.5, 10.0, 0], [4.0, 4.5, 10.0]], dtype=np.float32)       # |bx| = .45 ax, |cx| = .4 ax, |cy| = .45 by
CELL_BOX = np.diag([12.5, 15.5, 9.5]).astype(np.float32)                                    # floor(w / 3) = 4 x 5 x 3
CELL_SKEW = np.array([[13.0, 0, 0], [5.85, 13.0, 0], [5.2, 5.85, 13.0]], dtype=np.float32)


def _make_cases():
    cases = []

    def add(name, pos, batch, n_mol, seed, **kw):
        c = Case(name, np.ascontiguousarray(pos, dtype=np.float32), np.asarray(batch, dtype=np.int64), n_mol, **kw)
        if not c.borderline_ok:
            _nudge(c, seed)
        cases.append(c)
        return c

    R = np.random.default_rng
    # ---- brute force
    pos, bat = _mols(R(1), list(range(1, 71)))
    add("ladder_1_to_70", pos, bat, 70, 1)
    add("dense100", (R(2).uniform(0, 5.0, size=(100, 3))), np.zeros(100), 1, 2)
    pos = _blob(R(3), 20)
    pos[7] = pos[3]; pos[11] = pos[3]; pos[19] = pos[18]
    fx = np.zeros(20, dtype=bool); fx[[3, 7, 11, 18, 19]] = True
    add("coincident", pos, np.zeros(20), 1, 3, fixed=fx)
    pos, bat = _mols(R(4), [9, 14, 5, 11])
    add("empty_molecules", pos, np.array([0, 2, 3, 5])[bat], 7, 4)
    pos, bat = _mols(R(5), [20, 20, 20])
    o = np.arange(60).reshape(3, 20).T.reshape(-1)
    add("unsorted_batch", pos[o], bat[o], 3, 5)
    pos, bat = _mols(R(55), [100, 100, 100])
    o = np.arange(300).reshape(3, 100).T.reshape(-1)
    add("unsorted_300", pos[o], bat[o], 3, 55)  # above the small-system kernel: the general kernels of the static build
    add("box_ortho", _in_box(R(6), 90, ORTHO), np.zeros(90), 1, 6, box=ORTHO, box_mode=1)
    add("box_skew", _in_box(R(7), 100, SKEW), np.zeros(100), 1, 7, box=SKEW, box_mode=1)
    boxes = np.stack([ORTHO, SKEW, np.diag([30.0, 30.0, 30.0]).astype(np.float32)])
    sizes = [40, 50, 30]
    pos = np.concatenate([_in_box(R(8 + k), n, boxes[k]) for k, n in enumerate(sizes)])
    add("box_per_molecule", pos, np.repeat(np.arange(3), sizes), 3, 8, box=boxes, box_mode=2)
    rng = R(9)
    pos = _in_box(rng, 80, SKEW).astype(np.float64) + rng.integers(-3, 4, size=(80, 3)) @ SKEW.astype(np.float64)
    add("outside_box", pos, np.zeros(80), 1, 9, box=SKEW, box_mode=1)
    pos, bat = _mols(R(10), [33, 70, 1, 17])
    add("cutoff_lower", pos, bat, 4, 10, lo=1.5)
    pos, bat = _mols(R(11), [3] * 2731, spread=60.0)
    add("scan_8193", pos, bat, 2731, 11, mnn=8)
    # exactly representable distances: d^2 == up^2 is out, d^2 == lo^2 is in
    pts = np.array([[0, 0, 0], [3, 4, 0], [0, 0, 3], [0, -5, 0], [3, 4, 12], [6, 8, 0]], dtype=np.float32)
    add("exact_upper", pts, np.zeros(6), 1, 0, up=5.0, borderline_ok=True)
    add("exact_lower", pts, np.zeros(6), 1, 0, lo=5.0, up=8.0, borderline_ok=True)
    # ---- the one-launch small-system kernel of the static build and its thresholds
    for n in (1, 63, 64, 65, 255, 257):
        add(f"small_{n}", _blob(R(20 + n), n), np.zeros(n), 1, 20 + n)
    pos, bat = _mols(R(30), [64, 64, 64, 64], spread=8.0)
    add("small_256_four_molecules", pos, bat, 4, 30)
    pos, bat = _mols(R(31), [10, 13, 7, 10])
    add("small_300_slots", pos, np.array([2, 130, 257, 299])[bat], 300, 31)
    add("small_256_mnn65", _blob(R(32), 256), np.zeros(256), 1, 32, mnn=65)
    pos, bat = _mols(R(33), [15, 15])
    o = np.arange(30).reshape(2, 15).T.reshape(-1)
    add("small_unsorted", pos[o], bat[o], 2, 33)
    z = R(34).integers(1, MAX_Z, size=40)
    add("small_z", _blob(R(34), 40), np.zeros(40), 1, 34, z=z)
    zb = z.copy(); zb[5] = MAX_Z; zb[17] = -3; zb[39] = 1000
    add("small_z_out_of_range", _blob(R(35), 40), np.zeros(40), 1, 35, z=zb)
    bat = np.zeros(30, dtype=np.int64); bat[15:] = 1; bat[22] = 2; bat[4] = -1
    add("small_batch_out_of_range", _blob(R(36), 30), bat, 2, 36)
    add("general_z_out_of_range", _blob(R(37), 300), np.zeros(300), 1, 37, z=np.concatenate([zb, R(37).integers(1, MAX_Z, size=260)]))
    # overflow: a cube of edge 3 (12 pairs below 4, face diagonals above): E = 2 * 12 + 8 = 32 = ecap for max_num_neighbors 4;
    # a ninth atom over the middle of one edge adds two pairs: E = 2 * 14 + 9 = 37 = ecap + 1
    cube = np.array([[x, y, zc] for x in (0, 3) for y in (0, 3) for zc in (0, 3)], dtype=np.float32) + np.float32(0.25)
    add("overflow_E_equals_ecap", cube, np.zeros(8), 1, 0, mnn=4, fixed=np.ones(8, dtype=bool))
    h = 2.0 / np.sqrt(2.0)
    nine = np.concatenate([cube, np.array([[1.75, 0.25 - h, 0.25 - h]], dtype=np.float32)])
    add("overflow_E_equals_ecap_plus_1", nine, np.zeros(9), 1, 0, mnn=4, fixed=np.ones(9, dtype=bool))
    # ---- cell list (cutoff 3)
    p300 = _in_box(R(40), 300, CELL_BOX)
    for g in ("auto", (1, 1, 1), (1, 2, 3), (2, 2, 2), (3, 3, 3), (4, 5, 3)):
        tag = "auto" if g == "auto" else "x".join(map(str, g))
        add(f"cell_{tag}", p300.copy(), np.zeros(300), 1, 40, up=3.0, box=CELL_BOX, box_mode=1, cell=g, z=R(41).integers(1, MAX_Z, size=300))
    big = np.diag([33.5, 33.5, 33.5]).astype(np.float32)
    p600 = _in_box(R(42), 600, big)
    add("cell_11x11x11", p600.copy(), np.zeros(600), 1, 42, up=3.0, box=big, box_mode=1, cell=(11, 11, 11))
    add("cell_11x11x11_auto", p600.copy(), np.zeros(600), 1, 42, up=3.0, box=big, box_mode=1, cell="auto")
    b8 = np.diag([8.0, 8.0, 8.0]).astype(np.float32)
    pos = np.concatenate([R(43).uniform(0.2, 3.8, size=(90, 3)), _in_box(R(44), 30, b8)])
    add("cell_crowded", pos, np.zeros(120), 1, 43, up=3.0, box=b8, box_mode=1, cell=(2, 2, 2))
    b40 = np.diag([40.0, 40.0, 40.0]).astype(np.float32)
    pos = np.concatenate([R(45).uniform(1.0, 4.5, size=(5, 3)), R(45).uniform(20.0, 39.0, size=(3, 3))])
    add("cell_ncap_clamp", pos, np.zeros(8), 1, 45, up=3.0, box=b40, box_mode=1, cell="auto")
    add("cell_skew", _in_box(R(46), 350, CELL_SKEW), np.zeros(350), 1, 46, up=3.0, box=CELL_SKEW, box_mode=1, cell="auto")
    # atoms exactly on cell faces (box 16, 4 x 4 x 4: faces at 4, 8, 12), on the box face and a hair below zero (the wrapped fractional
    # coordinate rounds to 1.0 in fp32 and must be clamped into the last cell); no two placed coordinates half a box apart
    b16 = np.diag([16.0, 16.0, 16.0]).astype(np.float32)
    pos = _in_box(R(47), 200, b16)
    pos[0, 0] = 4.0; pos[1, 1] = 8.0; pos[2, 2] = 12.0; pos[3, 0] = 4.0; pos[3, 1] = 8.0
    pos[4, 0] = 16.0; pos[5, 0] = -1e-9; pos[6, 2] = -1e-9; pos[7] = (-1e-9, 3.3, -1e-9)
    fx = np.zeros(200, dtype=bool); fx[:8] = True
    add("cell_faces", pos, np.zeros(200), 1, 47, up=3.0, box=b16, box_mode=1, cell=(4, 4, 4), fixed=fx)
    rng = R(48)
    pos = p300.astype(np.float64) + rng.integers(-3, 4, size=(300, 3)) * np.diag(CELL_BOX).astype(np.float64)
    add("cell_outside_box", pos, np.zeros(300), 1, 48, up=3.0, box=CELL_BOX, box_mode=1, cell="auto")
    add("cell_three_molecules", p300.copy(), R(49).integers(0, 3, size=300), 3, 49, up=3.0, box=CELL_BOX, box_mode=1, cell="auto",
        z=R(50).integers(1, MAX_Z, size=300))
    add("cell_no_box", _blob(R(51), 300, density=0.15), np.zeros(300), 1, 51, up=3.0, cell="auto")
    add("cell_ghosts", p300.copy(), np.zeros(300), 1, 52, up=3.0, box=CELL_BOX, box_mode=1, cell="auto", static=False,
        weights=(R(52).uniform(size=300) > 0.3).astype(np.float32))
    return {c.name: c for c in cases}


CASES = _make_cases()
BRUTE = [n for n, c in CASES.items() if c.cell is None]
CELL = [n for n, c in CASES.items() if c.cell is not None]
SWITCH_CASES = [n for n in BRUTE if not n.startswith("overflow")]  # rebuilt by the children of the developer-switch test


# ------------------------------------------------------------------------------------------------ the device side
class Engine:
    """bare model handles (the weights are irrelevant to the graph), one per (cutoffs, max_num_neighbors)"""

    def __init__(self):
        import ctypes as C

        import torch
        from torchmdnet_amd import _C

        self.C, self.torch, self._C, self.L = C, torch, _C, _C.lib()
        self.handles = {}
        self.noop = _C.HALO_EXCHANGE_FN(lambda *a: 0)

    def handle(self, c: Case):
        key = (c.lo, c.up, c.mnn)
        if key not in self.handles:
            hp = self._C.HParams(hidden_channels=32, num_layers=1, num_rbf=8, max_z=MAX_Z, max_num_neighbors=c.mnn, group_o3=1,
                                 head_hidden=16, has_atomref=0, cutoff_lower=c.lo, cutoff_upper=c.up)
            h = self.C.c_void_p()
            assert self.L.tmdnet_create(self.C.byref(hp), self.C.byref(h)) == 0
            self.handles[key] = h
        return self.handles[key]

    def close(self):
        for h in self.handles.values():
            self.L.tmdnet_destroy(h)
        self.handles = {}

    def stream(self):
        return self.C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def build(self, c: Case, static=False, cell="case", slack=4096):
        """-> dict: rc, counts_host, rc_counts, arrays (numpy, whole capacity), tail (bytes behind the reported size), grid"""
        C, torch, L = self.C, self.torch, self.L
        h = self.handle(c)
        cell = c.cell if cell == "case" else cell
        g = (0, 0, 0) if cell is None else ((-1, -1, -1) if cell == "auto" else cell)
        assert L.tmdnet_set_cell_grid(h, *g) == 0
        dev = "cuda"
        pos = torch.from_numpy(c.pos).to(dev)
        bat = torch.from_numpy(c.batch).to(dev)
        z = None if c.z is None else torch.from_numpy(np.asarray(c.z, dtype=np.int64)).to(dev)
        box = None if c.box is None else torch.from_numpy(np.ascontiguousarray(c.box, dtype=np.float32)).to(dev)
        w = None if (c.weights is None or cell is None) else torch.from_numpy(c.weights).to(dev)
        need = C.c_size_t()
        assert L.tmdnet_graph_workspace_bytes(h, c.n, c.n_mol, C.byref(need)) == 0
        ws = torch.full((need.value + slack,), SENTINEL, dtype=torch.uint8, device=dev)
        ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
        if w is not None:
            L.tmdnet_set_halo_exchange(h, self.noop, None)
            L.tmdnet_set_atom_weights(h, ptr(w))
        counts = (C.c_int64 * 8)()
        try:
            if static:
                rc = L.tmdnet_build_graph_static(h, self.stream(), ptr(ws), need.value, c.n, c.n_mol, ptr(pos), ptr(bat), ptr(z), ptr(box),
                                                 c.box_mode)
            else:
                rc = L.tmdnet_build_graph(h, self.stream(), ptr(ws), need.value, c.n, c.n_mol, ptr(pos), ptr(bat), ptr(z), ptr(box),
                                          c.box_mode, counts)
        finally:
            if w is not None:
                L.tmdnet_set_halo_exchange(h, self._C.HALO_EXCHANGE_FN(), None)
                L.tmdnet_set_atom_weights(h, None)
        assert rc in (self._C.OK, self._C.ERR_INVALID, self._C.ERR_OVERFLOW), (c.name, rc, L.tmdnet_last_error(h))
        cnt2 = (C.c_int64 * 8)()
        rc_counts = L.tmdnet_graph_counts(h, self.stream(), ptr(ws), c.n, c.n_mol, cnt2)
        grid = (C.c_int64 * 4)()
        assert L.tmdnet_graph_cell_grid(h, self.stream(), ptr(ws), c.n, c.n_mol, grid) == 0
        arrays = {name: self.read(h, ws, c.n, c.n_mol, name, c.mnn) for name in DTYPES}
        torch.cuda.synchronize()
        return dict(rc=rc, counts_host=np.array(list(counts)), rc_counts=rc_counts, counts_query=np.array(list(cnt2)), arrays=arrays,
                    tail=ws[need.value:].cpu().numpy(), grid=tuple(int(v) for v in grid), ws=ws, need=need.value)

    def sizes(self, n, b, mnn):
        ecap = mnn * n
        pcap = ecap // 2 + 1
        return dict(counts=8, mstart=b, mend=b, nlow=n, ntot=n, rowptr=n + 1, pairptr=n + 1, col=ecap, epair=ecap, esign=ecap,
                    pair_i=pcap, pair_j=pcap, pd=pcap + 1, pdelta=3 * pcap, prhat=3 * pcap, perm=n, z_c=n, bat_c=n, cgrid=4, boxd=12,
                    cell_key_sorted=n, cell_start=8 * n + 2)

    def read(self, h, ws, n, b, name, mnn, numel=None):
        torch, C = self.torch, self.C
        numel = self.sizes(n, b, mnn)[name] if numel is None else numel
        dt = np.dtype(DTYPES[name])
        out = torch.zeros(max(numel, 1) * dt.itemsize, dtype=torch.uint8, device="cuda")
        rc = self.L.tmdnet_debug_graph(h, self.stream(), C.c_void_p(ws.data_ptr()), n, b, name.encode(), C.c_void_p(out.data_ptr()),
                                       numel * dt.itemsize)
        assert rc == 0, (name, rc, self.L.tmdnet_last_error(h))
        return out.cpu().numpy()[: numel * dt.itemsize].view(dt).copy()


def dump_brute(path):
    eng = Engine()
    out = {}
    for name in SWITCH_CASES:
        c = CASES[name]
        for static in ([False] if not c.static else [False, True]):
            r = eng.build(c, static=static, cell=None)
            for k, v in r["arrays"].items():
                out[f"{name}/{int(static)}/{k}"] = v
            out[f"{name}/{int(static)}/rc"] = np.array([r["rc"], r["rc_counts"]])
    eng.close()
    np.savez(path, **out)
    print("GRAPH_DUMP_OK")


if __name__ == "__main__":
    dump_brute(sys.argv[1])
