"""TEST INFRASTRUCTURE ONLY -- the cases of the kernel-level unit tests of the fused tensor linears (tmdnet_debug_tlin9) and of
the GEMM family (tmdnet_debug_gemm_ex): shapes, inputs, launches and the figures the tests assert on.  One statement of the
cases serves three users: tests/test_gpu_tlin9.py and tests/test_gpu_gemm_epilogues.py (assert), and
tools/tlin9_gemm_unit_floor.py (measures the fp32 rounding floor of the reference on these very inputs without a device, and the
errors observed on the device, into profiles/tlin9_gemm_unit_floor.json, from which the tests read their bounds).
"""
import ctypes as C
import json
import os

import torch

from tests import tlin9_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR_JSON = os.path.join(ROOT, "profiles", "tlin9_gemm_unit_floor.json")
SENTINEL = 0x7FC0BEEF  # a quiet NaN with a payload: what an output must still hold where the kernel may not write
TAIL = 64              # sentinel atoms / rows behind the last one
BOUND_MIN, BOUND_FACTOR, BOUND_CAP = 2e-6, 4.0, 1e-5
DEFAULT_CUS = 256      # MI355X; the device-less floor run sizes the CU-dependent shapes with it


def bound_of(floor):
    """max(2e-6, 4 x floor): 2e-6 is the project's bound for plain and silu products (test_mfma_gemm_unit); the factor covers another
    summation order (split-K waves, MFMA k-pair order, six-product split) and the rcp / __expf sigmoid.  Never above 1e-5: a floor
    that needs more means badly conditioned inputs, and those are to be tamed instead."""
    b = max(BOUND_MIN, BOUND_FACTOR * floor)
    assert b <= BOUND_CAP, f"rounding floor {floor:.3g} of the reference alone needs a bound above {BOUND_CAP}: tame the inputs"
    return b


def load_bounds():
    with open(FLOOR_JSON) as fh:
        return json.load(fh)


def sentinel(shape, device):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=device).view(torch.float32)


def bits(t):
    return t.view(torch.int32)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ====================================================================================== fused tensor linears
def tlin9_shapes(n_cu=DEFAULT_CUS):
    """(N, F): the smallest sizes that reach each mechanism of k_tlin9 (tile = 32 atoms x 128 channels, epilogue groups of 8 atoms,
    one persistent block per compute unit)."""
    return [
        (1, 128),    # a single clamped row
        (31, 128), (32, 128), (33, 128),  # tile boundary on both sides
        (77, 256),   # two column tiles, a partial epilogue group of 8
        (40, 384),   # three column tiles
        (32 * (n_cu // 2) + 41, 256),  # more tiles than compute units, partial last tile: a block walks a second tile
    ]


def tlin9_variants(name):
    """(random_kap, want_feat, alias) of each launch of a case."""
    if name == "update":
        return [(False, 1, False), (True, 1, False), (True, 0, False)]
    if name == "updbwd":
        return [(False, 1, False), (True, 1, False)]
    if name == "normbwd":
        return [(False, 1, False), (False, 1, True)]  # alias: C is e1, as in the reverse pass where both are G
    return [(False, 1, False)]


def tlin9_seed(name, N, F):
    return 100003 * list(O.COMBOS).index(name) + 131 * N + F


def tlin9_floor(name, N, F, random_kap):
    """per-output rounding floor: the reference in float32 against itself in float64, on the case's own fp32 inputs (CPU)."""
    t, Ws, kap = O.make_inputs(name, N, F, tlin9_seed(name, N, F), random_kap)
    lo = O.reference(name, t, Ws, kap)
    hi = O.reference(name, {k: v.double() for k, v in t.items()}, tuple(w.double() for w in Ws), None if kap is None else kap.double())
    return {k: O.per_atom_rel_err(lo[k], hi[k]) for k in hi}


def tlin9_scratch(lib, F, device):
    n = C.c_int64(0)
    rc = lib.tmdnet_debug_tlin9(None, 0, 0, 1, F, *([None] * 11), 0, None, None, None, None, C.byref(n))
    assert rc == 0 and n.value == 3 * 3 * F * F
    return torch.empty(n.value, dtype=torch.int16, device=device), n


def run_tlin9(lib, name, N, F, random_kap, want_feat=1, alias=False, device="cuda"):
    """Launch one case twice and return its figures: dict(err={output: per-atom rel err}, tail_ok, undefined_ok, deterministic)."""
    t, Ws, kap = O.make_inputs(name, N, F, tlin9_seed(name, N, F), random_kap)
    td = {k: v.to(device).contiguous() for k, v in t.items()}
    Wd = tuple(w.to(device).contiguous() for w in Ws)
    kd = None if kap is None else kap.to(device)
    ref = O.reference(name, {k: v.double() for k, v in td.items()}, tuple(w.double() for w in Wd), None if kd is None else kd.double())
    defined = dict(O.WRITES[name])
    if name == "update" and not want_feat:
        defined.pop("o2")
    comps = {"C": 9, "o1": O.WRITES[name].get("o1", 9), "o2": 3}
    scratch, n_scratch = tlin9_scratch(lib, F, device)
    pro, epi = O.COMBOS[name]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        out = {k: sentinel((N + TAIL, c, F), device) for k, c in comps.items()}
        ops = dict(td)
        if alias:
            out["C"][:N] = td["e1"]
            ops["e1"] = out["C"]
        rc = lib.tmdnet_debug_tlin9(stream, pro, epi, N, F, _p(ops["A"]), _p(ops.get("A2")), _p(out["C"]), _p(ops.get("e0")),
                                    _p(ops.get("e1")), _p(ops.get("e2")), _p(ops.get("e3")), _p(ops.get("e4")), _p(out["o1"]),
                                    _p(out["o2"]), _p(kd), want_feat, _p(Wd[0]), _p(Wd[1]), _p(Wd[2]), _p(scratch), C.byref(n_scratch))
        assert rc == 0, f"tmdnet_debug_tlin9 returned {rc}"
        torch.cuda.synchronize()
        return out

    a, b = launch(), launch()
    res = {"err": {k: O.per_atom_rel_err(a[k][:N], ref[k]) for k in defined}}
    res["tail_ok"] = all(bool((bits(a[k][N:]) == SENTINEL).all()) for k in a)
    res["undefined_ok"] = all(bool((bits(a[k]) == SENTINEL).all()) for k in a if k not in defined)
    res["deterministic"] = all(bool(torch.equal(bits(a[k]), bits(b[k]))) for k in a)
    return res


# ====================================================================================== GEMM family
ROUTE_NAMES = ["none", "skinny4", "skinny8", "tiles_128x128", "tiles_128x64", "tiles_128x32", "sb1_128", "sb1_64"]
# name -> (flags, pre saved): the seven epilogue kinds of epi_kind() and one mixed flag set of the generic one
EPILOGUES = {
    "plain": (0, False),
    "silu_pre": (O.GEMM_ACT_SILU, True),
    "silu_pre_rowscale": (O.GEMM_ACT_SILU | O.GEMM_ROWSCALE, True),
    "mulaux_pre": (O.GEMM_MUL_AUX, True),
    "muldsilu": (O.GEMM_MUL_DSILU_AUX, False),
    "accum": (O.GEMM_ACCUM, False),
    "generic_silu_nopre": (O.GEMM_ACT_SILU, False),  # silu without a saved pre-activation is no specialised kind
    "generic_mixed": (O.GEMM_ACT_SILU | O.GEMM_ROWSCALE | O.GEMM_ACCUM, True),
}
EXTREMES = [30.0, -30.0, 88.0, -88.0, 1e4, -1e4, 0.5]  # ends of the activation range (and one ordinary value)


def gemm_cases(n_cu=DEFAULT_CUS):
    """route -> [(layout, M, N, K)]: the smallest shapes that reach each kernel.  Layouts: g1 one group with padded leading
    dimensions; g3 three groups side by side; g3u the same with offsets that are no multiples of 4 (guarded scalar loads; split
    images are offered and must be declined); g9 the [M, 9, F] interleaved layout of the tensor linears (N = K = F).
    fp32 routes are offered no split image except in g3u; the split-bf16 routes get one per group."""
    big = max(128, n_cu)  # sb1 128-tile: at least 128 tiles and at least one per compute unit
    return {
        "skinny4": [("g1", 70, 50, 22), ("g1", 300, 128, 32), ("g1", 33, 33, 8), ("g3u", 70, 48, 32), ("g9", 70, 32, 32)],
        "skinny8": [("g1", 129, 96, 384), ("g3u", 129, 96, 384), ("g9", 129, 256, 256)],
        # tiles: no split image, at least 256 tiles of 128 x BN
        "tiles_128x128": [("g1", 128 * 256 + 5, 128, 32), ("g3", 128 * 86 + 5, 128, 32), ("g3u", 128 * 86 + 5, 128, 32),
                          ("g9", 128 * 29 + 5, 128, 128)],
        "tiles_128x64": [("g1", 128 * 128 + 5, 96, 32), ("g3", 128 * 43 + 5, 96, 32), ("g3u", 128 * 43 + 5, 96, 32),
                         ("g9", 128 * 15 + 5, 96, 96)],
        "tiles_128x32": [("g1", 128 * 256 + 5, 24, 32), ("g3", 128 * 86 + 5, 24, 32), ("g3u", 128 * 86 + 5, 24, 32),
                         ("g9", 128 * 29 + 5, 24, 24)],
        "sb1_128": [("g1", 128 * big + 5, 128, 128), ("g9", 128 * ((big + 8) // 9) + 5, 128, 128)],
        # fewer 128-tiles than compute units (but at least 128): the 64 x 64 half-tile kernel
        "sb1_64": [("g1", 128 * 128 + 5, 128, 128), ("g9", 128 * 15 + 5, 128, 128)],
    }


def gemm_layout(layout, N, K):
    pad = 8
    if layout == "g1":
        return dict(groups=1, wmap=[0], a_off=[0], lda=K + pad, c_off=[0], ldc=N + pad, pre_off=[0], ldpre=N + pad, aux_off=[0],
                    ldaux=N + pad, no_bias=[])
    if layout == "g3":
        g = range(3)
        return dict(groups=3, wmap=[0, 1, 2], a_off=[i * K for i in g], lda=3 * K + pad, c_off=[i * N for i in g], ldc=3 * N + pad,
                    pre_off=[i * N for i in g], ldpre=3 * N + pad, aux_off=[i * N for i in g], ldaux=3 * N + pad, no_bias=[1])
    if layout == "g3u":
        g = range(3)
        return dict(groups=3, wmap=[0, 1, 2], a_off=[1 + i * (K + 1) for i in g], lda=3 * (K + 1) + 2,
                    c_off=[1 + i * (N + 1) for i in g], ldc=3 * (N + 1) + 2, pre_off=[2 + i * (N + 1) for i in g], ldpre=3 * (N + 1) + 3,
                    aux_off=[3 + i * (N + 1) for i in g], ldaux=3 * (N + 1) + 4, no_bias=[1])
    assert layout == "g9" and N == K
    F = N
    return dict(groups=9, wmap=list(O.TYPE_OF), a_off=[c * F for c in range(9)], lda=9 * F, c_off=[c * F for c in range(9)], ldc=9 * F,
                pre_off=[c * F for c in range(9)], ldpre=9 * F + pad, aux_off=[t * F for t in O.TYPE_OF], ldaux=3 * F + pad, no_bias=[])


def gemm_inputs(layout, M, N, K, extreme=False):
    """fp32 operands on the CPU: rows of A scaled by a spread over (0, 2) (as test_mfma_gemm_unit), W ~ N(0, 1/K), a bias per group.
    extreme: the bias and the aux operand hold the ends of the activation range instead."""
    lay = gemm_layout(layout, N, K)
    g = torch.Generator().manual_seed(7919 * M + 31 * N + K + 1000003 * ["g1", "g3", "g3u", "g9"].index(layout))
    rn = lambda *s: torch.randn(*s, generator=g)
    d = dict(lay=lay)
    d["A"] = rn(M, lay["lda"]) * (torch.rand(M, 1, generator=g) * 2)
    d["Wd"] = [rn(N, K) / K ** 0.5 for _ in range(max(lay["wmap"]) + 1)]  # distinct weights (g9: one per component type)
    d["bias"] = [None if i in lay["no_bias"] else rn(N) for i in range(lay["groups"])]
    d["aux"] = rn(M, lay["ldaux"])
    d["rowscale"] = torch.rand(M, generator=g) + 0.5
    d["Cold"] = rn(M, lay["ldc"])
    if extreme:
        ext = torch.tensor(EXTREMES)
        d["bias"] = [ext[(torch.arange(N) + i) % len(EXTREMES)].clone() for i in range(lay["groups"])]
        d["aux"] = ext[(torch.arange(M)[:, None] + torch.arange(lay["ldaux"])[None, :]) % len(EXTREMES)].clone()
    return d


def _window_cols(off, N, ld, device):
    m = torch.zeros(ld, dtype=torch.bool, device=device)
    for o in off:
        m[o:o + N] = True
    return m


def _gemm_reference(d, N, K, flags, want_pre, rows, dtype):
    lay = d["lay"]
    cv = lambda x: None if x is None else x.to(dtype)
    spec = dict(lay, N=N, K=K, flags=flags, want_pre=want_pre)
    return O.gemm_epilogue_reference(cv(d["A"]), [cv(d["Wd"][i]) for i in lay["wmap"]], [cv(b) for b in d["bias"]], cv(d["Cold"]),
                                     cv(d["aux"]), cv(d["rowscale"]), spec, rows)


def gemm_floor(layout, M, N, K, epi, extreme=False):
    """rounding floor of (C, pre): the reference in float32 against itself in float64 on the case's own inputs (CPU)."""
    flags, want_pre = EPILOGUES[epi]
    d = gemm_inputs(layout, M, N, K, extreme)
    lo, hi = (_gemm_reference(d, N, K, flags, want_pre, M, dt) for dt in (torch.float32, torch.float64))
    lay = d["lay"]
    out = {"C": O.per_row_rel_err(lo[0], hi[0], _window_cols(lay["c_off"], N, lay["ldc"], "cpu"))}
    if want_pre:
        out["pre"] = O.per_row_rel_err(lo[1], hi[1], _window_cols(lay["pre_off"], N, lay["ldpre"], "cpu"))
    return out


class GemmCase:
    """Device copy of one (layout, M, N, K) with its split images; run() launches one epilogue on it."""

    def __init__(self, lib, layout, M, N, K, split, extreme=False, device="cuda"):
        self.lib, self.M, self.N, self.K, self.device = lib, M, N, K, device
        d = gemm_inputs(layout, M, N, K, extreme)
        self.lay = d["lay"]
        mv = lambda x: None if x is None else x.to(device).contiguous()
        self.d = {k: ([mv(x) for x in v] if isinstance(v, list) else (v if k == "lay" else mv(v))) for k, v in d.items()}
        self.img = None
        if split:
            self.img = []
            for w in d["Wd"]:
                wh = w.contiguous()
                n = lib.tmdnet_debug_split_weight(_p(wh), N, K, None)
                im = torch.empty(n, dtype=torch.int16)
                lib.tmdnet_debug_split_weight(_p(wh), N, K, _p(im))
                self.img.append(im.to(device))
        self._ref = {}

    def reference(self, epi):
        """fp64, all M rows, computed once per epilogue and left unchanged."""
        if epi not in self._ref:
            flags, want_pre = EPILOGUES[epi]
            self._ref[epi] = _gemm_reference(self.d, self.N, self.K, flags, want_pre, self.M, torch.float64)
        return self._ref[epi]

    def run(self, epi, m_dev=None, m_add=0):
        """-> dict(route, err={C, pre}, untouched_ok, deterministic, finite, rows)."""
        from torchmdnet_amd import _C

        lay, M, N, K, dev = self.lay, self.M, self.N, self.K, self.device
        flags, want_pre = EPILOGUES[epi]
        rows = M if m_dev is None else max(0, min(M, m_dev + m_add))
        cmask = _window_cols(lay["c_off"], N, lay["ldc"], dev)
        pmask = _window_cols(lay["pre_off"], N, lay["ldpre"], dev)
        c_init = sentinel((M + TAIL, lay["ldc"]), dev)
        if flags & O.GEMM_ACCUM:  # old values where the kernel reads them; the padding columns and the tail stay sentinel
            c_init[:M] = torch.where(cmask[None, :], self.d["Cold"], c_init[:M])
        mdev_t = None if m_dev is None else torch.tensor([m_dev], dtype=torch.int32, device=dev)
        x = _C.GemmExArgs()
        x.A, x.aux, x.rowscale = self.d["A"].data_ptr(), self.d["aux"].data_ptr(), self.d["rowscale"].data_ptr()
        for g in range(lay["groups"]):
            x.W[g] = self.d["Wd"][lay["wmap"][g]].data_ptr()
            x.bias[g] = None if self.d["bias"][g] is None else self.d["bias"][g].data_ptr()
            x.Wsbg[g] = None if self.img is None else self.img[lay["wmap"][g]].data_ptr()
            x.a_off[g], x.c_off[g], x.pre_off[g], x.aux_off[g] = lay["a_off"][g], lay["c_off"][g], lay["pre_off"][g], lay["aux_off"][g]
        x.lda, x.ldw, x.ldc, x.ldpre, x.ldaux = lay["lda"], K, lay["ldc"], lay["ldpre"], lay["ldaux"]
        x.M, x.N, x.K, x.groups, x.flags = M, N, K, lay["groups"], flags
        x.m_dev, x.m_add = (None if mdev_t is None else mdev_t.data_ptr()), m_add
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def launch():
            Cb = c_init.clone()
            Pb = sentinel((M + TAIL, lay["ldpre"]), dev) if want_pre else None
            x.C, x.pre = Cb.data_ptr(), (None if Pb is None else Pb.data_ptr())
            route = C.c_int32(-1)
            rc = self.lib.tmdnet_debug_gemm_ex(stream, C.byref(x), C.byref(route))
            assert rc == 0, f"tmdnet_debug_gemm_ex returned {rc}"
            torch.cuda.synchronize()
            return Cb, Pb, route.value

        (Ca, Pa, route), (Cb, Pb, _) = launch(), launch()
        ref_c, ref_p = self.reference(epi)
        res = dict(route=ROUTE_NAMES[route], rows=rows, err={"C": O.per_row_rel_err(Ca[:rows], ref_c[:rows], cmask)})
        # nothing outside rows [0, rows) x the groups' column windows may change, bit for bit
        ok = bool(torch.equal(bits(Ca[rows:]), bits(c_init[rows:]))) and bool(torch.equal(bits(Ca[:, ~cmask]), bits(c_init[:, ~cmask])))
        det = bool(torch.equal(bits(Ca), bits(Cb)))
        fin = bool(torch.isfinite(Ca[:rows][:, cmask]).all())
        if want_pre:
            res["err"]["pre"] = O.per_row_rel_err(Pa[:rows], ref_p[:rows], pmask)
            ok = ok and bool((bits(Pa[rows:]) == SENTINEL).all()) and bool((bits(Pa[:, ~pmask]) == SENTINEL).all())
            det = det and bool(torch.equal(bits(Pa), bits(Pb)))
            fin = fin and bool(torch.isfinite(Pa[:rows][:, pmask]).all())
        res.update(untouched_ok=ok, deterministic=det, finite=fin)
        if rows:
            # element-wise distance to the limit, in units of max(1, |ref|): silu and silu' are of that size over the whole range
            e = (Ca[:rows][:, cmask].double() - ref_c[:rows][:, cmask]).abs() / ref_c[:rows][:, cmask].abs().clamp_min(1.0)
            res["elem_err"] = float(e.max())
        return res


def m_dev_counts(M):
    """(*m_dev, m_add) with *m_dev + m_add in {0, 1, 128 k + 37, M, M + 1000} and m_add in {0, 1}."""
    k = (M // 128) // 2
    mid = 128 * k + 37 if 128 * k + 37 < M else M // 2
    return [(t - add, add) for t in (0, 1, mid, M, M + 1000) for add in (0, 1)]
