"""TEST INFRASTRUCTURE ONLY: the host parts of torchmd-net_amd/csrc/tn_loop.h (workspace carver, molecule slices and their sums, step
counter, header reset and status mapping, the FIRE unit state and its log rows) on the CPU, compiled host-only from tests/loop_host.hip into oracle/_build/libloop_host.so and called through ctypes.  The statements
are the header's own; tests/test_loop_host.py compares them with a Python spec."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libloop_host.so")
        csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
        src = [os.path.join(ROOT, "tests", "loop_host.hip")] + [os.path.join(csrc, h) for h in ("tn_loop.h", "tn_model.h", "tn_common.h", "tn_min_math.h", "tn_dimer_math.h", "tn_irc_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-fPIC", "-shared", src[0], "-o", so])
        _LIB = C.CDLL(so)
        _LIB.loop_mol_slices.restype = C.c_int
        _LIB.loop_slice_range.restype = None
        _LIB.loop_carve.restype = None
        _LIB.loop_step_roundtrip.restype = C.c_uint64
        _LIB.loop_slice_sums.restype = C.c_int
        _LIB.loop_head_reset.restype = None
        _LIB.loop_status_result.restype = C.c_int
        _LIB.loop_fire_load.restype = None
        _LIB.loop_fire_store.restype = None
    return _LIB


def _p(a):
    return C.c_void_p(0) if a is None else a.ctypes.data_as(C.c_void_p)


def mol_slices(N, B):
    return lib().loop_mol_slices(C.c_int64(N), C.c_int64(B))


def slice_range(counts, mstart, mend, N, S, batch, m, s):
    """-> (i0, i1, filter, member [N] bool: the atoms of the slice that the reduction adds)"""
    counts = None if counts is None else np.ascontiguousarray(counts, np.int32)
    mstart = None if mstart is None else np.ascontiguousarray(mstart, np.int32)
    mend = None if mend is None else np.ascontiguousarray(mend, np.int32)
    batch = None if batch is None else np.ascontiguousarray(batch, np.int64)
    out = np.zeros(3, np.int32)
    member = np.zeros(max(N, 1), np.uint8)
    lib().loop_slice_range(_p(counts), _p(mstart), _p(mend), C.c_int(N), C.c_int(S), _p(batch), C.c_int(m), C.c_int(s), _p(out), _p(member))
    return int(out[0]), int(out[1]), bool(out[2]), member[:N].astype(bool)


def carve(ws, counts, elems):
    """-> (start address of every array, bytes handed out, what the size entry answers)"""
    counts, elems = np.ascontiguousarray(counts, np.int64), np.ascontiguousarray(elems, np.int32)
    starts = np.zeros(len(counts), np.uint64)
    handed, entry = C.c_uint64(0), C.c_uint64(0)
    lib().loop_carve(C.c_uint64(ws), C.c_int64(len(counts)), _p(counts), _p(elems), _p(starts), C.byref(handed), C.byref(entry))
    return [int(x) for x in starts], handed.value, entry.value


def step_roundtrip(step):
    head = np.zeros(2, np.uint32)
    back = lib().loop_step_roundtrip(C.c_uint64(step), _p(head))
    return back, int(head[0]), int(head[1])


SLICE_SHAPES = {"fire": 0, "irc": 1, "dimer": 2}


def slice_sums(shape, slices, stride):
    """slice_sums of ``slices`` [S, stride] in the call shape ``shape`` -> [K]"""
    slices = np.ascontiguousarray(slices, np.float64)
    out = np.full(16, np.nan)
    K = lib().loop_slice_sums(C.c_int(SLICE_SHAPES[shape]), _p(slices), C.c_int(slices.shape[0]), C.c_int(stride), _p(out))
    return out[:K]


def head_reset(head, step0, cause_word):
    """loop_head_reset on a copy of ``head`` (uint32 words)"""
    head = np.array(head, np.uint32)
    lib().loop_head_reset(_p(head), C.c_uint64(step0), C.c_int(cause_word))
    return head


def status_result(head, cause_word, n_host):
    """-> (rc, host): ``host`` has three words that start from a sentinel, so a word the mapping does not write keeps it"""
    head = np.ascontiguousarray(head, np.uint32)
    host = np.full(3, 2 ** 64 - 1, np.uint64)
    rc = lib().loop_status_result(_p(head), C.c_int(cause_word), _p(host), C.c_int(n_host))
    return rc, [int(x) for x in host]


class FireArrays:
    """the per-unit FIRE arrays of a workspace and the seven log rows, on the host"""

    def __init__(self, units, rows=True):
        rng = np.random.default_rng(11)
        self.dt, self.alpha = rng.random(units) + 0.5, rng.random(units)
        self.conv = np.where(np.arange(units) % 2 == 0, -1, 7 + np.arange(units)).astype(np.int64)
        self.n_pos = rng.integers(0, 9, units).astype(np.int32)
        self.coef = rng.random((units, 3)).astype(np.float32)
        self.start = np.array([0.125, 0.75])
        f32, f64 = np.float32, np.float64
        shapes = ((f32, ()), (f32, ()), (f64, (4,)), (f32, (3,)), (f64, ()), (f64, ()), (np.int64, ()))
        self.rows = [np.full((units,) + sh, -5, t) if rows else None for t, sh in shapes]

    def state(self):
        return [a.copy() for a in (self.dt, self.alpha, self.conv, self.n_pos, self.coef)]


def fire_load(A, unit, fresh):
    """-> (dt, alpha, n_pos, converged_at)"""
    state, counts = np.zeros(2), np.zeros(2, np.int64)
    lib().loop_fire_load(_p(A.dt), _p(A.alpha), _p(A.conv), _p(A.n_pos), _p(A.coef), _p(A.start), C.c_int(unit), C.c_int(int(fresh)),
                         _p(state), _p(counts))
    return float(state[0]), float(state[1]), int(counts[0]), int(counts[1])


def fire_store(A, unit, dt, alpha, n_pos, conv, coef3, energy, sums4, fmax2):
    """fire_store and FireRows::write of ``unit`` into ``A`` (``energy``: a float, or None for a NULL pointer)"""
    state, counts = np.array([dt, alpha]), np.array([n_pos, conv], np.int64)
    coef3, sums4 = np.ascontiguousarray(coef3, np.float32), np.ascontiguousarray(sums4, np.float64)
    e = None if energy is None else np.array([energy], np.float32)
    lib().loop_fire_store(_p(A.dt), _p(A.alpha), _p(A.conv), _p(A.n_pos), _p(A.coef), C.c_int(unit), _p(state), _p(counts), _p(coef3),
                          _p(e), _p(sums4), C.c_double(fmax2), *[_p(r) for r in A.rows])
