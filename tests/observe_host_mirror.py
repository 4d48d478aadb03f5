"""TEST INFRASTRUCTURE ONLY: the arithmetic of the MD loop's observer (torchmd-net_amd/csrc/tn_observe_math.h) on the CPU, compiled
host-only from tests/observe_host.hip into oracle/_build/libobserve_host.so and called through ctypes on numpy arrays, and the exact
fp32 mirror of the histogram kernel: the pair vectors are the statement of tests/graph_oracle.py (``fp32_statement``: one subtraction,
fused shifts z -> y -> x, a fused multiply-add formed in fp64 and rounded once), the bin is the header's own."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import graph_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "observe_host.hip")
_LIB = None


def _sources():
    csrc = os.path.join(ROOT, "torchmd-net_amd", "csrc")
    return [SRC, os.path.join(csrc, "tn_observe_math.h"), os.path.join(csrc, "tn_md_math.h")]


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(ROOT, "oracle", "_build", "libobserve_host.so")
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in _sources()):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-fPIC", "-shared", SRC, "-o", so])
        _LIB = C.CDLL(so)
        for name in ("obs_sample_index", "obs_samples_at", "obs_lag_samples"):
            getattr(_LIB, name).restype = C.c_int64
        _LIB.obs_sample_step.restype = C.c_uint64
        _LIB.obs_ring_slot.restype = C.c_int32
        _LIB.obs_pair_types.restype = C.c_uint32
        for name in ("obs_pair_count", "obs_shell_volume", "obs_rdf_value"):
            getattr(_LIB, name).restype = C.c_double
        _LIB.obs_bins.restype = None
        _LIB.obs_histogram.restype = None
    return _LIB


def build_program(out, sanitize=True):
    """the stand-alone program of tests/observe_host.hip (its own main), a host build; -> the command that built it"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-DOBSERVE_HOST_MAIN"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd += [SRC, "-o", out]
    subprocess.check_call(cmd)
    return cmd


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def sample_index(s, s0, S):
    return int(lib().obs_sample_index(C.c_uint64(s), C.c_uint64(s0), C.c_uint64(S)))


def samples_at(step, s0, S):
    return int(lib().obs_samples_at(C.c_uint64(step), C.c_uint64(s0), C.c_uint64(S)))


def sample_step(j, s0, S):
    return int(lib().obs_sample_step(C.c_int64(j), C.c_uint64(s0), C.c_uint64(S)))


def ring_slot(j, capacity):
    return int(lib().obs_ring_slot(C.c_int64(j), C.c_int32(capacity)))


def lag_samples(n_samples, l):
    return int(lib().obs_lag_samples(C.c_int64(n_samples), C.c_int32(l)))


def pair_types(mi, mj):
    return int(lib().obs_pair_types(C.c_uint32(mi), C.c_uint32(mj)))


def pair_count(n_a, n_b, same):
    return float(lib().obs_pair_count(C.c_int64(n_a), C.c_int64(n_b), C.c_int32(int(same))))


def rdf_value(count, n_samples, n_pairs, b, bins, r_max, volume):
    shell = float(lib().obs_shell_volume(C.c_int32(b), C.c_int32(bins), C.c_double(r_max)))
    return float(lib().obs_rdf_value(C.c_int64(count), C.c_int64(n_samples), C.c_double(n_pairs), C.c_double(shell),
                                     C.c_double(volume or 0.0)))


def constants(r_max, bins):
    """(r_max2, inv_dr) as the caller of tmdnet_md_observe forms them: in fp64, rounded to fp32 once"""
    return np.float32(np.float64(r_max) * np.float64(r_max)), np.float32(np.float64(bins) / np.float64(r_max))


def bins_of(d2, r_max, bins):
    d2 = np.ascontiguousarray(d2, np.float32)
    out = np.zeros(len(d2), np.int32)
    r2, inv = constants(r_max, bins)
    lib().obs_bins(C.c_int64(len(d2)), _p(d2), C.c_float(r2), C.c_float(inv), C.c_int32(bins), _p(out))
    return out


def masks(z, pairs=(), msd=(), vacf=()):
    """the per-atom uint32 mask of tmdnet_md_observe: pair type p - selector a: bit 2p, selector b: bit 2p + 1; MSD group g: bit 8 + g;
    VACF group g: bit 16 + g"""
    z = np.asarray(z)
    hit = lambda sel: (np.ones(z.shape, bool) if sel is None else z == sel).astype(np.uint32)  # noqa: E731
    m = np.zeros(z.shape, np.uint32)
    for p, (a, b) in enumerate(pairs):
        m |= hit(a) << np.uint32(2 * p)
        m |= hit(b) << np.uint32(2 * p + 1)
    for g, sel in enumerate(msd):
        m |= hit(sel) << np.uint32(8 + g)
    for g, sel in enumerate(vacf):
        m |= hit(sel) << np.uint32(16 + g)
    return m


def pair_d2(pos, box, box_mode, batch):
    """All pairs lo < hi of the same molecule, in the caller's order, and the engine's fp32 squared distance: -> (lo, hi, d2)"""
    pos = np.asarray(pos, np.float32)
    batch = np.asarray(batch)
    lo, hi = np.triu_indices(len(pos), 1)
    keep = batch[lo] == batch[hi]
    lo, hi = lo[keep], hi[keep]
    mode = 0 if box is None else box_mode
    pbox = None if box is None else np.asarray(box, np.float32)
    d, _, _ = GO.fp32_statement({"_geom": (pos, pbox, mode, batch), "pair_i": hi, "pair_j": lo})
    f64 = np.float64
    fma = lambda a, b, c: (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(np.float32)  # noqa: E731
    return lo, hi, fma(d[:, 2], d[:, 2], fma(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))


def rdf_counts(z, pos, box, box_mode, batch, n_mol, pairs, r_max, bins):
    """the counts k_obs_rdf leaves after one sample: [B, P, bins] uint64"""
    lo, hi, d2 = pair_d2(pos, box, box_mode, batch)
    m = masks(z, pairs)
    batch = np.asarray(batch)
    out = np.zeros((n_mol, len(pairs), bins), np.uint64)
    r2, inv = constants(r_max, bins)
    for mol in range(n_mol):
        k = batch[lo] == mol
        dd, mi, mj = np.ascontiguousarray(d2[k]), np.ascontiguousarray(m[lo[k]]), np.ascontiguousarray(m[hi[k]])
        row = np.zeros((len(pairs), bins), np.uint64)
        lib().obs_histogram(C.c_int64(len(dd)), _p(dd), _p(mi), _p(mj), C.c_int32(len(pairs)), C.c_float(r2), C.c_float(inv),
                            C.c_int32(bins), _p(row))
        out[mol] = row
    return out
