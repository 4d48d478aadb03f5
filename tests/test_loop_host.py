"""The host parts of the captured loops' shared device layer (csrc/tn_loop.h), compiled host-only (tests/loop_host_mirror.py), against
a Python spec: the slice count and the slice ranges of the per-molecule reductions and their sums in slice order, the workspace carver,
the step counter, the header's reset and status mapping, and the FIRE unit state with its log rows."""
import os

import numpy as np
import pytest

from tests import loop_host_mirror as H


# ---- the spec -----------------------------------------------------------------------------------------------------------------------
def spec_slices(N, B):
    if B <= 0 or N <= 1024 * B:
        return 1
    return min(256, -(-N // (1024 * B)))


def spec_range(counts, mstart, mend, N, S, batch, m, s):
    filt = counts[3] != 0 if counts is not None else batch is not None
    a, b = 0, N
    if counts is not None and not filt:
        a = max(int(mstart[m]), 0)
        b = max(min(int(mend[m]), N), a)
    i0, i1 = a + (b - a) * s // S, a + (b - a) * (s + 1) // S
    member = np.zeros(N, bool)
    member[i0:i1] = True if not (filt and batch is not None) else np.asarray(batch[i0:i1]) == m
    return i0, i1, bool(filt), member


# ---- mol_slices ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [0, 1, 3, 300])
def test_mol_slices(B):
    for N in (0, 1, 1023, 1024, 1025, 2048, 2049, 3 * 1024, 3 * 1024 + 1, 300 * 1024 + 1, 255 * 1024 + 1, 256 * 1024, 256 * 1024 + 1,
              300000, 10 ** 6, 2 ** 29 - 1):
        assert H.mol_slices(N, B) == spec_slices(N, B), (N, B)
    assert H.mol_slices(1025, 1) == 2 and H.mol_slices(1024, 1) == 1
    assert H.mol_slices(2 ** 29 - 1, 1) == 256  # the cap
    assert H.mol_slices(10, -1) == 1


# ---- mol_slice_range ------------------------------------------------------------------------------------------------------------------
def _counts(unsorted):
    c = np.zeros(8, np.int32)
    c[3] = unsorted
    return c


def _check(counts, mstart, mend, N, S, batch, m):
    """every slice against the spec; the slices of a molecule are disjoint and together cover exactly its atoms"""
    covered = np.zeros(N, int)
    for s in range(S):
        got = H.slice_range(counts, mstart, mend, N, S, batch, m, s)
        want = spec_range(counts, mstart, mend, N, S, batch, m, s)
        assert got[:3] == want[:3], (S, s, got[:3], want[:3])
        assert np.array_equal(got[3], want[3]), (S, s)
        assert got[0] == got[1] or 0 <= got[0] < got[1] <= N  # empty (a range that starts behind the atoms), or inside the arrays
        covered += got[3]
    return covered


@pytest.mark.parametrize("S", [1, 2, 3, 256])
def test_slices_of_valid_ranges_partition_the_molecule(S):
    N = 3000
    mstart, mend = np.array([0, 1025, 1025, 2999]), np.array([1025, 1025, 2999, 3000])  # an empty molecule and a single atom among them
    batch = np.repeat(np.arange(4), mend - mstart)
    for m in range(4):
        covered = _check(_counts(0), mstart, mend, N, S, batch, m)
        assert np.array_equal(covered, (batch == m).astype(int))


@pytest.mark.parametrize("S", [1, 2, 256])
def test_filtered_slices_partition_the_molecule(S):
    N = 2051
    rng = np.random.default_rng(5)
    batch = rng.integers(0, 3, N)  # unsorted: the ranges are not valid
    junk = np.array([-7, 5000, 12]), np.array([9000, -3, 4])  # never read
    for m in range(3):
        assert np.array_equal(_check(_counts(1), junk[0], junk[1], N, S, batch, m), (batch == m).astype(int))
        # without a graph workspace the batch vector alone decides
        assert np.array_equal(_check(None, None, None, N, S, batch, m), (batch == m).astype(int))
    # neither a graph workspace nor a batch vector: one molecule, all atoms
    assert np.array_equal(_check(None, None, None, N, S, None, 0), np.ones(N, int))
    # a graph workspace, valid ranges, no batch vector
    assert np.array_equal(_check(_counts(0), np.array([0]), np.array([N]), N, S, None, 0), np.ones(N, int))


@pytest.mark.parametrize("S", [1, 2, 256])
@pytest.mark.parametrize("a,b", [(-5, 1500), (100, 5000), (-5, 5000), (1500, 100), (-9, -2), (4000, 5000)])
def test_ranges_outside_the_atoms_are_clamped(S, a, b):
    N = 2051
    lo = max(a, 0)
    hi = max(min(b, N), lo)
    covered = _check(_counts(0), np.array([a]), np.array([b]), N, S, None, 0)  # (_check: no slice reaches outside [0, N])
    want = np.zeros(N, int)
    want[lo:hi] = 1
    assert np.array_equal(covered, want)


# ---- the carver -----------------------------------------------------------------------------------------------------------------------
def _align(n):
    return (n + 255) // 256 * 256


@pytest.mark.parametrize("ws", [0, 256, 4096 + 1, 4096 + 255, 2 ** 40 + 17])
def test_carver_hands_out_aligned_arrays_in_turn(ws):
    counts = [64, 0, 1, 3 * 1025, 256, 257, 0, 7]
    elems = [4, 8, 1, 4, 1, 1, 4, 8]
    starts, handed, entry = H.carve(ws, counts, elems)
    sizes = [_align(c * e) for c, e in zip(counts, elems)]
    assert handed == sum(sizes)         # the total is the sum of the aligned sizes ...
    assert entry == sum(sizes) + 256    # ... and the size entry adds the room to align the caller's pointer
    if ws:
        base = _align(ws)
        assert base - ws < 256 and base + handed <= ws + entry  # whatever the pointer's alignment, the arrays fit
        assert starts == [base + sum(sizes[:k]) for k in range(len(sizes))]
    else:
        assert starts == [0] * len(sizes)  # a null base hands out null pointers: only the count matters


def test_step_counter_round_trip():
    for step in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 63 + 11, 2 ** 64 - 1):
        back, lo, hi = H.step_roundtrip(step)
        assert back == step and lo == step % 2 ** 32 and hi == step >> 32


# ---- slice_sums -----------------------------------------------------------------------------------------------------------------------
def spec_slice_sums(slices, K, maxmask):
    """from 0.0, the slices in order: the sum, or the maximum where the mask bit is set - one rounding per step, as the header"""
    out = [np.float64(0.0)] * K
    for row in slices:
        for k in range(K):
            v = np.float64(row[k])
            out[k] = (v if v > out[k] else out[k]) if (maxmask >> k) & 1 else out[k] + v
    return np.array(out)


# (call shape, K, the entries that take the maximum, stride): FIRE's four, the IRC's six, the dimer's ten in rows three wider
_SHAPES = [("fire", 4, 1 << 3, 4), ("irc", 6, 1 << 2, 6), ("dimer", 10, 1 << 3, 13)]


@pytest.mark.parametrize("S", [1, 2, 3, 256])
@pytest.mark.parametrize("shape,K,mask,stride", _SHAPES)
def test_slice_sums_in_slice_order(shape, K, mask, stride, S):
    rng = np.random.default_rng(S)
    order = np.array([1e16, 1.0, -1e16, 1.0])  # ((1e16 + 1) - 1e16) + 1 = 1, any other order gives 0 or 2
    slices = np.full((S, stride), 1e300)  # (the columns behind K are never read: a sum that took them would overflow)
    for k in range(K):
        col = order[(np.arange(S) + k) % 4] if k % 2 == 0 else rng.standard_normal(S) * 10.0 ** rng.integers(-8, 8, S)
        slices[:, k] = np.abs(col) if (mask >> k) & 1 else col
    got = H.slice_sums(shape, slices, stride)
    want = spec_slice_sums(slices, K, mask)
    assert got.shape == (K,) and np.array_equal(got, want), (got, want)
    if S == 256:  # the order matters for these values: 64 times (((x + 1e16) + 1) - 1e16) + 1 leaves 1, the reverse order 0
        assert want[0] == 1.0 and spec_slice_sums(slices[::-1], K, mask)[0] == 0.0
    for k in range(K):  # a maximum starts from 0.0 as well
        if (mask >> k) & 1:
            assert got[k] == max(0.0, slices[:, k].max())
    neg = slices.copy()
    neg[:, :K] = -np.abs(neg[:, :K])
    assert all(H.slice_sums(shape, neg, stride)[k] == 0.0 for k in range(K) if (mask >> k) & 1)


# ---- the header: reset and status mapping ----------------------------------------------------------------------------------------------
OK, ERR_STATE, ERR_OVERFLOW = 0, 5, 3


def test_status_codes_are_the_public_ones():
    import re

    text = open(os.path.join(H.ROOT, "include", "tmdnet_amd.h")).read()
    for name, value in (("TMDNET_OK", OK), ("TMDNET_ERR_STATE", ERR_STATE), ("TMDNET_ERR_OVERFLOW", ERR_OVERFLOW)):
        assert int(re.search(rf"{name}\s*=?\s*(-?\d+)", text).group(1)) == value


@pytest.mark.parametrize("step", [0, 41, 2 ** 32 + 5, 2 ** 63 + 11])
@pytest.mark.parametrize("cause_word", [-1, 4, 8])
@pytest.mark.parametrize("status", [0, 1, 2, 7])
def test_status_mapping(status, cause_word, step):
    head = np.arange(100, 164, dtype=np.uint32)  # every word distinct: a wrong index shows
    head[0], head[1], head[2] = step % 2 ** 32, step >> 32, status
    want_rc = OK if status == 0 else ERR_OVERFLOW if status == 1 else ERR_STATE
    cause = int(head[cause_word]) if status == 2 and cause_word >= 0 else 0
    sentinel = 2 ** 64 - 1
    assert H.status_result(head, cause_word, 3) == (want_rc, [step, status, cause])
    assert H.status_result(head, cause_word, 2) == (want_rc, [step, status, sentinel])  # a two-word entry writes two words


@pytest.mark.parametrize("cause_word", [-1, 4, 5, 8])
def test_head_reset(cause_word):
    before = np.arange(100, 164, dtype=np.uint32)
    for step0 in (0, 2 ** 32 + 5):
        after = H.head_reset(before, step0, cause_word)
        want = before.copy()
        want[0], want[1], want[2], want[3] = step0 % 2 ** 32, step0 >> 32, 0, 1
        if cause_word >= 0:
            want[cause_word] = 0
        assert np.array_equal(after, want)  # and no other word
        assert H.status_result(after, cause_word, 3) == (OK, [step0, 0, 0])


# ---- the FIRE unit state ----------------------------------------------------------------------------------------------------------------
def test_fire_load_fresh_and_not():
    A = H.FireArrays(5)
    for unit in range(5):
        assert H.fire_load(A, unit, False) == (A.dt[unit], A.alpha[unit], int(A.n_pos[unit]), int(A.conv[unit]))
        assert H.fire_load(A, unit, True) == (0.125, 0.75, 0, -1)  # the start values of the header, whatever the arrays hold


@pytest.mark.parametrize("rows", [True, False])
@pytest.mark.parametrize("energy", [None, -3.25])
def test_fire_store_and_rows(rows, energy):
    A = H.FireArrays(5, rows)
    before, rows_before = A.state(), [None if r is None else r.copy() for r in A.rows]
    unit, coef3, sums4 = 3, np.array([0.5, 0.25, 2.0], np.float32), np.array([1.5, 9.0, -2.0, 6.25])
    H.fire_store(A, unit, 0.3, 0.07, 4, 12, coef3, energy, sums4, 2.25)  # (fmax2 need not be sums4[3]: the cell passes another)
    others = np.arange(5) != unit
    for a, b in zip(A.state(), before):
        assert np.array_equal(a[others], b[others])  # only this unit
    assert (A.dt[unit], A.alpha[unit], A.n_pos[unit], A.conv[unit]) == (0.3, 0.07, 4, 12) and np.array_equal(A.coef[unit], coef3)
    if not rows:
        return  # every row NULL: nothing but the state was written (and nothing was dereferenced)
    for r, b in zip(A.rows, rows_before):
        assert np.array_equal(r[others], b[others])
    epot, fmax, sums, coef, dt, alpha, conv = (r[unit] for r in A.rows)
    assert epot == (np.float32(energy) if energy is not None else -5)  # no energy: the row is left alone
    assert fmax == np.float32(1.5) and np.array_equal(sums, sums4) and np.array_equal(coef, coef3)
    assert (dt, alpha, conv) == (0.3, 0.07, 12)
