"""The host parts of the captured loops' shared device layer (csrc/tn_loop.h), compiled host-only (tests/loop_host_mirror.py), against
a Python spec: the slice count and the slice ranges of the per-molecule reductions, the workspace carver and the step counter."""
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
