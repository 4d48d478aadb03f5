"""TEST INFRASTRUCTURE ONLY -- float64 numpy specification of the MD loop's observer (torchmd-net_amd/csrc/tn_observe.hip), written
independently of its arithmetic: the histogram by np.histogram on fp64 distances (nearest image over the 27 neighbouring cells, not the
engine's sequential shifts), MSD and VACF by direct sums, sample index and ring slot by plain Python integers."""
import itertools
import math

import numpy as np


# ---- sampling: Python integers -------------------------------------------------------------------------------------------------------
def sample_index(s, s0, S):
    """index of the sample taken at step s, or -1"""
    if s <= s0 or (s - s0) % S:
        return -1
    return (s - s0) // S - 1


def samples_at(step, s0, S):
    return max(step - s0, 0) // S


def sample_step(j, s0, S):
    return s0 + (j + 1) * S


def ring_slot(j, capacity):
    return j % capacity


def lag_samples(n_samples, l):
    return max(n_samples - l, 0)


# ---- selectors -------------------------------------------------------------------------------------------------------------------------
def matches(z, sel):
    z = np.asarray(z)
    return np.ones(z.shape, bool) if sel is None else z == sel


def pair_counts(z, a, b):
    """(N_a, N_b, n_pairs): N_a N_b, or N_a (N_a - 1) / 2 when the two selectors are the same"""
    na, nb = int(matches(z, a).sum()), int(matches(z, b).sum())
    return na, nb, (na * (na - 1) / 2 if a == b else na * nb)


# ---- distances -------------------------------------------------------------------------------------------------------------------------
def nearest_image_distances(pos, box):
    """pos [n,3] (any float, widened), box [3,3] rows = cell vectors or None -> (i, j, d) of all pairs i < j in fp64, d the distance to
    the NEAREST of the 27 neighbouring images"""
    x = np.asarray(pos, np.float64)
    i, j = np.triu_indices(len(x), 1)
    d = x[j] - x[i]
    if box is None:
        return i, j, np.sqrt((d * d).sum(1))
    b = np.asarray(box, np.float64)
    best = np.full(len(i), np.inf)
    # bring the difference near the origin cell with the fractional coordinates, then look at that cell and its 26 neighbours
    frac = d @ np.linalg.inv(b)
    d0 = (frac - np.round(frac)) @ b
    for k in itertools.product((-1, 0, 1), repeat=3):
        e = d0 + np.asarray(k, np.float64) @ b
        best = np.minimum(best, np.sqrt((e * e).sum(1)))
    return i, j, best


def rdf_counts(z, pos, box, pairs, r_max, bins):
    """[P, bins] int64: np.histogram of the fp64 distances of the pairs of each type - one atom matches selector a and the other
    selector b, in either orientation, once.  A distance of exactly r_max is not counted."""
    z = np.asarray(z)
    i, j, d = nearest_image_distances(pos, box)
    out = np.zeros((len(pairs), bins), np.int64)
    for p, (a, b) in enumerate(pairs):
        ma, mb = matches(z, a), matches(z, b)
        sel = ((ma[i] & mb[j]) | (mb[i] & ma[j])) & (d < r_max)
        out[p] = np.histogram(d[sel], bins=bins, range=(0.0, r_max))[0]
    return out


def edge_margin(z, pos, box, pairs, r_max, bins):
    """(i, j, rel): for every pair that some type counts or nearly counts, the distance of d from the nearest bin edge (r_max
    included), relative to d"""
    z = np.asarray(z)
    i, j, d = nearest_image_distances(pos, box)
    any_type = np.zeros(len(i), bool)
    for a, b in pairs:
        ma, mb = matches(z, a), matches(z, b)
        any_type |= (ma[i] & mb[j]) | (mb[i] & ma[j])
    dr = r_max / bins
    k = np.clip(np.round(d / dr), 0, bins)  # the nearest edge; beyond r_max the nearest edge is r_max itself
    rel = np.abs(d - k * dr) / np.maximum(d, 1e-300)
    keep = any_type
    return i[keep], j[keep], rel[keep]


def rdf_g(counts, n_samples, n_pairs, r_max, volume=None):
    """counts [bins] -> g [bins]: counts / (n_samples n_pairs shell / V) with a volume, counts / (n_samples n_pairs) without"""
    bins = len(counts)
    out = np.zeros(bins)
    for b in range(bins):
        lo, hi = r_max * b / bins, r_max * (b + 1) / bins
        ideal = n_samples * n_pairs
        if volume is not None:
            ideal *= (4.0 * math.pi / 3.0) * (hi ** 3 - lo ** 3) / volume
        out[b] = counts[b] / ideal
    return out


# ---- MSD and VACF: direct sums -----------------------------------------------------------------------------------------------------------
def msd_sums(z, batch, n_mol, groups, origin, frames):
    """frames [n,N,3] -> (sum [n,B,G], terms [n,B,G]): sum over the group's atoms of |x - x0|^2, and the sum of the absolute values
    of the terms that were added (here the same) for the rounding bound"""
    z, batch = np.asarray(z), np.asarray(batch)
    x0 = np.asarray(origin, np.float64)
    out = np.zeros((len(frames), n_mol, len(groups)))
    for n, fr in enumerate(frames):
        e = ((np.asarray(fr, np.float64) - x0) ** 2)
        for m in range(n_mol):
            for g, sel in enumerate(groups):
                out[n, m, g] = math.fsum(e[(batch == m) & matches(z, sel)].reshape(-1))
    return out, out.copy()


def vacf_sums(z, batch, n_mol, groups, vel_frames, lags):
    """vel_frames [n,N,3] -> (acc [B,G,L], terms [B,G,L]): acc[m,g,l] = sum_j>=l sum_i v_i(j) . v_i(j - l), and the sum of |terms|"""
    z, batch = np.asarray(z), np.asarray(batch)
    v = np.asarray(vel_frames, np.float64)
    acc, mag = np.zeros((n_mol, len(groups), lags)), np.zeros((n_mol, len(groups), lags))
    for m in range(n_mol):
        for g, sel in enumerate(groups):
            idx = (batch == m) & matches(z, sel)
            for l in range(lags):
                terms = [(v[j][idx] * v[j - l][idx]).reshape(-1) for j in range(l, len(v))]
                if terms:
                    t = np.concatenate(terms)
                    acc[m, g, l], mag[m, g, l] = math.fsum(t), math.fsum(np.abs(t))
    return acc, mag


def sum_bound(n_terms, magnitude):
    """two fp64 summation orders of n terms differ by at most n 2^-52 sum|terms| (each partial sum rounds once, relative 2^-53, in
    either order); the products are exact in fp64"""
    return n_terms * 2.0 ** -52 * magnitude
