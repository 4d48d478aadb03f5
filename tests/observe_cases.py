"""TEST INFRASTRUCTURE ONLY: hand-built systems for the MD loop's observer - 5 atoms without a box, 64 atoms in an orthorhombic box,
300 atoms in a triclinic box (the smallest molecule with the tile pairs (0,0), (0,1) and (1,1)) and a batch of the three - with 7 and
1024 bins and pair lists that hold a wildcard, a same-species and a cross-species type.

The margin condition.  Coordinates are multiples of 2^-6 (a jittered lattice) plus a seeded jitter.  The generator redraws,
deterministically, the jitter of any atom in a counted pair whose fp64 distance lies within MARGIN = 1e-5 relative of a bin edge or of
r_max, until none is left.  fp32 carries a relative error of a few 2^-24 = 6e-8 per operation on coordinates below 16 and distances
above 0.5, far inside the margin, so the fp32 mirror, the fp64 oracle and the device agree on every bin and the comparisons can be
exact (the rule of tests/test_graph_oracle.py)."""
import numpy as np

from tests import observe_oracle as O

MARGIN = 1e-5
PAIRS = [(None, None), (8, 8), (1, 8)]  # a wildcard, a same-species and a cross-species type


def _lattice(rng, n, cells, spacing):
    """n atoms on distinct sites of a cells^3 lattice, in multiples of 2^-6, in the order the sites were drawn"""
    sites = rng.permutation(cells ** 3)[:n]
    ijk = np.stack([sites // (cells * cells), (sites // cells) % cells, sites % cells], 1)
    return np.round(ijk * spacing * 64.0) / 64.0


def _jitter(rng, n):
    return rng.uniform(-0.25, 0.25, (n, 3))


def _settle(z, base, box, r_max, bins_list, seed):
    """jitter the lattice until no counted pair is within MARGIN of an edge, for every bin count of the case"""
    rng = np.random.default_rng(seed)
    jit = _jitter(rng, len(base))
    for _ in range(200):
        pos = (base + jit).astype(np.float32)
        bad = set()
        for bins in bins_list:
            i, j, rel = O.edge_margin(z, pos, box, PAIRS, r_max, bins)
            k = rel < MARGIN
            bad |= set(i[k].tolist()) | set(j[k].tolist())
        if not bad:
            return pos
        for a in sorted(bad):
            jit[a] = _jitter(rng, 1)[0]
    raise AssertionError("the case did not settle")


def _species(rng, n):
    z = np.where(np.arange(n) % 3 == 0, 8, 1)  # water-like: one O, two H
    return z[rng.permutation(n)].astype(np.int64)


def five():
    """5 atoms, no box"""
    rng = np.random.default_rng(11)
    z = np.array([8, 1, 1, 8, 1], np.int64)
    base = _lattice(rng, 5, 2, 1.25)
    r_max, bins = 3.0, [7, 1024]
    return dict(name="five", z=z, pos=_settle(z, base, None, r_max, bins, 12), box=None, r_max=r_max, bins=bins)


def sixty_four():
    """64 atoms in an orthorhombic box"""
    rng = np.random.default_rng(21)
    z = _species(rng, 64)
    box = np.diag([8.0, 8.5, 9.0]).astype(np.float32)
    base = _lattice(rng, 64, 4, 2.0)
    r_max, bins = 4.0, [7, 1024]
    return dict(name="sixty_four", z=z, pos=_settle(z, base, box, r_max, bins, 22), box=box, r_max=r_max, bins=bins)


def three_hundred():
    """300 atoms in a triclinic (lower-triangular) box: tiles (0,0), (0,1), (1,1)"""
    rng = np.random.default_rng(31)
    z = _species(rng, 300)
    box = np.array([[14.0, 0.0, 0.0], [1.5, 14.5, 0.0], [-1.0, 2.0, 15.0]], np.float32)
    base = _lattice(rng, 300, 7, 2.0)
    r_max, bins = 3.5, [7, 1024]
    return dict(name="three_hundred", z=z, pos=_settle(z, base, box, r_max, bins, 32), box=box, r_max=r_max, bins=bins)


_CACHE = {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = {"five": five, "sixty_four": sixty_four, "three_hundred": three_hundred}[name]()
    return _CACHE[name]


def batch_of_three():
    """the three systems as one batch: the 5 atoms get a box large enough that no image is nearer than the atom itself; one r_max
    (the smallest of the three)"""
    if "batch" not in _CACHE:
        cs = [case("five"), case("sixty_four"), case("three_hundred")]
        boxes = np.stack([np.diag([40.0, 40.0, 40.0]).astype(np.float32), cs[1]["box"], cs[2]["box"]])
        z = np.concatenate([c["z"] for c in cs])
        batch = np.concatenate([np.full(len(c["z"]), m, np.int64) for m, c in enumerate(cs)])
        r_max, bins = 3.0, [7]
        pos = []
        for m, c in enumerate(cs):  # settle every molecule again for the shared r_max (the 5 atoms now have a box)
            base = np.round(c["pos"].astype(np.float64) * 64.0) / 64.0
            pos.append(_settle(c["z"], base, boxes[m], r_max, bins, 40 + m))
        _CACHE["batch"] = dict(name="batch", z=z, pos=np.concatenate(pos), box=boxes, batch=batch, n_mol=3, r_max=r_max, bins=bins)
    return _CACHE["batch"]


def velocities(n, seed, steps):
    """[steps, n, 3] fp32: a smooth random series, so that lags have signal and terms of both signs"""
    rng = np.random.default_rng(seed)
    phase, amp = rng.uniform(0, 2 * np.pi, (n, 3)), rng.normal(0, 1, (n, 3))
    t = np.arange(steps)[:, None, None]
    return (amp[None] * np.cos(0.4 * t + phase[None]) + 0.1 * rng.normal(0, 1, (steps, n, 3))).astype(np.float32)
