"""TEST INFRASTRUCTURE ONLY: the committee's definitions in float64 numpy, written from the definitions and not from the kernel.

For M members with energies E [M,B] and forces F [M,N,3]:
    mean = (1/M) sum_k x_k,   std = sqrt(sum_k (x_k - mean)^2 / (M - 1))     (numpy's ddof=1, the reference's torch.std)
    d_i  = sqrt(sum_c std_i,c^2), taken as +inf when it is not finite
    D_m  = max over the atoms of molecule m, a_m the smallest index that attains it; no atoms: D_m = 0, a_m = -1
Atoms whose batch entry is outside [0, B) belong to no molecule."""
import numpy as np

SIZES = [1, 5, 64, 0, 65, 300]  # wave and block boundaries, and an empty molecule id in the middle


def synthetic(M, seed, unsorted=False, scale=1.0):
    """-> E [M,B], F [M,N,3] fp32, batch [N] int64, B: M members around one random force field, molecules of SIZES atoms"""
    rng = np.random.default_rng(seed)
    batch = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    N, B = len(batch), len(SIZES)
    F0 = rng.normal(size=(N, 3))
    F = (F0[None] + 0.05 * scale * rng.normal(size=(M, N, 3))).astype(np.float32)
    E = (-1000.0 * rng.random(B)[None] + 0.02 * rng.normal(size=(M, B))).astype(np.float32)
    if unsorted:
        batch = batch[rng.permutation(N)]
    return E, F, batch, B


def reduce(E, F, batch, B):
    E = np.asarray(E, dtype=np.float64).reshape(len(E), -1)
    F = np.asarray(F, dtype=np.float64)
    N = F.shape[1]
    with np.errstate(all="ignore"):
        energy, forces = E.mean(axis=0), F.mean(axis=0)
        energy_std, forces_std = E.std(axis=0, ddof=1), F.std(axis=0, ddof=1)
        d = np.sqrt((forces_std ** 2).sum(axis=1))
    d = np.where(np.isfinite(d), d, np.inf)
    batch = np.zeros(N, dtype=np.int64) if batch is None else np.asarray(batch, dtype=np.int64)
    D, a = np.zeros(B), np.full(B, -1, dtype=np.int64)
    for i in range(N):
        m = int(batch[i])
        if 0 <= m < B and (a[m] < 0 or d[i] > D[m]):  # strictly larger: the first index keeps a tie
            D[m], a[m] = d[i], i
    return dict(energy=energy, forces=forces, energy_std=energy_std, forces_std=forces_std, deviation=d, max_deviation=D, max_atom=a)


def ulps(got, want):
    """|got - want| in units of the fp32 spacing at `want` (float64), elementwise; 0 where both are the same infinity or both NaN;
    inf where one is finite and the other is not"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(all="ignore"):
        sp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        u = np.abs(got - want) / sp
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    return np.where(same, 0.0, np.where(np.isfinite(u), u, np.inf))


def argmax_of(deviation, batch, B):
    """D_m, a_m of the fp32 deviations as they are: the maximum is exact (no arithmetic), the smallest index keeps a tie"""
    d = np.asarray(deviation)
    batch = np.zeros(len(d), dtype=np.int64) if batch is None else np.asarray(batch, dtype=np.int64)
    D, a = np.zeros(B, dtype=d.dtype), np.full(B, -1, dtype=np.int64)
    for i in range(len(d)):
        m = int(batch[i])
        if 0 <= m < B and (a[m] < 0 or d[i] > D[m]):
            D[m], a[m] = d[i], i
    return D, a


def check(got, want, batch, B, bound=4.0):
    """every float field of `got` (fp32) within `bound` fp32 ulps of the float64 `want`, exact zeros exact -> the worst figure per
    field.  max_deviation / max_atom are ALSO held exactly to the maximum and the lowest-index argmax of `got`'s own fp32 deviations
    (rounding can merge two float64 values into one fp32 tie; the definition is on the rounded outputs), and max_atom to the
    oracle's wherever the oracle's maximum is separated from the runner-up by more than the bound."""
    worst = {}
    D, a = argmax_of(got["deviation"], batch, B)
    assert np.array_equal(np.asarray(got["max_atom"]).astype(np.int64), a), (got["max_atom"], a)
    assert np.array_equal(np.asarray(got["max_deviation"]).view(np.int32), D.view(np.int32))
    bat = np.zeros(len(got["deviation"]), dtype=np.int64) if batch is None else np.asarray(batch, dtype=np.int64)
    for m in range(B):
        dm = np.sort(want["deviation"][bat == m])[::-1]
        if len(dm) == 1 or (len(dm) > 1 and dm[0] - dm[1] > 2 * bound * np.spacing(np.float32(dm[0]))):
            assert a[m] == want["max_atom"][m], (m, a[m], want["max_atom"][m])
    for k, w in want.items():
        g = np.asarray(got[k])
        if k == "max_atom":
            continue
        u = ulps(g, w)
        worst[k] = float(u.max()) if u.size else 0.0
        assert worst[k] <= bound, (k, worst[k])
        assert np.all(g[np.asarray(w) == 0.0] == 0.0), k
    return worst
