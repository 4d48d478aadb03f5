"""TEST INFRASTRUCTURE ONLY: temperature replica exchange as the scheme states it, in Python integers and fp64 floats, independent of
the engine's sources (the Philox of tests/md_oracle.py is written from the algorithm's definition).

G ladders of R slots, replica b = g R + r starts in slot r.  After n completed steps attempt a = n // X tries the slot pairs
(s, s + 1), s = a & 1, (a & 1) + 2, ... while s + 1 < R.  With i, j the replicas that hold s and s + 1:
    D = (beta[s] - beta[s+1]) (E_i - E_j),   accept iff D >= 0 or u < exp(D),
u = ((w >> 8) + 0.5) 2^-24 from word 0 of Philox4x32-10 with key = seed and counter = (n lo, n hi, g (R - 1) + s, 2).
Also: the canonical-sampling protocol of the harmonic well (its parameters, its statistics and the bounds, with their basis)."""
import math

import numpy as np

from tests import md_oracle as O

MASK = 0xFFFFFFFF


def pairs(a, R):
    return list(range(a & 1, R - 1, 2))


def uniform(seed, n, g, s, R):
    w = O.philox4x32_10((n & MASK, n >> 32, g * (R - 1) + s, 2), (seed & MASK, seed >> 32))
    return O.uniform(w[0])


def decide(beta_lo, beta_hi, E_i, E_j, u):
    """-> (accept, undecidable): undecidable when u and exp(D) are within 4 fp64 ulp of each other (another libm may differ)"""
    with np.errstate(invalid="ignore", over="ignore"):
        D = float((np.float64(beta_lo) - np.float64(beta_hi)) * (np.float64(np.float32(E_i)) - np.float64(np.float32(E_j))))
    if D >= 0.0:
        return True, False
    if math.isnan(D):
        return False, False
    p = math.exp(D)
    return u < p, abs(u - p) <= 4 * math.ulp(p)


def probability(beta_lo, beta_hi, E_i, E_j):
    """min(1, exp D), arrays"""
    D = (beta_lo - beta_hi) * (np.asarray(E_i, np.float64) - np.asarray(E_j, np.float64))
    return np.exp(np.minimum(D, 0.0))


class Ladders:
    def __init__(self, G, R, beta, every, seed):
        self.G, self.R, self.every, self.seed = G, R, every, seed
        self.beta = [float(b) for b in beta]
        self.slot = [[r for r in range(R)] for _ in range(G)]  # slot[g][r]: the slot of replica g R + r
        self.holder = [[s for s in range(R)] for _ in range(G)]
        self.attempts = np.zeros((G, R - 1), np.int64)
        self.accepts = np.zeros((G, R - 1), np.int64)
        self.undecidable = []

    def attempt(self, n, epot):
        """-> (slot of every replica [G R], accepted [G, R-1] with 0 for the pairs not tried)"""
        G, R = self.G, self.R
        acc = np.zeros((G, R - 1), np.uint8)
        for g in range(G):
            for s in pairs(n // self.every, R):
                i, j = self.holder[g][s], self.holder[g][s + 1]
                u = uniform(self.seed, n, g, s, R)
                ok, und = decide(self.beta[s], self.beta[s + 1], epot[g * R + i], epot[g * R + j], u)
                if und:
                    self.undecidable.append((n, g, s))
                self.attempts[g, s] += 1
                if ok:
                    self.accepts[g, s] += 1
                    acc[g, s] = 1
                    self.holder[g][s], self.holder[g][s + 1] = j, i
                    self.slot[g][i], self.slot[g][j] = s + 1, s
        return np.array(self.slot, np.int32).reshape(-1), acc


def check_inverse(slot, holder, G, R):
    slot, holder = np.asarray(slot).reshape(G, R), np.asarray(holder).reshape(G, R)
    for g in range(G):
        assert sorted(slot[g].tolist()) == list(range(R)) and sorted(holder[g].tolist()) == list(range(R)), (slot[g], holder[g])
        assert (slot[g][holder[g]] == np.arange(R)).all() and (holder[g][slot[g]] == np.arange(R)).all(), (slot[g], holder[g])


# ---- canonical sampling in a harmonic well -------------------------------------------------------------------------------------------
# One ladder of R = 4 replicas of n = 10 atoms (m = 1) in E = 0.5 k |x|^2, k = 1: omega = 1, d = 30 degrees of freedom.  dt = 0.1
# (omega dt = 0.1), friction = 1: the velocity correlation time is 1 / friction = 10 steps, positions relax with the envelope
# exp(-friction t / 2) (underdamped, friction < 2 omega), 20 steps, and the energies, being quadratic, in half of each.  An attempt
# every 60 steps is 6 and 3 correlation times of the amplitudes apart (12 and 6 of the energies).  2 000 attempts.
SAMPLING = dict(G=1, R=4, n=10, attempts=2000, every=60, dt=0.1, friction=1.0, k=1.0, kT=[1.0, 1.3, 1.7, 2.2], seed=2 ** 41 + 17)


def sampling_state(seed=11):
    """x, v [R n, 3] fp32 drawn at each slot's temperature (k = m = 1: both have variance kT)"""
    e = SAMPLING
    rng = np.random.default_rng(seed)
    sd = np.sqrt(np.repeat(np.asarray(e["kT"]), e["n"]))[:, None]
    return (rng.normal(size=(e["R"] * e["n"], 3)) * sd).astype(np.float32), (rng.normal(size=(e["R"] * e["n"], 3)) * sd).astype(np.float32)


def slots_before(slot_log, R):
    """the slot every replica held DURING the steps before each attempt: the row after the attempt before (identity at first)"""
    first = np.tile(np.arange(R, dtype=slot_log.dtype), slot_log.shape[1] // R)[None]
    return np.concatenate([first, slot_log[:-1]])


def sampling_statistics(epot, ekin, slot_log, accept_log, kT, n, force_scale=1.0):
    """Followed by slot (one ladder): mean potential and kinetic energy per slot in units of their canonical value (d/2) kT[s] minus
    one, in units of the bound; the acceptance per pair against the mean of min(1, exp D) on the logged energies.
    Bounds.  The potential (kinetic) energy of d harmonic (free) degrees of freedom is Gamma(d/2, kT): mean (d/2) kT, standard
    deviation sqrt(d/2) kT.  The standard error of a mean over N attempts is taken with N_eff = N / 2 (the residual correlation at 3
    to 12 correlation times, and the coupling of the slots through the swaps), and the bound is 5 of them.  The time-step error of
    the splitting is O((omega dt)^2 / 4) = 0.25 % of the mean, against a bound of 5 / sqrt(15 * 1000) = 4.1 %.
    Acceptance: given the energies, every decision is a Bernoulli draw of probability min(1, exp D); the bound is 4 binomial
    standard errors sqrt(p (1 - p) / N_pair)."""
    kT = np.asarray(kT, np.float64)
    R = len(kT)
    N = epot.shape[0]
    d = 3 * n
    before = slots_before(slot_log, R)
    out = dict(attempts=N, epot=[], ekin=[], acceptance=[])
    bound = 5.0 * math.sqrt(d / 2.0) / math.sqrt(N / 2.0)  # in units of kT[s]
    for s in range(R):
        who = before == s
        assert (who.sum(1) == 1).all()
        for name, log in (("epot", epot.astype(np.float64)), ("ekin", ekin.astype(np.float64) / force_scale)):
            mean = float(log[who].mean())
            out[name].append(dict(slot=s, mean=mean, expected=0.5 * d * kT[s], deviation=mean - 0.5 * d * kT[s], bound=bound * kT[s]))
    beta = 1.0 / kT
    for s in range(R - 1):
        tried = np.array([s in pairs(a + 1, R) for a in range(N)])  # row a is attempt a + 1: the step counter reads (a + 1) X
        i, j = (before == s).argmax(1), (before == s + 1).argmax(1)
        rows = np.arange(N)
        p = probability(beta[s], beta[s + 1], epot[rows, i], epot[rows, j])[tried]
        got = float(accept_log.reshape(N, R - 1)[tried, s].mean())
        exp = float(p.mean())
        out["acceptance"].append(dict(pair=s, measured=got, expected=exp, deviation=got - exp,
                                      bound=4.0 * math.sqrt(exp * (1.0 - exp) / int(tried.sum())), tried=int(tried.sum())))
    return out


def assert_sampling(stats):
    for name in ("epot", "ekin"):
        for row in stats[name]:
            assert abs(row["deviation"]) < row["bound"], (name, row)
    for row in stats["acceptance"]:
        assert 0.0 < row["measured"] < 1.0 and abs(row["deviation"]) < row["bound"], row
