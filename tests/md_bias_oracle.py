"""TEST INFRASTRUCTURE ONLY: an independent float64 statement of the collective-variable bias of the device-resident MD loop, against
which tests/test_md_bias_host.py checks torchmd-net_amd/csrc/tn_bias_math.h.  Nothing here shares a formula's FORM with the header:
the CVs are torch autograd on sqrt / acos / the projected-bond torsion, the wrap is math.remainder, the hill bookkeeping is Python
integers, the sums are math.fsum.  The recorded figures (largest deviations, the sampling protocol's scatter and bounds) live in
profiles/md_bias.json; ``python -m tests.md_bias_oracle`` measures the host part of that file again."""
import json
import math
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "md_bias.json")


def recorded():
    with open(RECORD) as fh:
        return json.load(fh)


# ---- collective variables -------------------------------------------------------------------------------------------------------
def cv_torch(kind, x):
    """x [4,3] float64 tensor (requires_grad) -> the CV as a 0-dim tensor.  distance: sqrt; angle: acos of the normalised dot
    product; torsion: the bonds b1, b3 projected onto the plane normal to b2, atan2 of their sine and cosine (IUPAC sign)."""
    if kind == "distance":
        return ((x[0] - x[1]) ** 2).sum().sqrt()
    if kind == "angle":
        a, b = x[0] - x[1], x[2] - x[1]
        return torch.acos((a * b).sum() / (a.norm() * b.norm()))
    b1, b2, b3 = x[1] - x[0], x[2] - x[1], x[3] - x[2]
    u = b2 / b2.norm()
    v = b1 - (b1 * u).sum() * u
    w = b3 - (b3 * u).sum() * u
    # looking along b2 the front bond is -b1 and the rear bond b3: the angle from -v to w, clockwise positive
    return torch.atan2((torch.linalg.cross(u, -v) * w).sum(), -(v * w).sum())


def cv(kind, x32):
    """fp32 positions [4,3] (numpy) -> (value, gradient [4,3]) in float64 by autograd"""
    x = torch.tensor(np.asarray(x32, np.float32).astype(np.float64), requires_grad=True)
    s = cv_torch(kind, x)
    (g,) = torch.autograd.grad(s, x)
    return float(s.detach()), g.numpy()


def diff(kind, a, b):
    d = a - b
    if kind != "torsion":
        return d
    d = math.remainder(d, 2.0 * math.pi)
    return d + 2.0 * math.pi if d <= -math.pi else d


def torsion_geometry(phi, scale=1.0, shift=0.0):
    """four atoms with torsion phi by construction: j at the origin, k on +z, i on +x, l at the standard angle phi about z.  Seen
    from j towards k a positive standard angle is a clockwise turn of the front bond onto the rear one: IUPAC positive."""
    x = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.3], [0.9 * math.cos(phi), 0.9 * math.sin(phi), 1.7]])
    return (scale * x + shift).astype(np.float32)


def angle_geometry(theta, scale=1.0, shift=0.0):
    x = np.array([[1.1, 0.0, 0.0], [0.0, 0.0, 0.0], [0.8 * math.cos(theta), 0.8 * math.sin(theta), 0.0], [0.0, 0.0, 0.0]])
    return (scale * x + shift).astype(np.float32)


def cv_cases():
    """[(name, kind, x [4,3] fp32)]: a diatomic; angles of 10, 90 and 170 degrees; torsions at 0, 60 degrees and +-(pi - 1e-3);
    everything again displaced to |x| ~ 100"""
    rot = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])  # a rotation: nothing is axis-aligned
    out = []
    for tag, shift in (("", 0.0), (" at |x| ~ 100", np.array([57.0, -61.0, 55.0]))):
        base = [("diatomic", "distance", np.array([[0.3, -0.2, 0.9], [-0.4, 0.5, 0.1], [0, 0, 0], [0, 0, 0]], np.float32))]
        base += [(f"angle {d} deg", "angle", angle_geometry(math.radians(d))) for d in (10, 90, 170)]
        base += [(f"torsion {name}", "torsion", torsion_geometry(p)) for name, p in
                 (("0", 0.0), ("60 deg", math.radians(60)), ("pi - 1e-3", math.pi - 1e-3), ("-(pi - 1e-3)", -(math.pi - 1e-3)))]
        for name, kind, x in base:
            out.append((name + tag, kind, (x.astype(np.float64) @ rot.T + shift).astype(np.float32)))
    return out


# ---- energies ---------------------------------------------------------------------------------------------------------------------
def restraint_energy(kind, kappa, delta):
    on = kind == "harmonic" or (kind == "upper" and delta > 0) or (kind == "lower" and delta < 0)
    return 0.5 * kappa * delta * delta if on else 0.0


def hills_energy(kinds, s, centres, heights, sigma):
    """V(s) of a hill list: kinds / s / sigma per metad dimension, centres [n][dm], heights [n]"""
    terms = []
    for c, w in zip(centres, heights):
        q = math.fsum((diff(k, sd, cd) / sg) ** 2 for k, sd, cd, sg in zip(kinds, s, c, sigma))
        terms.append(w * math.exp(-0.5 * q))
    return math.fsum(terms)


def bias_energy(x64, cvs, restraints=(), hills=None):
    """total bias energy of ONE walker at float64 positions x64 [n,3].  restraints = [(cv, kind, kappa, center)]; hills =
    dict(cvs=[...], sigma=[...], centres=[n][dm], heights=[n]).  Values by the oracle's own CV formulas (no autograd needed)."""
    x = torch.tensor(np.asarray(x64, np.float64))
    s = []
    for c in cvs:
        idx = list(c[1:]) + [0] * (5 - len(c))
        s.append(float(cv_torch(c[0], x[idx])))
    e = math.fsum(restraint_energy(kind, kappa, diff(cvs[c][0], s[c], center)) for c, kind, kappa, center in restraints)
    if hills is not None:
        e += hills_energy([cvs[c][0] for c in hills["cvs"]], [s[c] for c in hills["cvs"]], hills["centres"], hills["heights"], hills["sigma"])
    return e


def minus_central_difference(x32, cvs, restraints=(), hills=None, h=1e-5):
    """-dE/dx [n,3] of bias_energy at the fp32 positions widened to float64"""
    x = np.asarray(x32, np.float32).astype(np.float64)
    f = np.zeros_like(x)
    for i in range(x.shape[0]):
        for d in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, d] += h
            xm[i, d] -= h
            f[i, d] = -(bias_energy(xp, cvs, restraints, hills) - bias_energy(xm, cvs, restraints, hills)) / (2 * h)
    return f


# ---- which hills exist (Python integers) -----------------------------------------------------------------------------------------
def visible(n, step0, pace, W, base, H):
    return min(H, base + ((n - step0) // pace) * W) if n >= step0 else min(H, base)


def slot(n, step0, pace, W, w, base, H):
    if n + 1 <= step0 or (n + 1 - step0) % pace:
        return -1
    s = base + ((n + 1 - step0) // pace - 1) * W + w
    return s if s < H else -1


def height(h0, V, kT, gamma):
    return h0 * math.exp(-V / (kT * (gamma - 1.0))) if gamma else h0


# ---- hill bookkeeping over many deposits ------------------------------------------------------------------------------------------
BOOK_CVS = [("distance", 0, 1), ("torsion", 0, 1, 2, 3)]


def book_positions(rng, B):
    """B walkers of 4 atoms: a bent chain, jittered - every CV stays well away from a degenerate geometry"""
    base = np.array([[1.0, 0.2, 0.0], [0.0, 0.0, 0.0], [0.1, 0.0, 1.4], [0.9, 0.8, 1.9]])
    return (base[None] + 0.25 * rng.standard_normal((B, 4, 3))).astype(np.float32).reshape(-1, 3)


def run_bookkeeping(HM, W, dm, deposits=200, step0=7, base=5, pace=3, G=2, gamma=6.0):
    """`deposits` deposit steps of G groups of W walkers on positions drawn anew every step, the mirror against this oracle: the
    visible count and the written slots as Python integers (asserted here, exactly), the hill centres against the oracle's CVs,
    and the bias energy and the heights against the oracle's own hill lists.  -> largest relative deviation of (V, height)"""
    rng = np.random.default_rng(1000 * W + dm)
    B, H = G * W, base + deposits * W
    metad = dict(cvs=[1, 0][:dm], sigma=[0.35, 0.12][:dm], height=0.7, pace=pace, kT=0.9, bias_factor=gamma)
    wk = HM.Walkers(B, 4, BOOK_CVS, metad=metad, W=W, H=H, step0=step0, base=base)
    kinds = [BOOK_CVS[c][0] for c in metad["cvs"]]
    lists = []
    for g in range(G):  # the hills the run starts from
        c = np.stack([rng.uniform(-3.0, 3.0, base) if k == "torsion" else rng.uniform(0.8, 2.0, base) for k in kinds], 1)
        w = rng.uniform(0.1, 0.7, base)
        wk.hills[g, :dm, :base], wk.hills[g, dm, :base] = c.T, w
        lists.append(([list(r) for r in c], list(w)))
    dev_V = dev_h = 0.0
    for n in range(step0, step0 + deposits * pace):
        pos = book_positions(rng, B)
        nvis = visible(n, step0, pace, W, base, H)
        assert HM.visible(n, step0, pace, W, base, H) == nvis == len(lists[0][1]), n
        out = wk.launch(n, pos, np.zeros_like(pos))
        assert wk.status[0] == 0
        due = (n + 1 - step0) % pace == 0
        new = [[] for _ in range(G)]
        for b in range(B):
            g, w = divmod(b, W)
            sl = slot(n, step0, pace, W, w, base, H)
            assert HM.slot(n, step0, pace, W, w, base, H) == sl and (sl >= 0) == due
            if not due:
                continue
            x = torch.tensor(pos[4 * b:4 * b + 4].astype(np.float64))
            s = [float(cv_torch(BOOK_CVS[c][0], x[list(BOOK_CVS[c][1:]) + [0] * (5 - len(BOOK_CVS[c]))])) for c in metad["cvs"]]
            V = hills_energy(kinds, s, lists[g][0], lists[g][1], metad["sigma"])
            h = height(metad["height"], V, metad["kT"], gamma)
            dev_V = max(dev_V, abs(out["bias"][b] - V) / max(abs(V), 1.0))
            dev_h = max(dev_h, abs(wk.hills[g, dm, sl] - h) / h)
            assert np.abs(wk.hills[g, :dm, sl] - np.array(s)).max() < 1e-12
            new[g].append((sl, s, h))
        for g in range(G):
            for sl, s, h in new[g]:
                assert sl == len(lists[g][1])  # slots are written densely, in walker order
                lists[g][0].append(s)
                lists[g][1].append(h)
    assert len(lists[0][1]) == H and not np.isnan(wk.hills).any()
    return dev_V, dev_h


# ---- the sampling protocol --------------------------------------------------------------------------------------------------------
SAMPLING = dict(B=4, W=4, r0=1.5, dt=0.005, friction=5.0, kT=1.0, gamma=8.0, h0=0.3, sigma=0.1, pace=100, steps=75000,
                seeds=[11, 12, 13, 14, 15, 16, 17, 18], mirror_seed=2024)


def potential(r):
    return 8.0 * ((r - 2.0) ** 2 / 0.25 - 1.0) ** 2


def exact_free_energy(r, kT=1.0):
    return potential(r) - 2.0 * kT * np.log(r)


def estimate(r, centres, heights, sigma, gamma):
    """-gamma / (gamma - 1) V(r) of one hill list, numpy float64"""
    r, c, w = np.asarray(r, np.float64), np.asarray(centres, np.float64), np.asarray(heights, np.float64)
    V = (w[None, :] * np.exp(-0.5 * ((r[:, None] - c[None, :]) / sigma) ** 2)).sum(1)
    return -(gamma / (gamma - 1.0)) * V


def _basin(F, r, lo, hi, kT):
    m = (r >= lo) & (r <= hi)
    y, x = np.exp(-F[m] / kT), r[m]
    return -kT * math.log(float((0.5 * (y[1:] + y[:-1]) * (x[1:] - x[:-1])).sum()))


def sampling_errors(centres, heights, e=SAMPLING):
    """-> (mean-removed RMS of estimate - exact on 1.35..2.65, basin difference F(2.0..2.8) - F(1.2..2.0) of the estimate)"""
    r = np.linspace(1.35, 2.65, 131)
    d = estimate(r, centres, heights, e["sigma"], e["gamma"]) - exact_free_energy(r, e["kT"])
    rms = float(np.sqrt(((d - d.mean()) ** 2).mean()))
    rb = np.linspace(1.2, 2.8, 801)
    Fb = estimate(rb, centres, heights, e["sigma"], e["gamma"])
    return rms, _basin(Fb, rb, 2.0, 2.8, e["kT"]) - _basin(Fb, rb, 1.2, 2.0, e["kT"])


def exact_basin_difference(kT=1.0):
    rb = np.linspace(1.2, 2.8, 801)
    F = exact_free_energy(rb, kT)
    return _basin(F, rb, 2.0, 2.8, kT) - _basin(F, rb, 1.2, 2.0, kT)


def sample(seed, e=SAMPLING):
    """The protocol in numpy float64 with numpy's generator: B walkers of one group, one mobile atom of mass 1 bound to the origin,
    B A [F + bias] B O per step, a hill per walker every `pace` steps at the value and the V(s) of that step's evaluation.
    -> (centres [n], heights [n])"""
    rng = np.random.default_rng(seed)
    B, dt, kT, sg, gamma = e["B"], e["dt"], e["kT"], e["sigma"], e["gamma"]
    c1 = math.exp(-e["friction"] * dt)
    c2 = math.sqrt(1.0 - c1 * c1)
    H = (e["steps"] // e["pace"]) * B
    cen, hgt, nh = np.zeros(H), np.zeros(H), 0
    x = np.zeros((B, 3))
    x[:, 0] = e["r0"]
    v = np.zeros((B, 3))

    def force(x, nvis):
        r = np.sqrt((x * x).sum(1))
        u = r - 2.0
        dU = 8.0 * 2.0 * (u * u / 0.25 - 1.0) * (2.0 * u / 0.25)
        dl = r[:, None] - cen[None, :nvis]
        t = hgt[None, :nvis] * np.exp(-0.5 * (dl / sg) ** 2)
        V = t.sum(1)
        dV = -(t * dl).sum(1) / (sg * sg)
        return -((dU + dV) / r)[:, None] * x, r, V

    f, _, _ = force(x, 0)
    for n in range(e["steps"]):
        v += 0.5 * dt * f
        x += dt * v
        f, r, V = force(x, nh)
        if (n + 1) % e["pace"] == 0:
            cen[nh:nh + B] = r
            hgt[nh:nh + B] = e["h0"] * np.exp(-V / (kT * (gamma - 1.0)))
            nh += B
        v += 0.5 * dt * f
        v = c1 * v + c2 * math.sqrt(kT) * rng.standard_normal((B, 3))
    return cen[:nh], hgt[:nh]


# ---- recording --------------------------------------------------------------------------------------------------------------------
def measure_host():
    """the host part of profiles/md_bias.json: the largest deviations of the header from this oracle and the sampling scatter"""
    from tests import md_bias_host_mirror as HM

    out = {}
    worst_s, worst_g = 0.0, 0.0
    for name, kind, x in cv_cases():
        s, g = HM.cv([kind], x[None])
        so, go = cv(kind, x)
        n = {"distance": 2, "angle": 3, "torsion": 4}[kind]
        worst_s = max(worst_s, abs(s[0] - so) / max(abs(so), 1.0))
        worst_g = max(worst_g, float(np.abs(g[0, :n] - go[:n]).max() / np.abs(go[:n]).max()))
    out["cv_value_rel_dev"], out["cv_gradient_rel_dev"] = worst_s, worst_g
    devs = [run_bookkeeping(HM, W, dm) for W in (1, 3) for dm in (1, 2)]
    out["hill_energy_rel_dev"], out["hill_height_rel_dev"] = max(d[0] for d in devs), max(d[1] for d in devs)
    errs = [sampling_errors(*sample(seed)) for seed in SAMPLING["seeds"]]
    exact = exact_basin_difference()
    rms = np.array([r for r, _ in errs])
    bas = np.array([abs(b - exact) for _, b in errs])
    out["sampling"] = dict(protocol={k: v for k, v in SAMPLING.items()}, exact_basin_difference=exact,
                           oracle_rms=rms.tolist(), oracle_basin_difference=[b for _, b in errs],
                           rms_bound=float(rms.mean() + 4 * rms.std(ddof=1)),
                           basin_error_bound=float(bas.mean() + 4 * bas.std(ddof=1)))
    return out


if __name__ == "__main__":
    rec = recorded() if os.path.exists(RECORD) else {}
    rec.setdefault("host", {}).update(measure_host())
    with open(RECORD, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec["host"], indent=1))
