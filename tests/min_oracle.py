"""TEST INFRASTRUCTURE ONLY: the specification of the device-resident FIRE minimiser, independent of the engine's sources.

FIRE (Bitzek, Koskinen, Gaehler, Moseler, Gumbsch, Phys. Rev. Lett. 97, 170201, 2006) as ASE ships it - unit masses, the step of a
whole molecule clamped to max_step - with one controller per molecule.  After every force evaluation, per molecule:
    vf = sum v.F,  ff = sum F.F,  vv = sum v.v,  fmax2 = max_i |F_i|^2          (fixed atoms left out)
    converged before: nothing.   a sum not finite: unusable.   sqrt(fmax2) < fmax: converged at this step.
    vf > 0:   c_v = 1 - alpha,  mix = alpha sqrt(vv / ff) (0 unless ff > 0 and vv > 0);
              n_pos > n_min: dt = min(dt f_inc, dt_max), alpha = alpha f_alpha;   n_pos += 1
    else:     c_v = 0, mix = 0, alpha = alpha0, dt = dt f_dec, n_pos = 0
    c_f = mix + dt;   |v_new|^2 = c_v^2 vv + 2 c_v c_f vf + c_f^2 ff;   len = dt |v_new|;   d = dt min(1, max_step / len)
and per atom v <- c_v v + c_f F, x <- x + d v (frozen molecule or fixed atom: v <- 0).  Python floats are IEEE fp64 and math.sqrt is
correctly rounded, so the controller below is a sequence of single fp64 operations; the coefficients are rounded to fp32 once."""
import math

import numpy as np

#: ASE's defaults, under the key names of TorchMD_Net.capture_minimize(fire=...), plus the convergence bound
FIRE = dict(dt=0.1, dt_max=1.0, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, max_step=0.2, fmax=0.05)

MOVING, FROZEN, UNUSABLE = 0, 1, 2


def new_state(p, n_mol):
    return [dict(dt=float(p["dt"]), alpha=float(p["alpha"]), n_pos=0, converged_at=-1) for _ in range(n_mol)]


def control64(s, p, vf, ff, vv, fmax2, step):
    """One molecule, its state dict updated in place -> (ret, (c_v, c_f, d) as Python floats)"""
    zero = (0.0, 0.0, 0.0)
    if s["converged_at"] >= 0:
        return FROZEN, zero
    if not all(math.isfinite(t) for t in (vf, ff, vv, fmax2)):
        return UNUSABLE, zero
    if math.sqrt(fmax2) < p["fmax"]:
        s["converged_at"] = step
        return FROZEN, zero
    if vf > 0.0:
        c_v = 1.0 - s["alpha"]
        mix = s["alpha"] * math.sqrt(vv / ff) if ff > 0.0 and vv > 0.0 else 0.0
        if s["n_pos"] > p["n_min"]:
            s["dt"] = min(s["dt"] * p["f_inc"], p["dt_max"])
            s["alpha"] = s["alpha"] * p["f_alpha"]
        s["n_pos"] += 1
    else:
        c_v, mix = 0.0, 0.0
        s["alpha"] = float(p["alpha"])
        s["dt"] = s["dt"] * p["f_dec"]
        s["n_pos"] = 0
    dt = s["dt"]
    c_f = mix + dt
    n2 = c_v * c_v * vv + 2.0 * c_v * c_f * vf + c_f * c_f * ff
    length = dt * math.sqrt(max(n2, 0.0))
    d = dt * (p["max_step"] / length) if length > p["max_step"] else dt
    return MOVING, (c_v, c_f, d)


def control(s, p, vf, ff, vv, fmax2, step):
    """-> (ret, (c_v, c_f, d) rounded to np.float32 once)"""
    ret, c = control64(s, p, vf, ff, vv, fmax2, step)
    return ret, tuple(np.float32(t) for t in c)


def sums(batch, n_mol, v, f, fixed=None):
    """fp64 sums of fp64 terms -> [n_mol, 4]: vf, ff, vv, fmax2"""
    v, f = np.asarray(v, np.float64), np.asarray(f, np.float64)
    free = np.ones(len(v)) if fixed is None else (np.asarray(fixed) == 0).astype(np.float64)
    out = np.zeros((n_mol, 4))
    ff = (f * f).sum(1) * free
    np.add.at(out[:, 0], batch, (v * f).sum(1) * free)
    np.add.at(out[:, 1], batch, ff)
    np.add.at(out[:, 2], batch, (v * v).sum(1) * free)
    np.maximum.at(out[:, 3], batch, ff)
    return out


def wells(batch, n_mol, kspring, x0, x, p, max_steps, fixed=None):
    """Harmonic wells F = -k (x - x0) in fp64, the coefficients used unrounded -> steps taken, converged_at [n_mol], final x"""
    batch = np.asarray(batch)
    k = np.asarray(kspring, np.float64)[:, None]
    x0, x = np.asarray(x0, np.float64), np.asarray(x, np.float64).copy()
    still = np.zeros(len(x), bool) if fixed is None else np.asarray(fixed) != 0
    v = np.zeros_like(x)
    state = new_state(p, n_mol)
    coef = np.zeros((n_mol, 3))
    step = 0
    while True:
        if step > 0:
            frozen = np.array([s["converged_at"] >= 0 for s in state])[batch] | still
            c = coef[batch]
            v = np.where(frozen[:, None], 0.0, c[:, 0:1] * v + c[:, 1:2] * f)
            x = np.where(frozen[:, None], x, x + c[:, 2:3] * v)
        f = -k * (x - x0)
        S = sums(batch, n_mol, v, f, fixed)
        for m in range(n_mol):
            ret, coef[m] = control64(state[m], p, *S[m], step)
            assert ret != UNUSABLE
        conv = np.array([s["converged_at"] for s in state])
        if (conv >= 0).all() or step == max_steps:
            return step, conv, x
        step += 1


# ---- the test problem: harmonic wells of five sizes -------------------------------------------------------------------------------
WELL_SIZES = (1, 3, 40, 64, 1500)
WELL_K = (0.5, 2.0, 10.0, 1.0, 4.0)


def wells_problem(seed=0, interleave=False):
    """-> batch [N] int64, kspring [N], x0 [N,3], x [N,3] (fp32-representable, x = x0 + 0.3 N(0,1)).  interleave: the atoms in a
    random order, so that no molecule is a contiguous range."""
    rng = np.random.default_rng(seed)
    batch = np.repeat(np.arange(len(WELL_SIZES)), WELL_SIZES)
    if interleave:
        batch = batch[rng.permutation(len(batch))]
    kspring = np.asarray(WELL_K, np.float32)[batch]
    x0 = (4.0 * rng.normal(size=(len(batch), 3))).astype(np.float32)
    x = (x0 + 0.3 * rng.normal(size=x0.shape)).astype(np.float32)
    return batch, kspring, x0, x


def ulp_distance(a, b):
    """|a - b| in units in the last place of fp32 (same-sign finite values)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
