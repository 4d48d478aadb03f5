// Arithmetic of the device-resident minima hopping (tn_hop.hip): the per-atom terms of the sums every phase needs, the aligned RMSD
// from the 18 sums of a pair of geometries, the removal of momentum and angular momentum, the per-walker phase machine and the
// per-atom move it decides.  Minima hopping: Goedecker, J. Chem. Phys. 120, 9911 (2004), parameters named as in ASE's MinimaHopping;
// the quench is FIRE (tn_min_math.h), the escape an NVE run (tn_md_math.h).  __host__ __device__: tests/hop_host.hip compiles this
// header host-only, so the statements a GPU lane runs are the statements the host checker runs.
//
// Rounding.  Everything per atom that moves an atom is fp32 under the contract of tn_md_math.h: one md_mul or md_add per operation,
// in the order written.  The terms of the sums of LAUNCH and COMPARE are fp64 products of widened fp32 values (exact for a product of
// two fp32 values), summed in fp64.  Everything per walker is fp64 in the order written and rounded to fp32 once where atoms consume
// it: FIRE's coefficients, the centroid, u and omega of the launch, sqrt(kT).  tn_hop.hip and the host checker compile with fp
// contraction off, so an fp64 product is never fused into the sum that consumes it.
#pragma once
#include "tn_min_math.h"

namespace tn_hop {

using tn_md::md_add;
using tn_md::md_mul;

enum { PH_QUENCH = 0, PH_COMPARE = 1, PH_LAUNCH = 2, PH_MD = 3 };
// what a step decided for its walker (the `outcome` log): nothing, the start geometry's minimum, the four classifications of a hop,
// a quench that ran out of steps, and - logged at the LAUNCH step - an inertia tensor too singular to remove the rotation
enum { OUT_NONE = 0, OUT_START = 1, OUT_SAME = 2, OUT_KNOWN = 3, OUT_ACCEPTED = 4, OUT_REJECTED = 5, OUT_UNCONVERGED = 6, OUT_SINGULAR = 7 };
enum { ALIGN_NONE = 0, ALIGN_TRANSLATION = 1, ALIGN_ROTATION = 2 };
// what the per-atom kernel does with the walker's atoms
enum { ACT_NONE = 0, ACT_FIRE = 1, ACT_RECORD = 2, ACT_LAUNCH = 3, ACT_MD = 4, ACT_STOP = 5, ACT_HALT = 6 };

constexpr int kMaxCapacity = 64;
constexpr int kPair = 18;      // sums of a pair (a, b): n, sum a (3), sum b (3), sum a.a, sum b.b, sum a_i b_j (9, row i)
constexpr int kLaunch = 17;    // sum m, m d (3), m v (3), m d x v (3), m dx dx, dy dy, dz dz, dx dy, dx dz, dy dz; then f.f, which
                               // the controller only asks to be finite: the launch's opening half-step consumes the forces
constexpr int kSumsLog = 16;   // width of a row of the `sums` log
constexpr int kCoefLog = 10;   // c_v, c_f, d, u (3), omega (3), sqrt(kT)
constexpr int kCounters = 7;   // n_hops, n_same, n_known, n_new, n_accepted, n_unconverged, n_recorded
constexpr int kJacobiSweeps = 12;

struct HopParams {
  tn_min::FireParams fire;
  double dt0;  // FIRE's start time step
  double beta1, beta2, beta3, alpha1, alpha2, rmsd_tol, energy_tol;
  uint64_t seed;
  float dt;  // the MD time step
  int32_t mdmin, md_steps, opt_steps, capacity, align;
};

// the parameters of a tmdnet_hop_args (include/tmdnet_amd.h; a template, so that this header needs no other): the ONE place they are
// read, for the kernels and for the host checker alike
template <class Args>
inline HopParams hop_params(const Args& a) {
  HopParams p;
  p.fire.dt_max = a.dt_max;
  p.fire.f_inc = a.f_inc;
  p.fire.f_dec = a.f_dec;
  p.fire.alpha0 = a.alpha0;
  p.fire.f_alpha = a.f_alpha;
  p.fire.max_step = a.max_step;
  p.fire.fmax = a.fmax;
  p.fire.n_min = a.n_min;
  p.dt0 = a.dt0;
  p.beta1 = a.beta1;
  p.beta2 = a.beta2;
  p.beta3 = a.beta3;
  p.alpha1 = a.alpha1;
  p.alpha2 = a.alpha2;
  p.rmsd_tol = a.rmsd_tol;
  p.energy_tol = a.energy_tol;
  p.seed = a.seed;
  p.dt = a.dt;
  p.mdmin = a.mdmin;
  p.md_steps = a.md_steps;
  p.opt_steps = a.opt_steps;
  p.capacity = a.capacity;
  p.align = a.align;
  return p;
}

struct Walker {  // per walker, in the workspace
  double kT, ediff, dt, alpha, e_cur, e_best, e_prev2, e_prev1;
  double cen[3];  // the centroid of the current minimum
  double natoms;  // the walker's number of atoms, as the last COMPARE step counted them
  int64_t n[kCounters];
  int32_t phase, n_pos, quench_steps, md_k, md_count, has_cur;
};

struct Decision {  // per walker, from the controller to the per-atom kernel
  int32_t action, slot, accept, best, outcome, phase;  // slot: the ring slot that receives pos, or -1; phase: the one this step ran in
  uint32_t hop_lo, hop_hi;
  float coef[3], u[3], w[3], cen[3], vscale;
};

struct Ring {  // one walker's view of the history
  double* energy;    // [capacity]
  int64_t* found_at; // [capacity]
  int64_t* visits;   // [capacity]
};

// ---- per-atom terms ---------------------------------------------------------------------------------------------------------------
// MD: t[0] the kinetic energy of the closed velocity kick(v, hk, f), t[1] = f.f, t[2] = 0, t[3] = f.f (its maximum is taken)
MD_FN void md_terms(const float v[3], const float f[3], float hk, float m, int fixed, float t[4]) {
  t[0] = t[1] = t[2] = t[3] = 0.f;
  if (fixed) return;
  t[0] = tn_md::kinetic(m, tn_md::kick(v[0], hk, f[0]), tn_md::kick(v[1], hk, f[1]), tn_md::kick(v[2], hk, f[2]));
  t[1] = tn_min::dot3(f, f);
  t[3] = t[1];
}

// QUENCH: FIRE's terms and, in t[3], f.f again for the maximum
MD_FN void quench_terms(const float v[3], const float f[3], int fixed, float t[4]) {
  tn_min::atom_terms(v, f, fixed, t);
  t[3] = t[1];
}

// LAUNCH: d = x - cen in fp32 (one md_add per component), then fp64 products of the widened values; last, f.f
MD_FN void launch_terms(const float x[3], const float v[3], const float f[3], float m, const float cen[3], int fixed,
                        double t[kLaunch]) {
  for (int k = 0; k < kLaunch; ++k) t[k] = 0.0;
  if (fixed) return;
  const double dx = (double)md_add(x[0], -cen[0]), dy = (double)md_add(x[1], -cen[1]), dz = (double)md_add(x[2], -cen[2]);
  const double vx = v[0], vy = v[1], vz = v[2], mm = m;
  t[0] = mm;
  t[1] = mm * dx;
  t[2] = mm * dy;
  t[3] = mm * dz;
  t[4] = mm * vx;
  t[5] = mm * vy;
  t[6] = mm * vz;
  t[7] = mm * (dy * vz - dz * vy);
  t[8] = mm * (dz * vx - dx * vz);
  t[9] = mm * (dx * vy - dy * vx);
  t[10] = mm * (dx * dx);
  t[11] = mm * (dy * dy);
  t[12] = mm * (dz * dz);
  t[13] = mm * (dx * dy);
  t[14] = mm * (dx * dz);
  t[15] = mm * (dy * dz);
  const double fx = f[0], fy = f[1], fz = f[2];
  t[16] = (fx * fx + fy * fy) + fz * fz;
}

// COMPARE: the terms of one atom of the pair (new geometry a, reference b)
MD_FN void pair_terms(const float a[3], const float b[3], double t[kPair]) {
  const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2];
  t[0] = 1.0;
  t[1] = ax;
  t[2] = ay;
  t[3] = az;
  t[4] = bx;
  t[5] = by;
  t[6] = bz;
  t[7] = (ax * ax + ay * ay) + az * az;
  t[8] = (bx * bx + by * by) + bz * bz;
  t[9] = ax * bx;
  t[10] = ax * by;
  t[11] = ax * bz;
  t[12] = ay * bx;
  t[13] = ay * by;
  t[14] = ay * bz;
  t[15] = az * bx;
  t[16] = az * by;
  t[17] = az * bz;
}

// ---- the aligned RMSD ---------------------------------------------------------------------------------------------------------------
// largest eigenvalue of a symmetric 4 x 4 matrix (upper triangle of A read, A destroyed): kJacobiSweeps cyclic Jacobi sweeps
MD_FN double jacobi_max4(double A[4][4]) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < i; ++j) A[i][j] = A[j][i];
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) {  // columns p, q
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {  // rows p, q
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
      }
  double mx = A[0][0];
  for (int i = 1; i < 4; ++i) mx = A[i][i] > mx ? A[i][i] : mx;
  return mx;
}

// rmsd^2 of the pair from its sums.  ALIGN_ROTATION: Horn's quaternion method (J. Opt. Soc. Am. A 4, 629, 1987) on the centred
// cross-covariance - proper rotations only, so a mirror image keeps a positive distance; fewer than 3 atoms: translation only.
// Never negative; not finite only when a sum is not.
MD_FN double pair_rmsd2(const double s[kPair], int align) {
  const double n = s[0];
  if (!(n > 0.0)) return 0.0;
  double r2;
  if (align == ALIGN_NONE) {
    r2 = ((s[7] + s[8]) - 2.0 * ((s[9] + s[13]) + s[17])) / n;
  } else {
    const double ga = s[7] - ((s[1] * s[1] + s[2] * s[2]) + s[3] * s[3]) / n;
    const double gb = s[8] - ((s[4] * s[4] + s[5] * s[5]) + s[6] * s[6]) / n;
    double S[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) S[i][j] = s[9 + 3 * i + j] - (s[1 + i] * s[4 + j]) / n;
    double lam;
    if (align == ALIGN_ROTATION && n >= 3.0) {
      double A[4][4];
      A[0][0] = (S[0][0] + S[1][1]) + S[2][2];
      A[0][1] = S[1][2] - S[2][1];
      A[0][2] = S[2][0] - S[0][2];
      A[0][3] = S[0][1] - S[1][0];
      A[1][1] = (S[0][0] - S[1][1]) - S[2][2];
      A[1][2] = S[0][1] + S[1][0];
      A[1][3] = S[2][0] + S[0][2];
      A[2][2] = (S[1][1] - S[0][0]) - S[2][2];
      A[2][3] = S[1][2] + S[2][1];
      A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
      lam = jacobi_max4(A);
    } else {
      lam = (S[0][0] + S[1][1]) + S[2][2];
    }
    r2 = ((ga + gb) - 2.0 * lam) / n;
  }
  return r2 < 0.0 ? 0.0 : r2;  // (a NaN stays a NaN)
}

// ---- the launch: remove momentum and, with ALIGN_ROTATION, angular momentum ---------------------------------------------------------
// From the sums about the centroid `cen`: v_com = P / M; about the centre of mass d_cm = (sum m d) / M the angular momentum is
// L - d_cm x P and the inertia tensor I - M (|d_cm|^2 1 - d_cm d_cm^T); omega solves I omega = L by an LDL^T elimination.  The
// atoms then take v <- v - (u + omega x d) with u = v_com - omega x d_cm.  A pivot below 1e-10 of the trace (a linear or a
// one-atom molecule): omega = 0 and *singular = 1.  No free mass: everything zero.
MD_FN void launch_solve(const double t[kLaunch], int align, float u32[3], float w32[3], int* singular) {
  *singular = 0;
  double u[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
  const double M = t[0];
  if (M > 0.0) {
    const double dcm[3] = {t[1] / M, t[2] / M, t[3] / M}, vcm[3] = {t[4] / M, t[5] / M, t[6] / M};
    if (align == ALIGN_ROTATION) {
      const double L[3] = {t[7] - (dcm[1] * t[6] - dcm[2] * t[5]), t[8] - (dcm[2] * t[4] - dcm[0] * t[6]),
                           t[9] - (dcm[0] * t[5] - dcm[1] * t[4])};
      const double xx = t[10] - M * (dcm[0] * dcm[0]), yy = t[11] - M * (dcm[1] * dcm[1]), zz = t[12] - M * (dcm[2] * dcm[2]);
      const double xy = t[13] - M * (dcm[0] * dcm[1]), xz = t[14] - M * (dcm[0] * dcm[2]), yz = t[15] - M * (dcm[1] * dcm[2]);
      const double a00 = yy + zz, a11 = xx + zz, a22 = xx + yy, a01 = -xy, a02 = -xz, a12 = -yz;
      const double floor_ = 1e-10 * ((a00 + a11) + a22);
      // LDL^T in the order written
      const double d0 = a00;
      bool ok = d0 > floor_ && floor_ > 0.0;
      double l10 = 0.0, l20 = 0.0, l21 = 0.0, d1 = 0.0, d2 = 0.0;
      if (ok) {
        l10 = a01 / d0;
        l20 = a02 / d0;
        d1 = a11 - l10 * a01;
        ok = d1 > floor_;
      }
      if (ok) {
        l21 = (a12 - l20 * a01) / d1;
        d2 = (a22 - l20 * a02) - (l21 * l21) * d1;
        ok = d2 > floor_;
      }
      if (ok) {
        const double y0 = L[0], y1 = L[1] - l10 * y0, y2 = (L[2] - l20 * y0) - l21 * y1;
        w[2] = y2 / d2;
        w[1] = y1 / d1 - l21 * w[2];
        w[0] = (y0 / d0 - l10 * w[1]) - l20 * w[2];
        ok = isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]);
      }
      if (!ok) {
        w[0] = w[1] = w[2] = 0.0;
        *singular = 1;
      }
    }
    u[0] = vcm[0] - (w[1] * dcm[2] - w[2] * dcm[1]);
    u[1] = vcm[1] - (w[2] * dcm[0] - w[0] * dcm[2]);
    u[2] = vcm[2] - (w[0] * dcm[1] - w[1] * dcm[0]);
  }
  for (int k = 0; k < 3; ++k) {
    u32[k] = (float)u[k];
    w32[k] = (float)w[k];
  }
}

// ---- the phase machine ------------------------------------------------------------------------------------------------------------
MD_FN void walker_reset(Walker* w, const HopParams& p, double kT, double ediff, int keep_history) {
  w->kT = kT;
  w->ediff = ediff;
  w->dt = p.dt0;
  w->alpha = p.fire.alpha0;
  w->e_cur = w->e_prev1 = w->e_prev2 = 0.0;
  w->cen[0] = w->cen[1] = w->cen[2] = 0.0;
  w->natoms = 0.0;
  w->phase = PH_QUENCH;
  w->n_pos = w->quench_steps = w->md_k = w->md_count = w->has_cur = 0;
  if (!keep_history) {
    w->e_best = 0.0;
    for (int k = 0; k < kCounters; ++k) w->n[k] = 0;
  }
}

// live entries of the ring
MD_FN int ring_live(const Walker& w, int capacity) { return w.n[6] < capacity ? (int)w.n[6] : capacity; }

// is reference r of a COMPARE step looked at?  r = 0: the current minimum (always: its pair also carries the new geometry's own
// sums; without a current minimum the new geometry is paired with itself); r >= 1: ring slot r - 1, when it is live and its
// energy lies within energy_tol of E
MD_FN bool ref_considered(const Walker& w, const double* ring_energy, int capacity, int r, double E, double energy_tol) {
  if (r == 0) return true;
  return r - 1 < ring_live(w, capacity) && fabs(E - ring_energy[r - 1]) < energy_tol;
}

// how many leading entries of the walker's sums this step uses in QUENCH, MD and LAUNCH (COMPARE: kPair per considered reference)
MD_FN int phase_sums(int phase) { return phase == PH_LAUNCH ? kLaunch : 4; }

// are the energy and every sum this step's control reads finite?
MD_FN bool walker_usable(const Walker& w, const Ring& ring, const HopParams& p, const double* tot, double E) {
  if (!isfinite(E)) return false;
  if (w.phase != PH_COMPARE) {
    for (int k = 0; k < phase_sums(w.phase); ++k)
      if (!isfinite(tot[k])) return false;
    return true;
  }
  for (int r = 0; r <= p.capacity; ++r) {
    if (!ref_considered(w, ring.energy, p.capacity, r, E, p.energy_tol)) continue;
    for (int k = 0; k < kPair; ++k)
      if (!isfinite(tot[r * kPair + k])) return false;
  }
  return true;
}

// the ring slot whose geometry is the new one (rmsd < rmsd_tol among the considered entries; the lowest slot wins), or -1
MD_FN int ring_match(const Walker& w, const Ring& ring, const HopParams& p, const double* tot, double E, int align, double* best_r2) {
  int hit = -1;
  *best_r2 = -1.0;
  for (int r = 1; r <= p.capacity; ++r) {
    if (!ref_considered(w, ring.energy, p.capacity, r, E, p.energy_tol)) continue;
    const double r2 = pair_rmsd2(tot + r * kPair, align);
    if (*best_r2 < 0.0 || r2 < *best_r2) *best_r2 = r2;
    if (hit < 0 && r2 < p.rmsd_tol * p.rmsd_tol) hit = r - 1;
  }
  return hit;
}

// the geometry at pos goes into the ring: slot n_recorded mod capacity, the oldest entry is overwritten
MD_FN int ring_record(Walker* w, const Ring& ring, const HopParams& p, double E, int64_t step) {
  const int slot = (int)(w->n[6] % p.capacity);
  ring.energy[slot] = E;
  ring.found_at[slot] = step;
  ring.visits[slot] = 1;
  w->n[6] += 1;
  return slot;
}

// the launch that follows a COMPARE step or an UNCONVERGED quench: the per-atom kernel records / restores and draws velocities
MD_FN void decide_record(const Walker& w, Decision* d) {
  d->action = ACT_RECORD;
  d->vscale = (float)sqrt(w.kT);
  d->hop_lo = (uint32_t)(uint64_t)w.n[0];
  d->hop_hi = (uint32_t)((uint64_t)w.n[0] >> 32);
}

// One step of one walker that walker_usable() has passed: the state, the ring's books and the decision, and the row of the `sums`
// log (zero-filled behind what the phase uses; COMPARE: rmsd^2 to the current minimum or -1, the smallest rmsd^2 to a considered
// ring entry or -1, the number of atoms).  E: this step's energy; `tot`: this step's sums; `step`: the step this is.
MD_FN void walker_control(Walker* w, const Ring& ring, const HopParams& p, const double* tot, double E, int64_t step, Decision* d,
                          double sums_log[kSumsLog]) {
  const int align = p.align;
  d->action = ACT_NONE;
  d->slot = -1;
  d->accept = d->best = 0;
  d->outcome = OUT_NONE;
  d->phase = w->phase;
  d->hop_lo = d->hop_hi = 0u;
  d->vscale = 0.f;
  for (int k = 0; k < 3; ++k) {
    d->coef[k] = d->u[k] = d->w[k] = 0.f;
    d->cen[k] = (float)w->cen[k];
  }
  for (int k = 0; k < kSumsLog; ++k) sums_log[k] = 0.0;
  if (w->phase != PH_COMPARE)
    for (int k = 0; k < phase_sums(w->phase) && k < kSumsLog; ++k) sums_log[k] = tot[k];

  if (w->phase == PH_QUENCH) {
    tn_min::FireState s = {w->dt, w->alpha, w->n_pos, -1};
    const int ret = tn_min::fire_control(&s, p.fire, tot[0], tot[1], tot[2], tot[3], step, d->coef);
    if (ret == tn_min::FIRE_FROZEN) {  // converged: the walker does not move
      w->phase = PH_COMPARE;
      d->action = ACT_HALT;
    } else if (w->has_cur && w->quench_steps >= p.opt_steps) {  // out of steps: back to the current minimum, kT and ediff untouched
      d->coef[0] = d->coef[1] = d->coef[2] = 0.f;
      d->outcome = OUT_UNCONVERGED;
      w->n[0] += 1;
      w->n[5] += 1;
      w->phase = PH_LAUNCH;
      decide_record(*w, d);
    } else {
      w->dt = s.dt;
      w->alpha = s.alpha;
      w->n_pos = s.n_pos;
      w->quench_steps += 1;
      d->action = ACT_FIRE;
    }
    return;
  }

  if (w->phase == PH_COMPARE) {
    const double n = tot[0];
    const double cen[3] = {tot[1] / n, tot[2] / n, tot[3] / n};
    double ring_r2;
    const int hit = ring_match(*w, ring, p, tot, E, align, &ring_r2);
    sums_log[0] = -1.0;
    sums_log[1] = ring_r2;
    sums_log[2] = n;
    w->natoms = n;
    if (!w->has_cur) {  // the start: record (unless a kept history knows it), accept, change no parameter
      d->outcome = OUT_START;
      if (hit >= 0) {
        ring.visits[hit] += 1;
      } else {
        d->slot = ring_record(w, ring, p, E, step);
      }
      d->accept = 1;
    } else {
      const double r2 = pair_rmsd2(tot, align);
      sums_log[0] = r2;
      w->n[0] += 1;
      if (fabs(E - w->e_cur) < p.energy_tol && r2 < p.rmsd_tol * p.rmsd_tol) {
        d->outcome = OUT_SAME;
        w->kT = w->kT * p.beta1;
        w->n[1] += 1;
      } else if (hit >= 0) {
        d->outcome = OUT_KNOWN;
        w->kT = w->kT * p.beta2;
        ring.visits[hit] += 1;
        w->n[2] += 1;
      } else {
        w->kT = w->kT * p.beta3;
        w->n[3] += 1;
        d->slot = ring_record(w, ring, p, E, step);
        if (E < w->e_cur + w->ediff) {
          d->outcome = OUT_ACCEPTED;
          w->ediff = w->ediff * p.alpha1;
          w->n[4] += 1;
          d->accept = 1;
        } else {
          d->outcome = OUT_REJECTED;
          w->ediff = w->ediff * p.alpha2;
        }
      }
    }
    if (d->slot >= 0 && (w->n[6] == 1 || E < w->e_best)) {  // (n_recorded == 1: the first entry ever)
      w->e_best = E;
      d->best = 1;
    }
    if (d->accept) {
      w->has_cur = 1;
      w->e_cur = E;
      for (int k = 0; k < 3; ++k) w->cen[k] = cen[k];
    }
    w->phase = PH_LAUNCH;
    decide_record(*w, d);
    return;
  }

  if (w->phase == PH_LAUNCH) {
    int singular;  // (fewer than 3 atoms have no inertia tensor to invert: the translation path)
    launch_solve(tot, align == ALIGN_ROTATION && w->natoms < 3.0 ? ALIGN_TRANSLATION : align, d->u, d->w, &singular);
    if (singular) d->outcome = OUT_SINGULAR;
    d->action = ACT_LAUNCH;
    w->e_prev1 = w->e_prev2 = E;  // E_0
    w->md_k = 0;
    w->md_count = 0;
    w->phase = PH_MD;
    return;
  }

  // PH_MD: E is E_k of this escape
  const int k = w->md_k + 1;
  if (k >= 2 && w->e_prev1 < w->e_prev2 && w->e_prev1 <= E) w->md_count += 1;
  w->e_prev2 = w->e_prev1;
  w->e_prev1 = E;
  w->md_k = k;
  if (w->md_count < p.mdmin && k < p.md_steps) {
    d->action = ACT_MD;
    return;
  }
  // the escape ends in this step: v = 0, FIRE starts afresh and moves at once - no evaluation is spent on the transition
  tn_min::FireState s = {p.dt0, p.fire.alpha0, 0, -1};
  const int ret = tn_min::fire_control(&s, p.fire, 0.0, tot[1], 0.0, tot[3], step, d->coef);
  w->dt = s.dt;
  w->alpha = s.alpha;
  w->n_pos = s.n_pos;
  if (ret == tn_min::FIRE_FROZEN) {  // (the escape ended on a stationary point)
    w->quench_steps = 0;
    w->phase = PH_COMPARE;
    d->action = ACT_HALT;
  } else {
    w->quench_steps = 1;
    w->phase = PH_QUENCH;
    d->action = ACT_STOP;
  }
}

// ---- the per-atom move ------------------------------------------------------------------------------------------------------------
// the velocity draw of a launch: counter (hop lo, hop hi, the caller's atom index, 2) - word 3 keeps the stream apart from the
// Langevin (0) and barostat (1) streams
MD_FN void launch_noise(uint64_t seed, uint32_t hop_lo, uint32_t hop_hi, uint32_t atom, float xi[3]) {
  const uint32_t c[4] = {hop_lo, hop_hi, atom, 2u};
  const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  tn_md::philox4x32_10(c, k, w);
  tn_md::normals3(w, xi);
}

// What the walker's decision does to one atom.  x, v in / out; cur, ring, best: this atom's row of the current minimum, of the ring
// slot d.slot (NULL when d.slot < 0) and of the best minimum.  sig = sqrt(force_scale / m), hk = dt force_scale / (2 m); a fixed
// atom never moves and has zero velocity.
MD_FN void atom_apply(const Decision& d, float dt, uint64_t seed, uint32_t atom, int fixed, float hk, float sig, const float f[3],
                      float x[3], float v[3], float* cur, float* ring, float* best) {
  switch (d.action) {
    case ACT_FIRE:
      if (fixed) {
        v[0] = v[1] = v[2] = 0.f;
      } else {
        tn_min::atom_move(x, v, f, d.coef[0], d.coef[1], d.coef[2]);
      }
      break;
    case ACT_STOP:
      v[0] = v[1] = v[2] = 0.f;
      if (!fixed) tn_min::atom_move(x, v, f, d.coef[0], d.coef[1], d.coef[2]);
      break;
    case ACT_HALT:
      v[0] = v[1] = v[2] = 0.f;
      break;
    case ACT_MD:
      if (!fixed) {
        for (int k = 0; k < 3; ++k) v[k] = tn_md::kick(v[k], hk, f[k]);  // close_step without a thermostat
        tn_md::open_step(x, v, f, hk, dt);
      }
      break;
    case ACT_LAUNCH:
      if (!fixed) {
        const float e[3] = {md_add(x[0], -d.cen[0]), md_add(x[1], -d.cen[1]), md_add(x[2], -d.cen[2])};
        const float c[3] = {md_add(md_mul(d.w[1], e[2]), -md_mul(d.w[2], e[1])), md_add(md_mul(d.w[2], e[0]), -md_mul(d.w[0], e[2])),
                            md_add(md_mul(d.w[0], e[1]), -md_mul(d.w[1], e[0]))};
        for (int k = 0; k < 3; ++k) v[k] = md_add(v[k], -md_add(d.u[k], c[k]));
        tn_md::open_step(x, v, f, hk, dt);
      }
      break;
    case ACT_RECORD: {
      if (ring)
        for (int k = 0; k < 3; ++k) ring[k] = x[k];
      if (d.best)
        for (int k = 0; k < 3; ++k) best[k] = x[k];
      if (d.accept) {
        for (int k = 0; k < 3; ++k) cur[k] = x[k];
      } else {
        for (int k = 0; k < 3; ++k) x[k] = cur[k];
      }
      if (fixed) {
        v[0] = v[1] = v[2] = 0.f;
      } else {
        float xi[3];
        launch_noise(seed, d.hop_lo, d.hop_hi, atom, xi);
        const float s = md_mul(d.vscale, sig);
        for (int k = 0; k < 3; ++k) v[k] = md_mul(s, xi[k]);
      }
      break;
    }
    default:
      break;
  }
}

}  // namespace tn_hop
