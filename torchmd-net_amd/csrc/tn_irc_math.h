// Arithmetic of the device-resident intrinsic-reaction-coordinate follower (tn_irc.hip): the start images, the closing kick, the
// extrapolated point of the error estimate, the per-atom terms of the path sums, the damping and the controller of one path.  The
// damped velocity Verlet path follower: Hratchian and Schlegel, J. Phys. Chem. A 106, 165 (2002) - a classical trajectory with
// a = force_scale F / m whose speed is put back to a constant v0 after every step, so that dx/dt is parallel to F / m: the IRC in
// Cartesian coordinates.  __host__ __device__: tests/irc_host.hip compiles this header host-only, so the statements a GPU lane
// runs are the statements the host checker runs.
//
// Rounding.  Per-atom arithmetic is fp32 under the contract of tn_md_math.h: every product is one md_mul, every sum one md_add, in
// the order written; the opening half of a step is tn_md::open_step, unchanged.  Everything per path is fp64 in the order written,
// from fp64 sums of the fp32 terms; the two numbers a lane multiplies with - the damping c and the time step dt - are rounded to
// fp32 once.  The cube root of the step controller is the C library's cbrt.
#pragma once
#include "tn_md_math.h"

namespace tn_irc {

using tn_md::md_add;
using tn_md::md_mul;

enum { IRC_OK = 0, IRC_BAD_FORCES = 1, IRC_BAD_VELOCITY = 2, IRC_BAD_ENERGY = 3 };  // the detail of status 2
enum { IRC_MOVING = 0, IRC_FINISHED = 1, IRC_FROZEN = 2, IRC_UNUSABLE = 3 };        // what irc_control answers
enum { REASON_NONE = 0, REASON_FMAX = 1, REASON_UPHILL = 2 };                       // why a path finished
// the sums of one path over its free atoms
enum { S_VV = 0, S_P, S_FMAX2, S_D2, S_DS2, S_FREE, N_SUMS };  // |v'|^2, F.v', max |F|^2, |x - x'|^2, m |x - x_prev|^2, count
constexpr unsigned kMaxMask = 1u << S_FMAX2;                   // the entry of the sums that is a maximum

MD_FN float dot3(const float a[3], const float b[3]) {
  return md_add(md_add(md_mul(a[0], b[0]), md_mul(a[1], b[1])), md_mul(a[2], b[2]));
}

// an atom that never moves and is left out of every sum: fixed, or of infinite mass (ca = force_scale / (2 m) = 0)
MD_FN int still_atom(int fixed, float ca) { return fixed || !(ca > 0.f); }

// the start images of one atom: x0 = x_ts + (sigma step) u, v0 = (sigma speed) u, one rounded product (and sum) per component;
// sigma = +1 / -1 changes a sign only, so the two directions are mirror images bit for bit
MD_FN void start_image(const float x_ts[3], const float u[3], float sigma, float step, float speed, float x[3], float v[3]) {
  const float ds = md_mul(sigma, step), dv = md_mul(sigma, speed);
  for (int k = 0; k < 3; ++k) {
    x[k] = md_add(x_ts[k], md_mul(ds, u[k]));
    v[k] = md_mul(dv, u[k]);
  }
}

// the closing kick v' = v_half + hk F with the hk of the opening half (hk = md_mul(dt, ca))
MD_FN void close_kick(const float vh[3], const float f[3], float hk, float vp[3]) {
  for (int k = 0; k < 3; ++k) vp[k] = tn_md::kick(vh[k], hk, f[k]);
}

// x' = (x2 + T v2) + (T T) (ca F2): where a trajectory of constant acceleration from the state two steps back would be now
MD_FN void extrapolate(const float x2[3], const float v2[3], const float f2[3], float T, float ca, float xp[3]) {
  const float tt = md_mul(T, T);
  for (int k = 0; k < 3; ++k) xp[k] = md_add(md_add(x2[k], md_mul(T, v2[k])), md_mul(tt, md_mul(ca, f2[k])));
}

// |a - b|^2 of one atom
MD_FN float dist2(const float a[3], const float b[3]) {
  float d[3];
  for (int k = 0; k < 3; ++k) d[k] = md_add(a[k], -b[k]);
  return dot3(d, d);
}

// The five terms of one free atom after the evaluation at x: v' (returned too), |v'|^2, F.v', |F|^2, |x - x'|^2 (0 without a second
// generation) and m |x - x1|^2 (x1: where the step began).  hk = 0 and x1 = x at the start images, where nothing was opened.
MD_FN void sum_terms(const float x[3], const float vh[3], const float f[3], float hk, float ca, float mass, const float x1[3],
                     int has2, const float x2[3], const float v2[3], const float f2[3], float T, float vp[3], float t[5]) {
  close_kick(vh, f, hk, vp);
  t[S_VV] = dot3(vp, vp);
  t[S_P] = dot3(f, vp);
  t[S_FMAX2] = dot3(f, f);
  t[S_D2] = 0.f;
  if (has2) {
    float xp[3];
    extrapolate(x2, v2, f2, T, ca, xp);
    t[S_D2] = dist2(x, xp);
  }
  t[S_DS2] = md_mul(mass, dist2(x, x1));
}

// the damping of one atom: v <- c v', one product
MD_FN void damp(const float vp[3], float c, float v[3]) {
  for (int k = 0; k < 3; ++k) v[k] = md_mul(c, vp[k]);
}

struct IrcParams {
  double fmax, v0, error, dt_min, dt_max;
  int32_t every, capacity;  // the path record: every `every`-th accepted step of a path, at most `capacity` frames
};

struct IrcPath {           // what a path carries from step to step
  double dt, arc;          // the time step of the next opening half; the mass-weighted arc length so far
  int64_t converged_at;    // -1 while the path moves
  int32_t reason, n_acc, n_rec;  // REASON_*; accepted steps since the start; frames counted (it keeps counting beyond the capacity)
};

// The controller of one path after the evaluation of a step (start = 1: of the start images, where nothing was opened - no time
// step to judge, no arc).  fp64 in the order written.  out[0] = fp32(c), out[1] = fp32 of the time step the closing kick of THIS
// step uses (0 at the start), *slot = the frame this step is recorded in or -1, *cause = IRC_* when the answer is IRC_UNUSABLE
// (then *s is untouched).  The energy is looked at first, then the forces, then the velocity sums; a path without a free atom is
// finished as it stands.
MD_FN int irc_control(IrcPath* s, const IrcParams& p, const double sums[N_SUMS], float energy, int start, int64_t step, float out[2],
                      int* slot, int* cause) {
  out[0] = 1.f;
  out[1] = 0.f;
  *slot = -1;
  *cause = IRC_OK;
  if (s->converged_at >= 0) return IRC_FROZEN;
  const int has_free = sums[S_FREE] > 0.0;
  const int has2 = !start && s->n_acc >= 1;
  double c = 1.0, dt = s->dt, arc = s->arc;
  int reason = REASON_FMAX;
  if (has_free) {
    if (!isfinite(energy)) *cause = IRC_BAD_ENERGY;
    else if (!isfinite(sums[S_P]) || !isfinite(sums[S_FMAX2])) *cause = IRC_BAD_FORCES;
    else if (!isfinite(sums[S_VV]) || !(sums[S_VV] > 0.0) || (has2 && !isfinite(sums[S_D2])) || !isfinite(sums[S_DS2]))
      *cause = IRC_BAD_VELOCITY;
    if (*cause) return IRC_UNUSABLE;
    c = p.v0 / sqrt(sums[S_VV]);
    if (has2 && sums[S_D2] > 0.0) {
      double r = cbrt(p.error / sqrt(sums[S_D2]));
      r = r < 0.5 ? 0.5 : (r > 2.0 ? 2.0 : r);
      dt = s->dt * r;
      dt = dt < p.dt_min ? p.dt_min : (dt > p.dt_max ? p.dt_max : dt);
    }
    if (!start) arc = s->arc + sqrt(sums[S_DS2]);
    reason = sqrt(sums[S_FMAX2]) < p.fmax ? REASON_FMAX : (sums[S_P] <= 0.0 ? REASON_UPHILL : REASON_NONE);
  }
  out[0] = (float)c;
  out[1] = start ? 0.f : (float)s->dt;
  s->dt = dt;
  s->arc = arc;
  s->n_acc = start ? 0 : s->n_acc + 1;
  if (reason != REASON_NONE) {
    s->converged_at = step;
    s->reason = reason;
  }
  if (reason != REASON_NONE || s->n_acc % (p.every > 0 ? p.every : 1) == 0) {
    if (s->n_rec < p.capacity) *slot = s->n_rec;
    if (s->n_rec < INT32_MAX) s->n_rec += 1;
  }
  return reason != REASON_NONE ? IRC_FINISHED : IRC_MOVING;
}

}  // namespace tn_irc
