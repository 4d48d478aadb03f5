// Arithmetic of the device-resident FIRE minimiser (tn_min.hip): the per-atom terms of the three scalar products, the
// per-molecule controller and the per-atom update.  FIRE: Bitzek, Koskinen, Gaehler, Moseler, Gumbsch, Phys. Rev. Lett. 97, 170201
// (2006), in the form ASE ships (unit masses, the whole-molecule step clamp), one controller per molecule.  __host__ __device__:
// tests/min_host.hip compiles this header host-only, so the statements a GPU lane runs are the statements the host checker runs.
//
// Rounding.  The per-atom terms and the per-atom update are fp32 under the contract of tn_md_math.h: every product is one md_mul,
// every sum one md_add, in the order written.  The controller is fp64 in the order written; its three outputs c_v, c_f, d are
// rounded to fp32 once.  (The device compiler may contract an fp64 product into the sum that consumes it; every state update -
// dt, alpha - is a single operation and does not depend on that.)
#pragma once
#include "tn_md_math.h"

namespace tn_min {

using tn_md::md_add;
using tn_md::md_mul;

struct FireParams {  // the caller's parameters (dt0 and alpha0 also live in the workspace header: tmdnet_min_reset)
  double dt_max, f_inc, f_dec, alpha0, f_alpha, max_step, fmax;
  int32_t n_min;
};

struct FireState {  // per molecule
  double dt, alpha;
  int32_t n_pos;
  int64_t converged_at;  // -1 until the molecule converges
};

enum { FIRE_MOVING = 0, FIRE_FROZEN = 1, FIRE_UNUSABLE = 2 };

// (ax bx + ay by) + az bz
MD_FN float dot3(const float a[3], const float b[3]) { return md_add(md_add(md_mul(a[0], b[0]), md_mul(a[1], b[1])), md_mul(a[2], b[2])); }

// t[0] = v.f, t[1] = f.f, t[2] = v.v of one atom; a fixed atom contributes nothing
MD_FN void atom_terms(const float v[3], const float f[3], int fixed, float t[3]) {
  if (fixed) {
    t[0] = t[1] = t[2] = 0.f;
    return;
  }
  t[0] = dot3(f, v);
  t[1] = dot3(f, f);
  t[2] = dot3(v, v);
}

// One controller move of one molecule from its sums vf, ff, vv and fmax2 = max_i |f_i|^2 after `step` steps.  Updates *s, writes
// coef = {c_v, c_f, d}.  FIRE_FROZEN: the molecule had converged before (nothing is written but coef = 0) or converges now;
// FIRE_UNUSABLE: a sum is not finite - *s is untouched, coef = 0, and the caller latches status 2.
MD_FN int fire_control(FireState* s, const FireParams& p, double vf, double ff, double vv, double fmax2, int64_t step, float coef[3]) {
  coef[0] = coef[1] = coef[2] = 0.f;
  if (s->converged_at >= 0) return FIRE_FROZEN;
  if (!isfinite(vf) || !isfinite(ff) || !isfinite(vv) || !isfinite(fmax2)) return FIRE_UNUSABLE;
  if (sqrt(fmax2) < p.fmax) {
    s->converged_at = step;
    return FIRE_FROZEN;
  }
  double c_v, mix;
  if (vf > 0.0) {
    c_v = 1.0 - s->alpha;
    mix = (ff > 0.0 && vv > 0.0) ? s->alpha * sqrt(vv / ff) : 0.0;
    if (s->n_pos > p.n_min) {
      const double grown = s->dt * p.f_inc;
      s->dt = grown < p.dt_max ? grown : p.dt_max;
      s->alpha = s->alpha * p.f_alpha;
    }
    s->n_pos += 1;
  } else {
    c_v = 0.0;
    mix = 0.0;
    s->alpha = p.alpha0;
    s->dt = s->dt * p.f_dec;
    s->n_pos = 0;
  }
  const double dt = s->dt;
  const double c_f = mix + dt;
  // |v_new|^2 of v_new = c_v v + c_f f from the sums: the whole-molecule step clamp needs no second reduction
  const double n2 = ((c_v * c_v) * vv + ((2.0 * c_v) * c_f) * vf) + (c_f * c_f) * ff;
  const double len = dt * sqrt(n2 > 0.0 ? n2 : 0.0);
  const double d = len > p.max_step ? dt * (p.max_step / len) : dt;
  coef[0] = (float)c_v;
  coef[1] = (float)c_f;
  coef[2] = (float)d;
  return FIRE_MOVING;
}

// v <- c_v v + c_f f, then x <- x + d v, of one atom of a moving molecule
MD_FN void atom_move(float x[3], float v[3], const float f[3], float c_v, float c_f, float d) {
  for (int k = 0; k < 3; ++k) {
    v[k] = md_add(md_mul(c_v, v[k]), md_mul(c_f, f[k]));
    x[k] = md_add(x[k], md_mul(d, v[k]));
  }
}

}  // namespace tn_min
