// Arithmetic of the device-resident nudged elastic band (tn_neb.hip): the per-atom terms of the five path sums, the improved
// tangent's two weights, the two coefficients of an image's band force and the per-atom projection.  NEB with the improved tangent:
// Henkelman and Jonsson, J. Chem. Phys. 113, 9978 (2000); the climbing image: Henkelman, Uberuaga and Jonsson, J. Chem. Phys. 113,
// 9901 (2000).  The optimiser is tn_min_math.h's FIRE, one controller per band.  __host__ __device__: tests/neb_host.hip compiles this
// header host-only, so the statements a GPU lane runs are the statements the host checker runs.
//
// Rounding.  The per-atom terms and the projection are fp32 under the contract of tn_md_math.h: every product is one md_mul, every
// sum one md_add, in the order written.  Weights and coefficients are fp64 in the order written; the two coefficients s+, s- are
// rounded to fp32 once.  (The device compiler may contract an fp64 product into the sum that consumes it.)
#pragma once
#include "tn_min_math.h"

namespace tn_neb {

using tn_md::md_add;
using tn_md::md_mul;

enum { NEB_OK = 0, NEB_BAD_SUMS = 1, NEB_BAD_PATH = 2, NEB_BAD_ENERGY = 3 };  // the detail of status 2

// d+ = R_{i+1} - R_i and d- = R_i - R_{i-1} of one atom, one rounded sum per component (no minimum image: the path is unwrapped)
MD_FN void path_diff(const float prev[3], const float cur[3], const float next[3], float dp[3], float dm[3]) {
  for (int k = 0; k < 3; ++k) {
    dp[k] = md_add(next[k], -cur[k]);
    dm[k] = md_add(cur[k], -prev[k]);
  }
}

// t = d+.d+, d-.d-, d+.d-, F.d+, F.d- of one atom; a fixed atom contributes nothing
MD_FN void path_terms(const float dp[3], const float dm[3], const float f[3], int fixed, float t[5]) {
  if (fixed) {
    t[0] = t[1] = t[2] = t[3] = t[4] = 0.f;
    return;
  }
  t[0] = tn_min::dot3(dp, dp);
  t[1] = tn_min::dot3(dm, dm);
  t[2] = tn_min::dot3(dp, dm);
  t[3] = tn_min::dot3(f, dp);
  t[4] = tn_min::dot3(f, dm);
}

// The improved tangent tau = w+ d+ + w- d- of an interior image from its energy and its neighbours': the uphill neighbour alone on a
// slope, the two energy differences as weights at an extremum (an exact tie counts as an extremum).
MD_FN void tangent_weights(double e_prev, double e, double e_next, double* wp, double* wm) {
  if (e_next > e && e > e_prev) {
    *wp = 1.0;
    *wm = 0.0;
    return;
  }
  if (e_next < e && e < e_prev) {
    *wp = 0.0;
    *wm = 1.0;
    return;
  }
  const double up = fabs(e_next - e), dn = fabs(e_prev - e);
  const double hi = up > dn ? up : dn, lo = up > dn ? dn : up;
  if (e_next > e_prev) {
    *wp = hi;
    *wm = lo;
  } else {
    *wp = lo;
    *wm = hi;
  }
}

// 1 when the M energies of a band are all finite
MD_FN int energies_finite(const float* e, int n_images) {
  int ok = 1;
  for (int i = 0; i < n_images; ++i) ok &= isfinite(e[i]) ? 1 : 0;
  return ok;
}

// the climbing image of a band: the lowest interior index with the largest energy (M >= 3)
MD_FN int climber(const float* e, int n_images) {
  int best = 1;
  for (int i = 2; i < n_images - 1; ++i)
    if (e[i] > e[best]) best = i;
  return best;
}

// The two coefficients of F_neb = (F + s+ d+) + s- d- of one image from its path sums S = a, b, c, p, q and its weights:
//   |tau|^2 = (w+^2 a + 2 w+ w- c) + w-^2 b,   F.tau = w+ p + w- q
//   plain:    g = (-(F.tau) / |tau| + k (sqrt a - sqrt b)) / |tau|      F - (F.tau^) tau^ + k (|d+| - |d-|) tau^
//   climbing: g = -2 (F.tau) / |tau|^2                                  F - 2 (F.tau^) tau^, no spring
//   s+ = fp32(g w+), s- = fp32(g w-)
// NEB_BAD_PATH: |tau|^2 is zero or not finite (coincident images); NEB_BAD_SUMS: F.tau is not finite.  Then s = 0.
MD_FN int image_coef(const double S[5], double wp, double wm, double k, int climbs, float s[2]) {
  s[0] = s[1] = 0.f;
  const double tau2 = ((wp * wp) * S[0] + ((2.0 * wp) * wm) * S[2]) + (wm * wm) * S[1];
  if (!isfinite(tau2) || !(tau2 > 0.0)) return NEB_BAD_PATH;
  const double ft = wp * S[3] + wm * S[4];
  if (!isfinite(ft)) return NEB_BAD_SUMS;
  double g;
  if (climbs) {
    g = (-2.0 * ft) / tau2;
  } else {
    const double tau = sqrt(tau2);
    g = (-(ft / tau) + k * (sqrt(S[0]) - sqrt(S[1]))) / tau;
  }
  s[0] = (float)(g * wp);
  s[1] = (float)(g * wm);
  return NEB_OK;
}

// Everything per image in one call, as the projection kernel makes it: e = the band's M energies, i the interior image, S its path
// sums.  Writes the weights and the coefficients; returns NEB_OK or the cause (an energy of the band first, then the path, then F.tau).
// has_free = 0: every atom is fixed, the image has no degree of freedom and needs no tangent - s = 0 and nothing is unusable (the
// band then converges as it stands, as a molecule of fixed atoms does in the minimiser).
MD_FN int image_control(const float* e, int n_images, int i, const double S[5], double k, int climb, int has_free, double w[2],
                        float s[2]) {
  w[0] = w[1] = 0.0;
  s[0] = s[1] = 0.f;
  if (!has_free) return NEB_OK;
  if (!energies_finite(e, n_images)) return NEB_BAD_ENERGY;
  tangent_weights((double)e[i - 1], (double)e[i], (double)e[i + 1], &w[0], &w[1]);
  return image_coef(S, w[0], w[1], k, climb && climber(e, n_images) == i, s);
}

// F_neb = (F + s+ d+) + s- d- of one atom
MD_FN void project(const float f[3], const float dp[3], const float dm[3], float sp, float sm, float out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = md_add(md_add(f[k], md_mul(sp, dp[k])), md_mul(sm, dm[k]));
}

}  // namespace tn_neb
