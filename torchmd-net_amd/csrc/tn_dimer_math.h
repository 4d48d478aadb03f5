// Arithmetic of the device-resident dimer saddle search (tn_dimer.hip): the curvature rows of the three images, the 2 x 2 rotation
// of the dimer axis, the interpolated curvature, the inverted force, the next partner direction and the per-atom update.  The dimer
// method: Henkelman and Jonsson, J. Chem. Phys. 111, 7010 (1999); the rotation from two curvature rows: Kaestner and Sherwood,
// J. Chem. Phys. 128, 014106 (2008), with the trial image at a right angle and evaluated in the same batch; forward differences as
// in Heyden, Bell and Keil, J. Chem. Phys. 123, 224101 (2005).  The optimiser is tn_min_math.h's FIRE, one controller per dimer.
// __host__ __device__: tests/dimer_host.hip compiles this header host-only, so the statements a GPU lane runs are the statements the
// host checker runs.
//
// Rounding.  Per-atom arithmetic is fp32 under the contract of tn_md_math.h: every product is one md_mul, every sum one md_add, in
// the order written.  Everything per dimer is fp64 in the order written, from fp64 sums of the fp32 terms; every coefficient a lane
// multiplies with is rounded to fp32 once.  The two norms that would suffer cancellation - nu of the rotated axis and |T| of the
// residual - are sums over the vectors themselves, never differences of the Gram sums a, b, c; the term of nu^2 is the one per-atom
// quantity formed in fp64 (nu2_term), so that nu does not see the rounding of fp32(co), fp32(si).
#pragma once
#include "tn_min_math.h"

namespace tn_dimer {

using tn_md::md_add;
using tn_md::md_mul;
using tn_min::dot3;

enum { DIMER_OK = 0, DIMER_BAD_SUMS = 1, DIMER_BAD_MODE = 2, DIMER_BAD_ENERGY = 3 };  // the detail of status 2
enum { ROT_KEEP = 0, ROT_SWAP = 1, ROT_ANGLE = 2 };                                   // which branch the rotation took
enum { PARTNER_RESIDUAL = 0, PARTNER_ROTATED = 1, PARTNER_NONE = 2 };                 // where the next partner came from

// the sums of the first launch, per dimer over the atoms that are not fixed
enum { S_A = 0, S_B1, S_B2, S_C, S_PN, S_PM, S_FF, S_FREE, N_SUMS };  // N.HN, N.HM, M.HN, M.HM, F0.N, F0.M, |F0|^2+|F1|^2+|F2|^2, count
// the sums of the second launch besides the four of FIRE
enum { P_TT = 0, P_TN, P_NN, P_RR, P_RN, P_HH, N_PART };  // T.T, T.N', N'.N', R.R, R.N', HN'.HN'
// the fp32 coefficients of a dimer's step
enum { C_CN = 0, C_SN, C_CC, C_K0, C_E, C_CO, C_SI, C_MT, C_MR, C_MN, N_COEF };

// |T|^2 at or below this fraction of |HN'|^2 does not define a direction: the partner is then the rotated old one
#define TN_DIMER_FLOOR2 9.094947017729282e-13 /* 2^-40: |T| <= 2^-20 |HN'| */

// image i of atom a: x0 + delta n, one rounded product and one rounded sum per component
MD_FN void image_pos(const float x0[3], float dl, const float n[3], float x[3]) {
  for (int k = 0; k < 3; ++k) x[k] = md_add(x0[k], md_mul(dl, n[k]));
}

// h = -(Fi - F0) / delta = (F0 - Fi) inv of one atom
MD_FN void curv_row(const float f0[3], const float fi[3], float inv, float h[3]) {
  for (int k = 0; k < 3; ++k) h[k] = md_mul(md_add(f0[k], -fi[k]), inv);
}

// u = p a + q b of one atom
MD_FN void mix(const float a[3], const float b[3], float p, float q, float u[3]) {
  for (int k = 0; k < 3; ++k) u[k] = md_add(md_mul(p, a[k]), md_mul(q, b[k]));
}

// |co N + si M|^2 of one atom in fp64: the term of nu^2, which is summed over the vectors themselves
MD_FN double nu2_term(const float N[3], const float M[3], double co, double si) {
  const double u0 = co * (double)N[0] + si * (double)M[0], u1 = co * (double)N[1] + si * (double)M[1],
               u2 = co * (double)N[2] + si * (double)M[2];
  return (u0 * u0 + u1 * u1) + u2 * u2;
}

// the seven terms of the first launch of one atom (the count is the kernel's); a fixed atom contributes nothing
MD_FN void sum_terms(const float N[3], const float M[3], const float f0[3], const float f1[3], const float f2[3], float inv, int fixed,
                     float t[7]) {
  if (fixed) {
    for (int k = 0; k < 7; ++k) t[k] = 0.f;
    return;
  }
  float hn[3], hm[3];
  curv_row(f0, f1, inv, hn);
  curv_row(f0, f2, inv, hm);
  t[S_A] = dot3(N, hn);
  t[S_B1] = dot3(N, hm);
  t[S_B2] = dot3(M, hn);
  t[S_C] = dot3(M, hm);
  t[S_PN] = dot3(f0, N);
  t[S_PM] = dot3(f0, M);
  t[S_FF] = md_add(md_add(dot3(f0, f0), dot3(f1, f1)), dot3(f2, f2));
}

// (co, si), co >= 0: the unit eigenvector of [[a, b], [b, c]] for the smaller eigenvalue.  b = 0 is decided without an angle: a <= c
// keeps the axis (the tie a = c too), a > c takes the partner.  Otherwise theta = atan2(-2 b, c - a) / 2 minimises
// (a + c) / 2 + ((a - c) / 2) cos 2 theta + b sin 2 theta, and |theta| < pi / 2 makes co > 0.
MD_FN int rotation(double a, double b, double c, double* co, double* si) {
  if (b == 0.0) {
    if (a <= c) {
      *co = 1.0;
      *si = 0.0;
      return ROT_KEEP;
    }
    *co = 0.0;
    *si = 1.0;
    return ROT_SWAP;
  }
  const double theta = 0.5 * atan2(-2.0 * b, c - a);
  *co = cos(theta);
  *si = sin(theta);
  return ROT_ANGLE;
}

// What can be said before nu is known, from the sums S[N_SUMS] and the three energies: the cause, the 2 x 2 entries q = a, b, c
// and the rotation.  An energy first (cause 3), then the forces (cause 1: |F|^2, F0.N or F0.M not finite), then the 2 x 2 problem
// (cause 2).  has_free = 0: every atom is fixed, there is no mode and nothing is unusable.
MD_FN int mode_rotation(const double* S, const float* e, int has_free, double q[3], double* co, double* si, int* branch) {
  q[0] = q[1] = q[2] = 0.0;
  *co = 1.0;
  *si = 0.0;
  *branch = ROT_KEEP;
  if (!has_free) return DIMER_OK;
  if (!isfinite(e[0]) || !isfinite(e[1]) || !isfinite(e[2])) return DIMER_BAD_ENERGY;
  if (!isfinite(S[S_FF]) || !isfinite(S[S_PN]) || !isfinite(S[S_PM])) return DIMER_BAD_SUMS;
  q[0] = S[S_A];
  q[1] = 0.5 * (S[S_B1] + S[S_B2]);
  q[2] = S[S_C];
  if (!isfinite(q[0]) || !isfinite(q[1]) || !isfinite(q[2])) return DIMER_BAD_MODE;
  *branch = rotation(q[0], q[1], q[2], co, si);
  return DIMER_OK;
}

// The coefficients of the step once nu^2 = |co N + si M|^2 has been summed over the vectors (nu2_term):
//   N' = cn N + sn M,  HN' = cn HN + sn HM   with cn = fp32(co / nu), sn = fp32(si / nu)
//   C = ((co co) a + ((2 co) si) b + (si si) c) / nu^2,   p = (co F0.N + si F0.M) / nu
//   T = HN' - cc N',  cc = fp32(C)
//   F_eff = k0 F0 + e N':  C < 0: k0 = 1, e = fp32(-2 p);   otherwise k0 = 0, e = fp32(-p)
// coef[C_CN .. C_SI] are written (C_CO, C_SI = fp32(co), fp32(si): the rotated partner R = -si32 N + co32 M).  DIMER_BAD_MODE:
// nu^2 is zero or not finite.
MD_FN int mode_coef(const double q[3], const double* S, double co, double si, double nu2, int has_free, float* coef, double* C, double* p) {
  for (int k = 0; k <= C_SI; ++k) coef[k] = 0.f;
  *C = 0.0;
  *p = 0.0;
  if (!has_free) return DIMER_OK;
  if (!isfinite(nu2) || !(nu2 > 0.0)) return DIMER_BAD_MODE;
  const double nu = sqrt(nu2);
  *C = (((co * co) * q[0] + ((2.0 * co) * si) * q[1]) + (si * si) * q[2]) / nu2;
  *p = (co * S[S_PN] + si * S[S_PM]) / nu;
  coef[C_CN] = (float)(co / nu);
  coef[C_SN] = (float)(si / nu);
  coef[C_CC] = (float)*C;
  if (*C < 0.0) {
    coef[C_K0] = 1.f;
    coef[C_E] = (float)(-2.0 * *p);
  } else {
    coef[C_K0] = 0.f;
    coef[C_E] = (float)(-*p);
  }
  coef[C_CO] = (float)co;
  coef[C_SI] = (float)si;
  return DIMER_OK;
}

// One atom of the second launch: the pending axis N', the residual T, F_eff, and the six partner terms.  A fixed atom has
// N' = T = 0, keeps the evaluation's force and contributes nothing.
MD_FN void project_atom(const float N[3], const float M[3], const float f0[3], const float f1[3], const float f2[3], float inv,
                        const float* coef, int fixed, float np[3], float t[3], float feff[3], float terms[N_PART]) {
  if (fixed) {
    for (int k = 0; k < 3; ++k) {
      np[k] = t[k] = 0.f;
      feff[k] = f0[k];
    }
    for (int k = 0; k < N_PART; ++k) terms[k] = 0.f;
    return;
  }
  float hn[3], hm[3], hp[3], r[3];
  curv_row(f0, f1, inv, hn);
  curv_row(f0, f2, inv, hm);
  mix(N, M, coef[C_CN], coef[C_SN], np);
  mix(hn, hm, coef[C_CN], coef[C_SN], hp);
  mix(N, M, -coef[C_SI], coef[C_CO], r);
  for (int k = 0; k < 3; ++k) {
    t[k] = md_add(hp[k], -md_mul(coef[C_CC], np[k]));
    feff[k] = md_add(md_mul(coef[C_K0], f0[k]), md_mul(coef[C_E], np[k]));
  }
  terms[P_TT] = dot3(t, t);
  terms[P_TN] = dot3(t, np);
  terms[P_NN] = dot3(np, np);
  terms[P_RR] = dot3(r, r);
  terms[P_RN] = dot3(r, np);
  terms[P_HH] = dot3(hp, hp);
}

// The next partner M' = mt T + mr R + mn N' from the partner sums: T made orthogonal to N' and normalised,
//   k = T.N' / N'.N',  |T_perp|^2 = T.T - k T.N',  mt = 1 / |T_perp|,  mn = -k mt
// (T.T is the sum over the vector; the correction k T.N' is of second order in the rounding of C) - unless |T_perp|^2 is zero, not
// finite or at most TN_DIMER_FLOOR2 |HN'|^2: then the rotated old partner R takes T's place (mr, mn likewise), so a converged mode
// keeps a defined partner; and when R has no length either, M' = 0.  *resid = |T| = sqrt(T.T).
MD_FN int partner_coef(const double P[N_PART], int has_free, float* coef, double* resid) {
  coef[C_MT] = coef[C_MR] = coef[C_MN] = 0.f;
  *resid = 0.0;
  if (!has_free) return PARTNER_NONE;
  *resid = sqrt(P[P_TT]);
  if (!isfinite(P[P_NN]) || !(P[P_NN] > 0.0)) return PARTNER_NONE;
  const double kt = P[P_TN] / P[P_NN];
  const double t2 = P[P_TT] - kt * P[P_TN];
  if (isfinite(t2) && t2 > 0.0 && t2 > TN_DIMER_FLOOR2 * P[P_HH]) {
    const double s = 1.0 / sqrt(t2);
    coef[C_MT] = (float)s;
    coef[C_MN] = (float)(-(kt * s));
    return PARTNER_RESIDUAL;
  }
  const double kr = P[P_RN] / P[P_NN];
  const double r2 = P[P_RR] - kr * P[P_RN];
  if (isfinite(r2) && r2 > 0.0) {
    const double s = 1.0 / sqrt(r2);
    coef[C_MR] = (float)s;
    coef[C_MN] = (float)(-(kr * s));
    return PARTNER_ROTATED;
  }
  return PARTNER_NONE;
}

// One atom of the accept: the new axis is the pending N', the new partner (mt T + mr R) + mn N' with R from the OLD N and M
MD_FN void accept_atom(const float N[3], const float M[3], const float np[3], const float t[3], const float* coef, int fixed,
                       float n_new[3], float m_new[3]) {
  if (fixed) {
    for (int k = 0; k < 3; ++k) n_new[k] = m_new[k] = 0.f;
    return;
  }
  float r[3];
  mix(N, M, -coef[C_SI], coef[C_CO], r);
  for (int k = 0; k < 3; ++k) {
    m_new[k] = md_add(md_add(md_mul(coef[C_MT], t[k]), md_mul(coef[C_MR], r[k])), md_mul(coef[C_MN], np[k]));
    n_new[k] = np[k];
  }
}

// The controller of one dimer: tn_min::fire_control, unchanged, on the sums of F_eff - with the bound it converges by switched off
// while the curvature is not negative (a dimer converges when sqrt(fmax2) < fmax AND C < 0).  translate = 0: a mode search, no
// move and no convergence - the coefficients are zero and *s is untouched.  has_free = 0: no degree of freedom, the sums are zero
// and the dimer converges as it stands.
MD_FN int dimer_fire(tn_min::FireState* s, const tn_min::FireParams& p, const double sums[4], double C, int translate, int has_free,
                     int64_t step, float coef[3]) {
  if (!has_free) return tn_min::fire_control(s, p, sums[0], sums[1], sums[2], sums[3], step, coef);
  if (!translate) {
    coef[0] = coef[1] = coef[2] = 0.f;
    if (s->converged_at >= 0) return tn_min::FIRE_FROZEN;
    if (!isfinite(sums[0]) || !isfinite(sums[1]) || !isfinite(sums[2]) || !isfinite(sums[3])) return tn_min::FIRE_UNUSABLE;
    return tn_min::FIRE_MOVING;
  }
  tn_min::FireParams q = p;
  if (!(C < 0.0)) q.fmax = 0.0;  // sqrt(fmax2) < 0 never holds
  return tn_min::fire_control(s, q, sums[0], sums[1], sums[2], sums[3], step, coef);
}

}  // namespace tn_dimer
