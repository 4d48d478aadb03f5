// Arithmetic of the collective-variable bias of the device-resident MD loop (tn_bias.hip): distance, angle and torsion with their
// gradients, harmonic / one-sided restraints, the Gaussian hills of metadynamics and the rule that says which hills exist.
// __host__ __device__ like tn_md_math.h: tests/md_bias_host.hip compiles this header host-only, and the statements a GPU lane runs
// are the statements the host checker runs.
//
// Everything here is fp64 on positions widened from fp32 (the engine's unwrapped positions, no minimum image).  The one fp32
// operation is the last: the bias force on an atom is the fp64 sum of its contributions in (CV, slot) order, rounded to fp32 ONCE
// (atom_force); the caller adds it to the model's force with one md_add under the rounding contract of tn_md_math.h.
//   distance(i, j)        s = |x_i - x_j|
//   angle(i, j, k)        s = atan2(|r1 x r2|, r1.r2),  r1 = x_i - x_j, r2 = x_k - x_j   (no acos: smooth at 0 and pi in the value)
//   torsion(i, j, k, l)   F = x_i - x_j, G = x_j - x_k, H = x_l - x_k, A = F x G, B = H x G,
//                         s = atan2((B x A).G / |G|, A.B) in (-pi, pi], the IUPAC sign; gradients in the form of Blondel and
//                         Karplus (J. Comput. Chem. 17, 1132, 1996), which has no 1 / sin(s)
// A degenerate geometry (coincident atoms, a collinear angle or torsion) divides by zero: the value or a gradient is then not
// finite, which the caller tests - nothing here branches on it.
#pragma once
#include "tn_md_math.h"

namespace tn_bias {

constexpr int kMaxCv = 8;        // CVs per walker
constexpr int kMaxAtoms = 32;    // distinct atoms of one walker's CVs, and entries of its (cv, slot) table
constexpr int kDistance = 0, kAngle = 1, kTorsion = 2;
constexpr int kNone = 0, kHarmonic = 1, kUpper = 2, kLower = 3;
constexpr unsigned kStatusBias = 4u;  // the status word of a walker whose CV, gradient or bias is not finite

MD_FN double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

MD_FN void cross3(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

MD_FN int cv_atoms(int kind) { return kind == kDistance ? 2 : kind == kAngle ? 3 : 4; }

MD_FN double cv_distance(const double xi[3], const double xj[3], double gi[3], double gj[3]) {
  const double r[3] = {xi[0] - xj[0], xi[1] - xj[1], xi[2] - xj[2]};
  const double s = sqrt(dot3(r, r));
  for (int d = 0; d < 3; ++d) {
    gi[d] = r[d] / s;
    gj[d] = -gi[d];
  }
  return s;
}

MD_FN double cv_angle(const double xi[3], const double xj[3], const double xk[3], double gi[3], double gj[3], double gk[3]) {
  const double r1[3] = {xi[0] - xj[0], xi[1] - xj[1], xi[2] - xj[2]};
  const double r2[3] = {xk[0] - xj[0], xk[1] - xj[1], xk[2] - xj[2]};
  double c[3], a[3], b[3];
  cross3(r1, r2, c);
  const double cn = sqrt(dot3(c, c));
  cross3(r1, c, a);  // d s / d r1 = (r1 x c) / (|c| |r1|^2)
  cross3(c, r2, b);  // d s / d r2 = (c x r2) / (|c| |r2|^2)
  const double pa = 1.0 / (cn * dot3(r1, r1)), pb = 1.0 / (cn * dot3(r2, r2));
  for (int d = 0; d < 3; ++d) {
    gi[d] = a[d] * pa;
    gk[d] = b[d] * pb;
    gj[d] = -(gi[d] + gk[d]);
  }
  return atan2(cn, dot3(r1, r2));
}

MD_FN double cv_torsion(const double xi[3], const double xj[3], const double xk[3], const double xl[3], double gi[3], double gj[3],
                        double gk[3], double gl[3]) {
  const double F[3] = {xi[0] - xj[0], xi[1] - xj[1], xi[2] - xj[2]};
  const double G[3] = {xj[0] - xk[0], xj[1] - xk[1], xj[2] - xk[2]};
  const double H[3] = {xl[0] - xk[0], xl[1] - xk[1], xl[2] - xk[2]};
  double A[3], B[3], BA[3];
  cross3(F, G, A);
  cross3(H, G, B);
  cross3(B, A, BA);
  const double g = sqrt(dot3(G, G)), a2 = dot3(A, A), b2 = dot3(B, B);
  const double fg = dot3(F, G), hg = dot3(H, G);
  const double pa = -g / a2, pb = g / b2, qa = fg / (a2 * g), qb = hg / (b2 * g);
  for (int d = 0; d < 3; ++d) {
    const double t = qa * A[d] - qb * B[d];
    gi[d] = pa * A[d];
    gl[d] = pb * B[d];
    gj[d] = t - gi[d];
    gk[d] = -t - gl[d];
  }
  return atan2(dot3(BA, G) / g, dot3(A, B));
}

// value and gradients of one CV; the slots a kind does not use get zero gradients
MD_FN double cv_eval(int kind, const double xi[3], const double xj[3], const double xk[3], const double xl[3], double gi[3], double gj[3],
                     double gk[3], double gl[3]) {
  for (int d = 0; d < 3; ++d) gk[d] = gl[d] = 0.0;
  if (kind == kDistance) return cv_distance(xi, xj, gi, gj);
  if (kind == kAngle) return cv_angle(xi, xj, xk, gi, gj, gk);
  return cv_torsion(xi, xj, xk, xl, gi, gj, gk, gl);
}

// a - b; for a torsion wrapped into (-pi, pi]
MD_FN double diff(int kind, double a, double b) {
  const double pi = 3.14159265358979323846, d = a - b;
  if (kind != kTorsion) return d;
  return d - 2.0 * pi * ceil((d - pi) / (2.0 * pi));
}

// V = 0.5 kappa delta^2 and dV/ds = kappa delta where the restraint is active: harmonic always, upper for delta > 0, lower for
// delta < 0.  (A NaN delta is active in no one-sided kind; the harmonic kind passes it on.)
MD_FN void restraint(int kind, double kappa, double delta, double* V, double* dV) {
  const bool on = kind == kHarmonic || (kind == kUpper && delta > 0.0) || (kind == kLower && delta < 0.0);
  *V = on ? (0.5 * kappa) * (delta * delta) : 0.0;
  *dV = on ? kappa * delta : 0.0;
}

// one hill of a dm-dimensional list at the walker's (s0, s1): V += w e, dV/ds_d -= w e delta_d / sigma_d^2, with
// e = exp(-0.5 (delta_0^2 / sigma_0^2 [+ delta_1^2 / sigma_1^2])); is0 = 1 / sigma_0^2
MD_FN void hill_term(int dm, int kind0, int kind1, double s0, double s1, double c0, double c1, double is0, double is1, double w, double* V,
                     double* d0, double* d1) {
  const double e0 = diff(kind0, s0, c0);
  double q = (e0 * e0) * is0, e1 = 0.0;
  if (dm == 2) {
    e1 = diff(kind1, s1, c1);
    q = q + (e1 * e1) * is1;
  }
  const double t = w * exp(-0.5 * q);
  *V = *V + t;
  *d0 = *d0 - t * (e0 * is0);
  if (dm == 2) *d1 = *d1 - t * (e1 * is1);
}

// height of the hill a walker deposits where the bias it already feels is V: well-tempered for a bias factor gamma > 1,
// plain metadynamics (gamma == 0) otherwise
MD_FN double hill_height(double h0, double V, double kT, double gamma) { return gamma > 1.0 ? h0 * exp(-V / (kT * (gamma - 1.0))) : h0; }

// Which hills exist.  n = completed steps (the loop's counter, advanced by the closing launch only), step0 / base = the counter
// and the number of hills per group at the last reset, W walkers per group, H the capacity.  A launch at counter n reads the slots
// below hills_visible(n) and, when step n + 1 is a deposit step, walker w writes hill_slot(n) >= hills_visible(n): no launch reads a
// slot it writes, and there is no counter to race on.
MD_FN int64_t hills_visible(uint64_t n, uint64_t step0, uint64_t pace, int W, uint64_t base, int64_t H) {
  const uint64_t done = n >= step0 ? (n - step0) / pace : 0;
  const uint64_t v = base + done * (uint64_t)W;
  return v > (uint64_t)H ? H : (int64_t)v;
}

// the slot walker w writes in the launch at counter n, or -1 when step n + 1 is no deposit step or the slot is past the capacity
MD_FN int64_t hill_slot(uint64_t n, uint64_t step0, uint64_t pace, int W, int w, uint64_t base, int64_t H) {
  if (n + 1 <= step0 || (n + 1 - step0) % pace != 0) return -1;
  const uint64_t s = base + ((n + 1 - step0) / pace - 1) * (uint64_t)W + (uint64_t)w;
  return s >= (uint64_t)H ? -1 : (int64_t)s;
}

// the bias force on one distinct atom: entries e0..e1 of the walker's table name (cv << 2 | slot) in CV order, then slot order;
// dV[cv] is the total dV/ds of that CV, grad [kMaxCv][4][3] the gradients.  fp64 sum, rounded once.
MD_FN void atom_force(const int32_t* entries, int e0, int e1, const double* dV, const double* grad, float f[3]) {
  double acc[3] = {0.0, 0.0, 0.0};
  for (int e = e0; e < e1; ++e) {
    const int cv = (entries[e] >> 2) & (kMaxCv - 1), slot = entries[e] & 3;
    for (int d = 0; d < 3; ++d) acc[d] = acc[d] - dV[cv] * grad[(cv * 4 + slot) * 3 + d];
  }
  for (int d = 0; d < 3; ++d) f[d] = (float)acc[d];
}

}  // namespace tn_bias
