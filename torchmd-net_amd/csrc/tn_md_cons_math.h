// Arithmetic of the distance constraints of the device-resident MD loop (tn_md_cons.hip): SHAKE on the positions after the drift
// and RATTLE on the velocities after the closing kick (Andersen, J. Comput. Phys. 52, 24, 1983), one constraint at a time in the
// order of the cluster's table (Gauss-Seidel).  __host__ __device__ like tn_md_math.h: tests/md_cons_host.hip compiles this header
// host-only, and the per-constraint statements a GPU lane runs are the statements the host checker runs.
//
// Everything here is fp64 on values widened from fp32.  w = 1 / m from the fp32 mass (1 / inf = 0: that end does not move).
//   SHAKE, constraint (a, b, d^2), reference direction s = xk_a - xk_b (the saved positions of the step's start):
//     r = x_a - x_b     diff = d^2 - r.r     within tolerance when |diff| <= 2 tol d^2; otherwise
//     g = diff / (2 (w_a + w_b) (s.r))       x_a <- x_a + (g w_a) s       x_b <- x_b - (g w_b) s
//   RATTLE, the same constraint at the final positions:
//     r = x_a - x_b     rv = r.(v_a - v_b)   within tolerance when |rv| dt <= tol d^2; otherwise
//     k = -rv / ((w_a + w_b) (r.r))          v_a <- v_a + (k w_a) r       v_b <- v_b - (k w_b) r
// A sweep visits every constraint of the cluster once; the iteration has converged when a whole sweep finds every constraint
// within tolerance, so the values that are kept satisfy all of them at once.  At most max_iter correcting sweeps are followed by one
// that only tests.  A comparison with a NaN is false, so a NaN is never "within tolerance".
// Rounding: x, v and the velocity Dx / dt that SHAKE adds are each rounded to fp32 ONCE, after the iteration (shake_finish,
// rattle_finish); the sum v + Dx / dt is one md_add under the contract of tn_md_math.h.
#pragma once
#include "tn_md_math.h"

namespace tn_md_cons {

constexpr int kMaxAtoms = 8;   // atoms of one cluster = lanes of one group
constexpr int kMaxCons = 12;   // constraints of one cluster
constexpr unsigned kFailShake = 1u, kFailRattle = 2u;  // bits of the fail word

MD_FN double inv_mass(float m) { return 1.0 / (double)m; }

MD_FN double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// one SHAKE test of constraint (a, b): 1 when within tolerance, else 0 and the multiplier g
MD_FN int shake_one(const double xa[3], const double xb[3], const double ka[3], const double kb[3], double wa, double wb, double d2,
                    double tol, double* g) {
  const double r[3] = {xa[0] - xb[0], xa[1] - xb[1], xa[2] - xb[2]};
  const double diff = d2 - dot3(r, r);
  *g = 0.0;
  if (fabs(diff) <= 2.0 * tol * d2) return 1;
  const double s[3] = {ka[0] - kb[0], ka[1] - kb[1], ka[2] - kb[2]};
  *g = diff / (2.0 * (wa + wb) * dot3(s, r));
  return 0;
}

// one RATTLE test of constraint (a, b): 1 when within tolerance, else 0 and the multiplier k
MD_FN int rattle_one(const double xa[3], const double xb[3], const double va[3], const double vb[3], double wa, double wb, double d2,
                     double dt, double tol, double* k) {
  const double r[3] = {xa[0] - xb[0], xa[1] - xb[1], xa[2] - xb[2]};
  const double u[3] = {va[0] - vb[0], va[1] - vb[1], va[2] - vb[2]};
  const double rv = dot3(r, u);
  *k = 0.0;
  if (fabs(rv) * dt <= tol * d2) return 1;
  *k = -rv / ((wa + wb) * dot3(r, r));
  return 0;
}

// y <- y + c (pa - pb): the move of one end of a constraint (c = g w_a or -g w_b with the saved positions; k w_a or -k w_b with
// the current ones)
MD_FN void move_along(double y[3], double c, const double pa[3], const double pb[3]) {
  for (int d = 0; d < 3; ++d) y[d] = y[d] + c * (pa[d] - pb[d]);
}

// after a converged SHAKE: x <- fp32(x64), v <- v + fp32((x64 - x0) / dt), x0 the position the drift gave.  0 when a result is
// not finite.
MD_FN int shake_finish(const double x64[3], float x[3], float v[3], double dt) {
  int ok = 1;
  for (int d = 0; d < 3; ++d) {
    const float dv = (float)((x64[d] - (double)x[d]) / dt);
    x[d] = (float)x64[d];
    v[d] = tn_md::md_add(v[d], dv);
    ok &= isfinite(x[d]) && isfinite(v[d]);
  }
  return ok;
}

// after a converged RATTLE: v <- fp32(v64).  0 when a result is not finite.
MD_FN int rattle_finish(const double v64[3], float v[3]) {
  int ok = 1;
  for (int d = 0; d < 3; ++d) {
    v[d] = (float)v64[d];
    ok &= isfinite(v[d]) ? 1 : 0;
  }
  return ok;
}

}  // namespace tn_md_cons
