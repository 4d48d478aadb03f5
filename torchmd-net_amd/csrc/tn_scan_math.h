// Arithmetic of the device-resident relaxed coordinate scan (tn_scan.hip): a FIRE minimisation of G copies of one molecule, each
// with D <= 4 collective variables (distance, angle, torsion: tn_bias_math.h) held at its own target.  Per step the force and the
// velocity are projected onto the tangent space of the constraints, FIRE (tn_min_math.h, unchanged) moves the atoms, the target is
// driven a bounded step towards its final value and a Gauss-Newton iteration puts the CV atoms back on the constraint surface.
// __host__ __device__: tests/scan_host.hip compiles this header host-only, so the statements a GPU lane runs are the statements
// the host checker runs.
//
// Rounding.  Everything per point is fp64 in the order written, on positions, forces and velocities widened from fp32.  Its
// coefficients - the multipliers lambda and mu - are rounded to fp32 once; the correction of a CV atom is the fp64 sum of its
// contributions in (CV, slot) order, rounded to fp32 once (tn_bias::atom_force with dV = fp32(lambda) widened) and added by the
// caller with one md_add.  The constraint step iterates on fp64 positions and rounds them to fp32 once at its end.
//
// Indexable state (the gradients [4][4][3], the Gram matrix, the positions of the CV atoms) lives in a Work the caller provides: LDS on
// the device, the stack on the host.
#pragma once
#include "tn_bias_math.h"
#include "tn_min_math.h"

namespace tn_scan {

constexpr int kMaxCv = 4;      // CVs per point
constexpr int kMaxAtoms = 16;  // distinct atoms of the CVs, and entries of the (cv, slot) table

enum { SCAN_OK = 0, SCAN_BAD_SUMS = 1, SCAN_BAD_CV = 2, SCAN_BAD_GRAM = 3, SCAN_BAD_STEP = 4 };  // the cause of status 2

// The CVs of a call and the table of their distinct atoms, as tn_bias.hip has it: atom_rel[a] is distinct atom a (ascending, within
// the molecule), its entries offsets[a]..offsets[a+1] name (cv << 2 | slot) in CV order, then slot order.
struct Tables {
  int32_t D, A;
  int32_t kind[kMaxCv];
  int32_t atoms[kMaxCv * 4];
  int32_t atom_rel[kMaxAtoms];
  int32_t offsets[kMaxAtoms + 1];
  int32_t entries[kMaxAtoms];
  int32_t where[kMaxCv * 4];  // (cv, slot) -> its distinct atom; unused slots: the CV's slot 0
};

struct Work {
  double x[kMaxAtoms * 3];     // the distinct atoms' positions
  double grad[kMaxCv * 12];    // [cv][slot][3]; rows on fixed atoms are zero
  double M[kMaxCv * kMaxCv];   // the Gram matrix, then its Cholesky factor (lower)
  double s[kMaxCv];            // the CVs
  double b[kMaxCv];            // a right-hand side, then the solution
  int32_t fx[kMaxAtoms];       // the distinct atom is fixed
};

// Build the table from the CVs' kinds and atoms (host only; the C entry and the host checker call it).  Returns 0, or 1 when D is not
// 1..4, a kind is unknown, an index lies outside 0..n-1 or is repeated within a CV.
inline int make_tables(int32_t D, const int32_t* kind, const int32_t* atoms, int64_t n, Tables* T) {
  if (D < 1 || D > kMaxCv || !kind || !atoms) return 1;
  *T = Tables();
  T->D = D;
  for (int c = 0; c < D; ++c) {
    if (kind[c] != tn_bias::kDistance && kind[c] != tn_bias::kAngle && kind[c] != tn_bias::kTorsion) return 1;
    const int na = tn_bias::cv_atoms(kind[c]);
    T->kind[c] = kind[c];
    for (int s = 0; s < 4; ++s) {
      const int32_t i = s < na ? atoms[c * 4 + s] : -1;
      if (s < na && (i < 0 || i >= n)) return 1;
      for (int r = 0; r < s && s < na; ++r)
        if (atoms[c * 4 + r] == i) return 1;
      T->atoms[c * 4 + s] = i;
    }
  }
  int A = 0;
  for (int32_t last = -1;;) {  // the distinct atoms, ascending
    int32_t next = -1;
    for (int e = 0; e < D * 4; ++e)
      if (T->atoms[e] > last && (next < 0 || T->atoms[e] < next)) next = T->atoms[e];
    if (next < 0) break;
    T->atom_rel[A++] = next;  // (at most 16: D <= 4 CVs of <= 4 atoms)
    last = next;
  }
  T->A = A;
  int ne = 0;
  for (int a = 0; a < A; ++a) {
    T->offsets[a] = ne;
    for (int e = 0; e < D * 4; ++e)
      if (T->atoms[e] == T->atom_rel[a]) {
        T->entries[ne++] = e;  // e = cv << 2 | slot
        T->where[e] = a;
      }
  }
  T->offsets[A] = ne;
  for (int a = A + 1; a <= kMaxAtoms; ++a) T->offsets[a] = ne;
  for (int e = 0; e < D * 4; ++e)
    if (T->atoms[e] < 0) T->where[e] = T->where[e & ~3];
  return 0;
}

// s_d and g_d of every CV at w->x; rows on fixed atoms zeroed.  Returns 1 when everything is finite.
MD_FN int cv_all(const Tables& T, Work* w) {
  int ok = 1;
  for (int c = 0; c < T.D; ++c) {
    double* g = w->grad + c * 12;
    const double s = tn_bias::cv_eval(T.kind[c], w->x + 3 * T.where[c * 4 + 0], w->x + 3 * T.where[c * 4 + 1], w->x + 3 * T.where[c * 4 + 2],
                                      w->x + 3 * T.where[c * 4 + 3], g, g + 3, g + 6, g + 9);
    w->s[c] = s;
    ok = ok && isfinite(s);
    for (int k = 0; k < 12; ++k) ok = ok && isfinite(g[k]);
    const int na = tn_bias::cv_atoms(T.kind[c]);
    for (int sl = 0; sl < na; ++sl)
      if (w->fx[T.where[c * 4 + sl]])
        for (int k = 0; k < 3; ++k) g[sl * 3 + k] = 0.0;
  }
  return ok;
}

// M = g g^T: atom by atom, the pairs of its entries in entry order
MD_FN void gram(const Tables& T, Work* w) {
  for (int k = 0; k < kMaxCv * kMaxCv; ++k) w->M[k] = 0.0;
  for (int a = 0; a < T.A; ++a)
    for (int p = T.offsets[a]; p < T.offsets[a + 1]; ++p)
      for (int q = T.offsets[a]; q < T.offsets[a + 1]; ++q) {
        const int ep = T.entries[p], eq = T.entries[q];
        const int m = (ep >> 2) * kMaxCv + (eq >> 2);
        w->M[m] = w->M[m] + tn_bias::dot3(w->grad + ep * 3, w->grad + eq * 3);
      }
}

// b_d = g_d . u for per-atom vectors u [A, 3]: atom by atom, its entries in entry order
MD_FN void grad_dot(const Tables& T, Work* w, const double* u) {
  for (int c = 0; c < kMaxCv; ++c) w->b[c] = 0.0;
  for (int a = 0; a < T.A; ++a)
    for (int p = T.offsets[a]; p < T.offsets[a + 1]; ++p) {
      const int e = T.entries[p];
      w->b[e >> 2] = w->b[e >> 2] + tn_bias::dot3(w->grad + e * 3, u + a * 3);
    }
}

// M = L L^T in place (the lower triangle becomes L).  Returns 1 when a pivot is not positive and finite.  Positive means beyond
// rounding: two identical CVs leave a pivot of a few ulp of its diagonal entry with either sign, so a pivot counts as positive when
// it exceeds kPivotFloor of that entry (a Gram matrix that ill-conditioned has no multiplier with a correct fp32 digit).
constexpr double kPivotFloor = 1e-12;
MD_FN int cholesky(int D, double* M) {
  for (int j = 0; j < D; ++j) {
    const double diag = M[j * kMaxCv + j];
    double p = diag;
    for (int k = 0; k < j; ++k) p = p - M[j * kMaxCv + k] * M[j * kMaxCv + k];
    if (!(p > kPivotFloor * diag) || !(p > 0.0) || !isfinite(p)) return 1;
    const double l = sqrt(p);
    M[j * kMaxCv + j] = l;
    for (int i = j + 1; i < D; ++i) {
      double t = M[i * kMaxCv + j];
      for (int k = 0; k < j; ++k) t = t - M[i * kMaxCv + k] * M[j * kMaxCv + k];
      M[i * kMaxCv + j] = t / l;
    }
  }
  return 0;
}

// L L^T y = b in place
MD_FN void chol_solve(int D, const double* L, double* b) {
  for (int i = 0; i < D; ++i) {
    double t = b[i];
    for (int k = 0; k < i; ++k) t = t - L[i * kMaxCv + k] * b[k];
    b[i] = t / L[i * kMaxCv + i];
  }
  for (int i = D - 1; i >= 0; --i) {
    double t = b[i];
    for (int k = i + 1; k < D; ++k) t = t - L[k * kMaxCv + i] * b[k];
    b[i] = t / L[i * kMaxCv + i];
  }
}

// The multipliers of one point at w->x (w->fx set): M lambda = g.F and M mu = g.v for the CV atoms' forces and velocities F, V [A, 3]
// (widened), each rounded to fp32 once.  Leaves s, grad and the factor in *w.  Returns SCAN_OK, SCAN_BAD_CV, SCAN_BAD_GRAM or - when a
// multiplier is not finite - SCAN_BAD_SUMS.
MD_FN int multipliers(const Tables& T, Work* w, const double* F, const double* V, float lam[kMaxCv], float mu[kMaxCv]) {
  for (int c = 0; c < kMaxCv; ++c) lam[c] = mu[c] = 0.f;
  if (!cv_all(T, w)) return SCAN_BAD_CV;
  gram(T, w);
  if (cholesky(T.D, w->M)) return SCAN_BAD_GRAM;
  grad_dot(T, w, F);
  chol_solve(T.D, w->M, w->b);
  for (int c = 0; c < T.D; ++c) lam[c] = (float)w->b[c];
  grad_dot(T, w, V);
  chol_solve(T.D, w->M, w->b);
  for (int c = 0; c < T.D; ++c) mu[c] = (float)w->b[c];
  for (int c = 0; c < T.D; ++c)
    if (!isfinite(lam[c]) || !isfinite(mu[c])) return SCAN_BAD_SUMS;  // (the CVs and the factor are finite: a force or a velocity is not)
  return SCAN_OK;
}

// the correction of distinct atom a: - sum_d coef_d g_d on it, fp64 in (CV, slot) order, rounded once; coef [4]: the fp32 multipliers
// widened (indexable: LDS on the device)
MD_FN void correction(const Tables& T, const Work* w, int a, const double* coef, float f[3]) {
  tn_bias::atom_force(T.entries, T.offsets[a], T.offsets[a + 1], coef, w->grad, f);
}

// t_cur one bounded step towards t_fin (a torsion the short way round, and back into (-pi, pi]); on arrival exactly t_fin
MD_FN double drive(int kind, double t_fin, double t_cur, double step) {
  const double d = tn_bias::diff(kind, t_fin, t_cur);
  if (fabs(d) <= step) return t_fin;
  return tn_bias::diff(kind, t_cur + (d > 0.0 ? step : -step), 0.0);
}

// every target has arrived
MD_FN int arrived(int D, const double* t_cur, const double* t_fin) {
  int ok = 1;
  for (int c = 0; c < D; ++c) ok = ok && t_cur[c] == t_fin[c];
  return ok;
}

// The constraint step on w->x (w->fx set): up to max_iter Gauss-Newton corrections x <- x - sum_d nu_d g_d with (g g^T) nu = sigma,
// sigma_d = diff(s_d(x), t_d), until max_d |sigma_d| < tol.  Returns SCAN_OK, or the cause; *iters = corrections made.
MD_FN int constrain(const Tables& T, Work* w, const double* t, double tol, int max_iter, int* iters) {
  for (int it = 0;; ++it) {
    *iters = it;
    if (!cv_all(T, w)) return SCAN_BAD_CV;
    double worst = 0.0;
    for (int c = 0; c < T.D; ++c) {
      const double sg = tn_bias::diff(T.kind[c], w->s[c], t[c]);
      w->b[c] = sg;
      worst = fabs(sg) > worst ? fabs(sg) : worst;
      if (!isfinite(sg)) return SCAN_BAD_CV;
    }
    if (worst < tol) return SCAN_OK;
    if (it >= max_iter) return SCAN_BAD_STEP;
    gram(T, w);
    if (cholesky(T.D, w->M)) return SCAN_BAD_GRAM;
    chol_solve(T.D, w->M, w->b);
    for (int a = 0; a < T.A; ++a)
      for (int p = T.offsets[a]; p < T.offsets[a + 1]; ++p) {
        const int e = T.entries[p];
        for (int k = 0; k < 3; ++k) w->x[a * 3 + k] = w->x[a * 3 + k] - w->b[e >> 2] * w->grad[e * 3 + k];
      }
  }
}

// The controller of one point: tn_min::fire_control, unchanged, on the sums of the projected force and velocity - with the bound it
// converges by switched off until the point's targets have arrived.
MD_FN int scan_fire(tn_min::FireState* s, const tn_min::FireParams& p, const double sums[4], int has_arrived, int64_t step, float coef[3]) {
  tn_min::FireParams q = p;
  if (!has_arrived) q.fmax = 0.0;  // sqrt(fmax2) < 0 never holds
  return tn_min::fire_control(s, q, sums[0], sums[1], sums[2], sums[3], step, coef);
}

// the projection of one atom's vector: one md_add per component
MD_FN void apply(float u[3], const float c[3]) {
  for (int k = 0; k < 3; ++k) u[k] = tn_md::md_add(u[k], c[k]);
}

}  // namespace tn_scan
