// TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident dimer saddle search (torchmd-net_amd/csrc/tn_dimer_math.h) compiled
// for the host (hipcc --cuda-host-only), one plain loop per kernel body, loaded through ctypes by tests/dimer_host_mirror.py.  The
// statements are the ones a GPU lane runs; tests/test_dimer_host.py compares them with tests/dimer_oracle.py without a GPU.  With
// -DDIMER_HOST_MAIN the file is a stand-alone program for the sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../torchmd-net_amd/csrc/tn_dimer_math.h"

using namespace tn_dimer;

namespace {

// the rows of atom a of dimer d: N, M [G n, 3]; F0, F1, F2 out of f [3 G n, 3]
struct Rows {
  const float *N, *M, *f0, *f1, *f2;
};

inline Rows rows(int64_t n, const float* mode, const float* partner, const float* f, int64_t d, int64_t a) {
  const int64_t r = d * n + a, r0 = 3 * d * n + a;
  return {mode + 3 * r, partner + 3 * r, f + 3 * r0, f + 3 * (r0 + n), f + 3 * (r0 + 2 * n)};
}

inline int has_free(int64_t n, const uint8_t* fixed) {
  int any = 0;
  for (int64_t a = 0; a < n; ++a) any |= !(fixed && fixed[a]);
  return any;
}

}  // namespace

extern "C" {

// the seven fp32 terms of every atom of every dimer: t[G n, 7]
void dimer_sum_terms(int64_t G, int64_t n, const float* mode, const float* partner, const float* f, const uint8_t* fixed, double delta,
                     float* t) {
  const float inv = (float)(1.0 / delta);
  for (int64_t d = 0; d < G; ++d)
    for (int64_t a = 0; a < n; ++a) {
      const Rows r = rows(n, mode, partner, f, d, a);
      sum_terms(r.N, r.M, r.f0, r.f1, r.f2, inv, fixed && fixed[a], t + 7 * (d * n + a));
    }
}

// k_dimer_sums + the slice loop of k_dimer_project, the atoms in index order: S[G, N_SUMS]
void dimer_sums(int64_t G, int64_t n, const float* mode, const float* partner, const float* f, const uint8_t* fixed, double delta,
                double* S) {
  const float inv = (float)(1.0 / delta);
  for (int64_t d = 0; d < G; ++d) {
    double* s = S + N_SUMS * d;
    for (int k = 0; k < N_SUMS; ++k) s[k] = 0.0;
    for (int64_t a = 0; a < n; ++a) {
      const Rows r = rows(n, mode, partner, f, d, a);
      float t[7];
      sum_terms(r.N, r.M, r.f0, r.f1, r.f2, inv, fixed && fixed[a], t);
      for (int k = 0; k < 7; ++k) s[k] += (double)t[k];
      s[S_FREE] += (fixed && fixed[a]) ? 0.0 : 1.0;
    }
  }
}

// nu^2 of every dimer from the vectors, the atoms in index order: rot[G, 2] = co, si
void dimer_nu2(int64_t G, int64_t n, const float* mode, const float* partner, const uint8_t* fixed, const double* rot, double* nu2) {
  for (int64_t d = 0; d < G; ++d) {
    nu2[d] = 0.0;
    for (int64_t a = 0; a < n; ++a) {
      if (fixed && fixed[a]) continue;
      nu2[d] += nu2_term(mode + 3 * (d * n + a), partner + 3 * (d * n + a), rot[2 * d], rot[2 * d + 1]);
    }
  }
}

// the rotation of every dimer from its sums and energies: cause[G], q[G, 3], rot[G, 2], branch[G]
void dimer_rotation(int64_t G, const double* S, const float* e, int32_t free_atoms, int32_t* cause, double* q, double* rot, int32_t* branch) {
  for (int64_t d = 0; d < G; ++d) {
    int br;
    cause[d] = mode_rotation(S + N_SUMS * d, e + 3 * d, free_atoms, q + 3 * d, rot + 2 * d, rot + 2 * d + 1, &br);
    branch[d] = br;
  }
}

// the coefficients once nu^2 is known (dimers whose cause is set are left with zeros): Cp[G, 2] = C, p; coef[G, N_COEF] entries 0..6
void dimer_mode_coef(int64_t G, const double* S, const double* q, const double* rot, const double* nu2, int32_t free_atoms, int32_t* cause,
                     double* Cp, float* coef) {
  for (int64_t d = 0; d < G; ++d) {
    for (int k = 0; k <= C_SI; ++k) coef[N_COEF * d + k] = 0.f;
    Cp[2 * d] = Cp[2 * d + 1] = 0.0;
    if (cause[d]) continue;
    cause[d] = mode_coef(q + 3 * d, S + N_SUMS * d, rot[2 * d], rot[2 * d + 1], nu2[d], free_atoms, coef + N_COEF * d, Cp + 2 * d, Cp + 2 * d + 1);
    if (cause[d]) Cp[2 * d] = Cp[2 * d + 1] = 0.0;
  }
}

// the per-atom half of k_dimer_project: np, t, feff [G n, 3], terms [G n, N_PART]
void dimer_project(int64_t G, int64_t n, const float* mode, const float* partner, const float* f, const uint8_t* fixed, double delta,
                   const float* coef, float* np, float* t, float* feff, float* terms) {
  const float inv = (float)(1.0 / delta);
  for (int64_t d = 0; d < G; ++d)
    for (int64_t a = 0; a < n; ++a) {
      const Rows r = rows(n, mode, partner, f, d, a);
      const int64_t i = d * n + a;
      project_atom(r.N, r.M, r.f0, r.f1, r.f2, inv, coef + N_COEF * d, fixed && fixed[a], np + 3 * i, t + 3 * i, feff + 3 * i, terms + N_PART * i);
    }
}

// the reductions of k_dimer_project, the atoms in index order: fsums[G, 4] = vf, ff, vv, fmax2 on F_eff; P[G, N_PART]
void dimer_part_sums(int64_t G, int64_t n, const float* vel, const float* feff, const float* terms, const uint8_t* fixed, double* fsums,
                     double* P) {
  for (int64_t d = 0; d < G; ++d) {
    double* s = fsums + 4 * d;
    s[0] = s[1] = s[2] = s[3] = 0.0;
    for (int k = 0; k < N_PART; ++k) P[N_PART * d + k] = 0.0;
    for (int64_t a = 0; a < n; ++a) {
      const int64_t i = d * n + a;
      float t[3];
      tn_min::atom_terms(vel + 3 * i, feff + 3 * i, fixed && fixed[a], t);
      s[0] += (double)t[0];
      s[1] += (double)t[1];
      s[2] += (double)t[2];
      s[3] = (double)t[1] > s[3] ? (double)t[1] : s[3];
      for (int k = 0; k < N_PART; ++k) P[N_PART * d + k] += (double)terms[N_PART * i + k];
    }
  }
}

// the partner's coefficients: coef[G, N_COEF] entries 7..9, resid[G], branch[G]
void dimer_partner(int64_t G, const double* P, int32_t free_atoms, float* coef, double* resid, int32_t* branch) {
  for (int64_t d = 0; d < G; ++d) branch[d] = partner_coef(P + N_PART * d, free_atoms, coef + N_COEF * d, resid + d);
}

// the controller of every dimer: state in place, fcoef[G, 3], ret[G]
void dimer_fire_control(int64_t G, double* dt, double* alpha, int32_t* n_pos, int64_t* conv, const double* fsums, const double* Cp,
                        int32_t translate, int32_t free_atoms, int64_t step, double dt_max, int32_t n_min, double f_inc, double f_dec,
                        double alpha0, double f_alpha, double max_step, double fmax, float* fcoef, int32_t* ret) {
  tn_min::FireParams p;
  p.dt_max = dt_max;
  p.n_min = n_min;
  p.f_inc = f_inc;
  p.f_dec = f_dec;
  p.alpha0 = alpha0;
  p.f_alpha = f_alpha;
  p.max_step = max_step;
  p.fmax = fmax;
  for (int64_t d = 0; d < G; ++d) {
    tn_min::FireState s = {dt[d], alpha[d], n_pos[d], conv[d]};
    ret[d] = dimer_fire(&s, p, fsums + 4 * d, Cp[2 * d], translate, free_atoms, step, fcoef + 3 * d);
    dt[d] = s.dt;
    alpha[d] = s.alpha;
    n_pos[d] = s.n_pos;
    conv[d] = s.converged_at;
  }
}

// k_dimer_atoms in place.  accept[G] != 0: N <- N', M <- M' of that dimer; move != 0: the update of R0 (frozen[G] != 0, a fixed atom
// or translate = 0: v <- 0, x keeps its bits); then always the rewrite of images 1 and 2.  pos [3 G n, 3]; vel, mode, partner [G n, 3].
void dimer_atoms(int64_t G, int64_t n, const uint8_t* accept, int32_t move, const uint8_t* frozen, int32_t translate, const uint8_t* fixed,
                 double delta, const float* coef, const float* fcoef, const float* np, const float* t, const float* feff, float* pos,
                 float* vel, float* mode, float* partner) {
  const float dl = (float)delta;
  for (int64_t d = 0; d < G; ++d)
    for (int64_t a = 0; a < n; ++a) {
      const int64_t i = d * n + a, r0 = 3 * d * n + a;
      const int fx = fixed && fixed[a];
      if (accept[d]) {
        float nn[3], mn[3];
        accept_atom(mode + 3 * i, partner + 3 * i, np + 3 * i, t + 3 * i, coef + N_COEF * d, fx, nn, mn);
        for (int k = 0; k < 3; ++k) {
          mode[3 * i + k] = nn[k];
          partner[3 * i + k] = mn[k];
        }
      }
      if (!move) {
      } else if (frozen[d] || fx || !translate) {
        vel[3 * i] = vel[3 * i + 1] = vel[3 * i + 2] = 0.f;
      } else {
        tn_min::atom_move(pos + 3 * r0, vel + 3 * i, feff + 3 * i, fcoef[3 * d], fcoef[3 * d + 1], fcoef[3 * d + 2]);
      }
      image_pos(pos + 3 * r0, dl, mode + 3 * i, pos + 3 * (r0 + n));
      image_pos(pos + 3 * r0, dl, partner + 3 * i, pos + 3 * (r0 + 2 * n));
    }
}

// The analytic surface of tests/neb_oracle.py, evaluated in fp64 at the fp32 positions and rounded once: atom 0 feels
// (x^2 - 1)^2 + kappa (y - A (1 - x^2))^2 + kappa z^2, atoms j >= 1 feel kappa |r_j - s_j|^2 / 2.  e[n_img], f[n_img n, 3].
void dimer_surface(int64_t n_img, int64_t n, const float* x, const double* sites, double kappa, double A, float* e, float* f) {
  for (int64_t img = 0; img < n_img; ++img) {
    const float* r = x + 3 * img * n;
    float* fr = f + 3 * img * n;
    const double X = r[0], Y = r[1], Z = r[2];
    const double u = X * X - 1.0, w = Y + A * u;
    double E = u * u + kappa * w * w + kappa * Z * Z;
    fr[0] = (float)-(4.0 * X * u + 2.0 * kappa * w * (2.0 * A * X));
    fr[1] = (float)-(2.0 * kappa * w);
    fr[2] = (float)-(2.0 * kappa * Z);
    for (int64_t j = 1; j < n; ++j)
      for (int d = 0; d < 3; ++d) {
        const double dr = (double)r[3 * j + d] - sites[3 * j + d];
        E += 0.5 * kappa * dr * dr;
        fr[3 * j + d] = (float)-(kappa * dr);
      }
    e[img] = (float)E;
  }
}

// A whole search on the surface, the launch sequence written as loops: the control of the start images, then per step the move and
// the rewrite of the images, the evaluation, the sums, the rotation, nu^2, the coefficients, the projection, the partner, the
// controller and the accept, until every dimer has converged or max_steps is reached.  In place on pos [3 G n, 3], mode and partner
// [G n, 3]; conv[G], e[3 G], and curv[G], resid[G] of the last controlled step of each dimer.  Returns the steps taken, or -cause.
int64_t dimer_run(int64_t G, int64_t n, const double* sites, double kappa, double A, float* pos, float* mode, float* partner,
                  const uint8_t* fixed, double delta, int32_t translate, double dt0, double dt_max, int32_t n_min, double f_inc, double f_dec,
                  double alpha0, double f_alpha, double max_step, double fmax, int64_t max_steps, int64_t* conv, float* e, double* curv,
                  double* resid) {
  const int64_t N = G * n;
  const int32_t fa = has_free(n, fixed);
  float* vel = (float*)calloc(3 * N + 1, sizeof(float));
  float* f = (float*)malloc((9 * N + 1) * sizeof(float));
  float* np = (float*)malloc((3 * N + 1) * sizeof(float));
  float* t = (float*)malloc((3 * N + 1) * sizeof(float));
  float* feff = (float*)malloc((3 * N + 1) * sizeof(float));
  float* feff_keep = (float*)calloc(3 * N + 1, sizeof(float));
  float* terms = (float*)malloc((N_PART * N + 1) * sizeof(float));
  double* S = (double*)malloc(N_SUMS * G * sizeof(double));
  double* q = (double*)malloc(3 * G * sizeof(double));
  double* rot = (double*)malloc(2 * G * sizeof(double));
  double* nu2 = (double*)malloc(G * sizeof(double));
  double* Cp = (double*)malloc(2 * G * sizeof(double));
  double* P = (double*)malloc(N_PART * G * sizeof(double));
  double* fsums = (double*)malloc(4 * G * sizeof(double));
  double* rs = (double*)malloc(G * sizeof(double));
  float* coef = (float*)calloc(N_COEF * G, sizeof(float));
  float* fcoef = (float*)calloc(3 * G, sizeof(float));
  float* ftry = (float*)calloc(3 * G, sizeof(float));
  int32_t* cause = (int32_t*)malloc(G * sizeof(int32_t));
  int32_t* branch = (int32_t*)malloc(G * sizeof(int32_t));
  int32_t* ret = (int32_t*)malloc(G * sizeof(int32_t));
  double* dt = (double*)malloc(G * sizeof(double));
  double* alpha = (double*)malloc(G * sizeof(double));
  int32_t* n_pos = (int32_t*)calloc(G, sizeof(int32_t));
  uint8_t* accept = (uint8_t*)calloc(G, 1);
  uint8_t* frozen = (uint8_t*)calloc(G, 1);
  uint8_t* none = (uint8_t*)calloc(G, 1);
  for (int64_t d = 0; d < G; ++d) {
    dt[d] = dt0;
    alpha[d] = alpha0;
    conv[d] = -1;
    curv[d] = resid[d] = 0.0;
  }
  int64_t result = 0;
  for (int64_t step = 0;; ++step) {
    if (step > 0) dimer_atoms(G, n, none, 1, frozen, translate, fixed, delta, coef, fcoef, np, t, feff_keep, pos, vel, mode, partner);
    dimer_surface(3 * G, n, pos, sites, kappa, A, e, f);
    dimer_sums(G, n, mode, partner, f, fixed, delta, S);
    dimer_rotation(G, S, e, fa, cause, q, rot, branch);
    dimer_nu2(G, n, mode, partner, fixed, rot, nu2);
    dimer_mode_coef(G, S, q, rot, nu2, fa, cause, Cp, coef);
    dimer_project(G, n, mode, partner, f, fixed, delta, coef, np, t, feff, terms);
    dimer_part_sums(G, n, vel, feff, terms, fixed, fsums, P);
    int bad = 0;
    for (int64_t d = 0; d < G; ++d) {  // pass 1 on copies of the state
      if (frozen[d]) continue;
      int c = cause[d];
      double dt1 = dt[d], al1 = alpha[d];
      int32_t np1 = n_pos[d], r1;
      int64_t cv1 = conv[d];
      if (!c) {
        dimer_fire_control(1, &dt1, &al1, &np1, &cv1, fsums + 4 * d, Cp + 2 * d, translate, fa, step, dt_max, n_min, f_inc, f_dec, alpha0,
                           f_alpha, max_step, fmax, ftry + 3 * d, &r1);
        if (r1 == tn_min::FIRE_UNUSABLE) c = DIMER_BAD_SUMS;
      }
      bad = c > bad ? c : bad;
    }
    if (bad) {
      result = -bad;
      break;
    }
    int64_t open = 0;
    for (int64_t d = 0; d < G; ++d) {
      accept[d] = !frozen[d];
      if (frozen[d]) {
        fcoef[3 * d] = fcoef[3 * d + 1] = fcoef[3 * d + 2] = 0.f;
        continue;
      }
      dimer_partner(1, P + N_PART * d, fa, coef + N_COEF * d, rs + d, branch + d);
      dimer_fire_control(1, dt + d, alpha + d, n_pos + d, conv + d, fsums + 4 * d, Cp + 2 * d, translate, fa, step, dt_max, n_min, f_inc,
                         f_dec, alpha0, f_alpha, max_step, fmax, fcoef + 3 * d, ret + d);
      curv[d] = Cp[2 * d];
      resid[d] = rs[d];
      memcpy(feff_keep + 3 * d * n, feff + 3 * d * n, 3 * n * sizeof(float));
    }
    dimer_atoms(G, n, accept, 0, frozen, translate, fixed, delta, coef, fcoef, np, t, feff, pos, vel, mode, partner);
    for (int64_t d = 0; d < G; ++d) {
      frozen[d] = conv[d] >= 0;
      open += !frozen[d];
    }
    if (open == 0 || step == max_steps) {
      result = step;
      break;
    }
  }
  free(vel); free(f); free(np); free(t); free(feff); free(feff_keep); free(terms); free(S); free(q); free(rot); free(nu2); free(Cp);
  free(P); free(fsums); free(rs); free(coef); free(fcoef); free(ftry); free(cause); free(branch); free(ret); free(dt); free(alpha);
  free(n_pos); free(accept); free(frozen); free(none);
  return result;
}

}  // extern "C"

#ifdef DIMER_HOST_MAIN
// every entry of the mirror on heap arrays of exact size: one dimer of 3 atoms on the surface from the concave and (n = 1) the convex
// start, a mode search, a fixed atom, and a mode of length zero
static int64_t one(int64_t n, const double* sites, const float* x0, int zero_mode, const uint8_t* fixed, int32_t translate, int64_t max_steps,
                   int64_t* conv, double* curv) {
  float* pos = (float*)malloc(9 * n * sizeof(float));
  float* mode = (float*)calloc(3 * n, sizeof(float));
  float* partner = (float*)calloc(3 * n, sizeof(float));
  float* e = (float*)malloc(3 * sizeof(float));
  double resid;
  if (!zero_mode) {
    mode[0] = 0.6f;
    mode[1] = 0.8f;
    partner[0] = -0.8f;
    partner[1] = 0.6f;
  }
  for (int64_t j = 0; j < 3 * n; ++j) {
    pos[j] = x0[j];
    pos[3 * n + j] = x0[j] + 0.01f * mode[j];
    pos[6 * n + j] = x0[j] + 0.01f * partner[j];
  }
  const int64_t r = dimer_run(1, n, sites, 2.0, 0.5, pos, mode, partner, fixed, 0.01, translate, 0.1, 1.0, 5, 1.1, 0.5, 0.1, 0.99, 0.2, 1e-3,
                              max_steps, conv, e, curv, &resid);
  printf("n %lld translate %d: steps %lld converged_at %lld C %.6f |T| %.3e x0 %.5f %.5f %.5f E %.7f\n", (long long)n, translate, (long long)r,
         (long long)conv[0], curv[0], resid, pos[0], pos[1], pos[2], e[0]);
  free(pos);
  free(mode);
  free(partner);
  free(e);
  return r;
}

int main() {
  const int64_t n = 3;
  double* sites = (double*)malloc(3 * n * sizeof(double));
  float* x0 = (float*)malloc(3 * n * sizeof(float));
  uint8_t* fixed = (uint8_t*)calloc(n, 1);
  int64_t conv;
  double curv;
  for (int64_t j = 0; j < 3 * n; ++j) {
    sites[j] = 0.5 * (double)(j % 4) - 0.7;
    x0[j] = (float)(sites[j] + 0.02 * (double)(j % 3 - 1));
  }
  x0[0] = 0.4f;
  x0[1] = 0.3f;
  x0[2] = 0.1f;
  int bad = 0;
  int64_t r = one(n, sites, x0, 0, fixed, 1, 400, &conv, &curv);
  bad |= r <= 0 || conv < 0 || !(curv < 0.0);
  r = one(n, sites, x0, 0, fixed, 0, 20, &conv, &curv);
  bad |= r != 20 || conv != -1;
  fixed[1] = 1;
  r = one(n, sites, x0, 0, fixed, 1, 400, &conv, &curv);
  bad |= r <= 0 || conv < 0;
  fixed[1] = 0;
  r = one(n, sites, x0, 1, fixed, 1, 10, &conv, &curv);
  bad |= r != -DIMER_BAD_MODE;
  x0[0] = 0.9f;
  x0[1] = 0.1f;
  x0[2] = 0.05f;
  r = one(1, sites, x0, 0, fixed, 1, 400, &conv, &curv);
  bad |= r <= 0 || conv < 0;
  float* t = (float*)malloc(7 * n * sizeof(float));
  float* f = (float*)malloc(9 * n * sizeof(float));
  float* pos = (float*)malloc(9 * n * sizeof(float));
  float* e = (float*)malloc(3 * sizeof(float));
  for (int64_t j = 0; j < 9 * n; ++j) pos[j] = x0[j % (3 * n)];
  dimer_surface(3, n, pos, sites, 2.0, 0.5, e, f);
  dimer_sum_terms(1, n, x0, x0, f, fixed, 0.01, t);
  free(t);
  free(f);
  free(pos);
  free(e);
  free(sites);
  free(x0);
  free(fixed);
  return bad;
}
#endif
