// TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident nudged elastic band (torchmd-net_amd/csrc/tn_neb_math.h) compiled
// for the host (hipcc --cuda-host-only), one plain loop per kernel body, loaded through ctypes by tests/neb_host_mirror.py.  The
// statements are the ones a GPU lane runs; tests/test_neb_host.py compares them with tests/neb_oracle.py without a GPU.  With
// -DNEB_HOST_MAIN the file is a stand-alone program for the sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../torchmd-net_amd/csrc/tn_neb_math.h"

namespace {

inline bool interior(int64_t i, int64_t M) { return i > 0 && i < M - 1; }

// d+ and d- of row r (atom of an interior image): the rows n before and n after are the neighbouring images' atom
inline void diffs(const float* pos, int64_t r, int64_t n, float dp[3], float dm[3]) {
  tn_neb::path_diff(pos + 3 * (r - n), pos + 3 * r, pos + 3 * (r + n), dp, dm);
}

}  // namespace

extern "C" {

// the five fp32 terms of every row, zero on endpoint images: t[G M n, 5]
void neb_path_terms(int64_t G, int64_t M, int64_t n, const float* pos, const float* f, const uint8_t* fixed, float* t) {
  for (int64_t img = 0; img < G * M; ++img)
    for (int64_t a = 0; a < n; ++a) {
      const int64_t r = img * n + a;
      if (!interior(img % M, M)) {
        for (int k = 0; k < 5; ++k) t[5 * r + k] = 0.f;
        continue;
      }
      float dp[3], dm[3];
      diffs(pos, r, n, dp, dm);
      tn_neb::path_terms(dp, dm, f + 3 * r, fixed && fixed[a], t + 5 * r);
    }
}

// k_neb_path + the slice loop of k_neb_project, the atoms in index order: sums[G M, 5] (endpoints zero)
void neb_path_sums(int64_t G, int64_t M, int64_t n, const float* pos, const float* f, const uint8_t* fixed, double* sums) {
  for (int64_t img = 0; img < G * M; ++img) {
    double* s = sums + 5 * img;
    for (int k = 0; k < 5; ++k) s[k] = 0.0;
    if (!interior(img % M, M)) continue;
    for (int64_t a = 0; a < n; ++a) {
      const int64_t r = img * n + a;
      float dp[3], dm[3], t[5];
      diffs(pos, r, n, dp, dm);
      tn_neb::path_terms(dp, dm, f + 3 * r, fixed && fixed[a], t);
      for (int k = 0; k < 5; ++k) s[k] += (double)t[k];
    }
  }
}

// per image the weights, the coefficients and the cause; per band the climber: w[G M, 2], s[G M, 2], why[G M], climber[G].  has_free: some
// atom is not fixed (the kernel counts them with the path sums)
void neb_image_control(int64_t G, int64_t M, const float* e, const double* sums, double k, int32_t climb, int32_t has_free, double* w,
                       float* s, int32_t* why, int32_t* climber) {
  for (int64_t b = 0; b < G; ++b) {
    climber[b] = tn_neb::climber(e + b * M, (int)M);
    for (int64_t i = 0; i < M; ++i) {
      const int64_t img = b * M + i;
      w[2 * img] = w[2 * img + 1] = 0.0;
      s[2 * img] = s[2 * img + 1] = 0.f;
      why[img] = 0;
      if (interior(i, M)) why[img] = tn_neb::image_control(e + b * M, (int)M, (int)i, sums + 5 * img, k, climb, has_free, w + 2 * img, s + 2 * img);
    }
  }
}

// F_neb of every row (k_neb_project): zero on endpoints, F on fixed atoms
void neb_project(int64_t G, int64_t M, int64_t n, const float* pos, const float* f, const uint8_t* fixed, const float* s, float* fneb) {
  for (int64_t img = 0; img < G * M; ++img)
    for (int64_t a = 0; a < n; ++a) {
      const int64_t r = img * n + a;
      if (!interior(img % M, M)) {
        fneb[3 * r] = fneb[3 * r + 1] = fneb[3 * r + 2] = 0.f;
      } else if (fixed && fixed[a]) {
        for (int d = 0; d < 3; ++d) fneb[3 * r + d] = f[3 * r + d];
      } else {
        float dp[3], dm[3];
        diffs(pos, r, n, dp, dm);
        tn_neb::project(f + 3 * r, dp, dm, s[2 * img], s[2 * img + 1], fneb + 3 * r);
      }
    }
}

// the FIRE sums of every band on F_neb: per image in atom order, the images in image order: sums[G, 4]
void neb_fire_sums(int64_t G, int64_t M, int64_t n, const float* v, const float* fneb, const uint8_t* fixed, double* sums) {
  for (int64_t b = 0; b < G; ++b) {
    double* s = sums + 4 * b;
    s[0] = s[1] = s[2] = s[3] = 0.0;
    for (int64_t i = 1; i < M - 1; ++i) {
      double t4[4] = {0.0, 0.0, 0.0, 0.0};
      for (int64_t a = 0; a < n; ++a) {
        const int64_t r = (b * M + i) * n + a;
        float t[3];
        tn_min::atom_terms(v + 3 * r, fneb + 3 * r, fixed && fixed[a], t);
        t4[0] += (double)t[0];
        t4[1] += (double)t[1];
        t4[2] += (double)t[2];
        t4[3] = (double)t[1] > t4[3] ? (double)t[1] : t4[3];
      }
      s[0] += t4[0];
      s[1] += t4[1];
      s[2] += t4[2];
      s[3] = t4[3] > s[3] ? t4[3] : s[3];
    }
  }
}

// the per-row update (k_neb_atoms, MOVE) in place
void neb_move(int64_t G, int64_t M, int64_t n, const int64_t* conv, const uint8_t* fixed, const float* coef, float* x, float* v,
              const float* fneb) {
  for (int64_t img = 0; img < G * M; ++img)
    for (int64_t a = 0; a < n; ++a) {
      const int64_t r = img * n + a, b = img / M;
      if (!interior(img % M, M) || conv[b] >= 0 || (fixed && fixed[a])) {
        v[3 * r] = v[3 * r + 1] = v[3 * r + 2] = 0.f;
        continue;
      }
      tn_min::atom_move(x + 3 * r, v + 3 * r, fneb + 3 * r, coef[3 * b], coef[3 * b + 1], coef[3 * b + 2]);
    }
}

// The analytic surface of the tests, evaluated in fp64 at the fp32 positions and rounded once: atom 0 feels
// (x^2 - 1)^2 + kappa (y - A (1 - x^2))^2 + kappa z^2, atoms j >= 1 feel kappa |r_j - s_j|^2 / 2.  e[n_img], f[n_img n, 3].
void neb_surface(int64_t n_img, int64_t n, const float* x, const double* sites, double kappa, double A, float* e, float* f) {
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

// A whole band optimisation on the surface, the launch sequence written as loops: the control of the start path, then per step move,
// evaluation, path sums, coefficients, projection, FIRE sums, control, until every band has converged or max_steps is reached.  In
// place on x; conv[G], e[G M] and climber[G] of the last evaluated step.  Returns the steps taken, or -cause when a band was unusable.
int64_t neb_run(int64_t G, int64_t M, int64_t n, const double* sites, double kappa, double A, float* x, const uint8_t* fixed, double dt0,
                double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha0, double f_alpha, double max_step, double fmax,
                double spring_k, int32_t climb, int64_t max_steps, int64_t* conv, float* e, int32_t* climber) {
  tn_min::FireParams p;
  p.dt_max = dt_max;
  p.n_min = n_min;
  p.f_inc = f_inc;
  p.f_dec = f_dec;
  p.alpha0 = alpha0;
  p.f_alpha = f_alpha;
  p.max_step = max_step;
  p.fmax = fmax;
  const int64_t GM = G * M, N = GM * n;
  float* v = (float*)calloc(3 * N, sizeof(float));
  float* f = (float*)malloc(3 * N * sizeof(float));
  float* fneb = (float*)malloc(3 * N * sizeof(float));
  double* psums = (double*)malloc(5 * GM * sizeof(double));
  double* w = (double*)malloc(2 * GM * sizeof(double));
  float* s = (float*)malloc(2 * GM * sizeof(float));
  int32_t* why = (int32_t*)malloc(GM * sizeof(int32_t));
  double* fsums = (double*)malloc(4 * G * sizeof(double));
  float* coef = (float*)calloc(3 * G, sizeof(float));
  tn_min::FireState* st = (tn_min::FireState*)malloc(G * sizeof(tn_min::FireState));
  for (int64_t b = 0; b < G; ++b) {
    st[b].dt = dt0;
    st[b].alpha = alpha0;
    st[b].n_pos = 0;
    st[b].converged_at = -1;
    conv[b] = -1;
  }
  int32_t has_free = 0;
  for (int64_t a = 0; a < n; ++a) has_free |= !(fixed && fixed[a]);
  int64_t ret = 0;
  for (int64_t step = 0;; ++step) {
    if (step > 0) neb_move(G, M, n, conv, fixed, coef, x, v, fneb);
    neb_surface(GM, n, x, sites, kappa, A, e, f);
    neb_path_sums(G, M, n, x, f, fixed, psums);
    neb_image_control(G, M, e, psums, spring_k, climb, has_free, w, s, why, climber);
    neb_project(G, M, n, x, f, fixed, s, fneb);
    neb_fire_sums(G, M, n, v, fneb, fixed, fsums);
    int64_t open = 0;
    int cause = 0;
    for (int64_t b = 0; b < G && !cause; ++b) {
      if (st[b].converged_at >= 0) continue;
      for (int64_t i = 1; i < M - 1; ++i) cause = why[b * M + i] > cause ? why[b * M + i] : cause;
      if (!cause && tn_min::fire_control(&st[b], p, fsums[4 * b], fsums[4 * b + 1], fsums[4 * b + 2], fsums[4 * b + 3], step, coef + 3 * b) ==
                        tn_min::FIRE_UNUSABLE)
        cause = tn_neb::NEB_BAD_SUMS;
      conv[b] = st[b].converged_at;
      open += st[b].converged_at < 0;
    }
    if (cause) {
      ret = -cause;
      break;
    }
    if (open == 0 || step == max_steps) {
      ret = step;
      break;
    }
  }
  free(v);
  free(f);
  free(fneb);
  free(psums);
  free(w);
  free(s);
  free(why);
  free(fsums);
  free(coef);
  free(st);
  return ret;
}

}  // extern "C"

#ifdef NEB_HOST_MAIN
// every entry of the mirror on heap arrays of exact size: a band of 5 images x 3 atoms on the surface, plain and then climbing, and a
// path with coincident images
int main() {
  const int64_t M = 5, n = 3, N = M * n;
  double* sites = (double*)malloc(3 * n * sizeof(double));
  float* x = (float*)malloc(3 * N * sizeof(float));
  float* x0 = (float*)malloc(3 * N * sizeof(float));
  uint8_t* fixed = (uint8_t*)calloc(n, 1);
  int64_t* conv = (int64_t*)malloc(sizeof(int64_t));
  float* e = (float*)malloc(M * sizeof(float));
  int32_t* climber = (int32_t*)malloc(sizeof(int32_t));
  for (int64_t j = 0; j < 3 * n; ++j) sites[j] = 0.5 * (double)(j % 4) - 0.7;
  for (int64_t i = 0; i < M; ++i)
    for (int64_t a = 0; a < n; ++a)
      for (int d = 0; d < 3; ++d) {
        const double t = (double)i / (double)(M - 1);
        double r = a == 0 ? (d == 0 ? -1.0 + 2.0 * t : 0.0) : sites[3 * a + d];
        if (i > 0 && i < M - 1) r += 0.03 * (double)((7 * i + 3 * a + d) % 5 - 2);
        x0[3 * (i * n + a) + d] = (float)r;
      }
  int bad = 0;
  for (int climb = 0; climb < 2; ++climb) {
    for (int64_t j = 0; j < 3 * N; ++j) x[j] = x0[j];
    const int64_t steps = neb_run(1, M, n, sites, 2.0, 0.5, x, fixed, 0.1, 1.0, 5, 1.1, 0.5, 0.1, 0.99, 0.2, 1e-3, 0.1, climb, 400, conv, e, climber);
    printf("climb %d: steps %lld converged_at %lld climber %d barrier %.7f\n", climb, (long long)steps, (long long)conv[0], climber[0],
           (double)e[climber[0]] - (double)e[0]);
    bad |= steps <= 0 || conv[0] < 0;
  }
  fixed[1] = 1;
  for (int64_t j = 0; j < 3 * N; ++j) x[j] = x0[j];
  bad |= neb_run(1, M, n, sites, 2.0, 0.5, x, fixed, 0.1, 1.0, 5, 1.1, 0.5, 0.1, 0.99, 0.2, 1e-3, 1.0, 1, 400, conv, e, climber) <= 0;
  for (int64_t j = 0; j < 3 * n; ++j) x[3 * n * 2 + j] = x[3 * n * 1 + j] = x[3 * n * 3 + j];  // images 1, 2, 3 coincide
  const int64_t r = neb_run(1, M, n, sites, 2.0, 0.5, x, fixed, 0.1, 1.0, 5, 1.1, 0.5, 0.1, 0.99, 0.2, 1e-3, 0.1, 0, 10, conv, e, climber);
  printf("coincident images: %lld\n", (long long)r);
  bad |= r != -tn_neb::NEB_BAD_PATH;
  float* t = (float*)malloc(5 * N * sizeof(float));
  float* f = (float*)malloc(3 * N * sizeof(float));
  neb_surface(M, n, x0, sites, 2.0, 0.5, e, f);
  neb_path_terms(1, M, n, x0, f, fixed, t);
  free(t);
  free(f);
  free(sites);
  free(x);
  free(x0);
  free(fixed);
  free(conv);
  free(e);
  free(climber);
  return bad;
}
#endif
