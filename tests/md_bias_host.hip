// TEST INFRASTRUCTURE ONLY: the collective-variable bias of the device-resident MD loop (torchmd-net_amd/csrc/tn_bias_math.h) compiled
// for the host (hipcc --cuda-host-only), one plain loop per kernel body, loaded through ctypes by tests/md_bias_host_mirror.py.  The
// statements are the ones a GPU lane runs; tests/test_md_bias_host.py compares them with tests/md_bias_oracle.py without a GPU.
// With -DMD_BIAS_HOST_MAIN the file is a stand-alone program (its own main) that drives every entry once: the build the host test
// runs under -fsanitize=address,undefined.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../torchmd-net_amd/csrc/tn_bias_math.h"

extern "C" {

// n independent CVs: x [n, 4, 3] fp32 positions (unused slots ignored) -> s [n], g [n, 4, 3]
void bias_cv(int64_t n, const int32_t* kind, const float* x, double* s, double* g) {
  for (int64_t c = 0; c < n; ++c) {
    double p[4][3];
    for (int a = 0; a < 4; ++a)
      for (int d = 0; d < 3; ++d) p[a][d] = (double)x[(c * 4 + a) * 3 + d];
    s[c] = tn_bias::cv_eval(kind[c], p[0], p[1], p[2], p[3], g + c * 12, g + c * 12 + 3, g + c * 12 + 6, g + c * 12 + 9);
  }
}

void bias_diff(int64_t n, int32_t kind, const double* a, const double* b, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = tn_bias::diff(kind, a[i], b[i]);
}

void bias_restraint(int64_t n, const int32_t* kind, const double* kappa, const double* delta, double* V, double* dV) {
  for (int64_t i = 0; i < n; ++i) tn_bias::restraint(kind[i], kappa[i], delta[i], V + i, dV + i);
}

int64_t bias_visible(uint64_t n, uint64_t step0, uint64_t pace, int32_t W, uint64_t base, int64_t H) {
  return tn_bias::hills_visible(n, step0, pace, W, base, H);
}

int64_t bias_slot(uint64_t n, uint64_t step0, uint64_t pace, int32_t W, int32_t w, uint64_t base, int64_t H) {
  return tn_bias::hill_slot(n, step0, pace, W, w, base, H);
}

double bias_height(double h0, double V, double kT, double gamma) { return tn_bias::hill_height(h0, V, kT, gamma); }

static void load3(const float* pos, int64_t i, int64_t N, double x[3]) {
  const bool ok = i >= 0 && i < N;
  for (int d = 0; d < 3; ++d) x[d] = ok ? (double)pos[i * 3 + d] : (double)NAN;
}

// the lanes of one wave added by the xor tree (offsets 32, 16, .. 1): the value lane 0 ends with
static double wave_tree(const double* lane) {
  double v[64], u[64];
  for (int l = 0; l < 64; ++l) v[l] = lane[l];
  for (int o = 32; o >= 1; o >>= 1) {
    for (int l = 0; l < 64; ++l) u[l] = v[l] + v[l ^ o];
    for (int l = 0; l < 64; ++l) v[l] = u[l];
  }
  return v[0];
}

// k_md_bias: every block of the launch, in walker order.  `head` = {step0, hill_base}, `n` the loop's step counter, `status` the
// loop's status word (read once, as every block reads it when it starts; written 4), `overflow` the graph's counts[2].
void bias_launch(int32_t N, int32_t B, int32_t D, int32_t A, int32_t W, int32_t dm, int32_t mcv0, int32_t mcv1, int32_t deposit,
                 const float* pos, float* forces, const int32_t* cv_kind, const int32_t* cv_atoms, const int32_t* mol_start,
                 const int32_t* atom_rel, const int32_t* offsets, const int32_t* entries, const int32_t* res_kind, const double* kappa,
                 const double* center, double sigma0, double sigma1, double h0, double kT, double gamma, uint64_t pace, int64_t H,
                 const uint64_t* head, uint64_t n, double* hills, uint32_t* status, int32_t overflow, double* cv_row, double* res_row,
                 double* bias_row, float* force_row) {
  if (*status || overflow) return;
  const double is0 = dm > 0 ? 1.0 / (sigma0 * sigma0) : 0.0, is1 = dm == 2 ? 1.0 / (sigma1 * sigma1) : 0.0;
  if (dm < 2) mcv1 = mcv0;
  for (int b = 0; b < B; ++b) {
    double sh_s[tn_bias::kMaxCv], sh_er[tn_bias::kMaxCv], sh_dv[tn_bias::kMaxCv], sh_tot[tn_bias::kMaxCv], sh_grad[tn_bias::kMaxCv * 12];
    int bad = 0;
    const int64_t start = mol_start[b];
    for (int t = 0; t < D; ++t) {
      const int kind = cv_kind[t];
      double xi[3], xj[3], xk[3], xl[3];
      load3(pos, start + cv_atoms[t * 4 + 0], N, xi);
      load3(pos, start + cv_atoms[t * 4 + 1], N, xj);
      load3(pos, kind >= tn_bias::kAngle ? start + cv_atoms[t * 4 + 2] : start, N, xk);
      load3(pos, kind == tn_bias::kTorsion ? start + cv_atoms[t * 4 + 3] : start, N, xl);
      double* g = sh_grad + t * 12;
      const double s = tn_bias::cv_eval(kind, xi, xj, xk, xl, g, g + 3, g + 6, g + 9);
      double er = 0.0, dv = 0.0;
      if (res_kind[t] != tn_bias::kNone)
        tn_bias::restraint(res_kind[t], kappa[(int64_t)b * D + t], tn_bias::diff(kind, s, center[(int64_t)b * D + t]), &er, &dv);
      bool ok = isfinite(s) && isfinite(er) && isfinite(dv);
      for (int d = 0; d < 12; ++d) ok = ok && isfinite(g[d]);
      sh_s[t] = s;
      sh_er[t] = er;
      sh_dv[t] = dv;
      if (!ok) bad = 1;
    }
    double V = 0.0, d0 = 0.0, d1 = 0.0;
    const int g = b / W, w = b - g * W;
    double* c0 = hills ? hills + (int64_t)g * (dm + 1) * H : nullptr;
    if (dm > 0) {
      const int64_t nvis = tn_bias::hills_visible(n, head[0], pace, W, head[1], H);
      const double* c1 = c0 + (dm == 2 ? H : 0);
      const double* hw = c0 + (int64_t)dm * H;
      double lanes[3][256];
      for (int t = 0; t < 256; ++t) {
        double v = 0.0, a0 = 0.0, a1 = 0.0;
        for (int64_t h = t; h < nvis; h += 256)
          tn_bias::hill_term(dm, cv_kind[mcv0], cv_kind[mcv1], sh_s[mcv0], sh_s[mcv1], c0[h], c1[h], is0, is1, hw[h], &v, &a0, &a1);
        lanes[0][t] = v;
        lanes[1][t] = a0;
        lanes[2][t] = a1;
      }
      double r[3];
      for (int k = 0; k < 3; ++k)
        r[k] = ((wave_tree(lanes[k]) + wave_tree(lanes[k] + 64)) + wave_tree(lanes[k] + 128)) + wave_tree(lanes[k] + 192);
      V = r[0];
      d0 = r[1];
      d1 = r[2];
      if (!(isfinite(V) && isfinite(d0) && isfinite(d1))) bad = 1;
    }
    for (int t = 0; t < D; ++t) {
      double tot = sh_dv[t];
      if (dm > 0 && t == mcv0) tot = tot + d0;
      if (dm == 2 && t == mcv1) tot = tot + d1;
      sh_tot[t] = tot;
    }
    float f[tn_bias::kMaxAtoms][3];
    for (int t = 0; t < A; ++t) {
      int e0 = offsets[t], e1 = offsets[t + 1];
      e0 = e0 < 0 ? 0 : e0;
      e1 = e1 > tn_bias::kMaxAtoms ? tn_bias::kMaxAtoms : e1;
      tn_bias::atom_force(entries, e0, e1, sh_tot, sh_grad, f[t]);
      const int64_t i = start + atom_rel[t];
      if (!(isfinite(f[t][0]) && isfinite(f[t][1]) && isfinite(f[t][2])) || i < 0 || i >= N) bad = 1;
    }
    if (bad) {
      *status = tn_bias::kStatusBias;
      continue;
    }
    for (int t = 0; t < A; ++t) {
      const int64_t i = start + atom_rel[t];
      for (int d = 0; d < 3; ++d) {
        forces[i * 3 + d] = tn_md::md_add(forces[i * 3 + d], f[t][d]);
        if (force_row) force_row[((int64_t)b * A + t) * 3 + d] = f[t][d];
      }
    }
    for (int t = 0; t < D; ++t)
      if (cv_row) cv_row[(int64_t)b * D + t] = sh_s[t];
    double er = 0.0;
    for (int c = 0; c < D; ++c) er = er + sh_er[c];
    if (res_row) res_row[b] = er;
    if (bias_row) bias_row[b] = V;
    if (dm > 0 && deposit) {
      const int64_t slot = tn_bias::hill_slot(n, head[0], pace, W, w, head[1], H);
      if (slot >= 0) {
        c0[slot] = sh_s[mcv0];
        if (dm == 2) c0[H + slot] = sh_s[mcv1];
        c0[(int64_t)dm * H + slot] = tn_bias::hill_height(h0, V, kT, gamma);
      }
    }
  }
}

// The sampling protocol: B walkers (groups of W), each one atom of mass 1 (atom 1) bound to a fixed atom (atom 0, m = inf, hk = 0) by
// U(r) = 8 ((r - 2)^2 / 0.25 - 1)^2, under the loop's own Langevin step with metadynamics on the distance: the launch sequence of
// a captured replay written as loops - OPEN, then per step the force, the bias launch, CLOSE (the counter advances), OPEN.
// In place on x, v [2 B, 3]; hills [G, 2, H].
void bias_sample(int32_t B, int32_t W, int64_t steps, float* x, float* v, float dt, float c1, float c2, uint64_t seed, double sigma,
                 double h0, double kT, double gamma, uint64_t pace, int64_t H, double* hills, uint32_t* status) {
  const int N = 2 * B;
  const int32_t kind[1] = {tn_bias::kDistance}, atoms[4] = {1, 0, -1, -1}, rel[2] = {0, 1}, off[3] = {0, 1, 2};
  int32_t entries[tn_bias::kMaxAtoms] = {1, 0};  // atom 0 is slot 1 of cv 0, atom 1 its slot 0
  const int32_t res_kind[1] = {0};
  const uint64_t head[2] = {0, 0};
  int32_t* start = (int32_t*)malloc(sizeof(int32_t) * B);
  double* zero = (double*)calloc(B, sizeof(double));
  float* f = (float*)malloc(sizeof(float) * 3 * N);
  float* hk = (float*)malloc(sizeof(float) * N);
  float* mass = (float*)malloc(sizeof(float) * N);
  for (int b = 0; b < B; ++b) {
    start[b] = 2 * b;
    hk[2 * b] = 0.f;
    hk[2 * b + 1] = (float)(0.5 * (double)dt);
    mass[2 * b] = INFINITY;
    mass[2 * b + 1] = 1.f;
  }
  const float sig = 1.f;  // sqrt(kT / m) with kT = m = 1, force_scale 1
  auto model = [&]() {
    for (int b = 0; b < B; ++b) {
      double r[3], r2 = 0.0;
      for (int d = 0; d < 3; ++d) {
        r[d] = (double)x[(2 * b + 1) * 3 + d] - (double)x[(2 * b) * 3 + d];
        r2 += r[d] * r[d];
      }
      const double rr = sqrt(r2), u = rr - 2.0, dU = 8.0 * 2.0 * (u * u / 0.25 - 1.0) * (2.0 * u / 0.25);
      for (int d = 0; d < 3; ++d) {
        f[(2 * b + 1) * 3 + d] = (float)(-dU * r[d] / rr);
        f[(2 * b) * 3 + d] = (float)(dU * r[d] / rr);
      }
    }
  };
  auto bias = [&](uint64_t n, int deposit) {
    bias_launch(N, B, 1, 2, W, 1, 0, 0, deposit, x, f, kind, atoms, start, rel, off, entries, res_kind, zero, zero, sigma, 0.0, h0, kT,
                gamma, pace, H, head, n, hills, status, 0, nullptr, nullptr, nullptr, nullptr);
  };
  model();
  bias(0, 0);
  for (int i = 0; i < N; ++i) tn_md::open_step(x + 3 * i, v + 3 * i, f + 3 * i, hk[i], dt);
  for (uint64_t n = 0; n < (uint64_t)steps && !*status; ++n) {
    model();
    bias(n, 1);
    if (*status) break;
    for (int i = 0; i < N; ++i) {
      tn_md::close_step(v + 3 * i, f + 3 * i, hk[i], mass[i], 1, c1, c2, mass[i] == INFINITY ? 0.f : sig, seed, n, (uint32_t)i);
      tn_md::open_step(x + 3 * i, v + 3 * i, f + 3 * i, hk[i], dt);
    }
  }
  free(start);
  free(zero);
  free(f);
  free(hk);
  free(mass);
}

}  // extern "C"

#ifdef MD_BIAS_HOST_MAIN
// every entry once, on small inputs: a walker batch with all three CV kinds and a shared atom, restraints of every kind, a
// two-dimensional hill list that runs full, a non-finite walker, and a short sampling run
int main() {
  const int B = 6, n1 = 12, N = B * n1, D = 4, W = 3, dm = 2;
  const int64_t H = 8;
  float pos[N * 3], forces[N * 3];
  uint32_t r = 12345u;
  for (int i = 0; i < N * 3; ++i) {
    r = r * 1664525u + 1013904223u;
    pos[i] = (float)(i / 3 % n1) * 0.7f + (float)(r >> 8) * (1.f / 16777216.f);
    forces[i] = 0.25f;
  }
  const int32_t kind[D] = {0, 1, 2, 0}, atoms[D * 4] = {0, 1, -1, -1, 1, 2, 3, -1, 2, 3, 4, 5, 5, 7, -1, -1};
  const int32_t rel[7] = {0, 1, 2, 3, 4, 5, 7}, off[8] = {0, 1, 3, 5, 7, 8, 10, 11};
  int32_t entries[tn_bias::kMaxAtoms] = {0 << 2 | 0, 0 << 2 | 1, 1 << 2 | 0, 1 << 2 | 1, 2 << 2 | 0, 1 << 2 | 2, 2 << 2 | 1, 2 << 2 | 2,
                                         2 << 2 | 3, 3 << 2 | 0, 3 << 2 | 1};
  const int32_t res_kind[D] = {1, 2, 3, 0};
  int32_t start[B];
  double kappa[B * D], center[B * D], hills[2 * 3 * 8], cv[B * D], er[B], eb[B];
  float flog[B * 7 * 3];
  for (int b = 0; b < B; ++b) start[b] = b * n1;
  for (int i = 0; i < B * D; ++i) {
    kappa[i] = 3.0;
    center[i] = 0.5 + 0.1 * i;
  }
  const uint64_t head[2] = {5, 2};
  for (int i = 0; i < 2 * 3 * 8; ++i) hills[i] = 0.3;
  uint32_t status = 0;
  for (uint64_t n = 5; n < 12; ++n)
    bias_launch(N, B, D, 7, W, dm, 2, 0, 1, pos, forces, kind, atoms, start, rel, off, entries, res_kind, kappa, center, 0.3, 0.2, 0.1, 1.0,
                6.0, 2, H, head, n, hills, &status, 0, cv, er, eb, flog);
  if (status != 0) return 1;
  pos[3] = pos[0], pos[4] = pos[1], pos[5] = pos[2];  // coincident atoms: status 4
  bias_launch(N, B, D, 7, W, dm, 2, 0, 1, pos, forces, kind, atoms, start, rel, off, entries, res_kind, kappa, center, 0.3, 0.2, 0.1, 1.0,
              6.0, 2, H, head, 12, hills, &status, 0, cv, er, eb, flog);
  if (status != 4) return 2;
  float x[8 * 3] = {0, 0, 0, 1.5f, 0, 0, 0, 0, 0, 1.5f, 0, 0, 0, 0, 0, 1.5f, 0, 0, 0, 0, 0, 1.5f, 0, 0}, v[8 * 3] = {0};
  double* hl = (double*)calloc(2 * 64, sizeof(double));
  status = 0;
  bias_sample(4, 4, 1500, x, v, 0.005f, 0.97530991f, 0.22084063f, 7, 0.1, 0.3, 1.0, 8.0, 100, 64, hl, &status);
  const int bad = status != 0 || !(hl[64] > 0.0);
  free(hl);
  double s[1], g[12];
  const int32_t k1[1] = {2};
  bias_cv(1, k1, pos + 36, s, g);
  printf("md_bias_host: ok %d torsion %.6f visible %lld slot %lld height %.6f\n", !bad, s[0], (long long)bias_visible(12, 5, 2, 3, 2, H),
         (long long)bias_slot(6, 5, 2, 3, 1, 2, H), bias_height(0.3, 1.0, 1.0, 8.0));
  return bad ? 3 : 0;
}
#endif
