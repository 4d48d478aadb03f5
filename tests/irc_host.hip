// TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident IRC follower (torchmd-net_amd/csrc/tn_irc_math.h) compiled for
// the host (hipcc --cuda-host-only), one plain loop per kernel body, loaded through ctypes by tests/irc_host_mirror.py.  The
// statements are the ones a GPU lane runs, and the sums are added in the order the device adds them (threads striding a slice, the
// xor tree of a wave, the waves in turn, the slices in slice order); tests/test_irc_host.py compares them with tests/irc_oracle.py
// without a GPU.  With -DIRC_HOST_MAIN the file is a stand-alone program for the sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../torchmd-net_amd/csrc/tn_irc_math.h"

using namespace tn_irc;

namespace {

constexpr int kThreads = 256;

int mol_slices(int64_t n) {  // tn_loop.h's rule for one molecule
  if (n <= 1024) return 1;
  const int64_t s = (n + 1023) / 1024;
  return (int)(s > 256 ? 256 : s);
}

double combine(double a, double b, int is_max) { return is_max ? (b > a ? b : a) : a + b; }

// 256 per-thread values in the order of tn_loop.h's block reduction: the xor tree of each wave, then the waves left to right
double block_reduce(double* lane, int is_max) {
  double wave[kThreads / 64];
  for (int w = 0; w < kThreads / 64; ++w) {
    double* l = lane + 64 * w;
    for (int o = 1; o < 64; o <<= 1)
      for (int i = 0; i < 64; i += 2 * o) l[i] = combine(l[i], l[i + o], is_max);
    wave[w] = l[0];
  }
  double r = wave[0];
  for (int w = 1; w < kThreads / 64; ++w) r = combine(r, wave[w], is_max);
  return r;
}

IrcParams params(double fmax, double v0, double error, double dt_min, double dt_max, int32_t every, int32_t capacity) {
  IrcParams p;
  p.fmax = fmax;
  p.v0 = v0;
  p.error = error;
  p.dt_min = dt_min;
  p.dt_max = dt_max;
  p.every = every;
  p.capacity = capacity;
  return p;
}

}  // namespace

extern "C" {

// the start images: x_ts, u [G n, 3] -> pos, vel [G D n, 3], path p = g D + d with sigma = +1 (d = 0, or D = 1 and backward = 0) / -1
void irc_start(int64_t G, int64_t D, int64_t n, int32_t backward, const float* x_ts, const float* u, double initial_step, double v0,
               float* pos, float* vel) {
  for (int64_t g = 0; g < G; ++g)
    for (int64_t d = 0; d < D; ++d) {
      const float sigma = (D == 2 ? d == 1 : backward != 0) ? -1.f : 1.f;
      for (int64_t a = 0; a < n; ++a)
        start_image(x_ts + 3 * (g * n + a), u + 3 * (g * n + a), sigma, (float)initial_step, (float)v0, pos + 3 * ((g * D + d) * n + a),
                    vel + 3 * ((g * D + d) * n + a));
    }
}

// the per-atom terms of k_irc_sums for every atom (still atoms: zeros): vp [P n, 3], t [P n, 5]
void irc_terms(int64_t P, int64_t n, const float* pos, const float* vel, const float* f, const float* ca, const float* mass,
               const uint8_t* fixed, const float* dt, const float* dt_prev, const int32_t* has2, const float* x1, const float* x2,
               const float* v2, const float* f2, float* vp, float* t) {
  for (int64_t p = 0; p < P; ++p)
    for (int64_t a = 0; a < n; ++a) {
      const int64_t i = p * n + a;
      if (still_atom(fixed && fixed[a], ca[a])) {
        for (int k = 0; k < 3; ++k) vp[3 * i + k] = 0.f;
        for (int k = 0; k < 5; ++k) t[5 * i + k] = 0.f;
        continue;
      }
      const float T = has2[p] ? md_add(dt_prev[p], dt[p]) : 0.f;
      sum_terms(pos + 3 * i, vel + 3 * i, f + 3 * i, md_mul(dt[p], ca[a]), ca[a], mass[a], x1 + 3 * i, has2[p], x2 + 3 * i, v2 + 3 * i,
                f2 + 3 * i, T, vp + 3 * i, t + 5 * i);
    }
}

// x' of every atom: xp [P n, 3]
void irc_extrapolate(int64_t P, int64_t n, const float* x2, const float* v2, const float* f2, const float* ca, const float* T, float* xp) {
  for (int64_t p = 0; p < P; ++p)
    for (int64_t a = 0; a < n; ++a) extrapolate(x2 + 3 * (p * n + a), v2 + 3 * (p * n + a), f2 + 3 * (p * n + a), T[p], ca[a], xp + 3 * (p * n + a));
}

// v <- c v' of every atom
void irc_damp(int64_t P, int64_t n, const float* vp, const float* c, float* v) {
  for (int64_t p = 0; p < P; ++p)
    for (int64_t a = 0; a < n; ++a) damp(vp + 3 * (p * n + a), c[p], v + 3 * (p * n + a));
}

// k_irc_sums and the slice loop of the controller, in the device's order: sums [P, N_SUMS]
void irc_sums(int64_t P, int64_t n, int32_t start, const float* pos, const float* vel, const float* f, const float* ca, const float* mass,
              const uint8_t* fixed, const double* dt, const float* dt_used, const int32_t* n_acc, const float* x1, const float* x2,
              const float* v2, const float* f2, double* sums) {
  const int S = mol_slices(n);
  for (int64_t p = 0; p < P; ++p) {
    double* out = sums + N_SUMS * p;
    for (int k = 0; k < N_SUMS; ++k) out[k] = 0.0;
    const float dtf = start ? 0.f : (float)dt[p];
    const int has2 = !start && n_acc[p] >= 1;
    const float T = has2 ? md_add(dt_used[p], dtf) : 0.f;
    for (int s = 0; s < S; ++s) {
      const int64_t a0 = n * s / S, a1 = n * (s + 1) / S;
      double lane[N_SUMS][kThreads];
      for (int k = 0; k < N_SUMS; ++k)
        for (int t = 0; t < kThreads; ++t) lane[k][t] = 0.0;
      for (int64_t a = a0; a < a1; ++a) {
        if (still_atom(fixed && fixed[a], ca[a])) continue;
        const int t = (int)((a - a0) % kThreads);
        const int64_t i = p * n + a;
        float vp[3], term[5];
        sum_terms(pos + 3 * i, vel + 3 * i, f + 3 * i, md_mul(dtf, ca[a]), ca[a], mass[a], start ? pos + 3 * i : x1 + 3 * i, has2, x2 + 3 * i,
                  v2 + 3 * i, f2 + 3 * i, T, vp, term);
        for (int k = 0; k < 5; ++k) lane[k][t] = combine(lane[k][t], (double)term[k], k == S_FMAX2);
        lane[S_FREE][t] += 1.0;
      }
      for (int k = 0; k < N_SUMS; ++k) out[k] = combine(out[k], block_reduce(lane[k], k == S_FMAX2), k == S_FMAX2);
    }
  }
}

// irc_control of every path on given sums: the state in place, out [P, 2], slot [P], cause [P], ret [P]
void irc_control_table(int64_t P, const double* sums, const float* e, int32_t start, int64_t step, double fmax, double v0, double error,
                       double dt_min, double dt_max, int32_t every, int32_t capacity, double* dt, double* arc, int64_t* conv,
                       int32_t* reason, int32_t* n_acc, int32_t* n_rec, float* out, int32_t* slot, int32_t* cause, int32_t* ret) {
  const IrcParams prm = params(fmax, v0, error, dt_min, dt_max, every, capacity);
  for (int64_t p = 0; p < P; ++p) {
    IrcPath s = {dt[p], arc[p], conv[p], reason[p], n_acc[p], n_rec[p]};
    int sl, c;
    ret[p] = irc_control(&s, prm, sums + N_SUMS * p, e[p], start, step, out + 2 * p, &sl, &c);
    slot[p] = sl;
    cause[p] = c;
    dt[p] = s.dt;
    arc[p] = s.arc;
    conv[p] = s.converged_at;
    reason[p] = s.reason;
    n_acc[p] = s.n_acc;
    n_rec[p] = s.n_rec;
  }
}

// MIDDLE / CLOSE up to the move: k_irc_sums, k_irc_control (both passes) and the accept of k_irc_atoms.  Returns 0, or the cause of
// status 2 - then nothing is written but x and v of generation 1 put back on the paths that move (not at the start).
int32_t irc_close(int64_t P, int64_t n, int32_t start, int64_t step, const float* e, const float* f, const float* ca, const float* mass,
                  const uint8_t* fixed, double fmax, double v0, double error, double dt_min, double dt_max, int32_t every, int32_t capacity,
                  float* pos, float* vel, float* fkeep, const float* x1, const float* v1, const float* x2, const float* v2, const float* f2,
                  double* dt, double* arc, int64_t* conv, int32_t* reason, int32_t* n_acc, int32_t* n_rec, float* dt_used, float* dampc,
                  double* rec, double* frame_s, float* frame_e, float* frames) {
  const IrcParams prm = params(fmax, v0, error, dt_min, dt_max, every, capacity);
  double* sums = (double*)malloc(N_SUMS * P * sizeof(double));
  irc_sums(P, n, start, pos, vel, f, ca, mass, fixed, dt, dt_used, n_acc, x1, x2, v2, f2, sums);
  int32_t bad = 0;
  for (int64_t p = 0; p < P; ++p) {  // pass 1 on a copy of the state
    IrcPath s = {dt[p], arc[p], start ? -1 : conv[p], reason[p], start ? 0 : n_acc[p], start ? 0 : n_rec[p]};
    if (start) s.arc = 0.0;
    float out[2];
    int sl, c;
    if (irc_control(&s, prm, sums + N_SUMS * p, e[p], start, step, out, &sl, &c) == IRC_UNUSABLE) bad = c > bad ? c : bad;
  }
  if (bad) {
    if (!start)
      for (int64_t p = 0; p < P; ++p)
        if (conv[p] < 0) {
          memcpy(pos + 3 * p * n, x1 + 3 * p * n, 3 * n * sizeof(float));
          memcpy(vel + 3 * p * n, v1 + 3 * p * n, 3 * n * sizeof(float));
        }
    free(sums);
    return bad;
  }
  for (int64_t p = 0; p < P; ++p) {
    IrcPath s = {dt[p], arc[p], start ? -1 : conv[p], reason[p], start ? 0 : n_acc[p], start ? 0 : n_rec[p]};
    if (start) {
      s.arc = 0.0;
      s.reason = REASON_NONE;
    }
    float out[2];
    int sl, c;
    const int r = irc_control(&s, prm, sums + N_SUMS * p, e[p], start, step, out, &sl, &c);
    dt[p] = s.dt;
    arc[p] = s.arc;
    conv[p] = s.converged_at;
    reason[p] = s.reason;
    n_acc[p] = s.n_acc;
    n_rec[p] = s.n_rec;
    if (r == IRC_FROZEN) continue;
    dampc[p] = out[0];
    dt_used[p] = out[1];
    memcpy(rec + N_SUMS * p, sums + N_SUMS * p, N_SUMS * sizeof(double));
    if (sl >= 0) {
      frame_s[p * capacity + sl] = s.arc;
      frame_e[p * capacity + sl] = e[p];
    }
    for (int64_t a = 0; a < n; ++a) {
      const int64_t i = p * n + a;
      if (still_atom(fixed && fixed[a], ca[a])) {
        vel[3 * i] = vel[3 * i + 1] = vel[3 * i + 2] = 0.f;
      } else {
        float vp[3];
        close_kick(vel + 3 * i, f + 3 * i, md_mul(out[1], ca[a]), vp);
        damp(vp, out[0], vel + 3 * i);
      }
      for (int k = 0; k < 3; ++k) {
        fkeep[3 * i + k] = f[3 * i + k];
        if (sl >= 0) frames[((p * capacity + sl) * n + a) * 3 + k] = pos[3 * i + k];
      }
    }
  }
  free(sums);
  return 0;
}

// the move of k_irc_atoms for the paths that still move: the generations shifted, then tn_md::open_step with the path's time step
void irc_open(int64_t P, int64_t n, const float* ca, const uint8_t* fixed, const double* dt, const int64_t* conv, float* pos, float* vel,
              const float* fkeep, float* x1, float* v1, float* f1, float* x2, float* v2, float* f2) {
  for (int64_t p = 0; p < P; ++p) {
    if (conv[p] >= 0) continue;
    const float dtf = (float)dt[p];
    for (int64_t a = 0; a < n; ++a) {
      const int64_t i = p * n + a;
      for (int k = 0; k < 3; ++k) {
        x2[3 * i + k] = x1[3 * i + k];
        v2[3 * i + k] = v1[3 * i + k];
        f2[3 * i + k] = f1[3 * i + k];
        x1[3 * i + k] = pos[3 * i + k];
        v1[3 * i + k] = vel[3 * i + k];
        f1[3 * i + k] = fkeep[3 * i + k];
      }
      if (still_atom(fixed && fixed[a], ca[a])) continue;
      tn_md::open_step(pos + 3 * i, vel + 3 * i, fkeep + 3 * i, md_mul(dtf, ca[a]), dtf);
    }
  }
}

// The surface of tests/irc_oracle.py, evaluated in fp64 at the fp32 positions and rounded once.  X = x of atom 0, Y = y of atom 1:
// E = (X^2 - 1)^2 + kappa (Y - A (1 - X^2))^2 + kappa / 2 (every other coordinate - its site)^2.  e [P], f [P n, 3]; n >= 2.
void irc_surface(int64_t P, int64_t n, const float* x, const double* sites, double kappa, double A, float* e, float* f) {
  for (int64_t p = 0; p < P; ++p) {
    const float* r = x + 3 * p * n;
    float* fr = f + 3 * p * n;
    const double X = r[0], Y = r[4];
    const double u = X * X - 1.0, w = Y + A * u;
    double E = u * u + kappa * w * w;
    for (int64_t j = 0; j < 3 * n; ++j) {
      if (j == 0 || j == 4) continue;
      const double dr = (double)r[j] - sites[j];
      E += 0.5 * kappa * dr * dr;
      fr[j] = (float)-(kappa * dr);
    }
    fr[0] = (float)-(4.0 * X * u + 2.0 * kappa * w * (2.0 * A * X));
    fr[4] = (float)-(2.0 * kappa * w);
    e[p] = (float)E;
  }
}

// Whole paths on the surface, the launch sequence written as loops: the control of the start images, then per step the move, the
// evaluation and the close, until every path has finished or max_steps is reached.  pos, vel [P n, 3] hold the start images and end
// as the paths' last points; log [max_steps + 1, P, 4] receives dt, c, arc, power of every step when it is not NULL.  Returns the
// steps taken, or -cause.
int64_t irc_run(int64_t P, int64_t n, const double* sites, double kappa, double A, const float* ca, const float* mass, const uint8_t* fixed,
                double dt0, double fmax, double v0, double error, double dt_min, double dt_max, int32_t every, int32_t capacity,
                int64_t max_steps, float* pos, float* vel, float* fkeep, int64_t* conv, int32_t* reason, double* arc, double* dt,
                int32_t* n_rec, double* frame_s, float* frame_e, float* frames, double* log) {
  const int64_t N = P * n;
  float* gen = (float*)calloc(18 * N + 1, sizeof(float));
  float *x1 = gen, *v1 = gen + 3 * N, *f1 = gen + 6 * N, *x2 = gen + 9 * N, *v2 = gen + 12 * N, *f2 = gen + 15 * N;
  float* f = (float*)malloc((3 * N + 1) * sizeof(float));
  float* e = (float*)malloc(P * sizeof(float));
  int32_t* n_acc = (int32_t*)calloc(P, sizeof(int32_t));
  float* dt_used = (float*)calloc(P, sizeof(float));
  float* dampc = (float*)calloc(P, sizeof(float));
  double* rec = (double*)calloc(N_SUMS * P, sizeof(double));
  for (int64_t p = 0; p < P; ++p) {
    dt[p] = dt0;
    arc[p] = 0.0;
    conv[p] = -1;
    reason[p] = 0;
    n_rec[p] = 0;
  }
  int64_t result = 0;
  for (int64_t step = 0;; ++step) {
    if (step > 0) irc_open(P, n, ca, fixed, dt, conv, pos, vel, fkeep, x1, v1, f1, x2, v2, f2);
    irc_surface(P, n, pos, sites, kappa, A, e, f);
    const int32_t bad = irc_close(P, n, step == 0, step, e, f, ca, mass, fixed, fmax, v0, error, dt_min, dt_max, every, capacity, pos, vel,
                                  fkeep, x1, v1, x2, v2, f2, dt, arc, conv, reason, n_acc, n_rec, dt_used, dampc, rec, frame_s, frame_e, frames);
    if (bad) {
      result = -bad;
      break;
    }
    int64_t open = 0;
    for (int64_t p = 0; p < P; ++p) {
      open += conv[p] < 0;
      if (log) {
        double* row = log + (step * P + p) * 4;
        row[0] = dt[p];
        row[1] = dampc[p];
        row[2] = arc[p];
        row[3] = rec[N_SUMS * p + S_P];
      }
    }
    if (open == 0 || step == max_steps) {
      result = step;
      break;
    }
  }
  free(gen); free(f); free(e); free(n_acc); free(dt_used); free(dampc); free(rec);
  return result;
}

}  // extern "C"

#ifdef IRC_HOST_MAIN
// every entry of the mirror on heap arrays of exact size: both directions from the saddle of the surface with three atoms of unequal
// mass, a fixed atom, a record that fills up, a NaN start and a path without a free atom
static int64_t one(int64_t n, const double* sites, const float* mass_in, const uint8_t* fixed, int poison, int32_t capacity, int64_t* conv,
                   int32_t* reason, int32_t* n_rec) {
  const int64_t P = 2;
  float* x_ts = (float*)malloc(3 * n * sizeof(float));
  float* u = (float*)calloc(3 * n, sizeof(float));
  float* ca = (float*)malloc(n * sizeof(float));
  float* pos = (float*)malloc(3 * P * n * sizeof(float));
  float* vel = (float*)malloc(3 * P * n * sizeof(float));
  float* fkeep = (float*)calloc(3 * P * n, sizeof(float));
  double* arc = (double*)malloc(P * sizeof(double));
  double* dt = (double*)malloc(P * sizeof(double));
  double* frame_s = (double*)calloc(P * capacity, sizeof(double));
  float* frame_e = (float*)calloc(P * capacity, sizeof(float));
  float* frames = (float*)calloc(P * capacity * n * 3, sizeof(float));
  double* log = (double*)calloc(401 * P * 4, sizeof(double));
  for (int64_t j = 0; j < 3 * n; ++j) x_ts[j] = (float)sites[j];
  x_ts[0] = 0.f;
  x_ts[4] = 0.5f;
  if (!(fixed && fixed[0])) u[0] = 1.f;
  for (int64_t a = 0; a < n; ++a) ca[a] = (float)(1.0 / (2.0 * (double)mass_in[a]));
  irc_start(1, 2, n, 0, x_ts, u, 0.02, 0.04, pos, vel);
  if (poison) pos[1] = NAN;
  const int64_t r = irc_run(P, n, sites, 2.0, 0.5, ca, mass_in, fixed, 0.05, 1e-3, 0.04, 0.003, 0.05 / 16, 0.05 * 16, 1, capacity, 400, pos, vel,
                            fkeep, conv, reason, arc, dt, n_rec, frame_s, frame_e, frames, log);
  printf("n %lld: steps %lld converged_at %lld %lld reason %d %d arc %.5f %.5f x %.5f %.5f y %.5f frames %d\n", (long long)n, (long long)r,
         (long long)conv[0], (long long)conv[1], reason[0], reason[1], arc[0], arc[1], pos[0], pos[3 * n], pos[4], n_rec[0]);
  free(x_ts); free(u); free(ca); free(pos); free(vel); free(fkeep); free(arc); free(dt); free(frame_s); free(frame_e); free(frames); free(log);
  return r;
}

int main() {
  const int64_t n = 3;
  double* sites = (double*)malloc(3 * n * sizeof(double));
  float* mass = (float*)malloc(n * sizeof(float));
  uint8_t* fixed = (uint8_t*)calloc(n, 1);
  int64_t conv[2];
  int32_t reason[2], n_rec[2];
  for (int64_t j = 0; j < 3 * n; ++j) sites[j] = 0.5 * (double)(j % 4) - 0.7;
  mass[0] = 1.f;
  mass[1] = 16.f;
  mass[2] = 3.f;
  int bad = 0;
  int64_t r = one(n, sites, mass, fixed, 0, 512, conv, reason, n_rec);
  bad |= r <= 0 || conv[0] < 0 || conv[1] < 0 || conv[0] != conv[1] || n_rec[0] != (int32_t)conv[0] + 1;
  r = one(n, sites, mass, fixed, 0, 4, conv, reason, n_rec);
  bad |= r <= 0 || n_rec[0] != (int32_t)conv[0] + 1;
  fixed[2] = 1;
  r = one(n, sites, mass, fixed, 0, 512, conv, reason, n_rec);
  bad |= r <= 0 || conv[0] < 0;
  r = one(n, sites, mass, fixed, 1, 512, conv, reason, n_rec);
  bad |= r != -IRC_BAD_ENERGY;
  fixed[0] = fixed[1] = 1;
  r = one(n, sites, mass, fixed, 0, 512, conv, reason, n_rec);
  bad |= r != 0 || conv[0] != 0 || reason[0] != REASON_FMAX;
  free(sites);
  free(mass);
  free(fixed);
  return bad;
}
#endif
