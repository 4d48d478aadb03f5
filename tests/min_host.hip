// TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident FIRE minimiser (torchmd-net_amd/csrc/tn_min_math.h) compiled for the
// host (hipcc --cuda-host-only), one plain loop per kernel body, loaded through ctypes by tests/min_host_mirror.py.  The
// statements are the ones a GPU lane runs; tests/test_min_host.py compares them with tests/min_oracle.py without a GPU.
#include <stdint.h>

#include "../torchmd-net_amd/csrc/tn_min_math.h"

namespace {

tn_min::FireParams params(double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha0, double f_alpha, double max_step, double fmax) {
  tn_min::FireParams p;
  p.dt_max = dt_max;
  p.n_min = n_min;
  p.f_inc = f_inc;
  p.f_dec = f_dec;
  p.alpha0 = alpha0;
  p.f_alpha = f_alpha;
  p.max_step = max_step;
  p.fmax = fmax;
  return p;
}

// k_min_reduce + the slice loop of k_min_control for one molecule set, the atoms in index order: sums[n_mol, 4]
void reduce(int64_t n_mol, int64_t n_atoms, const int64_t* batch, const float* v, const float* f, const uint8_t* fixed, double* sums) {
  for (int64_t m = 0; m < 4 * n_mol; ++m) sums[m] = 0.0;
  for (int64_t i = 0; i < n_atoms; ++i) {
    float t[3];
    tn_min::atom_terms(v + 3 * i, f + 3 * i, fixed && fixed[i], t);
    double* s = sums + 4 * batch[i];
    s[0] += (double)t[0];
    s[1] += (double)t[1];
    s[2] += (double)t[2];
    s[3] = (double)t[1] > s[3] ? (double)t[1] : s[3];
  }
}

}  // namespace

extern "C" {

// the three fp32 terms of every atom: t[n, 3] = v.f, f.f, v.v
void min_terms(int64_t n, const float* v, const float* f, const uint8_t* fixed, float* t) {
  for (int64_t i = 0; i < n; ++i) tn_min::atom_terms(v + 3 * i, f + 3 * i, fixed && fixed[i], t + 3 * i);
}

// one controller move per molecule, the state in place: -> coef[n, 3], ret[n] (0 moving, 1 frozen, 2 unusable)
void min_control(int64_t n, double* dt, double* alpha, int32_t* n_pos, int64_t* conv, const double* sums, double dt_max, int32_t n_min,
                 double f_inc, double f_dec, double alpha0, double f_alpha, double max_step, double fmax, int64_t step, float* coef,
                 int32_t* ret) {
  const tn_min::FireParams p = params(dt_max, n_min, f_inc, f_dec, alpha0, f_alpha, max_step, fmax);
  for (int64_t m = 0; m < n; ++m) {
    tn_min::FireState s = {dt[m], alpha[m], n_pos[m], conv[m]};
    ret[m] = tn_min::fire_control(&s, p, sums[4 * m], sums[4 * m + 1], sums[4 * m + 2], sums[4 * m + 3], step, coef + 3 * m);
    dt[m] = s.dt;
    alpha[m] = s.alpha;
    n_pos[m] = s.n_pos;
    conv[m] = s.converged_at;
  }
}

// the per-atom update (k_min_atoms, MOVE) in place
void min_update(int64_t n_atoms, const int64_t* batch, const int64_t* conv, const uint8_t* fixed, const float* coef, float* x, float* v,
                const float* f) {
  for (int64_t i = 0; i < n_atoms; ++i) {
    const int64_t m = batch[i];
    if (conv[m] >= 0 || (fixed && fixed[i])) {
      v[3 * i] = v[3 * i + 1] = v[3 * i + 2] = 0.f;
      continue;
    }
    tn_min::atom_move(x + 3 * i, v + 3 * i, f + 3 * i, coef[3 * m], coef[3 * m + 1], coef[3 * m + 2]);
  }
}

// Harmonic wells F = -k (x - x0), the launch sequence of the minimiser written as loops: the control of the start geometry, then per
// step update, forces, reduce, control, until every molecule has converged or max_steps is reached.  In place on x; conv[n_mol] =
// converged_at.  Returns the number of steps taken, or -1 when a sum was not finite.
int64_t min_wells(int64_t n_mol, int64_t n_atoms, const int64_t* batch, const float* kspring, const float* x0, float* x, float* v, float* f,
                  const uint8_t* fixed, double dt0, double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha0,
                  double f_alpha, double max_step, double fmax, int64_t max_steps, double* dt, double* alpha, int32_t* n_pos,
                  int64_t* conv, double* sums, float* coef) {
  const tn_min::FireParams p = params(dt_max, n_min, f_inc, f_dec, alpha0, f_alpha, max_step, fmax);
  for (int64_t m = 0; m < n_mol; ++m) {
    dt[m] = dt0;
    alpha[m] = alpha0;
    n_pos[m] = 0;
    conv[m] = -1;
  }
  for (int64_t i = 0; i < 3 * n_atoms; ++i) v[i] = 0.f;
  for (int64_t step = 0;; ++step) {
    if (step > 0) min_update(n_atoms, batch, conv, fixed, coef, x, v, f);
    for (int64_t i = 0; i < n_atoms; ++i)
      for (int d = 0; d < 3; ++d) f[3 * i + d] = -(kspring[i] * (x[3 * i + d] - x0[3 * i + d]));
    reduce(n_mol, n_atoms, batch, v, f, fixed, sums);
    int64_t open = 0;
    for (int64_t m = 0; m < n_mol; ++m) {
      tn_min::FireState s = {dt[m], alpha[m], n_pos[m], conv[m]};
      if (tn_min::fire_control(&s, p, sums[4 * m], sums[4 * m + 1], sums[4 * m + 2], sums[4 * m + 3], step, coef + 3 * m) == tn_min::FIRE_UNUSABLE)
        return -1;
      dt[m] = s.dt;
      alpha[m] = s.alpha;
      n_pos[m] = s.n_pos;
      conv[m] = s.converged_at;
      open += s.converged_at < 0;
    }
    if (open == 0 || step == max_steps) return step;
  }
}

}  // extern "C"
