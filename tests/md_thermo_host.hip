// TEST INFRASTRUCTURE ONLY: the global-thermostat arithmetic of the device-resident MD loop (torchmd-net_amd/csrc/tn_md_thermo_math.h)
// compiled for the host (hipcc --cuda-host-only), one plain loop per kernel body, loaded through ctypes by
// tests/md_thermo_host_mirror.py.  The statements are the ones a GPU lane runs; tests/test_md_thermo_host.py compares them with
// tests/md_thermo_oracle.py without a GPU.  With -DMD_THERMO_HOST_MAIN the file is a program of its own (for the host sanitizers).
#include <stdint.h>
#include <stdio.h>

#include "../torchmd-net_amd/csrc/tn_md_thermo_math.h"

extern "C" {

void thermo_words(uint64_t seed, uint64_t step, uint32_t mol, uint32_t draw, uint32_t* out) { tn_md::thermo_words(seed, step, mol, draw, out); }

// k_md_thermo_factor: pass 1 on every molecule, pass 2 only when no move is unusable.  mols[n] are the molecules' indices (the
// counter's word 2); chain [n, 2, M] and reservoir [n] in place; alpha [n] and flag [n] (pass 1) out.  Returns the block's flag.
int32_t thermo_moves(int32_t kind, int64_t n, const uint32_t* mols, const float* ekin, const int32_t* ndof, double force_scale, double kT,
                     double tau, double dt, int32_t M, int32_t substeps, uint64_t seed, uint64_t step, double* chain, double* reservoir,
                     float* alpha, int32_t* flag) {
  const double c = exp(-dt / tau);
  int32_t bad = 0;
  float a;
  for (int64_t m = 0; m < n; ++m) {
    flag[m] = tn_md::thermo_move(kind, ekin[m], force_scale, ndof[m], kT, tau, dt, c, M, substeps, seed, step, mols[m], chain + 2 * M * m,
                                 reservoir + m, 0, &a);
    bad |= flag[m];
  }
  if (bad) return 1;
  for (int64_t m = 0; m < n; ++m)
    tn_md::thermo_move(kind, ekin[m], force_scale, ndof[m], kT, tau, dt, c, M, substeps, seed, step, mols[m], chain + 2 * M * m, reservoir + m,
                       1, alpha + m);
  return 0;
}

// k_md_thermo_scale<false>: v of every atom, in place
void thermo_scale(int64_t n_atoms, const int64_t* batch, const float* alpha, const float* hk, float* v) {
  for (int64_t i = 0; i < n_atoms; ++i) tn_md::thermo_scale(v + 3 * i, hk[i], alpha[batch[i]]);
}

// Independent harmonic atoms (f = -kappa x; kappa = 0: free flight) under a global thermostat, the launch sequence of a captured
// replay written as loops: OPEN, then per step the force, CLOSE (B, kinetic terms), their sum per molecule, the move, the scaling and
// the opening half of the next step.  R molecules of n atoms each (atom i belongs to molecule i / n), in place on x, v [R n, 3],
// chain [R, 2, M] and reservoir [R]; logs [steps, R]: epot (fp64, sum of kappa x^2 / 2), ekin (fp32, before the move), scale, the
// reservoir after the move.  kind < 0: no thermostat (scale = 1).  Returns the number of steps with an unusable move (0 expected).
int64_t thermo_run(int32_t kind, int64_t R, int64_t n, int64_t steps, uint64_t step0, float* x, float* v, const float* hk, const float* mass,
                   const int32_t* ndof, float dt, float kappa, double force_scale, double kT, double tau, int32_t M, int32_t substeps,
                   uint64_t seed, double* chain, double* reservoir, double* epot, float* ekin, float* scale, double* res_log) {
  const double c = exp(-(double)dt / tau);
  int64_t bad = 0;
  float f[3];
  for (int64_t i = 0; i < R * n; ++i) {
    for (int d = 0; d < 3; ++d) f[d] = tn_md::md_mul(-kappa, x[3 * i + d]);
    tn_md::open_step(x + 3 * i, v + 3 * i, f, hk[i], dt);
  }
  for (int64_t s = 0; s < steps; ++s) {
    for (int64_t m = 0; m < R; ++m) {
      float ke = 0.f;
      double ep = 0.0;
      for (int64_t i = m * n; i < (m + 1) * n; ++i) {
        for (int d = 0; d < 3; ++d) {
          f[d] = tn_md::md_mul(-kappa, x[3 * i + d]);
          ep += 0.5 * (double)kappa * (double)x[3 * i + d] * (double)x[3 * i + d];
        }
        ke += tn_md::close_step(v + 3 * i, f, hk[i], mass[i], 0, 1.f, 0.f, 0.f, 0, 0, 0);
      }
      float a = 1.f;
      if (kind >= 0 && tn_md::thermo_move(kind, ke, force_scale, ndof[m], kT, tau, (double)dt, c, M, substeps, seed, step0 + (uint64_t)s,
                                          (uint32_t)m, chain + 2 * M * m, reservoir + m, 1, &a)) {
        ++bad;
        a = 1.f;
      }
      epot[s * R + m] = ep;
      ekin[s * R + m] = ke;
      scale[s * R + m] = a;
      res_log[s * R + m] = reservoir[m];
      for (int64_t i = m * n; i < (m + 1) * n; ++i) {
        tn_md::thermo_scale(v + 3 * i, hk[i], a);
        if (s + 1 < steps) {
          for (int d = 0; d < 3; ++d) f[d] = tn_md::md_mul(-kappa, x[3 * i + d]);
          tn_md::open_step(x + 3 * i, v + 3 * i, f, hk[i], dt);
        }
      }
    }
  }
  return bad;
}

}  // extern "C"

#ifdef MD_THERMO_HOST_MAIN
// alpha for every kind and size of the host test's first case, the exact cases and the failure protocol
int main() {
  const int32_t sizes[6] = {1, 2, 3, 4, 9, 189};
  const uint32_t mols[4] = {0, 1, 2, 3};
  int wrong = 0, moves = 0;
  for (int k = 0; k < 6; ++k)
    for (uint64_t step = 0; step < 50; ++step) {
      const int32_t nd[4] = {sizes[k], sizes[k], sizes[k], sizes[k]};
      const double Kbar = 0.5 * sizes[k] * 0.025;
      const float ekin[4] = {(float)(0.01 * Kbar), (float)Kbar, (float)(3.0 * Kbar), (float)(100.0 * Kbar)};
      double chain[1] = {0.0}, res[4] = {0.0, 0.0, 0.0, 0.0};
      float alpha[4];
      int32_t flag[4];
      wrong += thermo_moves(tn_md::kThermoCsvr, 4, mols, ekin, nd, 1.0, 0.025, 5.0, 0.5, 0, 1, 77, step, chain, res, alpha, flag);
      for (int m = 0; m < 4; ++m) wrong += !(alpha[m] > 0.f) || !isfinite(res[m]);
      moves += 4;
    }
  const int32_t Ms[3] = {1, 3, 8}, subs[3] = {1, 2, 5};
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const int32_t M = Ms[a], nd[4] = {9, 9, 0, 189};
      double chain[4 * 2 * 8], res[4] = {0.0, 0.0, 7.0, 0.0};
      for (int j = 0; j < 4 * 2 * M; ++j) chain[j] = 0.01 * (j % 5);
      float ekin[4] = {0.2f, 0.05f, 1.f, 2.f}, alpha[4];
      int32_t flag[4];
      for (uint64_t step = 0; step < 200; ++step) {
        wrong += thermo_moves(tn_md::kThermoNhc, 4, mols, ekin, nd, 1.0, 0.025, 5.0, 0.5, M, subs[b], 0, step, chain, res, alpha, flag);
        for (int m = 0; m < 4; ++m) ekin[m] = ekin[m] * alpha[m] * alpha[m];
        moves += 4;
      }
      wrong += alpha[2] != 1.f || res[2] != 7.0;  // no degrees of freedom: untouched
    }
  // exact: 2 K = N kT with the chain at rest, and K = 0
  {
    const int32_t nd[2] = {8, 8};
    const float ekin[2] = {0.5f, 0.f};
    double chain[2 * 2 * 3] = {0}, res[2] = {0.0, 0.0};
    float alpha[2];
    int32_t flag[2];
    wrong += thermo_moves(tn_md::kThermoNhc, 2, mols, ekin, nd, 1.0, 0.125, 4.0, 1.0, 3, 2, 0, 0, chain, res, alpha, flag);
    wrong += alpha[0] != 1.f || alpha[1] != 1.f || chain[6] != 0.0;
    float v[6] = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f};
    const int64_t batch[2] = {0, 1};
    const float hk[2] = {0.5f, 0.f}, al[2] = {1.5f, 1.5f};
    thermo_scale(2, batch, al, hk, v);
    wrong += v[0] != 1.5f || v[3] != 4.f;
  }
  // failure: a NaN kinetic energy in molecule 1 of 4 - flag 1 and nothing written
  int forced;
  {
    const int32_t nd[4] = {9, 9, 9, 9};
    const float ekin[4] = {0.1f, NAN, 0.1f, 0.1f};
    double chain[4 * 2 * 3], res[4] = {1.0, 2.0, 3.0, 4.0};
    for (int j = 0; j < 24; ++j) chain[j] = 0.25;
    float alpha[4] = {-7.f, -7.f, -7.f, -7.f};
    int32_t flag[4];
    forced = thermo_moves(tn_md::kThermoNhc, 4, mols, ekin, nd, 1.0, 0.025, 5.0, 0.5, 3, 2, 0, 3, chain, res, alpha, flag);
    forced &= thermo_moves(tn_md::kThermoCsvr, 4, mols, ekin, nd, 1.0, 0.025, 5.0, 0.5, 0, 1, 0, 3, chain, res, alpha, flag);
    for (int j = 0; j < 24; ++j) wrong += chain[j] != 0.25;
    for (int m = 0; m < 4; ++m) wrong += alpha[m] != -7.f || res[m] != 1.0 + m;
  }
  printf("md_thermo_host: %d moves, wrong %d, forced fail %d\n", moves, wrong, forced);
  return wrong == 0 && forced == 1 ? 0 : 1;
}
#endif
