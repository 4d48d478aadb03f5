// TEST INFRASTRUCTURE ONLY: the barostat arithmetic of the device-resident MD loop (torchmd-net_amd/csrc/tn_md_math.h) compiled for the
// host (hipcc --cuda-host-only), one plain loop per kernel body, loaded through ctypes by tests/md_baro_host_mirror.py.  The
// statements are the ones a GPU lane runs; tests/test_md_barostat_host.py compares them with tests/md_baro_oracle.py without a GPU.
#include <stdint.h>

#include "../torchmd-net_amd/csrc/tn_md_math.h"

extern "C" {

// the barostat noise of mols[0..n) at `step`
void baro_noise(int64_t n, uint64_t seed, uint64_t step, const uint32_t* mols, double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = tn_md::baro_noise(seed, step, mols[i]);
}

// one move per molecule (pass 1 of k_md_baro): box[n,9], W[n,9], ekin[n] -> V, P (fp64), mu32, nu32, flag
void baro_move(int64_t n, const float* box, const float* W, const float* ekin, double force_scale, double P0, double kT, double a,
               uint64_t seed, uint64_t step, double* V, double* P, float* mu, float* nu, int32_t* flag) {
  for (int64_t m = 0; m < n; ++m)
    flag[m] = tn_md::baro_move(box + 9 * m, W + 9 * m, ekin[m], force_scale, P0, kT, a, seed, step, (uint32_t)m, V + m, P + m, mu + m, nu + m);
}

// pass 2 of k_md_baro and k_md_scale<false>: the boxes, then x and v of every atom, in place
void baro_scale(int64_t n_mol, int64_t n_atoms, const int64_t* batch, const float* mu, const float* nu, float* box, float* x, float* v) {
  for (int64_t m = 0; m < n_mol; ++m)
    for (int r = 0; r < 3; ++r) tn_md::scale3(box + 9 * m + 3 * r, mu[m]);
  for (int64_t i = 0; i < n_atoms; ++i) {
    tn_md::scale3(x + 3 * i, mu[batch[i]]);
    tn_md::scale3(v + 3 * i, nu[batch[i]]);
  }
}

// The ideal gas (F = 0, W = 0) under Langevin + barostat, the launch sequence of a captured NPT replay written as loops: OPEN, then
// per step CLOSE (B, O, kinetic terms), their sum per replica, the move, the scaling and the opening half of the next step.
// R replicas of n atoms each (atom i belongs to replica i / n), in place on box[R,9], x, v[R n,3]; volumes[steps,R] = V before each move.
// Returns the number of unusable moves (0 expected).
int64_t baro_ideal_gas(int64_t R, int64_t n, int64_t steps, float* box, float* x, float* v, const float* hk, const float* mass,
                       const float* sigma, float dt, float c1, float c2, uint64_t seed, double force_scale, double P0, double kT,
                       double compressibility, double tau, uint64_t baro_seed, float* volumes) {
  const float zero[3] = {0.f, 0.f, 0.f}, W[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const double a = compressibility * (double)dt / tau;
  int64_t bad = 0;
  for (int64_t i = 0; i < R * n; ++i) tn_md::open_step(x + 3 * i, v + 3 * i, zero, hk[i], dt);
  for (int64_t s = 0; s < steps; ++s) {
    for (int64_t m = 0; m < R; ++m) {
      float ekin = 0.f;
      for (int64_t i = m * n; i < (m + 1) * n; ++i)
        ekin += tn_md::close_step(v + 3 * i, zero, hk[i], mass[i], 1, c1, c2, sigma[i], seed, (uint64_t)s, (uint32_t)i);
      double V, P;
      float mu, nu;
      if (tn_md::baro_move(box + 9 * m, W, ekin, force_scale, P0, kT, a, baro_seed, (uint64_t)s, (uint32_t)m, &V, &P, &mu, &nu)) {
        ++bad;
        continue;
      }
      volumes[s * R + m] = (float)V;
      for (int r = 0; r < 3; ++r) tn_md::scale3(box + 9 * m + 3 * r, mu);
      for (int64_t i = m * n; i < (m + 1) * n; ++i) {
        tn_md::scale3(x + 3 * i, mu);
        tn_md::scale3(v + 3 * i, nu);
        tn_md::open_step(x + 3 * i, v + 3 * i, zero, hk[i], dt);
      }
    }
  }
  return bad;
}

}  // extern "C"
