// TEST INFRASTRUCTURE ONLY: the replica-exchange arithmetic of the device-resident MD loop (torchmd-net_amd/csrc/tn_remd_math.h)
// compiled for the host (hipcc --cuda-host-only), one plain loop per kernel body, loaded through ctypes by tests/remd_host_mirror.py.
// The statements are the ones a GPU lane runs; tests/test_remd_host.py compares them with tests/remd_oracle.py without a GPU.
#include <stdint.h>

#include "../torchmd-net_amd/csrc/tn_remd_math.h"

extern "C" {

// u of the pairs index[0..n) after `step` completed steps
void remd_uniform(int64_t n, uint64_t seed, uint64_t step, const uint32_t* index, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = tn_md::exchange_uniform(seed, step, index[i]);
}

// n independent decisions
void remd_decide(int64_t n, const double* beta_lo, const double* beta_hi, const float* E_i, const float* E_j, const float* u, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = tn_md::exchange_decide(beta_lo[i], beta_hi[i], E_i[i], E_j[i], u[i]);
}

// the pairs of attempt a: lower slots into out[], returns their number
int32_t remd_pairs(uint64_t a, int32_t R, int32_t* out) {
  const int n = tn_md::exchange_pair_count(a, R);
  for (int p = 0; p < n; ++p) out[p] = tn_md::exchange_pair_slot(a, p);
  return n;
}

// k_remd_decide: every lane of the launch, in lane order.  counters [2, G, R - 1].
void remd_attempt(int32_t G, int32_t R, uint64_t every, uint64_t seed, uint64_t step, const double* beta, const float* epot, int32_t* slot,
                  int32_t* holder, uint8_t* accept, int32_t* slot_log, uint8_t* accept_log, int64_t* counters) {
  for (int t = 0; t < G * R; ++t) {
    const int g = t / R, s = t - g * R;
    const int64_t row = (int64_t)g * R, prow = (int64_t)g * (R - 1);
    tn_md::exchange_lane(seed, step, step / every, g, s, R, beta, epot + row, slot + row, holder + row, accept + prow,
                         slot_log ? slot_log + row : nullptr, accept_log ? accept_log + prow : nullptr, counters ? counters + prow : nullptr,
                         counters ? counters + (int64_t)G * (R - 1) + prow : nullptr);
  }
}

// k_remd_atoms: every thread of the launch.  n atoms per replica.
void remd_atoms(int32_t G, int32_t R, int32_t n, uint64_t every, uint64_t step, float* vel, float* sigma, const int32_t* slot,
                const uint8_t* accept, const float* table, const float* up, const float* down) {
  for (int i = 0; i < G * R * n; ++i) {
    const int b = i / n, at = i - b * n, g = b / R, t = slot[b];
    float factor;
    if (!tn_md::exchange_moved(step / every, t, R, accept + (int64_t)g * (R - 1), up, down, &factor)) continue;
    tn_md::scale3(vel + 3 * (int64_t)i, factor);
    sigma[i] = table[(int64_t)t * n + at];
  }
}

// Replica exchange of G ladders of R replicas of n atoms in an isotropic harmonic well (E = 0.5 k |x|^2, F = -k x) under Langevin
// dynamics: the launch sequence of a captured replay written as loops - OPEN, then per step the force, CLOSE, the kinetic-energy sum,
// and after every `every` steps the two exchange launches, then OPEN.  In place on x, v [G R n, 3], sigma [G R n], slot, holder;
// rows per attempt: epot, ekin [attempts, G R] of the step before the attempt, slot_log [attempts, G R], accept_log [attempts, G (R-1)].
void remd_harmonic(int32_t G, int32_t R, int32_t n, int64_t attempts, uint64_t every, float* x, float* v, const float* hk, const float* mass,
                   float* sigma, float dt, float c1, float c2, uint64_t seed, float k, const double* beta, const float* table,
                   const float* up, const float* down, int32_t* slot, int32_t* holder, float* epot_log, float* ekin_log,
                   int32_t* slot_log, uint8_t* accept_log, int64_t* counters, uint8_t* accept) {
  const int64_t B = (int64_t)G * R, N = B * n;
  uint64_t step = 0;
  float f[3];
  for (int64_t i = 0; i < N; ++i) {
    for (int d = 0; d < 3; ++d) f[d] = tn_md::md_mul(-k, x[3 * i + d]);
    tn_md::open_step(x + 3 * i, v + 3 * i, f, hk[i], dt);
  }
  for (int64_t a = 0; a < attempts; ++a)
    for (uint64_t t = 0; t < every; ++t) {
      const bool last = t + 1 == every;
      for (int64_t b = 0; b < B; ++b) {
        float ekin = 0.f;
        double epot = 0.0;
        for (int64_t i = b * n; i < (b + 1) * n; ++i) {
          for (int d = 0; d < 3; ++d) {
            f[d] = tn_md::md_mul(-k, x[3 * i + d]);
            epot += 0.5 * (double)k * (double)x[3 * i + d] * (double)x[3 * i + d];
          }
          ekin += tn_md::close_step(v + 3 * i, f, hk[i], mass[i], 1, c1, c2, sigma[i], seed, step, (uint32_t)i);
        }
        if (last) {
          epot_log[a * B + b] = (float)epot;
          ekin_log[a * B + b] = ekin;
        }
      }
      ++step;
      if (last) {
        remd_attempt(G, R, every, seed, step, beta, epot_log + a * B, slot, holder, accept, slot_log + a * B,
                     accept_log + a * (int64_t)G * (R - 1), counters);
        remd_atoms(G, R, n, every, step, v, sigma, slot, accept, table, up, down);
      }
      for (int64_t i = 0; i < N; ++i) {
        for (int d = 0; d < 3; ++d) f[d] = tn_md::md_mul(-k, x[3 * i + d]);
        tn_md::open_step(x + 3 * i, v + 3 * i, f, hk[i], dt);
      }
    }
}

}  // extern "C"
