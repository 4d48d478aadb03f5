// TEST INFRASTRUCTURE ONLY: the arithmetic of the MD loop's observer (torchmd-net_amd/csrc/tn_observe_math.h) compiled for the host
// (hipcc --cuda-host-only) and loaded through ctypes by tests/observe_host_mirror.py.  The statements are the ones a GPU lane runs;
// tests/test_md_observe_host.py compares them with tests/observe_oracle.py without a GPU.  With -DOBSERVE_HOST_MAIN the file is a
// stand-alone program (its own main) that drives every entry once: the build the host test runs under
// -fsanitize=address,undefined.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../torchmd-net_amd/csrc/tn_observe_math.h"

extern "C" {

int64_t obs_sample_index(uint64_t s, uint64_t s0, uint64_t S) { return tn_obs::sample_index(s, s0, S); }
int64_t obs_samples_at(uint64_t step, uint64_t s0, uint64_t S) { return tn_obs::samples_at(step, s0, S); }
uint64_t obs_sample_step(int64_t j, uint64_t s0, uint64_t S) { return tn_obs::sample_step(j, s0, S); }
int32_t obs_ring_slot(int64_t j, int32_t capacity) { return tn_obs::ring_slot(j, capacity); }
int64_t obs_lag_samples(int64_t n_samples, int32_t l) { return tn_obs::lag_samples(n_samples, l); }
uint32_t obs_pair_types(uint32_t mi, uint32_t mj) { return tn_obs::pair_types(mi, mj); }
double obs_pair_count(int64_t n_a, int64_t n_b, int32_t same) { return tn_obs::pair_count(n_a, n_b, same); }
double obs_shell_volume(int32_t b, int32_t bins, double r_max) { return tn_obs::shell_volume(b, bins, r_max); }
double obs_rdf_value(int64_t count, int64_t n_samples, double n_pairs, double shell, double volume) {
  return tn_obs::rdf_value(count, n_samples, n_pairs, shell, volume);
}

// the bins of n squared distances (fp32), -1: not counted
void obs_bins(int64_t n, const float* d2, float r_max2, float inv_dr, int32_t bins, int32_t* out) {
  for (int64_t k = 0; k < n; ++k) out[k] = tn_obs::rdf_bin(d2[k], r_max2, inv_dr, bins);
}

// k_obs_rdf on pairs already formed: counts[p][bin] += 1 for every pair type the two masks match, as the kernel's inner loop does
void obs_histogram(int64_t n, const float* d2, const uint32_t* mi, const uint32_t* mj, int32_t P, float r_max2, float inv_dr,
                   int32_t bins, uint64_t* counts) {
  for (int64_t k = 0; k < n; ++k) {
    const uint32_t ty = tn_obs::pair_types(mi[k], mj[k]);
    if (!ty) continue;
    const int bin = tn_obs::rdf_bin(d2[k], r_max2, inv_dr, bins);
    if (bin < 0) continue;
    for (int p = 0; p < P; ++p)
      if ((ty >> (2 * p)) & 1u) counts[(int64_t)p * bins + bin] += 1;
  }
}

}  // extern "C"

#ifdef OBSERVE_HOST_MAIN
int main() {
  int ok = 1;
  // a counter that crosses 2^32
  const uint64_t s0 = (1ull << 32) - 7, S = 3;
  int64_t seen = 0;
  for (uint64_t s = s0 - 2; s < s0 + 40; ++s) {
    const int64_t j = obs_sample_index(s, s0, S);
    if (j >= 0) {
      ok &= j == seen && obs_sample_step(j, s0, S) == s && obs_samples_at(s, s0, S) == j + 1;
      ++seen;
    }
  }
  ok &= seen == 13 && obs_ring_slot(12, 5) == 2 && obs_lag_samples(4, 6) == 0 && obs_lag_samples(9, 6) == 3;
  const int n = 6;
  float* d2 = (float*)malloc(n * sizeof(float));
  uint32_t* mi = (uint32_t*)malloc(n * sizeof(uint32_t));
  uint32_t* mj = (uint32_t*)malloc(n * sizeof(uint32_t));
  int32_t* bin = (int32_t*)malloc(n * sizeof(int32_t));
  uint64_t* counts = (uint64_t*)calloc(2 * 7, sizeof(uint64_t));
  const float d[6] = {0.f, 0.5f, 1.0f, 3.4999f, 3.5f, 100.f};
  for (int k = 0; k < n; ++k) {
    d2[k] = d[k] * d[k];
    mi[k] = 0x1u | 0x8u;  // selector a of type 0, selector b of type 1
    mj[k] = k & 1 ? 0x2u : 0x4u;
  }
  obs_bins(n, d2, 3.5f * 3.5f, 2.0f, 7, bin);
  obs_histogram(n, d2, mi, mj, 2, 3.5f * 3.5f, 2.0f, 7, counts);
  ok &= bin[0] == 0 && bin[1] == 1 && bin[2] == 2 && bin[3] == 6 && bin[4] == -1 && bin[5] == -1;
  uint64_t total = 0;
  for (int k = 0; k < 14; ++k) total += counts[k];
  ok &= total == 4;
  ok &= obs_pair_count(5, 5, 1) == 10.0 && obs_pair_count(5, 3, 0) == 15.0;
  ok &= fabs(obs_rdf_value(3, 2, 10.0, obs_shell_volume(1, 7, 3.5), 100.0) - 3.0 / (2.0 * 10.0 * obs_shell_volume(1, 7, 3.5) / 100.0)) < 1e-12;
  printf("samples %lld bins %d %d %d %d %d %d total %llu\n", (long long)seen, bin[0], bin[1], bin[2], bin[3], bin[4], bin[5],
         (unsigned long long)total);
  printf("observe_host: ok %d\n", ok);
  free(d2);
  free(mi);
  free(mj);
  free(bin);
  free(counts);
  return ok ? 0 : 1;
}
#endif
