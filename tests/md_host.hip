// TEST INFRASTRUCTURE ONLY: the per-atom arithmetic of the device-resident MD loop (torchmd-net_amd/csrc/tn_md_math.h) compiled for
// the host (hipcc --cuda-host-only), one plain loop per kernel body, loaded through ctypes by tests/md_host_mirror.py.  The
// statements are the ones a GPU lane runs; tests/test_md_host.py compares them with tests/md_oracle.py without a GPU.
#include <stdint.h>

#include "../torchmd-net_amd/csrc/tn_md_math.h"

extern "C" {

void md_philox(int64_t n, const uint32_t* counters, const uint32_t* keys, uint32_t* out) {
  for (int64_t i = 0; i < n; ++i) tn_md::philox4x32_10(counters + 4 * i, keys + 2 * i, out + 4 * i);
}

void md_uniform(int64_t n, const uint32_t* words, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = tn_md::uniform_open(words[i]);
}

void md_normals(int64_t n, const uint32_t* words, float* out) {
  for (int64_t i = 0; i < n; ++i) tn_md::normals3(words + 4 * i, out + 3 * i);
}

// the noise of atoms[0..n) at `step`
void md_noise(int64_t n, uint64_t seed, uint64_t step, const uint32_t* atoms, float* out) {
  for (int64_t i = 0; i < n; ++i) tn_md::langevin_noise(seed, step, atoms[i], out + 3 * i);
}

// closing half (B, O when sigma != NULL, kinetic term) of atoms 0..n, in place on v[n,3]; ke[n]
void md_close(int64_t n, float* v, const float* f, const float* hk, const float* mass, const float* sigma, float c1, float c2,
              uint64_t seed, uint64_t step, float* ke) {
  for (int64_t i = 0; i < n; ++i)
    ke[i] = tn_md::close_step(v + 3 * i, f + 3 * i, hk[i], mass[i], sigma != nullptr, c1, c2, sigma ? sigma[i] : 0.f, seed, step, (uint32_t)i);
}

// opening half (B, A), in place on x[n,3] and v[n,3]
void md_open(int64_t n, float* x, float* v, const float* f, const float* hk, float dt) {
  for (int64_t i = 0; i < n; ++i) tn_md::open_step(x + 3 * i, v + 3 * i, f + 3 * i, hk[i], dt);
}

}  // extern "C"
