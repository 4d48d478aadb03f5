// TEST INFRASTRUCTURE ONLY: the pair arithmetic of the ZBL / D2 priors (torchmd-net_amd/csrc/tn_prior_math.h) compiled for the host
// (hipcc --cuda-host-only), one plain loop per entry, loaded through ctypes by tests/prior_host_mirror.py.  The statements are the
// ones a GPU lane runs; tests/test_prior_host.py compares them with tests/prior_oracle.py without a GPU.  With -DPRIOR_HOST_MAIN the
// file is a program of its own (for the host sanitizers).
#include <stdint.h>
#include <stdio.h>

#include "../torchmd-net_amd/csrc/tn_prior_math.h"

extern "C" {

// u [n] and du/dr [n] of ZBL pairs at the distances r [n]; z23 = Z_i^0.23 + Z_j^0.23 and zz = Z_i Z_j as the kernel forms them
void prior_zbl(int64_t n, const float* r, float z23i, float z23j, float Zi, float Zj, double cutoff, double distance_scale,
               double energy_scale, float* u, float* du) {
  const tn_prior::ZblConst c = tn_prior::zbl_constants(cutoff, distance_scale, energy_scale);
  for (int64_t k = 0; k < n; ++k) tn_prior::zbl_pair(r[k], z23i + z23j, Zi * Zj, c, u + k, du + k);
}

// the same for D2 pairs; sc6 = sqrt C6 and rr = R_r of the two species
void prior_d2(int64_t n, const float* r, float sc6i, float sc6j, float rri, float rrj, double cutoff, double distance_scale,
              double energy_scale, float* u, float* du) {
  const tn_prior::D2Const c = tn_prior::d2_constants(cutoff, distance_scale, energy_scale);
  for (int64_t k = 0; k < n; ++k) tn_prior::d2_pair(r[k], sc6i * sc6j, rri + rrj, c, u + k, du + k);
}

// the pair test on the squared distance
int32_t prior_in_cutoff(float d2, float cutoff) { return tn_prior::in_cutoff(d2, cutoff) ? 1 : 0; }

int32_t prior_max_molecule_atoms() { return tn_prior::kMaxMoleculeAtoms; }

}  // extern "C"

#ifdef PRIOR_HOST_MAIN
int main() {
  float r[64], u[64], du[64];
  for (int k = 0; k < 64; ++k) r[k] = 0.3f + 0.07f * k;
  prior_zbl(64, r, 1.0f, 1.5f, 1.0f, 6.0f, 5.0, 1e-10, 1.602176634e-19, u, du);
  double s = 0.0;
  for (int k = 0; k < 64; ++k) s += (double)u[k] - (double)du[k];
  prior_d2(64, r, 1.3f, 0.8f, 0.14f, 0.13f, 10.0, 1e-10, 1.602176634e-19, u, du);
  for (int k = 0; k < 64; ++k) s += (double)u[k] - (double)du[k];
  printf("prior_host ok %.6e %d\n", s, prior_in_cutoff(1.0f, 2.0f));
  return 0;
}
#endif
