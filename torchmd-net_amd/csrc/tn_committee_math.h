// Committee of M models (tn_committee.hip): mean and spread of the members' energies and forces, the per-atom and per-molecule force
// deviation and the gate on it.  __host__ __device__: tests/committee_host.hip compiles this header host-only, so the statements a GPU
// lane runs are the statements the host checker runs.
//
//   x_k, k = 0..M-1, the members' fp32 values of one energy or one force component, 2 <= M <= kMaxMembers:
//            mean = (1 / M) sum_k x_k
//            var  = sum_k (x_k - mean)^2 / (M - 1)          the unbiased estimator (torch.std)
//            std  = sqrt(var)
//   atom i:      d_i = sqrt(var_ix + var_iy + var_iz)       a d_i that is not finite is taken as +inf
//   molecule m:  D_m = max_{i in m} d_i,  a_m = the smallest i that attains it;  no atoms: D_m = 0, a_m = -1
//   gate:        fires when !(D_m <= threshold), so that a NaN can never pass as "certain"
//
// Two passes over the M values: the mean first, then the squared differences - never sum x^2 - M mean^2, which subtracts numbers of
// the size of the total energy.  Sums, the division and the square roots are fp64 in member order; every output is rounded to
// fp32 ONCE.  The mean of M equal fp32 values is that value (M x is exact in fp64 for M <= 16), and their spread is exactly 0.
//
// The maximum over a molecule is an integer maximum: d_i >= 0, so its bit pattern orders as an unsigned integer, and
// (bits(d_i) << 32) | (0xffffffff - i) ordered as a 64-bit unsigned integer picks the largest d_i and, among equals, the smallest i.
// No atom packs to 0 (i < 2^32 - 1), so 0 is the empty molecule.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COMMITTEE_FN __host__ __device__ inline
#else
#define COMMITTEE_FN inline
#endif

namespace tn_committee {

constexpr int kMaxMembers = 16;  // TMDNET_COMMITTEE_MAX_MEMBERS

// mean and std of x[0..M), rounded once each; returns the variance in fp64 (what the atom's deviation sums)
template <int M>
COMMITTEE_FN double mean_std(const float (&x)[M], float* mean, float* std) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < M; ++k) s += (double)x[k];
  const double mu = s / (double)M;
  double q = 0.0;
#pragma unroll
  for (int k = 0; k < M; ++k) {
    const double d = (double)x[k] - mu;
    q += d * d;
  }
  const double var = q / (double)(M - 1);
  *mean = (float)mu;
  *std = (float)sqrt(var);
  return var;
}

// d_i from the three variances; anything that is not a finite fp32 number becomes +inf and wins the maximum
COMMITTEE_FN float deviation(double vx, double vy, double vz) {
  const float d = (float)sqrt((vx + vy) + vz);
  return (d <= 3.402823466e+38f) ? d : INFINITY;  // (a NaN fails the comparison)
}

COMMITTEE_FN uint32_t float_bits(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, sizeof(u));
  return u;
}

COMMITTEE_FN float bits_float(uint32_t u) {
  float v;
  __builtin_memcpy(&v, &u, sizeof(v));
  return v;
}

// the word of atom (molecule) i with the non-negative value d; see the head of this file
COMMITTEE_FN uint64_t pack(float d, uint32_t i) { return ((uint64_t)float_bits(d) << 32) | (uint64_t)(0xffffffffu - i); }

// the maximum word of a molecule -> D_m, a_m; the empty word 0 -> 0, -1
COMMITTEE_FN void unpack(uint64_t w, float* D, int64_t* a) {
  if (!w) {
    *D = 0.0f;
    *a = -1;
    return;
  }
  *D = bits_float((uint32_t)(w >> 32));
  *a = (int64_t)(0xffffffffu - (uint32_t)w);
}

COMMITTEE_FN bool gate_fires(float D, float threshold) { return !(D <= threshold); }

}  // namespace tn_committee
