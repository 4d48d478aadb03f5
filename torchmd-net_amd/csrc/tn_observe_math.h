// The arithmetic of the MD loop's observer (tn_observe.hip), host-compilable as tn_md_math.h is: which steps are samples, where a
// sample lands in a ring, the bin of a pair distance, which pair types a pair of selector masks counts for, and the normalisations
// the host applies to the raw sums.  tests/observe_host.hip compiles it without a device; tests/test_md_observe_host.py holds it to
// the numpy oracle.
//
// Sampling.  s0 is the step counter at capture or reset, S the sampling interval.  Step s is a sample when s > s0 and
// (s - s0) % S == 0; its index is j = (s - s0) / S - 1, computed from the 64-bit counter on the device.  There is no sample
// counter: what has been recorded is a function of the loop's step counter alone (samples_at).
//
// The bin of a pair.  d2 is tn_common.h's pair_geometry in fp32.  The pair is counted when d2 < r_max2 (both fp32; r_max2 is
// r_max * r_max formed in fp64 and rounded once), in bin min((int)(sqrtf(d2) * inv_dr), bins - 1): sqrtf is the correctly rounded
// fp32 square root, the product is ONE rounded fp32 multiplication (md_mul), inv_dr is bins / r_max formed in fp64 and rounded
// once.  An fp32 mirror that rounds in the same places reproduces every bin.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tn_md_math.h"

namespace tn_obs {

constexpr int kMaxTypes = 4;    // pair types of the histogram; groups of the MSD; groups of the VACF
constexpr int kMaxBins = 1024;  // per pair type: kMaxTypes * kMaxBins u32 are the block's LDS histogram, 16 KB
constexpr int kMaxLags = 256;
constexpr int kTile = 256;  // atoms per tile of the pair sweep = threads per block

// bits of the per-atom selector mask the caller stages: pair type p - selector a: bit 2p, selector b: bit 2p + 1;
// MSD group g: bit 8 + g; VACF group g: bit 16 + g
constexpr uint32_t kPairBits = 0xffu;
constexpr int kMsdShift = 8, kVacfShift = 16;

// index of the sample taken at step s, or -1 when s is no sample
MD_FN int64_t sample_index(uint64_t s, uint64_t s0, uint64_t S) {
  if (S == 0 || s <= s0) return -1;
  const uint64_t d = s - s0;
  return d % S ? (int64_t)-1 : (int64_t)(d / S) - 1;
}

// samples recorded by a loop whose counter reads `step` completed steps
MD_FN int64_t samples_at(uint64_t step, uint64_t s0, uint64_t S) { return (S == 0 || step <= s0) ? 0 : (int64_t)((step - s0) / S); }

// the step sample j was taken at
MD_FN uint64_t sample_step(int64_t j, uint64_t s0, uint64_t S) { return s0 + ((uint64_t)j + 1u) * S; }

// slot of sample j in a ring of `capacity` rows
MD_FN int ring_slot(int64_t j, int capacity) { return (int)(j % (int64_t)capacity); }

// samples that contribute to lag l of the autocorrelation after n samples
MD_FN int64_t lag_samples(int64_t n_samples, int l) { return n_samples > l ? n_samples - l : 0; }

// bin of a pair at squared distance d2, -1 when it is not counted
MD_FN int rdf_bin(float d2, float r_max2, float inv_dr, int bins) {
  if (!(d2 < r_max2)) return -1;
  const int b = (int)tn_md::md_mul(sqrtf(d2), inv_dr);
  return b < bins - 1 ? b : bins - 1;
}

// Bit 2p of the result: pair type p counts the pair of atoms with masks mi and mj - one matches selector a and the other selector b,
// in either orientation, once.
MD_FN uint32_t pair_types(uint32_t mi, uint32_t mj) {
  mi &= kPairBits;
  mj &= kPairBits;
  return ((mi & (mj >> 1)) | ((mi >> 1) & mj)) & 0x55u;
}

// pairs the normalisation of type (a, b) divides by: N_a N_b, or N_a (N_a - 1) / 2 when a and b are the same selector
MD_FN double pair_count(int64_t n_a, int64_t n_b, int same) {
  return same ? 0.5 * (double)n_a * (double)(n_a - 1) : (double)n_a * (double)n_b;
}

// volume of the shell of bin b
MD_FN double shell_volume(int b, int bins, double r_max) {
  const double dr = r_max / (double)bins, lo = dr * (double)b, hi = dr * (double)(b + 1);
  return 4.0 * 3.14159265358979323846 / 3.0 * (hi * hi * hi - lo * lo * lo);
}

// g of a bin: with a box (volume > 0) counts / (n_samples n_pairs shell / volume), without one counts / (n_samples n_pairs)
MD_FN double rdf_value(int64_t count, int64_t n_samples, double n_pairs, double shell, double volume) {
  const double ideal = volume > 0.0 ? (double)n_samples * n_pairs * shell / volume : (double)n_samples * n_pairs;
  return (double)count / ideal;
}

}  // namespace tn_obs
