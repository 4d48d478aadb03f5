// Temperature replica exchange of the device-resident MD loop (tn_remd.hip): which slot pairs an attempt tries, the uniform number
// of a pair, the Metropolis decision and the slot / holder bookkeeping.  __host__ __device__, in the manner of tn_md_math.h:
// tests/remd_host.hip compiles this header host-only, so the statements a GPU lane runs are the statements the host checker runs.
//
// G independent ladders of R temperature slots; replica b = g R + r starts in slot r.  Replicas swap TEMPERATURES: slot[b] is the
// slot replica b holds, holder[g][s] the replica (0..R-1 within its ladder) that holds slot s - inverse permutations at all times.
// Attempt a = n / X after n completed steps tries the pairs (s, s + 1), s = (a & 1), (a & 1) + 2, ... while s + 1 < R.  The
// decision is fp64 in the order written; the noise is one Philox4x32-10 call of tn_md_math.h, counter word 3 = 2.
#pragma once
#include "tn_md_math.h"

namespace tn_md {

// is `s` the lower slot of a pair that attempt `a` tries?
MD_FN int exchange_is_lower(uint64_t a, int s, int R) {
  const int par = (int)(a & 1u);
  return s >= par && ((s - par) & 1) == 0 && s + 1 < R;
}

// is `s` the upper slot of such a pair?
MD_FN int exchange_is_upper(uint64_t a, int s, int R) { return s >= 1 && exchange_is_lower(a, s - 1, R); }

// the number of pairs attempt `a` tries, and the lower slot of its p-th pair
MD_FN int exchange_pair_count(uint64_t a, int R) { return (R - (int)(a & 1u)) / 2; }
MD_FN int exchange_pair_slot(uint64_t a, int p) { return (int)(a & 1u) + 2 * p; }

// u of pair (s, s + 1) of ladder g after `step` completed steps: uniform_open of word 0 of one Philox call,
// key = the 64-bit seed, counter = (step lo, step hi, g (R - 1) + s, 2) - apart from the atoms' stream (0) and the barostat's (1)
MD_FN float exchange_uniform(uint64_t seed, uint64_t step, uint32_t index) {
  const uint32_t c[4] = {(uint32_t)step, (uint32_t)(step >> 32), index, 2u};
  const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  philox4x32_10(c, k, w);
  return uniform_open(w[0]);
}

// Metropolis: D = (beta_s - beta_{s+1}) (E_i - E_j) with i the holder of s and j the holder of s + 1; accept iff D >= 0 or u < exp D.
// A NaN on the way (a NaN energy, inf - inf, 0 * inf) makes both comparisons false: a rejection.
MD_FN int exchange_decide(double beta_lo, double beta_hi, float E_i, float E_j, float u) {
  const double D = (beta_lo - beta_hi) * ((double)E_i - (double)E_j);
  return D >= 0.0 || (double)u < exp(D);
}

// an accepted swap of slots s and s + 1 in one ladder: slot[] and holder[] of that ladder (R entries each)
MD_FN void exchange_swap(int32_t* slot, int32_t* holder, int s) {
  const int32_t i = holder[s], j = holder[s + 1];
  slot[i] = s + 1;
  slot[j] = s;
  holder[s] = j;
  holder[s + 1] = i;
}

// One lane of the decision launch: slot s of ladder g in attempt a = step / X.  The lower slot of a tried pair decides, counts, swaps
// and logs the pair's two replicas; every other slot clears the flag of the pair it would be the lower slot of (not tried in this
// parity), and a slot in no pair logs its own holder.  Lanes of one launch touch disjoint entries.  epot, slot, slot_log: the
// ladder's R entries; holder, accept, accept_log, attempts, accepts: the ladder's R / R - 1 entries.  Returns the decision (0 / 1).
MD_FN int exchange_lane(uint64_t seed, uint64_t step, uint64_t a, int g, int s, int R, const double* beta, const float* epot,
                        int32_t* slot, int32_t* holder, uint8_t* accept, int32_t* slot_log, uint8_t* accept_log, int64_t* attempts,
                        int64_t* accepts) {
  if (!exchange_is_lower(a, s, R)) {
    if (s + 1 < R) {
      accept[s] = 0;
      if (accept_log) accept_log[s] = 0;
    }
    if (slot_log && !exchange_is_upper(a, s, R) && (uint32_t)holder[s] < (uint32_t)R) slot_log[holder[s]] = s;
    return 0;
  }
  const int32_t i = holder[s], j = holder[s + 1];
  if ((uint32_t)i >= (uint32_t)R || (uint32_t)j >= (uint32_t)R) {  // (a table the caller corrupted: nothing outside the ladder)
    accept[s] = 0;
    return 0;
  }
  const float u = exchange_uniform(seed, step, (uint32_t)(g * (R - 1) + s));
  const int acc = exchange_decide(beta[s], beta[s + 1], epot[i], epot[j], u);
  if (acc) exchange_swap(slot, holder, s);
  accept[s] = (uint8_t)acc;
  if (accept_log) accept_log[s] = (uint8_t)acc;
  if (attempts) attempts[s] += 1;
  if (accepts) accepts[s] += acc;
  if (slot_log) {
    slot_log[i] = slot[i];
    slot_log[j] = slot[j];
  }
  return acc;
}

// One lane of the per-atom launch: what happened to a replica that now holds slot t.  Returns 0 when its pair was not tried or was
// rejected; otherwise 1 and the factor for its velocities: it came up from s = t - 1 (up[s]) or down from s + 1 = t + 1 (down[s]).
MD_FN int exchange_moved(uint64_t a, int t, int R, const uint8_t* accept, const float* up, const float* down, float* factor) {
  int s;
  if (exchange_is_lower(a, t, R))
    s = t;
  else if (exchange_is_upper(a, t, R))
    s = t - 1;
  else
    return 0;
  if (!accept[s]) return 0;
  *factor = t == s ? down[s] : up[s];
  return 1;
}

}  // namespace tn_md
