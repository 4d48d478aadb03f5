// Arithmetic of the device-resident L-BFGS minimiser (tn_lbfgs.hip): the candidate pair of one atom, the Gram insertion, the two-loop
// recursion in coefficient space, the per-atom direction and the per-atom step clamp.  L-BFGS without line search in the form ASE
// ships (ase.optimize.LBFGS: H0 = 1 / alpha, the step of every ATOM clamped to max_step, damping), one optimiser per molecule, with one
// documented deviation: a pair enters the history only when s.y > 0.  __host__ __device__: tests/lbfgs_host.hip compiles this header
// host-only, so the statements a GPU wave runs are the statements the host checker runs - there with ONE lane (LBFGS_LANES = 1), so
// the order of the sums over the history differs from the device's 64 lanes and agrees to fp64 rounding, not bit for bit.
//
// Vector-free form.  Every vector of the recursion lies in the span of b = (s_slots, y_slots, g), g = -F.  The recursion therefore
// runs on the coefficients delta of that basis, given the Gram matrix of the basis: SS[a][b] = s_a.s_b, SY[a][b] = s_a.y_b,
// YY[a][b] = y_a.y_b indexed by ring SLOT, and the products of this step's g in `tot`.  The ring has memory + 1 slots; `order` is a
// permutation of them: order[0 .. h-1] are the pairs held, oldest first, and order[h] is the spare slot the candidate of this step
// was written to, so a rejected candidate overwrites nothing.
//
// `tot` of one molecule, fp64, 6 (memory + 1) + 4 entries: for slot a, tot[6a .. 6a+5] = s_c.s_a, s_c.y_a, y_c.s_a, y_c.y_a, g.s_a,
// g.y_a (c: the candidate; for a = c: s_c.s_c, s_c.y_c, s_c.y_c again, y_c.y_c, g.s_c, g.y_c), then ff = g.g, fmax2 = max |F_i|^2 and
// s_c.s_c, y_c.y_c once more at a place that does not depend on the ring (0 without a candidate).  Every product is of two widened
// fp32 values and exact in fp64; only the sums round.
//
// Rounding.  The candidate is one rounded fp32 subtraction per component, the move x + c p one rounded product and one rounded sum
// (tn_md_math.h); everything per molecule is fp64 in the order written; the direction is accumulated in fp64 and rounded to fp32
// once; the clamp factor is computed in fp64 and rounded to fp32 once.
#pragma once
#include "tn_md_math.h"

namespace tn_lbfgs {

using tn_md::md_add;
using tn_md::md_mul;

enum { LBFGS_MOVING = 0, LBFGS_FROZEN = 1, LBFGS_UNUSABLE = 2 };

constexpr int kMaxMemory = 512;  // the controller keeps 3.5 memory + 5 doubles per wave in LDS

struct Params {
  double alpha, max_step, damping, fmax;  // H0 = 1 / alpha
  int32_t memory;
};

struct MolState {  // views of one molecule's state
  int32_t* h;      // pairs held
  int32_t* order;  // [memory + 1]
  int64_t* conv;   // converged_at, -1 while it moves
  double* SS;      // [memory + 1][memory + 1] by slot
  double* SY;
  double* YY;
};

// ---- the lanes that share one molecule: a wave on the device, one on the host -------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
#define LBFGS_LANES 64
__device__ inline int lane() { return (int)(threadIdx.x & 63u); }
__device__ inline double lane_sum(double v) {  // every lane gets the sum: the xor tree
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline void lane_sync() { __threadfence_block(); }  // what one lane wrote (LDS, global) is what the others read next
// The same for the controller's scratch alone (delta, av, ord), which on the device is LDS: a wave's LDS instructions are carried out in
// the order it issues them, so the fence only has to keep the compiler from moving them - it must not wait for the Gram rows in flight.
__device__ inline void scratch_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
#else
#define LBFGS_LANES 1
inline int lane() { return 0; }
inline double lane_sum(double v) { return v; }
inline void lane_sync() {}
inline void scratch_sync() {}
#endif

MD_FN int tot_entries(int memory) { return 6 * (memory + 1) + 4; }

// (ax bx + ay by) + az bz of widened fp32 values: exact products, two rounded fp64 sums
MD_FN double dot3w(const float a[3], const float b[3]) {
  return ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2];
}

// the candidate pair of one atom after a move: s = x - x_prev, y = F_prev - F, one rounded subtraction each; a fixed atom: 0
MD_FN void candidate(const float x[3], const float x_prev[3], const float f[3], const float f_prev[3], int fixed, float s[3], float y[3]) {
  for (int k = 0; k < 3; ++k) {
    s[k] = fixed ? 0.f : md_add(x[k], -x_prev[k]);
    y[k] = fixed ? 0.f : md_add(f_prev[k], -f[k]);
  }
}

// Are the sums the controller is about to use finite?  A converged molecule is not looked at.  Three squares decide it: when g.g,
// s_c.s_c and y_c.y_c are finite, every component of g, s_c and y_c is, and every other scalar product - against pairs that passed
// this test when they were candidates - is bounded by Cauchy-Schwarz far below the range of fp64 (the vectors are fp32).
MD_FN int usable(int64_t conv, int memory, const double* tot, int moved) {
  if (conv >= 0) return 1;
  const int M1 = memory + 1;
  return isfinite(tot[6 * M1]) && (!moved || (isfinite(tot[6 * M1 + 2]) && isfinite(tot[6 * M1 + 3])));
}

// One row of the Gram matrix as the lanes hold it: for the target t = s_i (target_y = 0) or y_i (target_y = 1), i the ring position,
// lane l keeps G[s_a, t] and G[y_a, t] of the pairs at the positions l, l + LANES, ..., and every lane G[g, t] and s_i.y_i.  Loading a
// row does not depend on the coefficients, so the row of the NEXT step of a loop is requested before the current one is reduced:
// the loop's chain is then one reduction per step and not one trip to memory.
constexpr int kChunks = (kMaxMemory + LBFGS_LANES - 1) / LBFGS_LANES;

struct GramRow {
  double u[kChunks], w[kChunks], gt, diag;
};

MD_FN void gram_load(const MolState& st, int M1, int h, const double* tot, const int32_t* ord, int i, int target_y, GramRow* r) {
  const int ai = ord[i];
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const int p = lane() + k * LBFGS_LANES;
    if (p >= h) break;
    const int a = ord[p];
    r->u[k] = target_y ? st.SY[a * M1 + ai] : st.SS[a * M1 + ai];
    r->w[k] = target_y ? st.YY[a * M1 + ai] : st.SY[ai * M1 + a];
  }
  r->gt = tot[6 * ai + (target_y ? 5 : 4)];
  r->diag = st.SY[ai * M1 + ai];
}

// delta_j G[j, t] summed over the basis, from a loaded row: per lane the pairs in ring order, s then y; lane 0 adds g; the lane tree
MD_FN double gram_dot(int M1, int h, const double* delta, const int32_t* ord, const GramRow& r) {
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const int p = lane() + k * LBFGS_LANES;
    if (p >= h) break;
    const int a = ord[p];
    acc += delta[a] * r.u[k];
    acc += delta[M1 + a] * r.w[k];
  }
  if (lane() == 0) acc += delta[2 * M1] * r.gt;
  return lane_sum(acc);
}

// One control of one molecule after `step` steps, by the lanes that share it.  `moved`: a move preceded this evaluation, so the spare
// slot order[h] holds a candidate and tot its products.  The caller has checked `usable`.  Writes the state, delta [2 (memory + 1) + 1]
// (the coefficients of p = - sum_j delta_j b_j: entry a for s of slot a, memory + 1 + a for y of slot a, the last for g), *accepted and
// *gp = g.p; `av` and `ord` [memory + 1] are scratch (with delta in LDS on the device: `ord` is the ring order, read once).
// LBFGS_FROZEN: converged before (nothing is written) or now.
MD_FN int control(const MolState& st, const Params& p, const double* tot, int moved, int64_t step, double* delta, double* av,
                  int32_t* ord, int32_t* accepted, double* gp) {
  *accepted = 0;
  *gp = 0.0;
  if (*st.conv >= 0) return LBFGS_FROZEN;
  const int M1 = p.memory + 1;
  if (sqrt(tot[6 * M1 + 1]) < p.fmax) {
    if (lane() == 0) *st.conv = step;
    lane_sync();
    return LBFGS_FROZEN;
  }
  int h = *st.h;
  if (moved) {
    const int c = st.order[h];
    if (tot[6 * c + 1] > 0.0) {  // the curvature condition s_c.y_c > 0: the pair enters the history
      *accepted = 1;
      lane_sync();  // (every lane has read h and c)
      if (h == p.memory) {  // full: the oldest pair leaves, its slot becomes the spare one
        const int oldest = st.order[0];
        for (int base = 0; base < p.memory; base += LBFGS_LANES) {
          const int q = base + lane();
          const int next = q < p.memory ? st.order[q + 1] : 0;
          lane_sync();
          if (q < p.memory) st.order[q] = next;
          lane_sync();
        }
        if (lane() == 0) st.order[p.memory] = oldest;
      } else {
        h += 1;
        if (lane() == 0) *st.h = h;
      }
      lane_sync();
      for (int q = lane(); q < h; q += LBFGS_LANES) {  // the candidate's row and column of the three Gram blocks
        const int a = st.order[q];
        st.SS[c * M1 + a] = st.SS[a * M1 + c] = tot[6 * a + 0];
        st.SY[c * M1 + a] = tot[6 * a + 1];
        st.SY[a * M1 + c] = tot[6 * a + 2];
        st.YY[c * M1 + a] = st.YY[a * M1 + c] = tot[6 * a + 3];
      }
      lane_sync();
    }
  }
  // the two loops on the coefficients
  for (int q = lane(); q < h; q += LBFGS_LANES) ord[q] = st.order[q];
  for (int j = lane(); j < 2 * M1 + 1; j += LBFGS_LANES) delta[j] = j == 2 * M1 ? 1.0 : 0.0;
  lane_sync();
  GramRow cur, nxt;
  if (h > 0) gram_load(st, M1, h, tot, ord, h - 1, 0, &cur);
  for (int i = h - 1; i >= 0; --i) {  // newest ... oldest
    if (i > 0) gram_load(st, M1, h, tot, ord, i - 1, 0, &nxt);
    const double a = gram_dot(M1, h, delta, ord, cur) / cur.diag;
    scratch_sync();
    if (lane() == 0) {
      av[i] = a;
      delta[M1 + ord[i]] -= a;
    }
    scratch_sync();
    cur = nxt;
  }
  const double H0 = 1.0 / p.alpha;
  for (int j = lane(); j < 2 * M1 + 1; j += LBFGS_LANES) delta[j] = H0 * delta[j];
  scratch_sync();
  if (h > 0) gram_load(st, M1, h, tot, ord, 0, 1, &cur);
  for (int i = 0; i < h; ++i) {  // oldest ... newest
    if (i + 1 < h) gram_load(st, M1, h, tot, ord, i + 1, 1, &nxt);
    const double b = gram_dot(M1, h, delta, ord, cur) / cur.diag;
    scratch_sync();
    if (lane() == 0) delta[ord[i]] += av[i] - b;
    scratch_sync();
    cur = nxt;
  }
  double acc = 0.0;  // g.p = - sum_j delta_j G[j, g]
  for (int q = lane(); q < h; q += LBFGS_LANES) {
    const int a = ord[q];
    acc += delta[a] * tot[6 * a + 4];
    acc += delta[M1 + a] * tot[6 * a + 5];
  }
  if (lane() == 0) acc += delta[2 * M1] * tot[6 * M1];
  *gp = -lane_sum(acc);
  lane_sync();
  return LBFGS_MOVING;
}

// p_i = -(delta_g g_i + sum over the pairs held, oldest first, of (delta_s s_i + delta_y y_i)), g_i = -F_i: fp64, rounded to fp32 once.
// The rings S, Y are [memory + 1][n_atoms][3]; i is the atom.
MD_FN void atom_direction(const float f[3], int h, const int32_t* order, int M1, const double* delta, const float* S, const float* Y,
                          int64_t n_atoms, int64_t i, float p[3]) {
  double acc[3];
  for (int k = 0; k < 3; ++k) acc[k] = delta[2 * M1] * -(double)f[k];
#pragma unroll 4
  for (int q = 0; q < h; ++q) {  // (unrolled so that the ring rows of four pairs are in flight at once; the sums stay in this order)
    const int a = order[q];
    const float* s = S + ((int64_t)a * n_atoms + i) * 3;
    const float* y = Y + ((int64_t)a * n_atoms + i) * 3;
    for (int k = 0; k < 3; ++k) {
      acc[k] += delta[a] * (double)s[k];
      acc[k] += delta[M1 + a] * (double)y[k];
    }
  }
  for (int k = 0; k < 3; ++k) p[k] = (float)(-acc[k]);
}

// ASE's per-atom clamp: longest = max_i |p_i| (longest2 its square); c = damping (longest >= max_step ? max_step / longest : 1),
// fp64, rounded to fp32 once
MD_FN float clamp(double longest2, double max_step, double damping) {
  const double longest = sqrt(longest2);
  const double c = longest >= max_step ? damping * (max_step / longest) : damping;
  return (float)c;
}

// x <- x + c p of one atom of a moving molecule
MD_FN void atom_step(float x[3], float c, const float p[3]) {
  for (int k = 0; k < 3; ++k) x[k] = md_add(x[k], md_mul(c, p[k]));
}

}  // namespace tn_lbfgs
