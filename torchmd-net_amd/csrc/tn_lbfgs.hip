// Device-resident L-BFGS geometry minimisation: the kernels that sit between two energy+force evaluations of a captured step, so
// that K quasi-Newton steps replay as one HIP graph with no host work in between.  ASE's LBFGS without line search, one optimiser
// per molecule (replica): every molecule has its own history and freezes at its own step.  The arithmetic is tn_lbfgs_math.h.
//
// The two-loop recursion runs in coefficient space (the "vector-free" form): every vector of it lies in the span of the held s_j,
// y_j and g = -F, so given the Gram matrix of that basis the recursion is O(h^2) scalar work per molecule and needs no chain of
// 2 h dependent reductions over the atoms.  One step, after the forces F at the current positions are known:
//   dots       grid (B, S): the candidate pair s_c = x - x_prev, y_c = F_prev - F into the spare ring slot, and at most 6 h + 7
//              sums per molecule: s_c, y_c and g against every held s_j, y_j and against s_c, y_c; ff; fmax2 = max |F_i|^2.  Each of
//              the sixteen waves takes its own j and strides the slice's atoms; lanes add by the wave's xor tree.  Exact fp64 products of widened fp32
//              values, fp64 sums in a fixed order, no floating-point atomics: repeats are bit-identical.
//   control    one wave per molecule, four molecules per block: slices added in slice order; converged? a sum
//              not finite? else accept the candidate iff s_c.y_c > 0 (rotate the ring, insert its Gram row), the recursion on the
//              coefficients delta, the log rows.  The only kernel that writes the status word and the step counter.
//   direction  grid (B, S): p_i = -(delta_g g_i + sum_slots (delta_s s_i + delta_y y_i)) in fp64, rounded to fp32 once; the slice
//              maximum of |p_i|^2.
//   move       one thread per atom: accept the evaluation (keep its forces, or go back to x_prev when it overflowed), save x_prev and
//              F_prev, c = damping min(1, max_step / max_i |p_i|) rounded to fp32 once, x <- x + c p.
// TMDNET_MIN_MIDDLE is these four launches, TMDNET_MIN_CLOSE the same with a last one that only accepts (the kept forces and the way
// back after an overflow cannot wait for the next replay), TMDNET_MIN_OPEN the move alone: every evaluated force set drives the
// controller exactly once whatever K is, and a replay of K steps is 4 K + 1 launches beside the evaluations.  After a reset the
// first launch is a CLOSE on the forces of the start geometry (h = 0, p = F / alpha; it counts no step).
//
// Overflow and unusable sums follow tn_min.hip: the controller latches status 1 when the evaluation before it overflowed
// (counts[2]) and the move of the same launch puts x back from x_prev - the history is intact because the candidate sat in the
// spare slot; a sum that is not finite latches status 2 before anything of that step is written.  From then on every launch
// returns at once until tmdnet_lbfgs_reset.  Nothing allocates or synchronises; everything is capturable.
#include <cmath>

#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_lbfgs_math.h"
#include "tn_loop.h"
#include "tn_model.h"

namespace tn {

namespace {

constexpr int kLbDotsThreads = 1024;  // sixteen waves share the h + 1 tasks of a slice
constexpr int kLbCtlWaves = 4;  // molecules per block of the controller
constexpr int kLbCopyWord = 4;  // header words 4, 5, 7: the copy of words 0, 1, 3 that the controller's blocks read
constexpr int kLbCauseWord = 8; // the cause of status 2 (1: a sum)

// doubles of LDS per wave of the controller: delta [2 M1 + 1], av [M1] and the ring order as M1 int32 (<= 57 504 B per block at memory 512)
__host__ __device__ inline size_t lb_ctl_doubles(int M1) { return (size_t)(3 * M1 + 1) + (size_t)(M1 + 1) / 2; }

struct LbState {  // views into the caller's workspace
  uint32_t* head;   // [0] step lo, [1] step hi, [2] status (sticky: 1 overflow, 2 non-finite sums), [3] 1 = reset, not yet controlled,
                    // [4], [5], [7] the copy of [0], [1], [3] the controller's blocks read, [8] the cause of status 2 (1: a sum)
  int32_t* h;       // [B] pairs held
  int64_t* conv;    // [B] converged_at
  int32_t* order;   // [B, M1] ring order (tn_lbfgs_math.h)
  double* SS;       // [B, M1, M1]
  double* SY;
  double* YY;
  double* delta;    // [B, 2 M1 + 1] the coefficients of the move prepared
  double* tot;      // [B, NP] the sums of the last control, slices added
  double* part;     // [B, S, NP] slice partial sums
  double* dmax;     // [B, S] slice maxima of |p_i|^2
  float* cmove;     // [B] the clamp factor of the last move (0: the molecule was frozen)
  float* x_prev;    // [N, 3] positions before the last move
  float* f_prev;    // [N, 3] forces there
  float* ringS;     // [M1, N, 3]
  float* ringY;     // [M1, N, 3]
};

// the byte offsets of the sixteen arrays behind the 256-aligned base, then the total
void lb_layout(int64_t N, int64_t B, int64_t memory, size_t off[17]) {
  const size_t n = (size_t)(N > 0 ? N : 0), b = (size_t)(B > 0 ? B : 0), M1 = (size_t)memory + 1, NP = 6 * M1 + 4;
  const size_t S = (size_t)mol_slices(N, B);
  const size_t sizes[16] = {kHeaderBytes, b * 4,          b * 8,      b * M1 * 4, b * M1 * M1 * 8, b * M1 * M1 * 8, b * M1 * M1 * 8, b * (2 * M1 + 1) * 8,
                            b * NP * 8,     b * S * NP * 8, b * S * 8,  n * 12,     n * 12,          M1 * n * 12,     M1 * n * 12,     b * 4};
  size_t at = 0;
  for (int k = 0; k < 16; ++k) {
    off[k] = at;
    at += align256(sizes[k]);
  }
  off[16] = at;
}

LbState carve_lb(void* ws, int64_t N, int64_t B, int64_t memory) {
  char* p = reinterpret_cast<char*>(align256(reinterpret_cast<size_t>(ws)));
  size_t off[17];
  lb_layout(N, B, memory, off);
  LbState st;
  st.head = reinterpret_cast<uint32_t*>(p + off[0]);
  st.h = reinterpret_cast<int32_t*>(p + off[1]);
  st.conv = reinterpret_cast<int64_t*>(p + off[2]);
  st.order = reinterpret_cast<int32_t*>(p + off[3]);
  st.SS = reinterpret_cast<double*>(p + off[4]);
  st.SY = reinterpret_cast<double*>(p + off[5]);
  st.YY = reinterpret_cast<double*>(p + off[6]);
  st.delta = reinterpret_cast<double*>(p + off[7]);
  st.tot = reinterpret_cast<double*>(p + off[8]);
  st.part = reinterpret_cast<double*>(p + off[9]);
  st.dmax = reinterpret_cast<double*>(p + off[10]);
  st.x_prev = reinterpret_cast<float*>(p + off[11]);
  st.f_prev = reinterpret_cast<float*>(p + off[12]);
  st.ringS = reinterpret_cast<float*>(p + off[13]);
  st.ringY = reinterpret_cast<float*>(p + off[14]);
  st.cmove = reinterpret_cast<float*>(p + off[15]);
  return st;
}

// grid (B, S): slice s of molecule m -> part[m, s, :].  Task t = 0 .. h - 1: the six sums against the pair at ring position t; the
// last task: the candidate against itself (it also stores the candidate), ff and fmax2.  Wave w takes the tasks w, w + 16, ...
__global__ __launch_bounds__(kLbDotsThreads) void k_lbfgs_dots(LbState st, const int* __restrict__ counts, const int* __restrict__ mstart,
                                                           const int* __restrict__ mend, int N, int B, int S, int M1,
                                                           const int64_t* __restrict__ batch, const float* __restrict__ pos,
                                                           const float* __restrict__ forces, const uint8_t* __restrict__ fixed) {
  if (st.head[kHeadStatus]) return;  // frozen
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    // what the controller's blocks read of the header: block 0 of them rewrites the header itself while others may still start
    st.head[kLbCopyWord + kHeadStepLo] = st.head[kHeadStepLo];
    st.head[kLbCopyWord + kHeadStepHi] = st.head[kHeadStepHi];
    st.head[kLbCopyWord + kHeadFresh] = st.head[kHeadFresh];
  }
  if (counts && counts[2]) return;  // overflowed: stale forces, the controller latches it
  const int m = blockIdx.x, s = blockIdx.y;
  const bool fresh = st.head[kHeadFresh] != 0;
  const bool moved = !fresh && st.conv[m] < 0;  // a move preceded this evaluation: there is a candidate
  const int h = moved ? st.h[m] : 0;
  const int32_t* order = st.order + (int64_t)m * M1;
  const SliceRange r = mol_slice_range(counts, mstart, mend, N, S, batch, m, s);
  const int NP = 6 * M1 + 4;
  double* out = st.part + ((int64_t)m * S + s) * NP;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t = wave; t <= h; t += kLbDotsThreads / 64) {
    const bool last = t == h;
    const int a = moved ? order[t] : 0;  // the slot of this task (the last task: the spare slot)
    float* Sa = st.ringS + (int64_t)a * N * 3;
    float* Ya = st.ringY + (int64_t)a * N * 3;
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = r.i0 + lane; i < r.i1; i += 64) {
      if (slice_skips(r, batch, i, m)) continue;
      const int fx = fixed && fixed[i];
      float x[3], xp[3], f[3], fp[3], g[3], sc[3] = {0.f, 0.f, 0.f}, yc[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        f[d] = forces[i * 3 + d];
        g[d] = fx ? 0.f : -f[d];
      }
      if (moved) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          x[d] = pos[i * 3 + d];
          xp[d] = st.x_prev[i * 3 + d];
          fp[d] = st.f_prev[i * 3 + d];
        }
        tn_lbfgs::candidate(x, xp, f, fp, fx, sc, yc);
      }
      if (!last) {
        float sa[3], ya[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          sa[d] = Sa[i * 3 + d];
          ya[d] = Ya[i * 3 + d];
        }
        acc[0] += tn_lbfgs::dot3w(sc, sa);
        acc[1] += tn_lbfgs::dot3w(sc, ya);
        acc[2] += tn_lbfgs::dot3w(yc, sa);
        acc[3] += tn_lbfgs::dot3w(yc, ya);
        acc[4] += tn_lbfgs::dot3w(g, sa);
        acc[5] += tn_lbfgs::dot3w(g, ya);
      } else {
        if (moved) {
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            Sa[i * 3 + d] = sc[d];
            Ya[i * 3 + d] = yc[d];
          }
          acc[0] += tn_lbfgs::dot3w(sc, sc);
          acc[1] += tn_lbfgs::dot3w(sc, yc);
          acc[3] += tn_lbfgs::dot3w(yc, yc);
          acc[4] += tn_lbfgs::dot3w(g, sc);
          acc[5] += tn_lbfgs::dot3w(g, yc);
        }
        const double t_ff = tn_lbfgs::dot3w(g, g);
        acc[6] += t_ff;
        acc[7] = t_ff > acc[7] ? t_ff : acc[7];
      }
    }
    wave_reduce<8, 1u << 7>(acc);  // (per wave, not per block: a wave owns its task)
    if (lane == 0) {
      if (moved) {
        acc[2] = last ? acc[1] : acc[2];  // (y_c.s_c is s_c.y_c)
#pragma unroll
        for (int k = 0; k < 6; ++k) out[6 * a + k] = acc[k];
      }
      if (last) {
        out[6 * M1] = acc[6];
        out[6 * M1 + 1] = acc[7];
        out[6 * M1 + 2] = acc[0];  // s_c.s_c and y_c.y_c where the controller finds them without the ring (0: no candidate)
        out[6 * M1 + 3] = acc[3];
      }
    }
  }
}

struct LbCtlArgs {
  int B, S;
  tn_lbfgs::Params p;
  const int* counts;  // the graph's counters, or NULL
  const float* energy;
  float* epot_row;
  float* fmax_row;
  double* sums_row;       // [B, 4] ff, fmax2, s_c.y_c, g.p
  int32_t* pairs_row;     // [B]
  int32_t* accepted_row;  // [B]
  float* scale_row;       // [B] the clamp factor of the move that led to this evaluation
  int64_t* conv_row;      // [B]
  LbState st;
};

__device__ __forceinline__ tn_lbfgs::MolState lb_mol(const LbState& st, int m, int M1) {
  tn_lbfgs::MolState ms;
  ms.h = st.h + m;
  ms.order = st.order + (int64_t)m * M1;
  ms.conv = st.conv + m;
  ms.SS = st.SS + (int64_t)m * M1 * M1;
  ms.SY = st.SY + (int64_t)m * M1 * M1;
  ms.YY = st.YY + (int64_t)m * M1 * M1;
  return ms;
}

// One wave per molecule, kLbCtlWaves molecules per block, after k_lbfgs_dots.  Pass 1, by every block for ALL molecules: is a sum
// of a molecule that still moves unusable?  It reads only the slice sums (three squares per molecule, tn_lbfgs::usable) and
// converged_at, which a block changes only for a molecule whose sums are usable, so every block reaches the same answer and, when
// it is "yes", nothing is written but the status word (by block 0).  Pass 2: the slices added in slice order, then the molecule's
// history, coefficients and log rows.  Block 0 advances the step counter (the first control after a reset belongs to the start
// geometry and counts no step); the blocks read the copy of the header k_lbfgs_dots made.
__global__ __launch_bounds__(64 * kLbCtlWaves) void k_lbfgs_control(LbCtlArgs a) {
  extern __shared__ double lds[];
  const LbState& st = a.st;
  if (st.head[kHeadStatus]) return;  // frozen (or latched by block 0 a moment ago: the same outcome)
  if (a.counts && a.counts[2]) {
    if (blockIdx.x == 0 && threadIdx.x == 0) st.head[kHeadStatus] = 1u;
    return;
  }
  const bool fresh = st.head[kLbCopyWord + kHeadFresh] != 0;
  const uint64_t step = loop_step(st.head + kLbCopyWord) + (fresh ? 0 : 1);
  const int M1 = a.p.memory + 1, NP = 6 * M1 + 4;
  int flag = 0;
  for (int m = threadIdx.x; m < a.B; m += blockDim.x) {
    if (!fresh && st.conv[m] >= 0) continue;  // converged: not looked at
    const double* part = st.part + (int64_t)m * a.S * NP;
    double ff = 0.0, ss = 0.0, yy = 0.0;
    for (int k = 0; k < a.S; ++k) {
      ff += part[(int64_t)k * NP + 6 * M1];
      if (!fresh) {
        ss += part[(int64_t)k * NP + 6 * M1 + 2];
        yy += part[(int64_t)k * NP + 6 * M1 + 3];
      }
    }
    flag |= !(isfinite(ff) && isfinite(ss) && isfinite(yy));
  }
  if (__syncthreads_or(flag)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      st.head[kLbCauseWord] = 1u;
      st.head[kHeadStatus] = 2u;
    }
    return;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = blockIdx.x * kLbCtlWaves + wave;
  if (m < a.B) {
    const tn_lbfgs::MolState ms = lb_mol(st, m, M1);
    if (fresh) {  // the state a reset leaves: no pairs, the slots in order, not converged
      for (int q = lane; q < M1; q += 64) ms.order[q] = q;
      if (lane == 0) {
        *ms.h = 0;
        *ms.conv = -1;
      }
      tn_lbfgs::lane_sync();
    }
    const bool moved = !fresh && *ms.conv < 0;
    const int n = moved ? 6 * (*ms.h + 1) : 0;
    double* tot = st.tot + (int64_t)m * NP;
    const double* part = st.part + (int64_t)m * a.S * NP;
    for (int e = lane; e < n + 4; e += 64) {
      const int idx = e < n ? 6 * ms.order[e / 6] + e % 6 : 6 * M1 + (e - n);
      double v = 0.0;
      if (idx == 6 * M1 + 1) {
        for (int k = 0; k < a.S; ++k) v = part[(int64_t)k * NP + idx] > v ? part[(int64_t)k * NP + idx] : v;
      } else {
        for (int k = 0; k < a.S; ++k) v += part[(int64_t)k * NP + idx];
      }
      tot[idx] = v;
    }
    tn_lbfgs::lane_sync();
    double* delta = lds + (size_t)wave * lb_ctl_doubles(M1);
    double* av = delta + 2 * M1 + 1;
    int32_t* ord = reinterpret_cast<int32_t*>(av + M1);
    int32_t accepted;
    double gp;
    const int ret = tn_lbfgs::control(ms, a.p, tot, moved, (int64_t)step, delta, av, ord, &accepted, &gp);
    if (ret == tn_lbfgs::LBFGS_MOVING)
      for (int j = lane; j < 2 * M1 + 1; j += 64) st.delta[(int64_t)m * (2 * M1 + 1) + j] = delta[j];
    if (lane == 0) {
      if (a.energy && a.epot_row) a.epot_row[m] = a.energy[m];
      if (a.fmax_row) a.fmax_row[m] = (float)sqrt(tot[6 * M1 + 1]);
      if (a.sums_row) {
        a.sums_row[(int64_t)m * 4 + 0] = tot[6 * M1];
        a.sums_row[(int64_t)m * 4 + 1] = tot[6 * M1 + 1];
        // (the candidate's slot: the newest pair once accepted, the spare slot otherwise)
        a.sums_row[(int64_t)m * 4 + 2] = moved ? tot[6 * ms.order[*ms.h - accepted] + 1] : 0.0;
        a.sums_row[(int64_t)m * 4 + 3] = gp;
      }
      if (a.pairs_row) a.pairs_row[m] = *ms.h;
      if (a.accepted_row) a.accepted_row[m] = accepted;
      if (a.scale_row) a.scale_row[m] = fresh ? 0.f : st.cmove[m];
      if (a.conv_row) a.conv_row[m] = *ms.conv;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    loop_set_step(st.head, step);
    st.head[kHeadFresh] = 0u;
  }
}

// grid (B, S): the direction of every atom of slice s of molecule m from the coefficients, and the slice maximum of |p_i|^2
__global__ __launch_bounds__(kThreads) void k_lbfgs_direction(LbState st, const int* __restrict__ counts, const int* __restrict__ mstart,
                                                                const int* __restrict__ mend, int N, int B, int S, int M1,
                                                                const int64_t* __restrict__ batch, const float* __restrict__ forces,
                                                                const uint8_t* __restrict__ fixed, float* __restrict__ direction) {
  __shared__ double sh[1][kThreads / 64];
  if (st.head[kHeadStatus]) return;  // frozen (an overflow: the controller has just latched it)
  const int m = blockIdx.x, s = blockIdx.y;
  if (st.conv[m] >= 0) return;  // converged: it never moves again
  const int h = st.h[m];
  const int32_t* order = st.order + (int64_t)m * M1;
  const double* delta = st.delta + (int64_t)m * (2 * M1 + 1);
  const SliceRange r = mol_slice_range(counts, mstart, mend, N, S, batch, m, s);
  double mx[1] = {0.0};
  for (int i = r.i0 + (int)threadIdx.x; i < r.i1; i += kThreads) {
    if (slice_skips(r, batch, i, m)) continue;
    float f[3], p[3] = {0.f, 0.f, 0.f};
    if (!(fixed && fixed[i])) {
#pragma unroll
      for (int d = 0; d < 3; ++d) f[d] = forces[i * 3 + d];
      tn_lbfgs::atom_direction(f, h, order, M1, delta, st.ringS, st.ringY, N, i, p);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) direction[i * 3 + d] = p[d];
    const double n2 = tn_lbfgs::dot3w(p, p);
    mx[0] = n2 > mx[0] ? n2 : mx[0];
  }
  block_reduce_waves<1, 1u>(mx, sh);
  if (threadIdx.x == 0) st.dmax[(int64_t)m * S + s] = block_reduce_row(sh[0], true);
}

struct LbAtomArgs {
  int N, B, S;
  double max_step, damping;
  float* pos;
  const float* forces;
  float* forces_keep;
  const float* direction;
  const uint8_t* fixed;
  const int64_t* batch;
  const int* counts;  // the graph's counters, or NULL
  LbState st;
};

__device__ __forceinline__ float lb_scale(const LbAtomArgs& a, int64_t m) {
  double longest2 = 0.0;
  for (int k = 0; k < a.S; ++k) longest2 = a.st.dmax[m * a.S + k] > longest2 ? a.st.dmax[m * a.S + k] : longest2;
  return tn_lbfgs::clamp(longest2, a.max_step, a.damping);
}

// one thread per atom, the caller's atom order (and thread m < B keeps molecule m's clamp factor for the next controller's log row).  ACCEPT (after the
// controller): keep the forces of the evaluation, or, when it overflowed, go back to the positions the last move saved.  MOVE: save
// x and F, then x <- x + c p.
template <bool ACCEPT, bool MOVE>
__global__ __launch_bounds__(kThreads) void k_lbfgs_move(LbAtomArgs a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t status = a.st.head[kHeadStatus], fresh = a.st.head[kHeadFresh];
  if (status) {
    // the evaluation before this launch overflowed (the controller has just latched it): back to the last completed step.  A
    // later launch that finds the flag still set writes the same values again; nothing was ever saved before the first control.
    if (ACCEPT && status == 1u && !fresh && a.counts && a.counts[2] && i < a.N) {
#pragma unroll
      for (int d = 0; d < 3; ++d) a.pos[i * 3 + d] = a.st.x_prev[i * 3 + d];
    }
    return;
  }
  if (fresh) return;  // (OPEN straight after a reset: there is no direction yet)
  if (MOVE && i < a.B) a.st.cmove[i] = a.st.conv[i] >= 0 ? 0.f : lb_scale(a, i);  // (the next controller logs it)
  if (i >= a.N) return;
  float x[3], f[3], p[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) f[d] = a.forces[i * 3 + d];
  if (ACCEPT && a.forces_keep)
#pragma unroll
    for (int d = 0; d < 3; ++d) a.forces_keep[i * 3 + d] = f[d];
  if (MOVE) {
    const int64_t m = a.batch ? a.batch[i] : 0;
    if (m < 0 || m >= a.B) return;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      x[d] = a.pos[i * 3 + d];
      a.st.x_prev[i * 3 + d] = x[d];
      a.st.f_prev[i * 3 + d] = f[d];
    }
    if (a.st.conv[m] >= 0 || (a.fixed && a.fixed[i])) return;  // frozen: a branch, not a product with 0 - x keeps its bits
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] = a.direction[i * 3 + d];
    tn_lbfgs::atom_step(x, lb_scale(a, m), p);
#pragma unroll
    for (int d = 0; d < 3; ++d) a.pos[i * 3 + d] = x[d];
  }
}

__global__ void k_lbfgs_reset(LbState st, uint64_t step0) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    loop_head_reset(st.head, step0, kLbCauseWord);
  }
}

bool lb_sizes_ok(int64_t n_atoms, int64_t n_mol, int32_t memory) {
  if (n_atoms < 0 || n_atoms > INT32_MAX / 4 || n_mol < 0 || n_mol > INT32_MAX / 16 || memory < 1 || memory > tn_lbfgs::kMaxMemory) return false;
  return (double)(memory + 1) * (double)n_atoms * 3.0 < (double)INT64_MAX / 8.0;
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_lbfgs_workspace_bytes(int64_t n_atoms, int64_t n_mol, int32_t memory, size_t* bytes) {
  if (!bytes || !lb_sizes_ok(n_atoms, n_mol, memory)) return TMDNET_ERR_INVALID;
  size_t off[17];
  lb_layout(n_atoms, n_mol, memory, off);
  *bytes = off[16] + 256;  // + room to align the pointer
  return TMDNET_OK;
}

int tmdnet_lbfgs_layout(int64_t n_atoms, int64_t n_mol, int32_t memory, int64_t offsets[17]) {
  if (!offsets || !lb_sizes_ok(n_atoms, n_mol, memory)) return TMDNET_ERR_INVALID;
  size_t off[17];
  lb_layout(n_atoms, n_mol, memory, off);
  for (int k = 0; k < 17; ++k) offsets[k] = (int64_t)off[k];
  return TMDNET_OK;
}

int tmdnet_lbfgs_reset(void* stream, void* lbfgs_ws, uint64_t step0) {
  if (!lbfgs_ws) return TMDNET_ERR_INVALID;
  hipLaunchKernelGGL(k_lbfgs_reset, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), carve_lb(lbfgs_ws, 0, 0, 1), step0);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_lbfgs_advance(tmdnet_model* m, void* stream, void* graph_ws, void* lbfgs_ws, int64_t n_atoms, int64_t n_mol, int32_t phase,
                         float* pos, const float* forces, const float* energy, const uint8_t* fixed, const int64_t* batch,
                         float* forces_keep, float* direction, int32_t memory, double alpha, double max_step, double damping, double fmax,
                         float* epot_log_row, float* fmax_log_row, double* sums_log_row, int32_t* pairs_log_row,
                         int32_t* accepted_log_row, float* scale_log_row, int64_t* converged_log_row) {
  if (!lbfgs_ws || !pos || !forces || !direction || n_mol < 1 || !lb_sizes_ok(n_atoms, n_mol, memory)) return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MIN_OPEN && phase != TMDNET_MIN_MIDDLE && phase != TMDNET_MIN_CLOSE) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (!(fmax > 0.0) || !(alpha > 0.0) || !(max_step > 0.0) || !(damping > 0.0) || !std::isfinite(alpha) || !std::isfinite(max_step) ||
      !std::isfinite(damping))
    return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n_atoms, B = (int)n_mol, M1 = memory + 1;
  const LbState st = carve_lb(lbfgs_ws, n_atoms, n_mol, memory);
  const LoopGraph g = loop_graph(m, graph_ws, n_atoms, n_mol);
  const int* counts = g.counts;
  const dim3 block(kThreads);
  const int S = mol_slices(n_atoms, n_mol);
  if (phase != TMDNET_MIN_OPEN) {
    hipLaunchKernelGGL(k_lbfgs_dots, dim3(B, S), dim3(kLbDotsThreads), 0, s, st, counts, g.mstart, g.mend, N, B, S, M1, batch, pos, forces, fixed);
    LbCtlArgs c;
    c.B = B;
    c.S = S;
    c.p.alpha = alpha;
    c.p.max_step = max_step;
    c.p.damping = damping;
    c.p.fmax = fmax;
    c.p.memory = memory;
    c.counts = counts;
    c.energy = energy;
    c.epot_row = epot_log_row;
    c.fmax_row = fmax_log_row;
    c.sums_row = sums_log_row;
    c.pairs_row = pairs_log_row;
    c.accepted_row = accepted_log_row;
    c.scale_row = scale_log_row;
    c.conv_row = converged_log_row;
    c.st = st;
    const size_t per_wave = lb_ctl_doubles(M1) * sizeof(double);
    hipLaunchKernelGGL(k_lbfgs_control, dim3((B + kLbCtlWaves - 1) / kLbCtlWaves), dim3(64 * kLbCtlWaves), per_wave * kLbCtlWaves, s, c);
    hipLaunchKernelGGL(k_lbfgs_direction, dim3(B, S), block, 0, s, st, counts, g.mstart, g.mend, N, B, S, M1, batch, forces, fixed, direction);
  }
  {
    LbAtomArgs a;
    a.N = N;
    a.B = B;
    a.S = S;
    a.max_step = max_step;
    a.damping = damping;
    a.pos = pos;
    a.forces = forces;
    a.forces_keep = forces_keep;
    a.direction = direction;
    a.fixed = fixed;
    a.batch = batch;
    a.counts = counts;
    a.st = st;
    const int threads = N > B ? N : B;
    const dim3 grid((threads + kThreads - 1) / kThreads);
    if (phase == TMDNET_MIN_OPEN)
      hipLaunchKernelGGL((k_lbfgs_move<false, true>), grid, block, 0, s, a);
    else if (phase == TMDNET_MIN_MIDDLE)
      hipLaunchKernelGGL((k_lbfgs_move<true, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((k_lbfgs_move<true, false>), grid, block, 0, s, a);
  }
  return loop_launch_result(m, "tmdnet_lbfgs_advance");
}

int tmdnet_lbfgs_status(void* stream, void* lbfgs_ws, uint64_t host[3]) {
  if (!lbfgs_ws || !host) return TMDNET_ERR_INVALID;
  return loop_read_status(stream, carve_lb(lbfgs_ws, 0, 0, 1).head, kLbCauseWord + 1, kLbCauseWord, host, 3);
}

}  // extern "C"
