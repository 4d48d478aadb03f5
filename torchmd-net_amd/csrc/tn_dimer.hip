// Device-resident dimer saddle search: the kernels that sit between two energy+force evaluations of a captured step, so that K
// steps of a minimum-mode-following search replay as one HIP graph with no host work in between.  A dimer is three images of the
// same n atoms - the midpoint R0, R0 + delta N and R0 + delta M with a unit axis N and a unit partner M at a right angle - and a
// call has G dimers; rows are image-major, atom a of image i of dimer g is row (g 3 + i) n + a, and the evaluation sees 3 G molecules
// of n atoms.  The arithmetic is tn_dimer_math.h (rotation, curvature, inverted force, partner) and tn_min_math.h (FIRE, one
// controller per dimer).  The scheme is stated with the entries in include/tmdnet_amd.h.
//
// One step, after the energies E and forces F of the three images are known - four launches:
//   sums      grid (dimer, slice): N.HN, N.HM, M.HN, M.HM, F0.N, F0.M, the forces' squares and the number of atoms that are not
//             fixed                                                                    (fp32 terms, fp64 sums, fixed order)
//   project   grid (dimer, slice): every block derives its dimer's rotation from the slice sums, sums nu^2 over the rotated axis of
//             the WHOLE dimer slice by slice (every block of a dimer computes the same bits), writes the pending N', T and F_eff
//             of its slice into the workspace and reduces the FIRE terms and the partner's six sums
//   control   ONE block, dimers strided: the slice sums added in slice order, the partner's coefficients, tn_dimer::dimer_fire, the
//             status word, the logs
//   atoms     per atom of a dimer (its three rows): accept (N', M', F_eff, F0 -> the caller's buffers, or the saved state back
//             after an overflow) and, in MIDDLE, the move of R0 and the rewrite of the three images from R0, N and M
// CLOSE omits the move, OPEN is the move alone from the coefficients the workspace holds and the kept F_eff.
//
// Reductions are tn_loop.h's, as in k_min_reduce.  No floating-point atomics: repeats are bit-identical.  Overflow, non-finite sums
// and unusable modes follow the minimiser's protocol: the controller is the only kernel that writes the status word; an overflowed
// evaluation latches status 1 and the per-atom kernel puts x and v back; a dimer that still moves and has an energy or a force sum
// that is not finite, or a mode without length, latches status 2 (the cause in header word 5) before anything of that step is
// accepted.  From then on every launch returns at once until tmdnet_dimer_reset.
#include <cmath>

#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_dimer_math.h"
#include "tn_loop.h"
#include "tn_model.h"

namespace tn {

namespace {

using namespace tn_dimer;

// The header: six uint32 words, then two doubles.  Words 0 / 1 the step counter (lo / hi), 2 the status, 3 "reset, not yet controlled",
constexpr int kDimerTranslateWord = 4;  // 1: the midpoint moves; 0: a mode search
constexpr int kDimerCauseWord = 5;      // which input was unusable when status 2 was latched (tn_dimer::DIMER_*)
constexpr int kDimerHeadWords = 6;      // words the status entry reads back
constexpr size_t kDimerStartByte = 32;  // dt0, alpha0 (fp64)
static_assert(kDimerTranslateWord > 3 && kDimerCauseWord != kDimerTranslateWord && kDimerCauseWord < kDimerHeadWords,
              "header words must not overlap");
static_assert(kDimerHeadWords * sizeof(uint32_t) <= kDimerStartByte && kDimerStartByte % sizeof(double) == 0 &&
                  kDimerStartByte + 2 * sizeof(double) <= kHeaderBytes,
              "the start values lie behind the header words, aligned, inside the header");

constexpr int kRec = 9;                // a, b, c, co, si, nu^2, C, p, |T| of a dimer's last controlled step
constexpr int kPartSlice = 4 + N_PART;  // vf, ff, vv, fmax2, then the partner sums

struct DimerState {  // views into the caller's workspace
  uint32_t* head;      // [0] step lo, [1] step hi, [2] status, [3] 1 = reset, not yet controlled, [4] translate, [5] cause of status 2
  double* start;       // [0] dt0, [1] alpha0
  double* dt;          // [G]
  double* alpha;       // [G]
  int64_t* conv;       // [G] converged_at
  int32_t* n_pos;      // [G]
  float* coef;         // [G, 3] c_v, c_f, d of the next move
  float* mcoef;        // [G, N_COEF] the mode's coefficients
  double* rec;         // [G, kRec]
  double* msums;       // [G, N_SUMS]
  double* psums;       // [G, N_PART]
  int32_t* why;        // [G] tn_dimer::DIMER_*
  double* sum_slices;  // [G, S, N_SUMS]
  double* part_slices; // [G, S, kPartSlice]
  float* x_keep;       // [G n, 3] R0 before the last move
  float* v_keep;       // [G n, 3]
  float* f_eff;        // [G n, 3] F_eff of the evaluation being controlled
  float* n_new;        // [G n, 3] the pending axis N'
  float* t_new;        // [G n, 3] the pending residual T
};

DimerState dimer_layout(LoopCarver& c, int64_t n, int64_t G) {
  const size_t g = (size_t)(G > 0 ? G : 0), N = g * (size_t)(n > 0 ? n : 0);
  const size_t S = (size_t)mol_slices(n, 1);  // slices per dimer: one image is the molecule
  DimerState st;
  st.head = c.take<uint32_t>(kHeaderBytes / sizeof(uint32_t));
  st.start = reinterpret_cast<double*>(reinterpret_cast<char*>(st.head) + kDimerStartByte);
  st.dt = c.take<double>(g);
  st.alpha = c.take<double>(g);
  st.conv = c.take<int64_t>(g);
  st.n_pos = c.take<int32_t>(g);
  st.coef = c.take<float>(g * 3);
  st.mcoef = c.take<float>(g * N_COEF);
  st.rec = c.take<double>(g * kRec);
  st.msums = c.take<double>(g * N_SUMS);
  st.psums = c.take<double>(g * N_PART);
  st.why = c.take<int32_t>(g);
  st.sum_slices = c.take<double>(g * S * N_SUMS);
  st.part_slices = c.take<double>(g * S * kPartSlice);
  st.x_keep = c.take<float>(N * 3);
  st.v_keep = c.take<float>(N * 3);
  st.f_eff = c.take<float>(N * 3);
  st.n_new = c.take<float>(N * 3);
  st.t_new = c.take<float>(N * 3);
  return st;
}

size_t dimer_bytes(int64_t n, int64_t G) {
  return layout_bytes([&](LoopCarver& c) { dimer_layout(c, n, G); });
}

DimerState carve_dimer(void* ws, int64_t n, int64_t G) {
  LoopCarver c(ws);
  return dimer_layout(c, n, G);
}

struct DimerGeom {
  int n, G, S;
  float dl, inv;  // fp32(delta), fp32(1 / delta)
};

struct DimerIn {  // what the two grid kernels read
  const int* counts;  // the graph's counters, or NULL
  const float* vel;     // [G n, 3]
  const float* mode;    // [G n, 3]
  const float* partner; // [G n, 3]
  const float* forces;  // [3 G n, 3]
  const float* energy;  // [3 G]
  const uint8_t* fixed; // [n] or NULL
};

// the six vectors of atom a of dimer g
__device__ __forceinline__ void dimer_load(const DimerIn& in, const DimerGeom& g, int d, int a, float N[3], float M[3], float f0[3],
                                           float f1[3], float f2[3]) {
  const int64_t r = (int64_t)d * g.n + a, r0 = ((int64_t)d * 3) * g.n + a;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    N[k] = in.mode[r * 3 + k];
    M[k] = in.partner[r * 3 + k];
    f0[k] = in.forces[r0 * 3 + k];
    f1[k] = in.forces[(r0 + g.n) * 3 + k];
    f2[k] = in.forces[(r0 + 2 * (int64_t)g.n) * 3 + k];
  }
}

__device__ __forceinline__ bool dimer_live(const DimerState& st, int d) { return st.head[kHeadFresh] != 0 || st.conv[d] < 0; }

// grid (G, S): slice s of dimer d -> sum_slices[d, s, 0..N_SUMS)
__global__ __launch_bounds__(kThreads) void k_dimer_sums(DimerState st, DimerGeom g, DimerIn in) {
  __shared__ double sh[N_SUMS][kThreads / 64];
  if (st.head[kHeadStatus]) return;                 // frozen
  if (in.counts && in.counts[2]) return;  // overflowed: stale forces, the controller latches it
  const int d = blockIdx.x, s = blockIdx.y;
  if (!dimer_live(st, d)) return;  // a dimer that has converged looks at nothing
  const int a0 = (int)((int64_t)g.n * s / g.S), a1 = (int)((int64_t)g.n * (s + 1) / g.S);
  double acc[N_SUMS];
#pragma unroll
  for (int k = 0; k < N_SUMS; ++k) acc[k] = 0.0;
  for (int a = a0 + (int)threadIdx.x; a < a1; a += kThreads) {
    const int fx = in.fixed && in.fixed[a];
    float N[3], M[3], f0[3], f1[3], f2[3], t[7];
    dimer_load(in, g, d, a, N, M, f0, f1, f2);
    sum_terms(N, M, f0, f1, f2, g.inv, fx, t);
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] += (double)t[k];
    acc[S_FREE] += fx ? 0.0 : 1.0;  // (a count: exact)
  }
  block_reduce_waves<N_SUMS, 0u>(acc, sh);
  if (threadIdx.x == 0) block_reduce_rows<N_SUMS, 0u>(sh, st.sum_slices + ((int64_t)d * g.S + s) * N_SUMS);
}

// grid (G, S), after k_dimer_sums: the dimer's rotation and coefficients (every block of the dimer computes the same bits; the block
// of slice 0 records them), N', T and F_eff of the slice's atoms into the workspace, part_slices[d, s, ...] = the FIRE terms of F_eff
// and the partner sums
__global__ __launch_bounds__(kThreads) void k_dimer_project(DimerState st, DimerGeom g, DimerIn in) {
  __shared__ double sh[kPartSlice][kThreads / 64];
  __shared__ double shn[1][kThreads / 64];
  if (st.head[kHeadStatus]) return;
  if (in.counts && in.counts[2]) return;
  const int d = blockIdx.x, s = blockIdx.y;
  if (!dimer_live(st, d)) return;
  double S[N_SUMS], q[3], co, si, C, p;
#pragma unroll
  for (int j = 0; j < N_SUMS; ++j) S[j] = 0.0;
  const double* sl = st.sum_slices + (int64_t)d * g.S * N_SUMS;
  for (int k = 0; k < g.S; ++k)
#pragma unroll
    for (int j = 0; j < N_SUMS; ++j) S[j] += sl[k * N_SUMS + j];
  const int has_free = S[S_FREE] > 0.0;
  int branch;
  int why = mode_rotation(S, in.energy + (int64_t)d * 3, has_free, q, &co, &si, &branch);
  // nu^2 = |co N + si M|^2 over the whole dimer, from the vectors in fp64: slice by slice in the order every other sum is added in
  double nu2 = 0.0;
  if (!why && has_free) {
    for (int k = 0; k < g.S; ++k) {
      const int b0 = (int)((int64_t)g.n * k / g.S), b1 = (int)((int64_t)g.n * (k + 1) / g.S);
      double acc[1] = {0.0};
      for (int a = b0 + (int)threadIdx.x; a < b1; a += kThreads) {
        if (in.fixed && in.fixed[a]) continue;
        const int64_t r = (int64_t)d * g.n + a;
        float N[3], M[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          N[j] = in.mode[r * 3 + j];
          M[j] = in.partner[r * 3 + j];
        }
        acc[0] += nu2_term(N, M, co, si);
      }
      block_reduce_waves<1, 0u>(acc, shn);
      nu2 += block_reduce_row(shn[0], false);
      __syncthreads();  // (shn is written again by the next slice)
    }
  }
  float coef[N_COEF];
#pragma unroll
  for (int j = 0; j < N_COEF; ++j) coef[j] = 0.f;
  if (!why) why = mode_coef(q, S, co, si, nu2, has_free, coef, &C, &p);
  if (why) C = p = 0.0;
  if (s == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < N_SUMS; ++j) st.msums[(int64_t)d * N_SUMS + j] = S[j];
#pragma unroll
    for (int j = 0; j <= C_SI; ++j) st.mcoef[(int64_t)d * N_COEF + j] = coef[j];
    double* rec = st.rec + (int64_t)d * kRec;
    rec[0] = q[0];
    rec[1] = q[1];
    rec[2] = q[2];
    rec[3] = co;
    rec[4] = si;
    rec[5] = nu2;
    rec[6] = C;
    rec[7] = p;
    st.why[d] = why;
  }
  const int a0 = (int)((int64_t)g.n * s / g.S), a1 = (int)((int64_t)g.n * (s + 1) / g.S);
  double acc[kPartSlice];
#pragma unroll
  for (int k = 0; k < kPartSlice; ++k) acc[k] = 0.0;
  for (int a = a0 + (int)threadIdx.x; a < a1; a += kThreads) {
    const int64_t r = (int64_t)d * g.n + a;
    const int fx = in.fixed && in.fixed[a];
    float N[3], M[3], f0[3], f1[3], f2[3], np[3], t[3], fe[3], v[3], pt[N_PART], ft[3];
    dimer_load(in, g, d, a, N, M, f0, f1, f2);
    project_atom(N, M, f0, f1, f2, g.inv, coef, fx, np, t, fe, pt);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = in.vel[r * 3 + k];
      st.n_new[r * 3 + k] = np[k];
      st.t_new[r * 3 + k] = t[k];
      st.f_eff[r * 3 + k] = fe[k];
    }
    tn_min::atom_terms(v, fe, fx, ft);
    acc[0] += (double)ft[0];
    acc[1] += (double)ft[1];
    acc[2] += (double)ft[2];
    acc[3] = (double)ft[1] > acc[3] ? (double)ft[1] : acc[3];
#pragma unroll
    for (int k = 0; k < N_PART; ++k) acc[4 + k] += (double)pt[k];
  }
  block_reduce_waves<kPartSlice, 8u>(acc, sh);
  if (threadIdx.x == 0) block_reduce_rows<kPartSlice, 8u>(sh, st.part_slices + ((int64_t)d * g.S + s) * kPartSlice);
}

struct DimerCtlArgs {
  DimerGeom g;
  tn_min::FireParams p;
  const int* counts;  // the graph's counters, or NULL
  const float* energy;
  FireRows rows;        // [G, ...]
  double* curv_row;     // [G]
  double* rot_row;      // [G, 2]
  double* resid_row;    // [G]
  double* quad_row;     // [G, 3]
  double* msums_row;    // [G, N_SUMS + 1 + N_PART]
  float* mcoef_row;     // [G, N_COEF]
  DimerState st;
};

// the sums of dimer d in slice order (FIRE's four, then the partner's), and its state (after a reset: the start values of the header)
__device__ __forceinline__ void dimer_ctl_load(const DimerCtlArgs& a, int d, bool fresh, double sums[kPartSlice], tn_min::FireState* s) {
  slice_sums<kPartSlice, 8u>(a.st.part_slices + (int64_t)d * a.g.S * kPartSlice, a.g.S, kPartSlice, sums);
  fire_load(fire_units(a.st), d, fresh, s);
}

// ONE block striding the dimers, after k_dimer_project: optimiser_control (tn_loop.h) with FIRE's two passes on F_eff and the
// projection's causes
__global__ __launch_bounds__(kThreads) void k_dimer_control(DimerCtlArgs a) {
  const int translate = a.st.head[kDimerTranslateWord] != 0;  // (no controller writes this word)
  optimiser_control(
      a.st.head, a.counts, kDimerCauseWord, true, a.g.G,
      [&](int d, bool fresh, uint64_t step) {
        double sums[kPartSlice];
        float coef[3];
        tn_min::FireState s;
        dimer_ctl_load(a, d, fresh, sums, &s);
        if (s.converged_at >= 0) return 0;  // a dimer that has converged looks at nothing
        int c = a.st.why[d];
        const int has_free = a.st.msums[(int64_t)d * N_SUMS + S_FREE] > 0.0;
        if (!c && dimer_fire(&s, a.p, sums, a.st.rec[(int64_t)d * kRec + 6], translate, has_free, (int64_t)step, coef) == tn_min::FIRE_UNUSABLE)
          c = DIMER_BAD_SUMS;
        return c;
      },
      [&](int d, bool fresh, uint64_t step) {
        double sums[kPartSlice];
        const double* P = sums + 4;
        float coef[3];
        tn_min::FireState s;
        dimer_ctl_load(a, d, fresh, sums, &s);
        double* rec = a.st.rec + (int64_t)d * kRec;
        float* mc = a.st.mcoef + (int64_t)d * N_COEF;
        if (s.converged_at < 0) {  // (a dimer that had converged keeps the records of the step it converged at)
          const int has_free = a.st.msums[(int64_t)d * N_SUMS + S_FREE] > 0.0;
          partner_coef(P, has_free, mc, &rec[8]);
#pragma unroll
          for (int k = 0; k < N_PART; ++k) a.st.psums[(int64_t)d * N_PART + k] = P[k];
          dimer_fire(&s, a.p, sums, rec[6], translate, has_free, (int64_t)step, coef);
        } else {
          coef[0] = coef[1] = coef[2] = 0.f;
        }
        fire_store(fire_units(a.st), d, s, coef);
        a.rows.write(d, a.energy + (int64_t)d * 3, sums, sums[3], coef, s);
        if (a.curv_row) a.curv_row[d] = rec[6];
        if (a.rot_row) {
          a.rot_row[(int64_t)d * 2 + 0] = rec[3];
          a.rot_row[(int64_t)d * 2 + 1] = rec[4];
        }
        if (a.resid_row) a.resid_row[d] = rec[8];
        if (a.quad_row)
#pragma unroll
          for (int k = 0; k < 3; ++k) a.quad_row[(int64_t)d * 3 + k] = rec[k];
        if (a.msums_row) {
          double* row = a.msums_row + (int64_t)d * (N_SUMS + 1 + N_PART);
#pragma unroll
          for (int k = 0; k < N_SUMS; ++k) row[k] = a.st.msums[(int64_t)d * N_SUMS + k];
          row[N_SUMS] = rec[5];
#pragma unroll
          for (int k = 0; k < N_PART; ++k) row[N_SUMS + 1 + k] = a.st.psums[(int64_t)d * N_PART + k];
        }
        if (a.mcoef_row)
#pragma unroll
          for (int k = 0; k < N_COEF; ++k) a.mcoef_row[(int64_t)d * N_COEF + k] = mc[k];
      });
}

struct DimerAtomArgs {
  DimerGeom g;
  int64_t N;  // G n
  float* pos;      // [3 G n, 3]
  float* vel;      // [G n, 3]
  float* mode;     // [G n, 3]
  float* partner;  // [G n, 3]
  const float* forces;  // ACCEPT: the evaluation's [3 G n, 3]; OPEN: the kept F_eff [G n, 3]
  float* forces_keep;       // [G n, 3] F_eff
  float* true_forces_keep;  // [G n, 3] F0
  const uint8_t* fixed;
  const int* counts;  // the graph's counters, or NULL
  DimerState st;
};

// One thread per atom of a dimer, which owns the atom's three rows.  ACCEPT (after k_dimer_control): take N', M', F_eff and F0 of the
// evaluation, or, when it overflowed, go back to the midpoint the last move saved.  MOVE: save x and v, the update of R0 with the
// dimer's coefficients (ACCEPT: on the F_eff just made, else on `forces`).  Every launch ends with images 1 and 2 rewritten from R0, N
// and M, so the position buffer is always R0, R0 + delta N, R0 + delta M.
template <bool ACCEPT, bool MOVE>
__global__ __launch_bounds__(kThreads) void k_dimer_atoms(DimerAtomArgs a) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.N) return;
  const int d = (int)(r / a.g.n), atom = (int)(r - (int64_t)d * a.g.n);
  const int64_t r0 = ((int64_t)d * 3) * a.g.n + atom, r1 = r0 + a.g.n, r2 = r1 + a.g.n;
  const uint32_t status = a.st.head[kHeadStatus], fresh = a.st.head[kHeadFresh];
  float x[3], v[3], f[3], N[3], M[3], xi[3];
  if (status) {
    if (ACCEPT && status == 1u && !fresh && a.counts && a.counts[2]) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        x[k] = a.st.x_keep[r * 3 + k];
        N[k] = a.mode[r * 3 + k];
        M[k] = a.partner[r * 3 + k];
        a.pos[r0 * 3 + k] = x[k];
        a.vel[r * 3 + k] = a.st.v_keep[r * 3 + k];
      }
      image_pos(x, a.g.dl, N, xi);
#pragma unroll
      for (int k = 0; k < 3; ++k) a.pos[r1 * 3 + k] = xi[k];
      image_pos(x, a.g.dl, M, xi);
#pragma unroll
      for (int k = 0; k < 3; ++k) a.pos[r2 * 3 + k] = xi[k];
    }
    return;
  }
  if (fresh) return;  // (OPEN straight after a reset: there are no coefficients yet)
  const int fx = a.fixed && a.fixed[atom];
  const int64_t conv = a.st.conv[d];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    N[k] = a.mode[r * 3 + k];
    M[k] = a.partner[r * 3 + k];
    f[k] = ACCEPT ? a.st.f_eff[r * 3 + k] : a.forces[r * 3 + k];
  }
  if (ACCEPT && (conv < 0 || conv == (int64_t)loop_step(a.st.head))) {  // (a dimer that converged at an earlier step keeps everything)
    float np[3], t[3], nn[3], mn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      np[k] = a.st.n_new[r * 3 + k];
      t[k] = a.st.t_new[r * 3 + k];
    }
    accept_atom(N, M, np, t, a.st.mcoef + (int64_t)d * N_COEF, fx, nn, mn);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      N[k] = nn[k];
      M[k] = mn[k];
      a.mode[r * 3 + k] = N[k];
      a.partner[r * 3 + k] = M[k];
      if (a.forces_keep) a.forces_keep[r * 3 + k] = f[k];
      if (a.true_forces_keep) a.true_forces_keep[r * 3 + k] = a.forces[r0 * 3 + k];
    }
  }
  if (MOVE) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[k] = a.pos[r0 * 3 + k];
      v[k] = a.vel[r * 3 + k];
      a.st.x_keep[r * 3 + k] = x[k];
      a.st.v_keep[r * 3 + k] = v[k];
    }
    if (conv >= 0 || fx || !a.st.head[kDimerTranslateWord]) {  // a branch: x keeps its bits
#pragma unroll
      for (int k = 0; k < 3; ++k) a.vel[r * 3 + k] = 0.f;
    } else {
      tn_min::atom_move(x, v, f, a.st.coef[d * 3 + 0], a.st.coef[d * 3 + 1], a.st.coef[d * 3 + 2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a.pos[r0 * 3 + k] = x[k];
        a.vel[r * 3 + k] = v[k];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = a.pos[r0 * 3 + k];
  }
  // the images follow R0, N and M at every launch (a frozen dimer: the same bits again)
  image_pos(x, a.g.dl, N, xi);
#pragma unroll
  for (int k = 0; k < 3; ++k) a.pos[r1 * 3 + k] = xi[k];
  image_pos(x, a.g.dl, M, xi);
#pragma unroll
  for (int k = 0; k < 3; ++k) a.pos[r2 * 3 + k] = xi[k];
}

__global__ void k_dimer_reset(DimerState st, uint64_t step0, double dt0, double alpha0, uint32_t translate) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    loop_head_reset(st.head, step0, kDimerCauseWord);
    st.head[kDimerTranslateWord] = translate;
    st.start[0] = dt0;
    st.start[1] = alpha0;
  }
}

bool dimer_shape_ok(int64_t n, int64_t G) {
  if (n < 0 || G < 1 || G > INT32_MAX / 64) return false;
  return n == 0 || G <= (INT32_MAX / 16) / n;  // 3 G n rows of 3 floats stay below 2^31
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_dimer_workspace_bytes(int64_t n_atoms_per_image, int64_t n_dimers, size_t* bytes) {
  if (!bytes || !dimer_shape_ok(n_atoms_per_image, n_dimers)) return TMDNET_ERR_INVALID;
  *bytes = dimer_bytes(n_atoms_per_image, n_dimers);
  return TMDNET_OK;
}

int tmdnet_dimer_reset(void* stream, void* dimer_ws, uint64_t step0, double dt0, double alpha0, int32_t translate) {
  if (!dimer_ws || !(dt0 > 0.0) || !(alpha0 >= 0.0) || (translate != 0 && translate != 1)) return TMDNET_ERR_INVALID;
  hipLaunchKernelGGL(k_dimer_reset, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), carve_dimer(dimer_ws, 0, 0), step0, dt0,
                     alpha0, (uint32_t)translate);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_dimer_advance(tmdnet_model* m, void* stream, void* graph_ws, void* dimer_ws, int64_t n_atoms_per_image, int64_t n_dimers,
                         int32_t phase, float* pos, float* vel, float* mode, float* partner, const float* forces, const float* energy,
                         const uint8_t* fixed, float* forces_keep, float* true_forces_keep, double dt_max, int32_t n_min, double f_inc,
                         double f_dec, double alpha0, double f_alpha, double max_step, double fmax, double delta, float* epot_log_row,
                         float* fmax_log_row, double* sums_log_row, float* coef_log_row, double* dt_log_row, double* alpha_log_row,
                         int64_t* converged_log_row, double* curvature_log_row, double* rotation_log_row, double* residual_log_row,
                         double* quad_log_row, double* mode_sums_log_row, float* mode_coef_log_row) {
  if (!dimer_ws || !pos || !vel || !mode || !partner || !forces || !dimer_shape_ok(n_atoms_per_image, n_dimers)) return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MIN_OPEN && phase != TMDNET_MIN_MIDDLE && phase != TMDNET_MIN_CLOSE) return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MIN_OPEN && !energy) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (!(fmax > 0.0) || !(dt_max > 0.0) || !(max_step > 0.0) || !(f_inc > 0.0) || !(f_dec > 0.0) || !(f_alpha > 0.0) || !(alpha0 >= 0.0) ||
      n_min < 0 || !(delta > 0.0) || !std::isfinite(delta))
    return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DimerGeom g;
  g.n = (int)n_atoms_per_image;
  g.G = (int)n_dimers;
  g.S = mol_slices(n_atoms_per_image, 1);
  g.dl = (float)delta;
  g.inv = (float)(1.0 / delta);
  const int64_t n_img = 3 * n_dimers, N = n_dimers * n_atoms_per_image;
  const DimerState st = carve_dimer(dimer_ws, n_atoms_per_image, n_dimers);
  const int* counts = loop_graph(m, graph_ws, 3 * N, n_img).counts;
  const dim3 block(kThreads);
  if (phase != TMDNET_MIN_OPEN) {
    DimerIn in;
    in.counts = counts;
    in.vel = vel;
    in.mode = mode;
    in.partner = partner;
    in.forces = forces;
    in.energy = energy;
    in.fixed = fixed;
    const dim3 grid((unsigned)n_dimers, (unsigned)g.S);
    hipLaunchKernelGGL(k_dimer_sums, grid, block, 0, s, st, g, in);
    hipLaunchKernelGGL(k_dimer_project, grid, block, 0, s, st, g, in);
    DimerCtlArgs c;
    c.g = g;
    c.p.dt_max = dt_max;
    c.p.f_inc = f_inc;
    c.p.f_dec = f_dec;
    c.p.alpha0 = alpha0;
    c.p.f_alpha = f_alpha;
    c.p.max_step = max_step;
    c.p.fmax = fmax;
    c.p.n_min = n_min;
    c.counts = counts;
    c.energy = energy;
    c.rows = {epot_log_row, fmax_log_row, sums_log_row, coef_log_row, dt_log_row, alpha_log_row, converged_log_row};
    c.curv_row = curvature_log_row;
    c.rot_row = rotation_log_row;
    c.resid_row = residual_log_row;
    c.quad_row = quad_log_row;
    c.msums_row = mode_sums_log_row;
    c.mcoef_row = mode_coef_log_row;
    c.st = st;
    hipLaunchKernelGGL(k_dimer_control, dim3(1), block, 0, s, c);
  }
  if (N > 0) {
    DimerAtomArgs a;
    a.g = g;
    a.N = N;
    a.pos = pos;
    a.vel = vel;
    a.mode = mode;
    a.partner = partner;
    a.forces = forces;
    a.forces_keep = forces_keep;
    a.true_forces_keep = true_forces_keep;
    a.fixed = fixed;
    a.counts = counts;
    a.st = st;
    const dim3 grid((unsigned)((N + kThreads - 1) / kThreads));
    if (phase == TMDNET_MIN_OPEN)
      hipLaunchKernelGGL((k_dimer_atoms<false, true>), grid, block, 0, s, a);
    else if (phase == TMDNET_MIN_MIDDLE)
      hipLaunchKernelGGL((k_dimer_atoms<true, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((k_dimer_atoms<true, false>), grid, block, 0, s, a);
  }
  return loop_launch_result(m, "tmdnet_dimer_advance");
}

int tmdnet_dimer_status(void* stream, void* dimer_ws, uint64_t host[3]) {
  if (!dimer_ws || !host) return TMDNET_ERR_INVALID;
  return loop_read_status(stream, carve_dimer(dimer_ws, 0, 0).head, kDimerHeadWords, kDimerCauseWord, host, 3);
}

}  // extern "C"
