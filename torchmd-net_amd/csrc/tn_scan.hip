// Device-resident relaxed coordinate scan: the kernels that sit between two energy+force evaluations of a captured step, so that K
// steps of a constrained FIRE minimisation replay as one HIP graph with no host work in between.  A call has G points, each a copy of
// the same n atoms (atom a of point g is row g n + a) with its own targets for the D <= 4 CVs all points share.  The arithmetic is
// tn_scan_math.h (multipliers, corrections, drive, constraint step), tn_bias_math.h (the CVs) and tn_min_math.h (FIRE, one
// controller per point).  The scheme is stated with the entries in include/tmdnet_amd.h.
//
// One step, after the energies E and forces F are known - four launches:
//   project   grid (point, slice): every block forms its point's CVs, gradients, lambda, mu and the corrections of the <= 16 CV atoms
//             itself (one lane, fp64, the same bits in every block; the block of slice 0 records them), then reduces FIRE's terms of
//             F_perp and v_perp over its slice
//   control   ONE block, points strided: the slice sums added in slice order, tn_scan::scan_fire, the status word, the logs
//   atoms     per atom: accept (F, F_perp and v_perp into the caller's buffers, or the saved state back) and, in MIDDLE, the move
//   constrain one wave per point, MIDDLE and OPEN only: the drive of the targets, then the Gauss-Newton constraint step on the moved
//             positions of the CV atoms.  It has a launch of its own: it must see the moved positions of all of a point's CV atoms,
//             and the four launches fit the budget of 4 K + 1 per replay.
// CLOSE omits the move and the constraint step, OPEN is those two alone from what the workspace and the kept F_perp hold.
//
// Reductions are tn_loop.h's, as in k_min_reduce.  No floating-point atomics: repeats are bit-identical.  Overflow, restore and
// status follow the minimiser's protocol: the controller is the only kernel that writes the status word.  A point that still moves
// and has a sum that is not finite (cause 1), a CV or gradient that is not finite (2), a Gram matrix that is not positive definite
// (3) or a constraint step that did not converge (4) latches status 2 with the cause in header word 4.  The constraint step runs
// after the move, so it only flags its point in the workspace; the controller of the next step latches it before anything of that step
// is accepted, and the per-atom kernel puts back the x and v the move had saved.
// The fp64 statements of a point must give the host checker's bits: no product is contracted into the sum that consumes it.
#pragma clang fp contract(off)
#include <cmath>

#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_loop.h"
#include "tn_model.h"
#include "tn_scan_math.h"

namespace tn {

namespace {

using namespace tn_scan;

// The header: words 0 / 1 the step counter (lo / hi), 2 the status, 3 "reset, not yet controlled", 4 the cause of status 2; then the
// start values dt0, alpha0 (fp64) at byte 32.
constexpr int kScanCauseWord = 4;
constexpr int kScanHeadWords = 5;
constexpr size_t kScanStartByte = 32;
static_assert(kScanHeadWords * sizeof(uint32_t) <= kScanStartByte && kScanStartByte + 2 * sizeof(double) <= kHeaderBytes,
              "the start values lie behind the header words, inside the header");

struct ScanState {  // views into the caller's workspace
  uint32_t* head;
  double* start;     // [0] dt0, [1] alpha0
  double* dt;        // [G]
  double* alpha;     // [G]
  int64_t* conv;     // [G] converged_at
  int32_t* n_pos;    // [G]
  float* coef;       // [G, 3] c_v, c_f, d of the next move
  int32_t* why;      // [G] what the projection found (SCAN_*)
  int32_t* why2;     // [G] what the last constraint step found
  double* t_cur;     // [G, 4] the targets the positions are constrained to
  double* cv;        // [G, 4] the CVs at the evaluation being controlled
  float* mult;       // [G, 8] lambda, mu
  float* corr;       // [G, 16, 2, 3] the corrections of F and v on the CV atoms
  double* slices;    // [G, S, 4] vf, ff, vv, fmax2
  float* x_keep;     // [G n, 3] positions before the last move
  float* v_keep;     // [G n, 3]
};

ScanState scan_layout(LoopCarver& c, int64_t n, int64_t G) {
  const size_t g = (size_t)(G > 0 ? G : 0), N = g * (size_t)(n > 0 ? n : 0);
  const size_t S = (size_t)mol_slices(n, 1);
  ScanState st;
  st.head = c.take<uint32_t>(kHeaderBytes / sizeof(uint32_t));
  st.start = reinterpret_cast<double*>(reinterpret_cast<char*>(st.head) + kScanStartByte);
  st.dt = c.take<double>(g);
  st.alpha = c.take<double>(g);
  st.conv = c.take<int64_t>(g);
  st.n_pos = c.take<int32_t>(g);
  st.coef = c.take<float>(g * 3);
  st.why = c.take<int32_t>(g);
  st.why2 = c.take<int32_t>(g);
  st.t_cur = c.take<double>(g * kMaxCv);
  st.cv = c.take<double>(g * kMaxCv);
  st.mult = c.take<float>(g * 2 * kMaxCv);
  st.corr = c.take<float>(g * kMaxAtoms * 6);
  st.slices = c.take<double>(g * S * 4);
  st.x_keep = c.take<float>(N * 3);
  st.v_keep = c.take<float>(N * 3);
  return st;
}

size_t scan_bytes(int64_t n, int64_t G) {
  return layout_bytes([&](LoopCarver& c) { scan_layout(c, n, G); });
}

ScanState carve_scan(void* ws, int64_t n, int64_t G) {
  LoopCarver c(ws);
  return scan_layout(c, n, G);
}

struct ScanGeom {
  int n, G, S;
};

__device__ __forceinline__ bool scan_live(const ScanState& st, int g) { return st.head[kHeadFresh] != 0 || st.conv[g] < 0; }

// the distinct CV atom that `atom` is, or -1
__device__ __forceinline__ int scan_find(const Tables& T, int atom) {
  int j = -1;
  for (int a = 0; a < T.A; ++a) j = T.atom_rel[a] == atom ? a : j;
  return j;
}

struct ScanProjectArgs {
  ScanGeom g;
  Tables T;
  const int* counts;  // the graph's counters, or NULL
  const float* pos;     // [G n, 3]
  const float* vel;     // [G n, 3]
  const float* forces;  // [G n, 3]
  const uint8_t* fixed; // [n] or NULL
  ScanState st;
};

// grid (G, S)
__global__ __launch_bounds__(kThreads) void k_scan_project(ScanProjectArgs a) {
  __shared__ double sh[4][kThreads / 64];
  __shared__ Work w;
  __shared__ double shF[kMaxAtoms * 3], shV[kMaxAtoms * 3];
  __shared__ float sh_mult[2 * kMaxCv], sh_corr[kMaxAtoms * 6];
  __shared__ double sh_dv[2 * kMaxCv];
  __shared__ int sh_why;
  if (a.st.head[kHeadStatus]) return;               // frozen
  if (a.counts && a.counts[2]) return;    // overflowed: stale forces, the controller latches it
  const int g = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
  if (!scan_live(a.st, g)) return;  // a point that has converged looks at nothing
  const bool fresh = a.st.head[kHeadFresh] != 0;
  const int64_t row0 = (int64_t)g * a.g.n;
  if (t < a.T.A) {
    const int64_t r = row0 + a.T.atom_rel[t];
    w.fx[t] = a.fixed && a.fixed[a.T.atom_rel[t]];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      w.x[t * 3 + k] = (double)a.pos[r * 3 + k];
      shF[t * 3 + k] = (double)a.forces[r * 3 + k];
      shV[t * 3 + k] = (double)a.vel[r * 3 + k];
    }
  }
  __syncthreads();
  if (t == 0) {
    sh_why = multipliers(a.T, &w, shF, shV, sh_mult, sh_mult + kMaxCv);
    for (int k = 0; k < 2 * kMaxCv; ++k) sh_dv[k] = (double)sh_mult[k];
  }
  __syncthreads();
  const int why = sh_why;
  if (t < a.T.A) {
    float c[3];
    correction(a.T, &w, t, sh_dv, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) sh_corr[t * 6 + k] = c[k];
    correction(a.T, &w, t, sh_dv + kMaxCv, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) sh_corr[t * 6 + 3 + k] = c[k];
  }
  __syncthreads();
  if (s == 0) {
    if (t == 0) a.st.why[g] = why;
    if (t < kMaxCv) {
      a.st.cv[g * kMaxCv + t] = t < a.T.D ? w.s[t] : 0.0;
      if (fresh) a.st.t_cur[g * kMaxCv + t] = t < a.T.D ? w.s[t] : 0.0;  // the CV of the start geometry
    }
    if (t < 2 * kMaxCv) a.st.mult[g * 2 * kMaxCv + t] = sh_mult[t];
    if (t < a.T.A * 6) a.st.corr[(int64_t)g * kMaxAtoms * 6 + t] = sh_corr[t];
  }
  if (why) return;  // (the whole block: the controller latches it and reads no sum of this point)
  const int a0 = (int)((int64_t)a.g.n * s / a.g.S), a1 = (int)((int64_t)a.g.n * (s + 1) / a.g.S);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = a0 + t; i < a1; i += kThreads) {
    const int64_t r = row0 + i;
    float v[3], f[3], tm[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = a.vel[r * 3 + k];
      f[k] = a.forces[r * 3 + k];
    }
    const int j = scan_find(a.T, i);
    if (j >= 0) {
      apply(f, sh_corr + j * 6);
      apply(v, sh_corr + j * 6 + 3);
    }
    tn_min::atom_terms(v, f, a.fixed && a.fixed[i], tm);
    acc[0] += (double)tm[0];
    acc[1] += (double)tm[1];
    acc[2] += (double)tm[2];
    acc[3] = (double)tm[1] > acc[3] ? (double)tm[1] : acc[3];
  }
  block_reduce_waves<4, 8u>(acc, sh);
  if (t == 0) block_reduce_rows<4, 8u>(sh, a.st.slices + ((int64_t)g * a.g.S + s) * 4);
}

struct ScanCtlArgs {
  ScanGeom g;
  int D, A;
  tn_min::FireParams p;
  const int* counts;
  const float* energy;    // [G]
  const double* t_fin;    // [G, D]
  FireRows rows;          // [G, ...]
  double* cv_row;         // [G, D]
  double* target_row;     // [G, D]
  float* mult_row;        // [G, 2, D] lambda, mu
  float* corr_row;        // [G, A, 2, 3]
  ScanState st;
};

// the sums of point g in slice order, its state (after a reset: the start values of the header), and whether it stands at its
// final targets
__device__ __forceinline__ void scan_ctl_load(const ScanCtlArgs& a, int g, bool fresh, double sums[4], tn_min::FireState* s, int* here) {
  slice_sums<4, 8u>(a.st.slices + (int64_t)g * a.g.S * 4, a.g.S, 4, sums);
  fire_load(fire_units(a.st), g, fresh, s);
  *here = arrived(a.D, a.st.t_cur + g * kMaxCv, a.t_fin + (int64_t)g * a.D);
}

// ONE block striding the points, after k_scan_project: optimiser_control (tn_loop.h) with FIRE's two passes and the causes of the
// projection and of the last constraint step
__global__ __launch_bounds__(kThreads) void k_scan_control(ScanCtlArgs a) {
  optimiser_control(
      a.st.head, a.counts, kScanCauseWord, true, a.g.G,
      [&](int g, bool fresh, uint64_t step) {
        int here;
        double sums[4];
        float coef[3];
        tn_min::FireState s;
        scan_ctl_load(a, g, fresh, sums, &s, &here);
        if (s.converged_at >= 0) return 0;  // a point that has converged looks at nothing
        int c = fresh ? 0 : a.st.why2[g];
        if (!c) c = a.st.why[g];
        if (!c && scan_fire(&s, a.p, sums, here, (int64_t)step, coef) == tn_min::FIRE_UNUSABLE) c = SCAN_BAD_SUMS;
        if (!c && !isfinite(a.energy[g])) c = SCAN_BAD_SUMS;
        return c;
      },
      [&](int g, bool fresh, uint64_t step) {
        int here;
        double sums[4];
        float coef[3];
        tn_min::FireState s;
        scan_ctl_load(a, g, fresh, sums, &s, &here);
        // (a point that had converged: its slice sums, CVs, multipliers and corrections are those of the step it converged at, since
        // the projection no longer looks at it, and every row below repeats them)
        scan_fire(&s, a.p, sums, here, (int64_t)step, coef);
        fire_store(fire_units(a.st), g, s, coef);
        a.rows.write(g, a.energy + g, sums, sums[3], coef, s);
        for (int c = 0; c < a.D; ++c) {
          if (a.cv_row) a.cv_row[(int64_t)g * a.D + c] = a.st.cv[g * kMaxCv + c];
          if (a.target_row) a.target_row[(int64_t)g * a.D + c] = a.st.t_cur[g * kMaxCv + c];
          if (a.mult_row) {
            a.mult_row[((int64_t)g * 2 + 0) * a.D + c] = a.st.mult[g * 2 * kMaxCv + c];
            a.mult_row[((int64_t)g * 2 + 1) * a.D + c] = a.st.mult[g * 2 * kMaxCv + kMaxCv + c];
          }
        }
        if (a.corr_row)
          for (int k = 0; k < a.A * 6; ++k) a.corr_row[(int64_t)g * a.A * 6 + k] = a.st.corr[(int64_t)g * kMaxAtoms * 6 + k];
      });
}

struct ScanAtomArgs {
  ScanGeom g;
  Tables T;
  int64_t N;  // G n
  float* pos;           // [G n, 3]
  float* vel;           // [G n, 3]
  const float* forces;  // ACCEPT: the evaluation's F; OPEN: the kept F_perp
  float* forces_keep;     // [G n, 3] F, or NULL
  float* projected_keep;  // [G n, 3] F_perp
  const uint8_t* fixed;
  const int* counts;
  ScanState st;
};

// One thread per atom of a point.  ACCEPT (after k_scan_control): F, F_perp and v_perp of the evaluation into the caller's buffers, or
// the x and v the last move saved when the evaluation overflowed or the constraint step before it had failed.  MOVE: save x and v,
// then tn_min::atom_move on (v_perp, F_perp) with the point's coefficients.
template <bool ACCEPT, bool MOVE>
__global__ __launch_bounds__(kThreads) void k_scan_atoms(ScanAtomArgs a) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.N) return;
  const int g = (int)(r / a.g.n), atom = (int)(r - (int64_t)g * a.g.n);
  const uint32_t status = a.st.head[kHeadStatus], fresh = a.st.head[kHeadFresh];
  if (status) {
    const bool overflowed = status == 1u && a.counts && a.counts[2];
    const bool off_surface = status == 2u && a.st.head[kScanCauseWord] == (uint32_t)SCAN_BAD_STEP;
    if (ACCEPT && !fresh && (overflowed || off_surface)) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a.pos[r * 3 + k] = a.st.x_keep[r * 3 + k];
        a.vel[r * 3 + k] = a.st.v_keep[r * 3 + k];
      }
    }
    return;
  }
  if (fresh) return;  // (OPEN straight after a reset: there are no coefficients yet)
  const int fx = a.fixed && a.fixed[atom];
  const int64_t conv = a.st.conv[g];
  float x[3], v[3], f[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    f[k] = a.forces[r * 3 + k];
    v[k] = a.vel[r * 3 + k];
  }
  if (ACCEPT && (conv < 0 || conv == (int64_t)loop_step(a.st.head))) {  // (a point that converged at an earlier step keeps everything)
    if (a.forces_keep)
#pragma unroll
      for (int k = 0; k < 3; ++k) a.forces_keep[r * 3 + k] = f[k];
    const int j = scan_find(a.T, atom);
    if (j >= 0) {
      const float* c = a.st.corr + ((int64_t)g * kMaxAtoms + j) * 6;
      apply(f, c);
      apply(v, c + 3);
#pragma unroll
      for (int k = 0; k < 3; ++k) a.vel[r * 3 + k] = v[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) a.projected_keep[r * 3 + k] = f[k];
  }
  if (MOVE) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[k] = a.pos[r * 3 + k];
      a.st.x_keep[r * 3 + k] = x[k];
      a.st.v_keep[r * 3 + k] = v[k];
    }
    if (conv >= 0 || fx) {  // a branch, not a product with 0: x keeps its bits
#pragma unroll
      for (int k = 0; k < 3; ++k) a.vel[r * 3 + k] = 0.f;
      return;
    }
    tn_min::atom_move(x, v, f, a.st.coef[g * 3 + 0], a.st.coef[g * 3 + 1], a.st.coef[g * 3 + 2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a.pos[r * 3 + k] = x[k];
      a.vel[r * 3 + k] = v[k];
    }
  }
}

struct ScanConsArgs {
  ScanGeom g;
  Tables T;
  float* pos;            // [G n, 3]
  const uint8_t* fixed;
  const double* t_fin;   // [G, D]
  double drive[kMaxCv];
  double tol;
  int max_iter;
  float* cons_row;       // [G, A, 3] the CV atoms' positions after the step, or NULL
  int32_t* iters_row;    // [G] or NULL
  ScanState st;
};

// grid (G), one wave, after the move: drive the point's targets, then the constraint step on its CV atoms.  Writes the CV atoms
// that are not fixed, or - when the step is unusable - nothing but the point's flag.
__global__ __launch_bounds__(64) void k_scan_constrain(ScanConsArgs a) {
  __shared__ Work w;
  __shared__ double sh_t[kMaxCv];
  __shared__ int sh_why, sh_iters;
  const int g = blockIdx.x, t = threadIdx.x;
  if (a.st.head[kHeadStatus] || a.st.head[kHeadFresh]) return;  // frozen, or straight after a reset
  if (a.st.conv[g] >= 0) return;             // a point that has converged keeps its bits
  const int64_t row0 = (int64_t)g * a.g.n;
  if (t < a.T.A) {
    const int64_t r = row0 + a.T.atom_rel[t];
    w.fx[t] = a.fixed && a.fixed[a.T.atom_rel[t]];
#pragma unroll
    for (int k = 0; k < 3; ++k) w.x[t * 3 + k] = (double)a.pos[r * 3 + k];
  }
  if (t < a.T.D) {
    const double tc = drive(a.T.kind[t], a.t_fin[(int64_t)g * a.T.D + t], a.st.t_cur[g * kMaxCv + t], a.drive[t]);
    sh_t[t] = tc;  // (stored only when the constraint step reaches it: after a failure t_cur is that of the last valid step)
  }
  __syncthreads();
  if (t == 0) {
    int iters = 0;
    sh_why = constrain(a.T, &w, sh_t, a.tol, a.max_iter, &iters);
    sh_iters = iters;
  }
  __syncthreads();
  if (t == 0) {
    a.st.why2[g] = sh_why;
    if (a.iters_row) a.iters_row[g] = sh_iters;
  }
  if (sh_why) return;
  if (t < a.T.D) a.st.t_cur[g * kMaxCv + t] = sh_t[t];
  if (t < a.T.A) {
    const int64_t r = row0 + a.T.atom_rel[t];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float xn = w.fx[t] ? a.pos[r * 3 + k] : (float)w.x[t * 3 + k];
      if (!w.fx[t]) a.pos[r * 3 + k] = xn;
      if (a.cons_row) a.cons_row[((int64_t)g * a.T.A + t) * 3 + k] = xn;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_scan_reset(ScanState st, int G, uint64_t step0, double dt0, double alpha0) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) {
    loop_head_reset(st.head, step0, kScanCauseWord);
    st.start[0] = dt0;
    st.start[1] = alpha0;
  }
  if (i < G) {
    st.why[i] = 0;
    st.why2[i] = 0;
    st.conv[i] = -1;
  }
}

bool scan_shape_ok(int64_t n, int64_t G) {
  if (n < 1 || G < 1 || G > INT32_MAX / 64) return false;
  return G <= (INT32_MAX / 16) / n;  // G n rows of 3 floats stay below 2^31
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_scan_workspace_bytes(int64_t n_atoms, int64_t n_points, size_t* bytes) {
  if (!bytes || !scan_shape_ok(n_atoms, n_points)) return TMDNET_ERR_INVALID;
  *bytes = scan_bytes(n_atoms, n_points);
  return TMDNET_OK;
}

int tmdnet_scan_reset(void* stream, void* scan_ws, int64_t n_atoms, int64_t n_points, uint64_t step0, double dt0, double alpha0) {
  if (!scan_ws || !scan_shape_ok(n_atoms, n_points) || !(dt0 > 0.0) || !(alpha0 >= 0.0)) return TMDNET_ERR_INVALID;
  hipLaunchKernelGGL(k_scan_reset, dim3((unsigned)((n_points + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), carve_scan(scan_ws, n_atoms, n_points), (int)n_points, step0, dt0, alpha0);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_scan_advance(tmdnet_model* m, void* stream, void* graph_ws, void* scan_ws, int64_t n_atoms, int64_t n_points, int32_t phase,
                        float* pos, float* vel, const float* forces, const float* energy, const uint8_t* fixed, float* forces_keep,
                        float* projected_keep, int32_t n_cv, const int32_t* cv_kind, const int32_t* cv_atoms, const double* targets,
                        const double* drive, double tol, int32_t max_iter, double dt_max, int32_t n_min, double f_inc, double f_dec,
                        double alpha0, double f_alpha, double max_step, double fmax, float* epot_log_row, float* fmax_log_row,
                        double* sums_log_row, float* coef_log_row, double* dt_log_row, double* alpha_log_row, int64_t* converged_log_row,
                        double* cv_log_row, double* target_log_row, float* multiplier_log_row, float* correction_log_row,
                        float* constrained_log_row, int32_t* iterations_log_row) {
  if (!scan_ws || !pos || !vel || !forces || !projected_keep || !targets || !drive || !scan_shape_ok(n_atoms, n_points))
    return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MIN_OPEN && phase != TMDNET_MIN_MIDDLE && phase != TMDNET_MIN_CLOSE) return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MIN_OPEN && !energy) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (!(fmax > 0.0) || !(dt_max > 0.0) || !(max_step > 0.0) || !(f_inc > 0.0) || !(f_dec > 0.0) || !(f_alpha > 0.0) || !(alpha0 >= 0.0) ||
      n_min < 0 || !(tol > 0.0) || max_iter < 1)
    return TMDNET_ERR_INVALID;
  Tables T;
  if (make_tables(n_cv, cv_kind, cv_atoms, n_atoms, &T)) return TMDNET_ERR_INVALID;  // (every index the kernels form lies inside a point)
  for (int c = 0; c < T.D; ++c)
    if (!(drive[c] > 0.0)) return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ScanGeom g;
  g.n = (int)n_atoms;
  g.G = (int)n_points;
  g.S = mol_slices(n_atoms, 1);
  const int64_t N = n_points * n_atoms;
  const ScanState st = carve_scan(scan_ws, n_atoms, n_points);
  const int* counts = loop_graph(m, graph_ws, N, n_points).counts;
  const dim3 block(kThreads);
  if (phase != TMDNET_MIN_OPEN) {
    ScanProjectArgs p;
    p.g = g;
    p.T = T;
    p.counts = counts;
    p.pos = pos;
    p.vel = vel;
    p.forces = forces;
    p.fixed = fixed;
    p.st = st;
    hipLaunchKernelGGL(k_scan_project, dim3((unsigned)n_points, (unsigned)g.S), block, 0, s, p);
    ScanCtlArgs c;
    c.g = g;
    c.D = T.D;
    c.A = T.A;
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
    c.t_fin = targets;
    c.rows = {epot_log_row, fmax_log_row, sums_log_row, coef_log_row, dt_log_row, alpha_log_row, converged_log_row};
    c.cv_row = cv_log_row;
    c.target_row = target_log_row;
    c.mult_row = multiplier_log_row;
    c.corr_row = correction_log_row;
    c.st = st;
    hipLaunchKernelGGL(k_scan_control, dim3(1), block, 0, s, c);
  }
  ScanAtomArgs a;
  a.g = g;
  a.T = T;
  a.N = N;
  a.pos = pos;
  a.vel = vel;
  a.forces = forces;
  a.forces_keep = forces_keep;
  a.projected_keep = projected_keep;
  a.fixed = fixed;
  a.counts = counts;
  a.st = st;
  const dim3 grid((unsigned)((N + kThreads - 1) / kThreads));
  if (phase == TMDNET_MIN_OPEN)
    hipLaunchKernelGGL((k_scan_atoms<false, true>), grid, block, 0, s, a);
  else if (phase == TMDNET_MIN_MIDDLE)
    hipLaunchKernelGGL((k_scan_atoms<true, true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((k_scan_atoms<true, false>), grid, block, 0, s, a);
  if (phase != TMDNET_MIN_CLOSE) {
    ScanConsArgs c;
    c.g = g;
    c.T = T;
    c.pos = pos;
    c.fixed = fixed;
    c.t_fin = targets;
    for (int k = 0; k < kMaxCv; ++k) c.drive[k] = k < T.D ? drive[k] : 0.0;
    c.tol = tol;
    c.max_iter = max_iter;
    c.cons_row = constrained_log_row;
    c.iters_row = iterations_log_row;
    c.st = st;
    hipLaunchKernelGGL(k_scan_constrain, dim3((unsigned)n_points), dim3(64), 0, s, c);
  }
  return loop_launch_result(m, "tmdnet_scan_advance");
}

int tmdnet_scan_status(void* stream, void* scan_ws, uint64_t host[3]) {
  if (!scan_ws || !host) return TMDNET_ERR_INVALID;
  return loop_read_status(stream, carve_scan(scan_ws, 0, 0).head, kScanHeadWords, kScanCauseWord, host, 3);
}

}  // extern "C"
