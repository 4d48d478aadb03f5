// Device-resident intrinsic-reaction-coordinate follower: the kernels that sit between two energy+force evaluations of a captured
// step, so that K steps of the damped velocity Verlet path follower (Hratchian and Schlegel, J. Phys. Chem. A 106, 165, 2002) replay
// as one HIP graph with no host work in between.  A call has P = G D paths of the same n atoms - G saddles, D directions, path
// p = g D + d - and the evaluation sees P molecules of n atoms; atom a of path p is row p n + a.  The arithmetic is tn_irc_math.h
// (the closing kick, the extrapolated point, the path sums, the controller) and tn_md_math.h (the opening half of a step).  The
// scheme is stated with the entries in include/tmdnet_amd.h.
//
// One step, after the energies E and forces F at x_{i+1} are known - three launches:
//   sums      grid (path, slice): |v'|^2, F.v', max |F|^2, |x - x'|^2, m |x - x_i|^2 and the number of free atoms, ONE pass over the
//             atoms for all six                                                         (fp32 terms, fp64 sums, fixed order)
//   control   ONE block, paths strided: the slice sums added in slice order, tn_irc::irc_control, the status word, the frame's slot,
//             arc length and energy, the logs
//   atoms     per atom: accept (v <- c v', F -> the caller's buffer, the frame; or generation 1 back after an overflow or an
//             unusable path) and, in MIDDLE, the move: generation 1 -> 2, (x, v, F) -> generation 1, tn_md::open_step
// CLOSE omits the move, OPEN is the move alone from the kept forces.
//
// Reductions are tn_loop.h's, as in k_min_reduce.  No floating-point atomics: repeats are bit-identical.  Overflow and unusable paths
// follow the minimiser's protocol: the controller is the only kernel that writes the status word; an overflowed evaluation latches
// status 1, a path that still moves and has an energy, a force sum or a velocity sum that cannot be used latches status 2 (the cause
// in header word 4) before anything of that step is accepted, and the per-atom kernel puts x and v of generation 1 back.  From then on
// every launch changes nothing until tmdnet_irc_reset.
#include <cmath>

#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_irc_math.h"
#include "tn_loop.h"
#include "tn_model.h"

namespace tn {

namespace {

using namespace tn_irc;

// The header: five uint32 words, then one double.  Words 0 / 1 the step counter (lo / hi), 2 the status, 3 "reset, not yet controlled",
constexpr int kIrcCauseWord = 4;      // which input was unusable when status 2 was latched (tn_irc::IRC_*)
constexpr int kIrcHeadWords = 5;      // words the status entry reads back
constexpr size_t kIrcStartByte = 32;  // dt0 (fp64)
static_assert(kIrcHeadWords * sizeof(uint32_t) <= kIrcStartByte && kIrcStartByte % sizeof(double) == 0 &&
                  kIrcStartByte + sizeof(double) <= kHeaderBytes,
              "the start value lies behind the header words, aligned, inside the header");

struct IrcState {  // views into the caller's workspace; the record comes first so that a caller can find it (tmdnet_amd.h)
  uint32_t* head;      // [0] step lo, [1] step hi, [2] status, [3] 1 = reset, not yet controlled, [4] cause of status 2
  double* start;       // [0] dt0
  int32_t* n_rec;      // [P] frames counted
  double* frame_s;     // [P, C] arc length of a frame
  float* frame_e;      // [P, C] energy of a frame
  float* frames;       // [P, C, n, 3]
  double* dt;          // [P] the time step of the next opening half
  double* arc;         // [P]
  int64_t* conv;       // [P] converged_at
  int32_t* reason;     // [P]
  int32_t* n_acc;      // [P] accepted steps since the start
  int32_t* slot;       // [P] the frame the step just controlled is recorded in, or -1
  float* damp;         // [P] fp32(c) of the step just controlled
  float* dt_used;      // [P] fp32 of the time step the step just controlled was opened with (0: the start images)
  double* rec;         // [P, N_SUMS] the sums of a path's last controlled step
  double* slices;      // [P, S, N_SUMS]
  float *x1, *v1, *f1;  // [P n, 3] generation 1: the state the last move began from
  float *x2, *v2, *f2;  // [P n, 3] generation 2: the one before
};

IrcState irc_layout(LoopCarver& c, int64_t n, int64_t P, int64_t C) {
  const size_t p = (size_t)(P > 0 ? P : 0), N = p * (size_t)(n > 0 ? n : 0), cap = (size_t)(C > 0 ? C : 0);
  const size_t S = (size_t)mol_slices(n, 1);  // slices per path: one path is the molecule
  IrcState st;
  st.head = c.take<uint32_t>(kHeaderBytes / sizeof(uint32_t));
  st.start = reinterpret_cast<double*>(reinterpret_cast<char*>(st.head) + kIrcStartByte);
  st.n_rec = c.take<int32_t>(p);
  st.frame_s = c.take<double>(p * cap);
  st.frame_e = c.take<float>(p * cap);
  st.frames = c.take<float>(N * cap * 3);
  st.dt = c.take<double>(p);
  st.arc = c.take<double>(p);
  st.conv = c.take<int64_t>(p);
  st.reason = c.take<int32_t>(p);
  st.n_acc = c.take<int32_t>(p);
  st.slot = c.take<int32_t>(p);
  st.damp = c.take<float>(p);
  st.dt_used = c.take<float>(p);
  st.rec = c.take<double>(p * N_SUMS);
  st.slices = c.take<double>(p * S * N_SUMS);
  st.x1 = c.take<float>(N * 3);
  st.v1 = c.take<float>(N * 3);
  st.f1 = c.take<float>(N * 3);
  st.x2 = c.take<float>(N * 3);
  st.v2 = c.take<float>(N * 3);
  st.f2 = c.take<float>(N * 3);
  return st;
}

size_t irc_bytes(int64_t n, int64_t P, int64_t C) {
  return layout_bytes([&](LoopCarver& c) { irc_layout(c, n, P, C); });
}

IrcState carve_irc(void* ws, int64_t n, int64_t P, int64_t C) {
  LoopCarver c(ws);
  return irc_layout(c, n, P, C);
}

struct IrcGeom {
  int n, P, S, C;
};

struct IrcIn {  // what the sums read
  const int* counts;    // the graph's counters, or NULL
  const float* pos;     // [P n, 3] x_{i+1}
  const float* vel;     // [P n, 3] v_half
  const float* forces;  // [P n, 3] F_{i+1}
  const float* ca;      // [n] fp32(force_scale / (2 m))
  const float* mass;    // [n]
  const uint8_t* fixed; // [n] or NULL
};

// a path is looked at while it moves (after a reset every path does)
__device__ __forceinline__ bool irc_live(const IrcState& st, int p) { return st.head[kHeadFresh] != 0 || st.conv[p] < 0; }

// grid (P, S): slice s of path p -> slices[p, s, 0..N_SUMS), all six entries from one pass over the atoms
__global__ __launch_bounds__(kThreads) void k_irc_sums(IrcState st, IrcGeom g, IrcIn in) {
  __shared__ double sh[N_SUMS][kThreads / 64];
  if (st.head[kHeadStatus]) return;                 // frozen
  if (in.counts && in.counts[2]) return;  // overflowed: stale forces, the controller latches it
  const int p = blockIdx.x, s = blockIdx.y;
  if (!irc_live(st, p)) return;  // a path that has finished looks at nothing
  const bool fresh = st.head[kHeadFresh] != 0;
  const float dt = fresh ? 0.f : (float)st.dt[p];
  const int has2 = !fresh && st.n_acc[p] >= 1;
  const float T = has2 ? md_add(st.dt_used[p], dt) : 0.f;
  const int a0 = (int)((int64_t)g.n * s / g.S), a1 = (int)((int64_t)g.n * (s + 1) / g.S);
  double acc[N_SUMS];
#pragma unroll
  for (int k = 0; k < N_SUMS; ++k) acc[k] = 0.0;
  for (int a = a0 + (int)threadIdx.x; a < a1; a += kThreads) {
    const float ca = in.ca[a];
    if (still_atom(in.fixed && in.fixed[a], ca)) continue;
    const int64_t r = ((int64_t)p * g.n + a) * 3;
    float x[3], vh[3], f[3], x1[3], x2[3], v2[3], f2[3], vp[3], t[5];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[k] = in.pos[r + k];
      vh[k] = in.vel[r + k];
      f[k] = in.forces[r + k];
      x1[k] = fresh ? x[k] : st.x1[r + k];
      x2[k] = has2 ? st.x2[r + k] : 0.f;
      v2[k] = has2 ? st.v2[r + k] : 0.f;
      f2[k] = has2 ? st.f2[r + k] : 0.f;
    }
    sum_terms(x, vh, f, md_mul(dt, ca), ca, in.mass[a], x1, has2, x2, v2, f2, T, vp, t);
    acc[S_VV] += (double)t[S_VV];
    acc[S_P] += (double)t[S_P];
    acc[S_FMAX2] = (double)t[S_FMAX2] > acc[S_FMAX2] ? (double)t[S_FMAX2] : acc[S_FMAX2];
    acc[S_D2] += (double)t[S_D2];
    acc[S_DS2] += (double)t[S_DS2];
    acc[S_FREE] += 1.0;  // (a count: exact)
  }
  block_reduce_waves<N_SUMS, kMaxMask>(acc, sh);
  if (threadIdx.x == 0) block_reduce_rows<N_SUMS, kMaxMask>(sh, st.slices + ((int64_t)p * g.S + s) * N_SUMS);
}

struct IrcCtlArgs {
  IrcGeom g;
  IrcParams p;
  const int* counts;  // the graph's counters, or NULL
  const float* energy;  // [P]
  float* epot_row;      // [P]
  float* fmax_row;      // [P]
  double* sums_row;     // [P, N_SUMS]
  float* coef_row;      // [P, 2]
  double* dt_row;       // [P]
  double* arc_row;      // [P]
  double* power_row;    // [P]
  int64_t* conv_out;    // [P]
  int32_t* reason_out;  // [P]
  double* dt_out;       // [P]
  double* arc_out;      // [P]
  int32_t* n_rec_out;   // [P]
  IrcState st;
};

// the sums of path p in slice order, and its state (after a reset: the start values)
__device__ __forceinline__ void irc_ctl_load(const IrcCtlArgs& a, int p, bool fresh, double sums[N_SUMS], IrcPath* s) {
  slice_sums<N_SUMS, kMaxMask>(a.st.slices + (int64_t)p * a.g.S * N_SUMS, a.g.S, N_SUMS, sums);
  if (fresh) {
    s->dt = a.st.start[0];
    s->arc = 0.0;
    s->converged_at = -1;
    s->reason = REASON_NONE;
    s->n_acc = 0;
    s->n_rec = 0;
  } else {
    s->dt = a.st.dt[p];
    s->arc = a.st.arc[p];
    s->converged_at = a.st.conv[p];
    s->reason = a.st.reason[p];
    s->n_acc = a.st.n_acc[p];
    s->n_rec = a.st.n_rec[p];
  }
}

// ONE block striding the paths, after k_irc_sums: optimiser_control (tn_loop.h).  Pass 1: is any path that still moves unusable?
// Pass 2: every path's state, coefficients, frame slot and log rows.
__global__ __launch_bounds__(kThreads) void k_irc_control(IrcCtlArgs a) {
  optimiser_control(
      a.st.head, a.counts, kIrcCauseWord, true, a.g.P,
      [&](int p, bool fresh, uint64_t step) {
        int slot, cause;
        double sums[N_SUMS];
        float out[2];
        IrcPath s;
        irc_ctl_load(a, p, fresh, sums, &s);
        return irc_control(&s, a.p, sums, a.energy[p], fresh, (int64_t)step, out, &slot, &cause) == IRC_UNUSABLE ? cause : 0;
      },
      [&](int p, bool fresh, uint64_t step) {
        int slot, cause;
        double sums[N_SUMS];
        float out[2];
        IrcPath s;
        irc_ctl_load(a, p, fresh, sums, &s);
        double* rec = a.st.rec + (int64_t)p * N_SUMS;
        if (irc_control(&s, a.p, sums, a.energy[p], fresh, (int64_t)step, out, &slot, &cause) != IRC_FROZEN) {
          a.st.damp[p] = out[0];
          a.st.dt_used[p] = out[1];
#pragma unroll
          for (int k = 0; k < N_SUMS; ++k) rec[k] = sums[k];
          if (slot >= 0) {
            a.st.frame_s[(int64_t)p * a.g.C + slot] = s.arc;
            a.st.frame_e[(int64_t)p * a.g.C + slot] = a.energy[p];
          }
        }  // (a path that had finished keeps the records of the step it finished at)
        a.st.slot[p] = slot;
        a.st.dt[p] = s.dt;
        a.st.arc[p] = s.arc;
        a.st.conv[p] = s.converged_at;
        a.st.reason[p] = s.reason;
        a.st.n_acc[p] = s.n_acc;
        a.st.n_rec[p] = s.n_rec;
        if (a.epot_row) a.epot_row[p] = a.energy[p];
        if (a.fmax_row) a.fmax_row[p] = (float)sqrt(rec[S_FMAX2]);
        if (a.sums_row)
#pragma unroll
          for (int k = 0; k < N_SUMS; ++k) a.sums_row[(int64_t)p * N_SUMS + k] = rec[k];
        if (a.coef_row) {
          a.coef_row[(int64_t)p * 2 + 0] = a.st.damp[p];
          a.coef_row[(int64_t)p * 2 + 1] = a.st.dt_used[p];
        }
        if (a.dt_row) a.dt_row[p] = s.dt;
        if (a.arc_row) a.arc_row[p] = s.arc;
        if (a.power_row) a.power_row[p] = rec[S_P];
        if (a.conv_out) a.conv_out[p] = s.converged_at;
        if (a.reason_out) a.reason_out[p] = s.reason;
        if (a.dt_out) a.dt_out[p] = s.dt;
        if (a.arc_out) a.arc_out[p] = s.arc;
        if (a.n_rec_out) a.n_rec_out[p] = s.n_rec;
      });
}

struct IrcAtomArgs {
  IrcGeom g;
  int64_t N;  // P n
  float* pos;           // [P n, 3]
  float* vel;           // [P n, 3]
  const float* forces;  // ACCEPT: the evaluation's; OPEN: the kept forces
  float* forces_keep;   // [P n, 3] or NULL
  const float* ca;      // [n]
  const uint8_t* fixed;
  IrcState st;
};

// One thread per atom.  ACCEPT (after k_irc_control): the closing kick again, v <- c v', the force into the caller's buffer and x
// into the frame the controller chose - or, when the step was refused, x and v of generation 1 back.  MOVE: generation 1 becomes
// generation 2, (x, v, F) generation 1, then the opening half of the next step with the path's new time step.  A path that finished
// at an earlier step keeps everything.
template <bool ACCEPT, bool MOVE>
__global__ __launch_bounds__(kThreads) void k_irc_atoms(IrcAtomArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.N) return;
  const int p = (int)(i / a.g.n), atom = (int)(i - (int64_t)p * a.g.n);
  const int64_t r = i * 3;
  const uint32_t status = a.st.head[kHeadStatus], fresh = a.st.head[kHeadFresh];
  if (status) {
    if (ACCEPT && !fresh && a.st.conv[p] < 0) {  // the step was opened and then refused: back to where it began
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a.pos[r + k] = a.st.x1[r + k];
        a.vel[r + k] = a.st.v1[r + k];
      }
    }
    return;
  }
  if (fresh) return;  // (OPEN straight after a reset: nothing has been controlled yet)
  const float ca = a.ca[atom];
  const int still = still_atom(a.fixed && a.fixed[atom], ca);
  const int64_t conv = a.st.conv[p];
  float x[3], v[3], f[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    x[k] = a.pos[r + k];
    v[k] = a.vel[r + k];
    f[k] = a.forces[r + k];
  }
  if (ACCEPT && (conv < 0 || conv == (int64_t)loop_step(a.st.head))) {
    if (still) {
      v[0] = v[1] = v[2] = 0.f;
    } else {
      float vp[3];
      close_kick(v, f, md_mul(a.st.dt_used[p], ca), vp);
      damp(vp, a.st.damp[p], v);
    }
    const int slot = a.st.slot[p];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a.vel[r + k] = v[k];
      if (a.forces_keep) a.forces_keep[r + k] = f[k];
      if (slot >= 0) a.st.frames[(((int64_t)p * a.g.C + slot) * a.g.n + atom) * 3 + k] = x[k];
    }
  }
  if (MOVE && conv < 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a.st.x2[r + k] = a.st.x1[r + k];
      a.st.v2[r + k] = a.st.v1[r + k];
      a.st.f2[r + k] = a.st.f1[r + k];
      a.st.x1[r + k] = x[k];
      a.st.v1[r + k] = v[k];
      a.st.f1[r + k] = f[k];
    }
    if (!still) {  // a branch: a still atom keeps the bits of x
      const float dt = (float)a.st.dt[p];
      tn_md::open_step(x, v, f, md_mul(dt, ca), dt);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a.pos[r + k] = x[k];
        a.vel[r + k] = v[k];
      }
    }
  }
}

__global__ void k_irc_reset(IrcState st, uint64_t step0, double dt0) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    loop_head_reset(st.head, step0, kIrcCauseWord);
    st.start[0] = dt0;
  }
}

bool irc_shape_ok(int64_t n, int64_t P, int64_t C) {
  if (n < 0 || P < 1 || P > INT32_MAX / 64 || C < 1 || C > INT32_MAX / 2) return false;
  if (n == 0) return true;
  if (P > (INT32_MAX / 16) / n) return false;     // P n rows of 3 floats stay below 2^31
  return C <= ((int64_t)1 << 36) / (P * n);        // and the frames below 2^36 rows
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_irc_workspace_bytes(int64_t n_atoms, int64_t n_paths, int64_t capacity, size_t* bytes) {
  if (!bytes || !irc_shape_ok(n_atoms, n_paths, capacity)) return TMDNET_ERR_INVALID;
  *bytes = irc_bytes(n_atoms, n_paths, capacity);
  return TMDNET_OK;
}

int tmdnet_irc_reset(void* stream, void* irc_ws, uint64_t step0, double dt0) {
  if (!irc_ws || !(dt0 > 0.0) || !std::isfinite(dt0)) return TMDNET_ERR_INVALID;
  hipLaunchKernelGGL(k_irc_reset, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), carve_irc(irc_ws, 0, 0, 0), step0, dt0);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_irc_advance(tmdnet_model* m, void* stream, void* graph_ws, void* irc_ws, int64_t n_atoms, int64_t n_paths, int64_t capacity,
                       int32_t every, int32_t phase, float* pos, float* vel, const float* forces, const float* energy,
                       const float* half_inv_mass, const float* masses, const uint8_t* fixed, float* forces_keep, double fmax, double v0,
                       double error, double dt_min, double dt_max, float* epot_log_row, float* fmax_log_row, double* sums_log_row,
                       float* coef_log_row, double* dt_log_row, double* arc_log_row, double* power_log_row, int64_t* converged_at,
                       int32_t* reason, double* step_size, double* arc_length, int32_t* n_recorded) {
  if (!irc_ws || !pos || !vel || !forces || !half_inv_mass || !masses || !irc_shape_ok(n_atoms, n_paths, capacity)) return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MIN_OPEN && phase != TMDNET_MIN_MIDDLE && phase != TMDNET_MIN_CLOSE) return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MIN_OPEN && !energy) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (!(fmax > 0.0) || !(v0 > 0.0) || !(error > 0.0) || !(dt_min > 0.0) || !(dt_max >= dt_min) || !std::isfinite(dt_max) || every < 1)
    return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  IrcGeom g;
  g.n = (int)n_atoms;
  g.P = (int)n_paths;
  g.S = mol_slices(n_atoms, 1);
  g.C = (int)capacity;
  const int64_t N = n_paths * n_atoms;
  const IrcState st = carve_irc(irc_ws, n_atoms, n_paths, capacity);
  const int* counts = loop_graph(m, graph_ws, N, n_paths).counts;
  const dim3 block(kThreads);
  if (phase != TMDNET_MIN_OPEN) {
    IrcIn in;
    in.counts = counts;
    in.pos = pos;
    in.vel = vel;
    in.forces = forces;
    in.ca = half_inv_mass;
    in.mass = masses;
    in.fixed = fixed;
    hipLaunchKernelGGL(k_irc_sums, dim3((unsigned)n_paths, (unsigned)g.S), block, 0, s, st, g, in);
    IrcCtlArgs c;
    c.g = g;
    c.p.fmax = fmax;
    c.p.v0 = v0;
    c.p.error = error;
    c.p.dt_min = dt_min;
    c.p.dt_max = dt_max;
    c.p.every = every;
    c.p.capacity = (int32_t)capacity;
    c.counts = counts;
    c.energy = energy;
    c.epot_row = epot_log_row;
    c.fmax_row = fmax_log_row;
    c.sums_row = sums_log_row;
    c.coef_row = coef_log_row;
    c.dt_row = dt_log_row;
    c.arc_row = arc_log_row;
    c.power_row = power_log_row;
    c.conv_out = converged_at;
    c.reason_out = reason;
    c.dt_out = step_size;
    c.arc_out = arc_length;
    c.n_rec_out = n_recorded;
    c.st = st;
    hipLaunchKernelGGL(k_irc_control, dim3(1), block, 0, s, c);
  }
  if (N > 0) {
    IrcAtomArgs a;
    a.g = g;
    a.N = N;
    a.pos = pos;
    a.vel = vel;
    a.forces = forces;
    a.forces_keep = phase == TMDNET_MIN_OPEN ? nullptr : forces_keep;
    a.ca = half_inv_mass;
    a.fixed = fixed;
    a.st = st;
    const dim3 grid((unsigned)((N + kThreads - 1) / kThreads));
    if (phase == TMDNET_MIN_OPEN)
      hipLaunchKernelGGL((k_irc_atoms<false, true>), grid, block, 0, s, a);
    else if (phase == TMDNET_MIN_MIDDLE)
      hipLaunchKernelGGL((k_irc_atoms<true, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((k_irc_atoms<true, false>), grid, block, 0, s, a);
  }
  return loop_launch_result(m, "tmdnet_irc_advance");
}

int tmdnet_irc_status(void* stream, void* irc_ws, uint64_t host[3]) {
  if (!irc_ws || !host) return TMDNET_ERR_INVALID;
  return loop_read_status(stream, carve_irc(irc_ws, 0, 0, 0).head, kIrcHeadWords, kIrcCauseWord, host, 3);
}

}  // extern "C"
