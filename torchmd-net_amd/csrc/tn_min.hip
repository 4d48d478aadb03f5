// Device-resident geometry minimisation: the FIRE kernels that sit between two energy+force evaluations of a captured step, so
// that K minimiser steps replay as one HIP graph with no host work in between.  One controller per molecule (replica): every
// molecule has its own time step and mixing factor and freezes at its own step.  The arithmetic is tn_min_math.h.
//
// One step, after the forces F at the current positions are known:
//   reduce    per molecule vf = sum v.F, ff = sum F.F, vv = sum v.v, fmax2 = max |F_i|^2   (fp32 terms, fp64 sums, fixed order)
//   control   one thread per molecule, fp64: converged?  else dt, alpha, n_pos and the fp32 coefficients c_v, c_f, d
//   update    per atom: v <- c_v v + c_f F,  x <- x + d v      (frozen molecule or fixed atom: v <- 0, x untouched)
// A launch after an evaluation (TMDNET_MIN_MIDDLE) is reduce, control and one per-atom kernel that accepts the evaluation (keeps
// its forces, or goes back to the saved state when it overflowed) and moves the atoms; TMDNET_MIN_CLOSE is the same without the
// move, TMDNET_MIN_OPEN is the move alone from the coefficients the workspace holds.  So every evaluated force set drives the
// controller exactly once whatever K is: a replay is OPEN, then K x { evaluation; MIDDLE, or CLOSE after the last }, and after a
// reset one CLOSE on the forces at the start (which counts no step).
//
// Reduction: grid (B, S), slices of at most 1 024 atoms on average (the geometry of k_md_ke_reduce); threads stride the atoms of a
// slice, lanes add by the wave's xor tree, waves in turn, and the controller adds the slices in slice order.  No floating-point
// atomics: repeats are bit-identical.  The atoms of a molecule are mstart..mend of the graph workspace when those ranges are valid,
// otherwise (Graph::counts[3], or no graph workspace) all atoms filtered by `batch`.
//
// Overflow and unusable sums.  The controller (one block) is the only kernel that writes the status word.  When the evaluation
// before it overflowed (counts[2]) it latches status 1, and the per-atom kernel of the same launch puts x and v back to what the
// last move saved; when a sum of a molecule that still moves is not finite it latches status 2 before anything of that step is
// written.  From then on every launch returns at once: positions, velocities, forces_keep, the logs and the step counter stay at
// the last valid step until tmdnet_min_reset.  Nothing allocates or synchronises; everything is capturable.
#include <string>

#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_min_math.h"
#include "tn_model.h"

namespace tn {

namespace {

constexpr int kMinThreads = 256;
constexpr size_t kMinHeaderBytes = 256;

struct MinState {  // views into the caller's workspace
  uint32_t* head;    // [0] step lo, [1] step hi, [2] status (sticky: 1 overflow, 2 non-finite sums), [3] 1 = reset, not yet controlled
  double* start;     // [0] dt0, [1] alpha0 (header bytes 16..31): what a molecule starts from at the first control after a reset
  double* dt;        // [B]
  double* alpha;     // [B]
  int64_t* conv;     // [B] converged_at
  int32_t* n_pos;    // [B]
  float* coef;       // [B, 3] c_v, c_f, d of the next move
  float* x_keep;     // [N, 3] positions before the last move
  float* v_keep;     // [N, 3]
  double* slices;    // [B, S, 4] vf, ff, vv, fmax2
};

inline size_t min_align256(size_t n) { return (n + 255) & ~size_t(255); }

int min_slices(int64_t N, int64_t B) {
  if (B <= 0 || N <= 1024 * B) return 1;
  const int64_t s = (N + 1024 * B - 1) / (1024 * B);
  return (int)(s > 256 ? 256 : s);
}

size_t min_bytes(int64_t N, int64_t B) {
  const size_t n = (size_t)(N > 0 ? N : 0), b = (size_t)(B > 0 ? B : 0);
  const size_t S = (size_t)min_slices(N, B);
  return kMinHeaderBytes + 3 * min_align256(b * 8) + min_align256(b * 4) + min_align256(b * 3 * sizeof(float)) +
         2 * min_align256(n * 3 * sizeof(float)) + min_align256(b * S * 4 * sizeof(double)) + 256;  // + room to align the pointer
}

MinState carve_min(void* ws, int64_t N, int64_t B) {
  char* p = reinterpret_cast<char*>(min_align256(reinterpret_cast<size_t>(ws)));
  const size_t n = (size_t)(N > 0 ? N : 0), b = (size_t)(B > 0 ? B : 0);
  MinState st;
  st.head = reinterpret_cast<uint32_t*>(p);
  st.start = reinterpret_cast<double*>(p + 16);
  p += kMinHeaderBytes;
  st.dt = reinterpret_cast<double*>(p);
  p += min_align256(b * 8);
  st.alpha = reinterpret_cast<double*>(p);
  p += min_align256(b * 8);
  st.conv = reinterpret_cast<int64_t*>(p);
  p += min_align256(b * 8);
  st.n_pos = reinterpret_cast<int32_t*>(p);
  p += min_align256(b * 4);
  st.coef = reinterpret_cast<float*>(p);
  p += min_align256(b * 3 * sizeof(float));
  st.x_keep = reinterpret_cast<float*>(p);
  p += min_align256(n * 3 * sizeof(float));
  st.v_keep = reinterpret_cast<float*>(p);
  p += min_align256(n * 3 * sizeof(float));
  st.slices = reinterpret_cast<double*>(p);
  return st;
}

__device__ __forceinline__ uint64_t min_step(const MinState& st) { return (uint64_t)st.head[0] | ((uint64_t)st.head[1] << 32); }

// grid (B, S): slice s of molecule m -> slices[m, s, 0..3].  Threads stride the atoms, lanes by the xor tree, waves in turn.
__global__ __launch_bounds__(kMinThreads) void k_min_reduce(MinState st, const int* __restrict__ counts, const int* __restrict__ mstart,
                                                            const int* __restrict__ mend, int N, int B, int S,
                                                            const int64_t* __restrict__ batch, const float* __restrict__ vel,
                                                            const float* __restrict__ forces, const uint8_t* __restrict__ fixed) {
  __shared__ double sh[4][kMinThreads / 64];
  if (st.head[2]) return;               // frozen
  if (counts && counts[2]) return;      // overflowed: stale forces, the controller latches it
  const int m = blockIdx.x, s = blockIdx.y;
  const bool filter = counts ? counts[3] != 0 : batch != nullptr;
  int a = 0, b = N;
  if (counts && !filter) {
    a = mstart[m];
    b = mend[m];
    a = a < 0 ? 0 : a;
    b = b > N ? N : b;
    b = b < a ? a : b;
  }
  const int64_t len = b - a;
  const int i0 = a + (int)(len * s / S), i1 = a + (int)(len * (s + 1) / S);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = i0 + (int)threadIdx.x; i < i1; i += kMinThreads) {
    if (filter && batch && batch[i] != m) continue;  // (no batch vector: one molecule)
    float v[3], f[3], t[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      v[d] = vel[i * 3 + d];
      f[d] = forces[i * 3 + d];
    }
    tn_min::atom_terms(v, f, fixed && fixed[i], t);
    acc[0] += (double)t[0];
    acc[1] += (double)t[1];
    acc[2] += (double)t[2];
    acc[3] = (double)t[1] > acc[3] ? (double)t[1] : acc[3];
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    acc[0] += __shfl_xor(acc[0], o, 64);
    acc[1] += __shfl_xor(acc[1], o, 64);
    acc[2] += __shfl_xor(acc[2], o, 64);
    const double other = __shfl_xor(acc[3], o, 64);
    acc[3] = other > acc[3] ? other : acc[3];
  }
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[k][threadIdx.x >> 6] = acc[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double* out = st.slices + ((int64_t)m * S + s) * 4;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = ((sh[k][0] + sh[k][1]) + sh[k][2]) + sh[k][3];
    double mx = sh[3][0];
#pragma unroll
    for (int w = 1; w < kMinThreads / 64; ++w) mx = sh[3][w] > mx ? sh[3][w] : mx;
    out[3] = mx;
  }
}

struct MinCtlArgs {
  int B, S;
  tn_min::FireParams p;
  const int* counts;  // the graph's counters, or NULL
  const float* energy;
  float* epot_row;
  float* fmax_row;
  double* sums_row;  // [B, 4]
  float* coef_row;   // [B, 3]
  double* dt_row;
  double* alpha_row;
  int64_t* conv_row;
  MinState st;
};

// the sums of molecule m (slices in slice order) and its state (after a reset: the start values of the header)
__device__ __forceinline__ void min_load(const MinCtlArgs& a, int m, bool fresh, double sums[4], tn_min::FireState* s) {
  const double* sl = a.st.slices + (int64_t)m * a.S * 4;
  sums[0] = sums[1] = sums[2] = sums[3] = 0.0;
  for (int k = 0; k < a.S; ++k) {
    sums[0] += sl[k * 4 + 0];
    sums[1] += sl[k * 4 + 1];
    sums[2] += sl[k * 4 + 2];
    sums[3] = sl[k * 4 + 3] > sums[3] ? sl[k * 4 + 3] : sums[3];
  }
  if (fresh) {
    s->dt = a.st.start[0];
    s->alpha = a.st.start[1];
    s->n_pos = 0;
    s->converged_at = -1;
  } else {
    s->dt = a.st.dt[m];
    s->alpha = a.st.alpha[m];
    s->n_pos = a.st.n_pos[m];
    s->converged_at = a.st.conv[m];
  }
}

// ONE block striding the molecules, after k_min_reduce.  Pass 1: is any molecule's move unusable?  Pass 2, only when none is:
// every molecule's state, coefficients and log rows; then thread 0 advances the step counter (the first control after a reset
// belongs to the start geometry and counts no step).  The move is a function of what pass 1 read, so pass 2 evaluates it again.
__global__ __launch_bounds__(kMinThreads) void k_min_control(MinCtlArgs a) {
  __shared__ int bad;
  if (a.st.head[2]) return;  // frozen
  if (a.counts && a.counts[2]) {
    if (threadIdx.x == 0) a.st.head[2] = 1u;
    return;
  }
  const bool fresh = a.st.head[3] != 0;
  const uint64_t step = min_step(a.st) + (fresh ? 0 : 1);
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();  // (every thread has read the header by now: thread 0 rewrites it at the end)
  int flag = 0;
  double sums[4];
  float coef[3];
  tn_min::FireState s;
  for (int m = threadIdx.x; m < a.B; m += kMinThreads) {
    min_load(a, m, fresh, sums, &s);
    flag |= tn_min::fire_control(&s, a.p, sums[0], sums[1], sums[2], sums[3], (int64_t)step, coef) == tn_min::FIRE_UNUSABLE;
  }
  if (flag) bad = 1;  // (every writer stores the same value)
  __syncthreads();
  if (bad) {
    if (threadIdx.x == 0) a.st.head[2] = 2u;
    return;
  }
  for (int m = threadIdx.x; m < a.B; m += kMinThreads) {
    min_load(a, m, fresh, sums, &s);
    tn_min::fire_control(&s, a.p, sums[0], sums[1], sums[2], sums[3], (int64_t)step, coef);
    a.st.dt[m] = s.dt;
    a.st.alpha[m] = s.alpha;
    a.st.n_pos[m] = s.n_pos;
    a.st.conv[m] = s.converged_at;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.st.coef[m * 3 + k] = coef[k];
    if (a.energy && a.epot_row) a.epot_row[m] = a.energy[m];
    if (a.fmax_row) a.fmax_row[m] = (float)sqrt(sums[3]);
    if (a.sums_row)
#pragma unroll
      for (int k = 0; k < 4; ++k) a.sums_row[(int64_t)m * 4 + k] = sums[k];
    if (a.coef_row)
#pragma unroll
      for (int k = 0; k < 3; ++k) a.coef_row[(int64_t)m * 3 + k] = coef[k];
    if (a.dt_row) a.dt_row[m] = s.dt;
    if (a.alpha_row) a.alpha_row[m] = s.alpha;
    if (a.conv_row) a.conv_row[m] = s.converged_at;
  }
  if (threadIdx.x == 0) {
    a.st.head[0] = (uint32_t)step;
    a.st.head[1] = (uint32_t)(step >> 32);
    a.st.head[3] = 0u;
  }
}

struct MinAtomArgs {
  int N, B;
  float* pos;
  float* vel;
  const float* forces;
  float* forces_keep;
  const uint8_t* fixed;
  const int64_t* batch;
  const int* counts;  // the graph's counters, or NULL
  MinState st;
};

// one thread per atom, the caller's atom order.  ACCEPT (after k_min_control): keep the forces of the evaluation, or, when it
// overflowed, go back to the state the last move saved.  MOVE: save x and v, then the update with the molecule's coefficients.
template <bool ACCEPT, bool MOVE>
__global__ __launch_bounds__(kMinThreads) void k_min_atoms(MinAtomArgs a) {
  const int i = blockIdx.x * kMinThreads + threadIdx.x;
  if (i >= a.N) return;
  const uint32_t status = a.st.head[2], fresh = a.st.head[3];
  if (status) {
    // the evaluation before this launch overflowed (the controller has just latched it): back to the last completed step.  A
    // later launch that finds the flag still set writes the same values again; nothing was ever saved before the first control.
    if (ACCEPT && status == 1u && !fresh && a.counts && a.counts[2]) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        a.pos[i * 3 + d] = a.st.x_keep[i * 3 + d];
        a.vel[i * 3 + d] = a.st.v_keep[i * 3 + d];
      }
    }
    return;
  }
  if (fresh) return;  // (OPEN straight after a reset: there are no coefficients yet)
  float x[3], v[3], f[3];
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
      v[d] = a.vel[i * 3 + d];
      a.st.x_keep[i * 3 + d] = x[d];
      a.st.v_keep[i * 3 + d] = v[d];
    }
    if (a.st.conv[m] >= 0 || (a.fixed && a.fixed[i])) {  // frozen: a branch, not a product with 0 - x keeps its bits
#pragma unroll
      for (int d = 0; d < 3; ++d) a.vel[i * 3 + d] = 0.f;
      return;
    }
    tn_min::atom_move(x, v, f, a.st.coef[m * 3 + 0], a.st.coef[m * 3 + 1], a.st.coef[m * 3 + 2]);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a.pos[i * 3 + d] = x[d];
      a.vel[i * 3 + d] = v[d];
    }
  }
}

__global__ void k_min_reset(MinState st, uint64_t step0, double dt0, double alpha0) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st.head[0] = (uint32_t)step0;
    st.head[1] = (uint32_t)(step0 >> 32);
    st.head[2] = 0u;
    st.head[3] = 1u;
    st.start[0] = dt0;
    st.start[1] = alpha0;
  }
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_min_workspace_bytes(int64_t n_atoms, int64_t n_mol, size_t* bytes) {
  if (!bytes || n_atoms < 0 || n_mol < 0 || n_atoms > INT32_MAX / 4 || n_mol > INT32_MAX / 16) return TMDNET_ERR_INVALID;
  *bytes = min_bytes(n_atoms, n_mol);
  return TMDNET_OK;
}

int tmdnet_min_reset(void* stream, void* min_ws, uint64_t step0, double dt0, double alpha0) {
  if (!min_ws || !(dt0 > 0.0) || !(alpha0 >= 0.0)) return TMDNET_ERR_INVALID;
  hipLaunchKernelGGL(k_min_reset, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), carve_min(min_ws, 0, 0), step0, dt0, alpha0);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_min_advance(tmdnet_model* m, void* stream, void* graph_ws, void* min_ws, int64_t n_atoms, int64_t n_mol, int32_t phase,
                       float* pos, float* vel, const float* forces, const float* energy, const uint8_t* fixed, const int64_t* batch,
                       float* forces_keep, double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha0, double f_alpha,
                       double max_step, double fmax, float* epot_log_row, float* fmax_log_row, double* sums_log_row,
                       float* coef_log_row, double* dt_log_row, double* alpha_log_row, int64_t* converged_log_row) {
  if (!min_ws || !pos || !vel || !forces || n_atoms < 0 || n_atoms > INT32_MAX / 4 || n_mol < 1 || n_mol > INT32_MAX / 16)
    return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MIN_OPEN && phase != TMDNET_MIN_MIDDLE && phase != TMDNET_MIN_CLOSE) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (!(fmax > 0.0) || !(dt_max > 0.0) || !(max_step > 0.0) || !(f_inc > 0.0) || !(f_dec > 0.0) || !(f_alpha > 0.0) || !(alpha0 >= 0.0) ||
      n_min < 0)
    return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n_atoms, B = (int)n_mol;
  const MinState st = carve_min(min_ws, n_atoms, n_mol);
  const int* counts = nullptr;
  const int* mstart = nullptr;
  const int* mend = nullptr;
  if (graph_ws) {
    const Graph g = carve_graph(graph_ws, n_atoms, n_mol, (int64_t)m->hp.max_num_neighbors * n_atoms, nullptr);
    counts = g.counts;
    mstart = g.mstart;
    mend = g.mend;
  }
  const dim3 block(kMinThreads);
  if (phase != TMDNET_MIN_OPEN) {
    const int S = min_slices(n_atoms, n_mol);
    hipLaunchKernelGGL(k_min_reduce, dim3(B, S), block, 0, s, st, counts, mstart, mend, N, B, S, batch, vel, forces, fixed);
    MinCtlArgs c;
    c.B = B;
    c.S = S;
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
    c.epot_row = epot_log_row;
    c.fmax_row = fmax_log_row;
    c.sums_row = sums_log_row;
    c.coef_row = coef_log_row;
    c.dt_row = dt_log_row;
    c.alpha_row = alpha_log_row;
    c.conv_row = converged_log_row;
    c.st = st;
    hipLaunchKernelGGL(k_min_control, dim3(1), block, 0, s, c);
  }
  if (N > 0) {
    MinAtomArgs a;
    a.N = N;
    a.B = B;
    a.pos = pos;
    a.vel = vel;
    a.forces = forces;
    a.forces_keep = forces_keep;
    a.fixed = fixed;
    a.batch = batch;
    a.counts = counts;
    a.st = st;
    const dim3 grid((N + kMinThreads - 1) / kMinThreads);
    if (phase == TMDNET_MIN_OPEN)
      hipLaunchKernelGGL((k_min_atoms<false, true>), grid, block, 0, s, a);
    else if (phase == TMDNET_MIN_MIDDLE)
      hipLaunchKernelGGL((k_min_atoms<true, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((k_min_atoms<true, false>), grid, block, 0, s, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return m ? fail(m, TMDNET_ERR_HIP, std::string("tmdnet_min_advance: ") + hipGetErrorString(e)) : TMDNET_ERR_HIP;
  return TMDNET_OK;
}

int tmdnet_min_status(void* stream, void* min_ws, uint64_t host[2]) {
  if (!min_ws || !host) return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint32_t head[3] = {0, 0, 0};
  if (hipMemcpyAsync(head, carve_min(min_ws, 0, 0).head, sizeof(head), hipMemcpyDeviceToHost, s) != hipSuccess) return TMDNET_ERR_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return TMDNET_ERR_HIP;
  host[0] = (uint64_t)head[0] | ((uint64_t)head[1] << 32);
  host[1] = head[2];
  return head[2] == 1 ? TMDNET_ERR_OVERFLOW : head[2] ? TMDNET_ERR_STATE : TMDNET_OK;
}

}  // extern "C"
