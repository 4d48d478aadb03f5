// What every captured loop needs on the device side, in one place: the MD loop and its barostats, thermostats, constraints, replica
// exchange, bias, observer and committee gate (tn_md*.hip, tn_remd.hip, tn_bias.hip, tn_observe.hip, tn_committee.hip) and the
// optimisers (tn_min.hip, tn_lbfgs.hip, tn_neb.hip, tn_dimer.hip, tn_irc.hip, tn_scan.hip, tn_hop.hip).  Workspace layout (align256,
// Carver), the slices of a molecule's atoms (mol_slices, mol_slice_range) and their sums in slice order (slice_sums), the header of a
// workspace - its 64-bit step counter, status and "fresh" words, its reset and its read-back (loop_head_reset, loop_status_result,
// loop_read_status) -, the fixed-order block reduction, the prelude and tail of a C entry (loop_graph, loop_launch_result), the
// per-unit FIRE state and its log rows (FireUnits, fire_load, fire_store, FireRows), the opening half of an MD step and the two
// one-block controllers (per_molecule_move of the MD loop, optimiser_control of the optimisers) on block_worst.  Nothing here belongs
// to one loop only.  Everything sits in an unnamed namespace: every file that includes this header gets its own copy.  The host parts
// compile without a device (tests/loop_host.hip).
//
// Not here: tmdnet_committee_status reads a 64-bit header of another shape (tn_committee.hip), and k_lbfgs_control, one wave per
// molecule over several blocks, keeps its own body - a lane adds one entry of the slices, as a thread of k_hop_finish does - and
// takes only the header's names, reset and read-back from this file.
#pragma once
#include <stdint.h>

#include <string>
#include <type_traits>

#include "tn_common.h"
#include "tn_md_math.h"
#include "tn_min_math.h"
#include "tn_model.h"

namespace tn {

namespace {

constexpr int kThreads = 256;
constexpr size_t kHeaderBytes = 256;

// ---- layout ---------------------------------------------------------------------------------------------------------------------
inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

// tn_model.h's bump Carver on a caller's loop workspace: it starts at the 256-aligned base, take<T>(count) hands out the arrays one
// after the other, each on a multiple of 256 bytes (null pointers from a null base), and bytes() reports what it has handed out.
// A workspace has ONE function that walks its arrays with take(); its size entry runs it from a null base (layout_bytes), its
// carve_*() from the caller's pointer, so the sum and the pointers cannot disagree.
struct LoopCarver : Carver {
  explicit LoopCarver(void* ws) : Carver(reinterpret_cast<void*>(align256(reinterpret_cast<size_t>(ws)))) {}
  size_t bytes() const { return off; }
};

// what a *_workspace_bytes entry answers for the arrays `walk` takes: their bytes and room to align the caller's pointer
template <class Walk>
inline size_t layout_bytes(Walk&& walk) {
  LoopCarver c(nullptr);
  walk(c);
  return c.bytes() + 256;
}

// ---- slices of a molecule ---------------------------------------------------------------------------------------------------------
// slices per molecule of a per-molecule reduction, grid (B, S): at most 1 024 atoms per slice on average, at most 256 slices
__host__ __device__ inline int mol_slices(int64_t N, int64_t B) {
  if (B <= 0 || N <= 1024 * B) return 1;
  const int64_t s = (N + 1024 * B - 1) / (1024 * B);
  return (int)(s > 256 ? 256 : s);
}

struct SliceRange {  // the atoms slice s of molecule m strides, and whether they are filtered by `batch`
  int i0, i1;
  bool filter;
};

// The atoms of molecule m are mstart[m]..mend[m] of the graph workspace when those ranges are valid; otherwise (Graph::counts[3]:
// unsorted batch, or molecules interleaved by the cell list; or no graph workspace) all N atoms, filtered by `batch`.  The range's
// start is clamped to >= 0, its end to <= N and to >= the start: for a valid graph that changes nothing, and whatever the ranges
// hold, a slice is empty or lies inside the arrays.
__host__ __device__ __forceinline__ SliceRange mol_slice_range(const int* counts, const int* mstart, const int* mend, int N, int S,
                                                               const int64_t* batch, int m, int s) {
  SliceRange r;
  r.filter = counts ? counts[3] != 0 : batch != nullptr;
  int a = 0, b = N;
  if (counts && !r.filter) {
    a = mstart[m];
    b = mend[m];
    a = a < 0 ? 0 : a;
    b = b > N ? N : b;
    b = b < a ? a : b;
  }
  const int64_t len = b - a;
  r.i0 = a + (int)(len * s / S);
  r.i1 = a + (int)(len * (s + 1) / S);
  return r;
}

// atom i of the range is not molecule m's (no batch vector: one molecule)
__host__ __device__ __forceinline__ bool slice_skips(const SliceRange& r, const int64_t* batch, int i, int m) {
  return r.filter && batch && batch[i] != m;
}

// ---- the step counter: 64 bits in words 0 (lo) and 1 (hi) of a workspace header ---------------------------------------------------
__host__ __device__ __forceinline__ uint64_t loop_step(const uint32_t* head) { return (uint64_t)head[0] | ((uint64_t)head[1] << 32); }

__host__ __device__ __forceinline__ void loop_set_step(uint32_t* head, uint64_t step) {
  head[0] = (uint32_t)step;
  head[1] = (uint32_t)(step >> 32);
}

// ---- the header protocol: status and "fresh" behind the counter ----------------------------------------------------------------------
// Word 2 is the sticky status: 0 running, 1 an evaluation overflowed, anything else the state was unusable (2 for the optimisers,
// with the cause in a word of the loop's own choosing).  Word 3 is 1 from a reset until the first control, which belongs to the start
// geometry and counts no step (the MD loop and minima hopping have no such word).  Once the status is set every launch returns at
// once, so everything stays that of the last completed step until the next reset.
constexpr int kHeadStepLo = 0, kHeadStepHi = 1, kHeadStatus = 2, kHeadFresh = 3;
constexpr uint32_t kStatusOverflow = 1u, kStatusUnusable = 2u;

// what the reset kernels of the optimisers share (one thread); a loop's own start values stay in its kernel
__host__ __device__ __forceinline__ void loop_head_reset(uint32_t* head, uint64_t step0, int cause_word) {
  loop_set_step(head, step0);
  head[kHeadStatus] = 0u;
  head[kHeadFresh] = 1u;
  if (cause_word >= 0) head[cause_word] = 0u;
}

// what a status entry answers from a copy of the header: host[0] the step, host[1] the status, host[2] (n_host > 2) the cause of
// status 2, 0 otherwise or without a cause word
__host__ __device__ inline int loop_status_result(const uint32_t* head, int cause_word, uint64_t* host, int n_host) {
  const uint32_t status = head[kHeadStatus];
  host[0] = loop_step(head);
  host[1] = status;
  if (n_host > 2) host[2] = status == kStatusUnusable && cause_word >= 0 ? head[cause_word] : 0;
  return status == kStatusOverflow ? TMDNET_ERR_OVERFLOW : status ? TMDNET_ERR_STATE : TMDNET_OK;
}

// the read-back of every status entry but the committee's: `words` header words from the device, one synchronisation
inline int loop_read_status(void* stream, const uint32_t* dev_head, int words, int cause_word, uint64_t* host, int n_host) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint32_t head[kHeaderBytes / sizeof(uint32_t)] = {};
  if (hipMemcpyAsync(head, dev_head, (size_t)words * sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess) return TMDNET_ERR_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return TMDNET_ERR_HIP;
  return loop_status_result(head, cause_word, host, n_host);
}

// ---- the sums of a unit: its slices in slice order -------------------------------------------------------------------------------
// out[k] starts from 0.0 and takes entry k of slices 0 .. S - 1 (rows of `stride` doubles) in that order: the sum, or, where bit k of
// MAXMASK is set, the maximum (the newcomer replaces the held value when it is greater) - the association of block_reduce_rows.
template <int K, unsigned MAXMASK>
__host__ __device__ __forceinline__ void slice_sums(const double* slices, int S, int stride, double* out) {
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = 0.0;
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double v = slices[(int64_t)s * stride + k];
      if ((MAXMASK >> k) & 1u)
        out[k] = v > out[k] ? v : out[k];
      else
        out[k] += v;
    }
}

// ---- the FIRE state of a unit (a molecule, a band, a dimer, a scan point) -------------------------------------------------------------
struct FireUnits {  // views into a workspace, filled from a loop's *State
  double* dt;           // [units]
  double* alpha;        // [units]
  int64_t* conv;        // [units] converged_at
  int32_t* n_pos;       // [units]
  float* coef;          // [units, 3] c_v, c_f, d of the next move
  const double* start;  // [0] dt0, [1] alpha0 of the header
};

template <class St>
__host__ __device__ __forceinline__ FireUnits fire_units(const St& st) {
  return {st.dt, st.alpha, st.conv, st.n_pos, st.coef, st.start};
}

// the state of `unit`; at the first control after a reset the start values of the header
__host__ __device__ __forceinline__ void fire_load(const FireUnits& u, int unit, bool fresh, tn_min::FireState* s) {
  if (fresh) {
    s->dt = u.start[0];
    s->alpha = u.start[1];
    s->n_pos = 0;
    s->converged_at = -1;
  } else {
    s->dt = u.dt[unit];
    s->alpha = u.alpha[unit];
    s->n_pos = u.n_pos[unit];
    s->converged_at = u.conv[unit];
  }
}

__host__ __device__ __forceinline__ void fire_store(const FireUnits& u, int unit, const tn_min::FireState& s, const float coef[3]) {
  u.dt[unit] = s.dt;
  u.alpha[unit] = s.alpha;
  u.n_pos[unit] = s.n_pos;
  u.conv[unit] = s.converged_at;
#pragma unroll
  for (int k = 0; k < 3; ++k) u.coef[unit * 3 + k] = coef[k];
}

struct FireRows {  // the log rows of one step, each [units, ...] or NULL
  float* epot;
  float* fmax;
  double* sums;  // [units, 4]
  float* coef;   // [units, 3]
  double* dt;
  double* alpha;
  int64_t* conv;

  // `energy`: the unit's energy, or NULL (a loop whose energy row has another shape passes epot = NULL and writes it itself);
  // fmax is the root of `fmax2`
  __host__ __device__ __forceinline__ void write(int unit, const float* energy, const double sums4[4], double fmax2, const float coef3[3],
                                                 const tn_min::FireState& s) const {
    if (energy && epot) epot[unit] = *energy;
    if (fmax) fmax[unit] = (float)sqrt(fmax2);
    if (sums)
#pragma unroll
      for (int k = 0; k < 4; ++k) sums[(int64_t)unit * 4 + k] = sums4[k];
    if (coef)
#pragma unroll
      for (int k = 0; k < 3; ++k) coef[(int64_t)unit * 3 + k] = coef3[k];
    if (dt) dt[unit] = s.dt;
    if (alpha) alpha[unit] = s.alpha;
    if (conv) conv[unit] = s.converged_at;
  }
};

// ---- the prelude and the tail of a C entry ------------------------------------------------------------------------------------------
struct LoopGraph {  // the graph workspace's counters and molecule ranges, or nulls without one
  int* counts;
  const int* mstart;
  const int* mend;
};

inline LoopGraph loop_graph(tmdnet_model* m, void* graph_ws, int64_t n_atoms, int64_t n_mol) {
  if (!graph_ws) return {nullptr, nullptr, nullptr};
  const Graph g = carve_graph(graph_ws, n_atoms, n_mol, (int64_t)m->hp.max_num_neighbors * n_atoms, nullptr);
  return {g.counts, g.mstart, g.mend};
}

// after the launches of an entry: TMDNET_OK, or the launch error (with its text in the handle when there is one)
inline int loop_launch_result(tmdnet_model* m, const char* entry) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return TMDNET_OK;
  return m ? fail(m, TMDNET_ERR_HIP, std::string(entry) + ": " + hipGetErrorString(e)) : TMDNET_ERR_HIP;
}

// ---- the fixed-order block reduction ------------------------------------------------------------------------------------------------
// K values per thread of a block of kThreads, reduced in ONE association whatever the type: lanes by the xor tree over the wave's 64
// lanes (1, 2, 4, ... 32), then the waves in wave order, left to right: ((w0 + w1) + w2) + w3.  Bit k of MAXMASK: entry k takes the
// maximum (the newcomer replaces the held value when it is greater) instead of the sum.  No atomics: repeats are bit-identical.

// the wave step, result in every lane (fp32 sums: tn_common.h's wave_sum pairs the same lanes with DPP moves)
template <int K, unsigned MAXMASK, class T>
__device__ __forceinline__ void wave_reduce(T (&acc)[K]) {
  if constexpr (std::is_same<T, float>::value && K == 1 && MAXMASK == 0) {
    acc[0] = wave_sum(acc[0]);
  } else {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const T other = __shfl_xor(acc[k], o, 64);
        if ((MAXMASK >> k) & 1u)
          acc[k] = other > acc[k] ? other : acc[k];
        else
          acc[k] += other;
      }
  }
}

// the wave step, then wave w's values into sh[k][w]; every thread may read them after it
template <int K, unsigned MAXMASK, class T>
__device__ __forceinline__ void block_reduce_waves(T (&acc)[K], T (*sh)[kThreads / 64]) {
  wave_reduce<K, MAXMASK>(acc);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k][threadIdx.x >> 6] = acc[k];
  __syncthreads();
}

// the waves of one entry in wave order (`max`: the entry takes the maximum)
template <class T>
__device__ __forceinline__ T block_reduce_row(const T* row, bool max) {
  if (!max) return ((row[0] + row[1]) + row[2]) + row[3];
  T mx = row[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) mx = row[w] > mx ? row[w] : mx;
  return mx;
}

// ... of all K entries (for the one thread that stores them)
template <int K, unsigned MAXMASK, class T>
__device__ __forceinline__ void block_reduce_rows(T (*sh)[kThreads / 64], T* out) {
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = block_reduce_row(sh[k], ((MAXMASK >> k) & 1u) != 0);
}

// fp32 sum over the block, result in every thread
__device__ __forceinline__ float block_sum(float v, float (*sh)[kThreads / 64]) {
  float acc[1] = {v};
  block_reduce_waves<1, 0u>(acc, sh);
  return block_reduce_row(sh[0], false);
}

// ---- pieces of the MD loop's kernels ------------------------------------------------------------------------------------------------
// The opening half of an MD step for atom i on the thread's registers: x and v become the saved state of the last completed step,
// then B, A.  The caller stores x and v.  (St: any view with x_keep and v_keep.)
template <class St>
__device__ __forceinline__ void md_save_and_open(const St& st, int i, float x[3], float v[3], const float f[3], float hk, float dt) {
#pragma unroll
  for (int d = 0; d < 3; ++d) st.x_keep[i * 3 + d] = x[d];
#pragma unroll
  for (int d = 0; d < 3; ++d) st.v_keep[i * 3 + d] = v[d];
  tn_md::open_step(x, v, f, hk, dt);
}

// ---- the one-block controllers ------------------------------------------------------------------------------------------------------
// the largest `mine` of a block, in every thread (an integer in LDS; mine >= 0).  Every thread of the block calls it, once per kernel.
__device__ __forceinline__ int block_worst(int mine) {
  __shared__ int worst;
  if (threadIdx.x == 0) worst = 0;
  __syncthreads();
  if (mine) atomicMax(&worst, mine);
  __syncthreads();
  return worst;
}

// The controller of a per-molecule move (a barostat, a global thermostat): ONE block of kThreads, after the closing launch and its
// kinetic-energy reduction, which has latched an overflow and advanced the step counter - the O step of this MD step used the
// value before, and so does the move.  Pass 1: eval(m, step) of every molecule, non-zero when its move is unusable; pass 2, only
// when none is: commit(m, step) writes.  Otherwise the status word becomes `status_code` and nothing else is written.  A molecule
// belongs to one thread in both passes (thread t: t, t + kThreads, ...), so with B <= kThreads what eval left in the thread's
// registers is still that molecule's in commit.
template <class St, class Eval, class Commit>
__device__ __forceinline__ void per_molecule_move(const St& st, const int* counts, int B, uint32_t status_code, Eval eval, Commit commit) {
  if (st.head[kHeadStatus]) return;  // frozen
  if (counts && counts[2]) return;   // (the reduction has latched it: everything stays that of the last completed step)
  const uint64_t step = loop_step(st.head) - 1;
  int flag = 0;
  for (int m = threadIdx.x; m < B; m += kThreads) flag |= eval(m, step);
  if (block_worst(flag != 0)) {
    if (threadIdx.x == 0) st.head[kHeadStatus] = status_code;
    return;
  }
  for (int m = threadIdx.x; m < B; m += kThreads) commit(m, step);
}

// The controller of an optimiser: ONE block of kThreads striding the units (molecules, bands, dimers, paths, points, walkers), after
// the reductions of the step.  It is the only kernel that writes the status word.  Frozen: nothing.  The evaluation before it
// overflowed (counts[2]): status 1, nothing else.  Pass 1: eval(unit, fresh, step) of every unit, 0 or the cause that makes its move
// unusable (a loop without causes answers 1).  Any: status 2 and, with a cause word, the largest cause; no row, state or counter
// is written.  Pass 2, only when none is: commit(unit, fresh, step) writes the unit's state, coefficients and log rows - the move is
// a function of what pass 1 read, so commit evaluates it again.  Then thread 0 advances the step counter and clears the fresh word;
// the first control after a reset counts no step (`uses_fresh`; false: no such word, the counter always advances).  Every thread
// has read the header before block_worst's barriers, and thread 0 rewrites it behind them.
template <class Eval, class Commit>
__device__ __forceinline__ void optimiser_control(uint32_t* head, const int* counts, int cause_word, bool uses_fresh, int n_units, Eval eval,
                                                  Commit commit) {
  if (head[kHeadStatus]) return;  // frozen
  if (counts && counts[2]) {
    if (threadIdx.x == 0) head[kHeadStatus] = kStatusOverflow;
    return;
  }
  const bool fresh = uses_fresh && head[kHeadFresh] != 0;
  const uint64_t step = loop_step(head) + (fresh ? 0 : 1);
  int cause = 0;
  for (int u = threadIdx.x; u < n_units; u += kThreads) {
    const int c = eval(u, fresh, step);
    cause = c > cause ? c : cause;
  }
  cause = block_worst(cause);
  if (cause) {
    if (threadIdx.x == 0) {
      if (cause_word >= 0) head[cause_word] = (uint32_t)cause;
      head[kHeadStatus] = kStatusUnusable;
    }
    return;
  }
  for (int u = threadIdx.x; u < n_units; u += kThreads) commit(u, fresh, step);
  if (threadIdx.x == 0) {
    loop_set_step(head, step);
    if (uses_fresh) head[kHeadFresh] = 0u;
  }
}

}  // namespace

}  // namespace tn
