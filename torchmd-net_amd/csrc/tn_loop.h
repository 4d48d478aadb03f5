// What every captured loop needs on the device side, in one place: the MD loop and its barostats, thermostats, constraints, replica
// exchange, bias, observer and committee gate (tn_md*.hip, tn_remd.hip, tn_bias.hip, tn_observe.hip, tn_committee.hip) and the
// optimisers (tn_min.hip, tn_lbfgs.hip, tn_neb.hip).  Workspace layout (align256, Carver), the slices of a molecule's atoms (mol_slices, mol_slice_range),
// the 64-bit step counter of a workspace header, the fixed-order block reduction, the prelude and tail of a C entry (loop_graph,
// loop_launch_result), the opening half of an MD step and the two-pass per-molecule controller.  Nothing here belongs to one loop
// only.  Everything sits in an unnamed namespace: every file that includes this header gets its own copy.  The host parts compile
// without a device (tests/loop_host.hip).
#pragma once
#include <stdint.h>

#include <string>
#include <type_traits>

#include "tn_common.h"
#include "tn_md_math.h"
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

// The controller of a per-molecule move (a barostat, a global thermostat): ONE block of kThreads, after the closing launch and its
// kinetic-energy reduction, which has latched an overflow and advanced the step counter - the O step of this MD step used the
// value before, and so does the move.  Pass 1: eval(m, step) of every molecule, non-zero when its move is unusable; pass 2, only
// when none is: commit(m, step) writes.  Otherwise the status word becomes `status_code` and nothing else is written.  A molecule
// belongs to one thread in both passes (thread t: t, t + kThreads, ...), so with B <= kThreads what eval left in the thread's
// registers is still that molecule's in commit.
template <class St, class Eval, class Commit>
__device__ __forceinline__ void per_molecule_move(const St& st, const int* counts, int B, uint32_t status_code, Eval eval, Commit commit) {
  __shared__ int bad;
  if (st.head[2]) return;           // frozen
  if (counts && counts[2]) return;  // (the reduction has latched it: everything stays that of the last completed step)
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const uint64_t step = loop_step(st.head) - 1;
  int flag = 0;
  for (int m = threadIdx.x; m < B; m += kThreads) flag |= eval(m, step);
  if (flag) bad = 1;  // (every writer stores the same value)
  __syncthreads();
  if (bad) {
    if (threadIdx.x == 0) st.head[2] = status_code;
    return;
  }
  for (int m = threadIdx.x; m < B; m += kThreads) commit(m, step);
}

}  // namespace

}  // namespace tn
