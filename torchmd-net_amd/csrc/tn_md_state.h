// State and kinetic-energy reduction of the device-resident MD loop, shared by the integrator launches of tn_md.hip (one thread per
// atom) and tn_md_cons.hip (one group of lanes per constraint cluster): the layout of the caller's workspace and the kernels that
// follow a closing launch.  Everything sits in an unnamed namespace: each of the two files gets its own copy.
#pragma once
#include <stdint.h>

#include "tn_common.h"

namespace tn {

namespace {

constexpr int kThreads = 256;
constexpr size_t kHeaderBytes = 256;

struct MdState {  // views into the caller's workspace
  uint32_t* head;  // [0] step lo, [1] step hi, [2] status (sticky, 1 = an evaluation overflowed, 2 = an unusable barostat move,
                   // 3 = a constraint cluster did not converge, 4 = a bias that was not finite, 5 = an unusable thermostat move,
                   // 6 = the gate of a committee stopped the loop at a completed step: tn_committee.hip)
  float* x_keep;   // [N, 3] positions at the last completed step
  float* v_keep;   // [N, 3]
  float* part;     // [N]    0.5 m v^2 per atom, caller's order
  float* slices;   // [B, S] (S > 1 only)
};

inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

inline int ke_slices(int64_t N, int64_t B) {
  if (B <= 0 || N <= 1024 * B) return 1;
  const int64_t s = (N + 1024 * B - 1) / (1024 * B);
  return (int)(s > 256 ? 256 : s);
}

inline size_t md_bytes(int64_t N, int64_t B) {
  const int S = ke_slices(N, B);
  const size_t n = (size_t)(N > 0 ? N : 0);
  size_t t = kHeaderBytes + 2 * align256(n * 3 * sizeof(float)) + align256(n * sizeof(float));
  if (S > 1) t += align256((size_t)B * S * sizeof(float));
  return t + 256;  // room to align the caller's pointer
}

inline MdState carve_md(void* ws, int64_t N, int64_t B) {
  char* p = reinterpret_cast<char*>(align256(reinterpret_cast<size_t>(ws)));
  const size_t n = (size_t)(N > 0 ? N : 0);
  MdState st;
  st.head = reinterpret_cast<uint32_t*>(p);
  p += kHeaderBytes;
  st.x_keep = reinterpret_cast<float*>(p);
  p += align256(n * 3 * sizeof(float));
  st.v_keep = reinterpret_cast<float*>(p);
  p += align256(n * 3 * sizeof(float));
  st.part = reinterpret_cast<float*>(p);
  p += align256(n * sizeof(float));
  st.slices = reinterpret_cast<float*>(p);
  return st;
}

// sum over the block in a fixed order (lanes by the wave tree, waves in turn), result in every thread
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// grid (B, S), after a closing launch: slice s of molecule m -> out[m * S + s] (S == 1: the log row itself).  Block (0, 0) also
// keeps the books of the step: it latches an overflow into the status word, or copies the energies into the log row and
// advances the step counter (plain stores from one vector lane; no other block of this launch reads the counter).  CONS (the
// constrained loop, tn_md_cons.hip): `fail` is the word a cluster ORs when its constraints did not converge; it is latched as
// status 3 in the same way, with no log row and no step.
template <bool CONS>
__global__ __launch_bounds__(kThreads) void k_md_ke_reduce(MdState st, const int* __restrict__ counts, const int* __restrict__ mstart,
                                                           const int* __restrict__ mend, int N, int B, int S,
                                                           const int64_t* __restrict__ batch, const float* __restrict__ energy,
                                                           float* __restrict__ epot_row, float* __restrict__ out,
                                                           const uint32_t* __restrict__ fail) {
  __shared__ float sh[4];
  if (st.head[2]) return;
  const int m = blockIdx.x, s = blockIdx.y;
  const bool first = m == 0 && s == 0 && threadIdx.x == 0;
  if (counts && counts[2]) {
    if (first) st.head[2] = 1u;
    return;
  }
  if (CONS && fail[0]) {
    if (first) st.head[2] = 3u;
    return;
  }
  const bool filter = counts ? counts[3] != 0 : batch != nullptr;
  int a = 0, b = N;
  if (counts && !filter) {
    a = mstart[m];
    b = mend[m];
  }
  const int64_t len = b - a;
  const int i0 = a + (int)(len * s / S), i1 = a + (int)(len * (s + 1) / S);
  float v = 0.f;
  for (int i = i0 + (int)threadIdx.x; i < i1; i += kThreads) {
    if (filter && batch && batch[i] != m) continue;  // (no batch vector: one molecule)
    v += st.part[i];
  }
  v = block_sum(v, sh);
  if (threadIdx.x == 0) {
    if (out) out[(int64_t)m * S + s] = v;
    if (s == 0 && energy && epot_row) epot_row[m] = energy[m];
  }
  if (first) {
    const uint64_t step = ((uint64_t)st.head[0] | ((uint64_t)st.head[1] << 32)) + 1;
    st.head[0] = (uint32_t)step;
    st.head[1] = (uint32_t)(step >> 32);
  }
}

// one thread per molecule: the slice sums in slice order.  The status word is already latched by k_md_ke_reduce.
__global__ __launch_bounds__(kThreads) void k_md_ke_finish(MdState st, const int* __restrict__ counts, int B, int S, float* __restrict__ ekin_row) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= B || st.head[2] || (counts && counts[2])) return;
  float v = 0.f;
  for (int s = 0; s < S; ++s) v += st.slices[(int64_t)m * S + s];
  ekin_row[m] = v;
}

}  // namespace

}  // namespace tn
