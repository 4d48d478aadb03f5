// State and kinetic-energy reduction of the device-resident MD loop, shared by everything that acts on its workspace: the
// integrator launches of tn_md.hip (one thread per atom) and tn_md_cons.hip (one group of lanes per constraint cluster), the
// barostats, thermostats, replica exchange, bias and committee gate.  The layout of the caller's workspace and the kernels that
// follow a closing launch.  Everything sits in an unnamed namespace: every file that includes this header gets its own copy.
#pragma once
#include <stdint.h>

#include "tn_common.h"
#include "tn_loop.h"

namespace tn {

namespace {

struct MdState {  // views into the caller's workspace
  uint32_t* head;  // [0] step lo, [1] step hi, [2] status (sticky, 1 = an evaluation overflowed, 2 = an unusable barostat move,
                   // 3 = a constraint cluster did not converge, 4 = a bias that was not finite, 5 = an unusable thermostat move,
                   // 6 = the gate of a committee stopped the loop at a completed step: tn_committee.hip)
  float* x_keep;   // [N, 3] positions at the last completed step
  float* v_keep;   // [N, 3]
  float* part;     // [N]    0.5 m v^2 per atom, caller's order
  float* slices;   // [B, S] (S > 1 only)
};

inline MdState md_layout(LoopCarver& c, int64_t N, int64_t B) {
  const int S = mol_slices(N, B);
  const size_t n = (size_t)(N > 0 ? N : 0);
  MdState st;
  st.head = c.take<uint32_t>(kHeaderBytes / sizeof(uint32_t));
  st.x_keep = c.take<float>(n * 3);
  st.v_keep = c.take<float>(n * 3);
  st.part = c.take<float>(n);
  st.slices = c.take<float>(S > 1 ? (size_t)B * S : 0);
  return st;
}

inline size_t md_bytes(int64_t N, int64_t B) {
  return layout_bytes([&](LoopCarver& c) { md_layout(c, N, B); });
}

inline MdState carve_md(void* ws, int64_t N, int64_t B) {
  LoopCarver c(ws);
  return md_layout(c, N, B);
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
  __shared__ float sh[1][kThreads / 64];
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
  const SliceRange r = mol_slice_range(counts, mstart, mend, N, S, batch, m, s);
  float v = 0.f;
  for (int i = r.i0 + (int)threadIdx.x; i < r.i1; i += kThreads) {
    if (slice_skips(r, batch, i, m)) continue;
    v += st.part[i];
  }
  v = block_sum(v, sh);
  if (threadIdx.x == 0) {
    if (out) out[(int64_t)m * S + s] = v;
    if (s == 0 && energy && epot_row) epot_row[m] = energy[m];
  }
  if (first) loop_set_step(st.head, loop_step(st.head) + 1);
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
