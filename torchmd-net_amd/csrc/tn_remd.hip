// Temperature replica exchange (parallel tempering) of the device-resident MD loop: two launches that sit between the closing and
// the opening half of a captured step, so that a batch of B = G R replicas of one system exchanges temperatures inside the HIP
// graph, with no read-back of the energies and no host decision.
//
// Replicas swap TEMPERATURES, not coordinates: nothing of size N moves.  A replica's temperature enters the loop in one place, the
// O step's sigma[i] = sqrt(kT force_scale / m_i), which tn_md.hip reads from device memory on every launch - so an accepted swap
// rewrites the sigma rows of the two replicas from a table per slot and scales their velocities by sqrt(kT_new / kT_old), one
// rounded fp32 product per component (tn_md_math.h: md_mul).  The arithmetic of the decision is tn_remd_math.h.
//
// Launch 1 (k_remd_decide, one lane per slot of every ladder): the lane of a tried pair's lower slot takes the decision and keeps
// the books - slot, holder, the accept flag, the counters and the log rows; the other lanes clear the flags of the pairs not
// tried.  Launch 2 (k_remd_atoms, one thread per atom): from the replica's new slot and the pair's flag, the velocity factor and
// the new sigma.  Both launches return at once when the status word is set or the evaluation of this step overflowed: a frozen
// loop exchanges nothing.  No atomics; the result is a function of (seed, step, energies).
#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_md_state.h"
#include "tn_model.h"
#include "tn_remd_math.h"

namespace tn {

namespace {

struct RemdArgs {
  int N, n, G, R;         // atoms, atoms per replica, ladders, slots per ladder
  uint64_t every, seed;
  float* vel;             // [N, 3]
  float* sigma;           // [N]
  const float* epot;      // [G R]
  const double* beta;     // [R]
  const float* table;     // [R, n] sigma per slot
  const float* up;        // [R - 1]
  const float* down;      // [R - 1]
  int32_t* slot;          // [G R]
  int32_t* holder;        // [G, R]
  uint8_t* accept;        // [G, R - 1] scratch: the flags of this attempt
  int32_t* slot_log;      // [G R] or NULL
  uint8_t* accept_log;    // [G, R - 1] or NULL
  int64_t* counters;      // [2, G, R - 1] attempts | accepts, or NULL
  const int* counts;      // the graph's counters, or NULL
  MdState st;
};

// the exchange workspace: one accept flag per neighbouring pair of every ladder
inline uint8_t* remd_layout(LoopCarver& c, int64_t G, int64_t R) { return c.take<uint8_t>((size_t)G * (size_t)(R - 1)); }

__device__ __forceinline__ bool remd_frozen(const RemdArgs& a) { return a.st.head[2] != 0u || (a.counts && a.counts[2]); }

// the closing launch's reduction has advanced the counter: it reads the number of completed steps
__device__ __forceinline__ uint64_t remd_step(const RemdArgs& a) { return loop_step(a.st.head); }

__global__ __launch_bounds__(kThreads) void k_remd_decide(RemdArgs a) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= a.G * a.R) return;
  if (remd_frozen(a)) return;
  const int g = t / a.R, s = t - g * a.R;
  const uint64_t step = remd_step(a);
  const int64_t row = (int64_t)g * a.R, prow = (int64_t)g * (a.R - 1);
  tn_md::exchange_lane(a.seed, step, step / a.every, g, s, a.R, a.beta, a.epot + row, a.slot + row, a.holder + row, a.accept + prow,
                       a.slot_log ? a.slot_log + row : nullptr, a.accept_log ? a.accept_log + prow : nullptr,
                       a.counters ? a.counters + prow : nullptr, a.counters ? a.counters + (int64_t)a.G * (a.R - 1) + prow : nullptr);
}

__global__ __launch_bounds__(kThreads) void k_remd_atoms(RemdArgs a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.N) return;
  if (remd_frozen(a)) return;
  const int b = i / a.n, at = i - b * a.n, g = b / a.R;
  const int t = a.slot[b];
  if (t < 0 || t >= a.R) return;  // (a slot table the caller corrupted: no read outside the tables)
  float factor;
  if (!tn_md::exchange_moved(remd_step(a) / a.every, t, a.R, a.accept + (int64_t)g * (a.R - 1), a.up, a.down, &factor)) return;
  float v[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) v[d] = a.vel[i * 3 + d];
  tn_md::scale3(v, factor);
#pragma unroll
  for (int d = 0; d < 3; ++d) a.vel[i * 3 + d] = v[d];
  a.sigma[i] = a.table[(int64_t)t * a.n + at];
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_md_exchange_workspace_bytes(int64_t n_mol, int32_t ladder, size_t* bytes) {
  if (!bytes || ladder < 2 || n_mol < 1 || n_mol > INT32_MAX / 16 || n_mol % ladder != 0) return TMDNET_ERR_INVALID;
  *bytes = layout_bytes([&](LoopCarver& c) { remd_layout(c, n_mol / ladder, ladder); });
  return TMDNET_OK;
}

int tmdnet_md_exchange(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* ex_ws, int64_t n_atoms, int64_t n_mol,
                       int32_t ladder, int64_t exchange_every, float* vel, float* sigma, const float* epot_row, const double* beta,
                       const float* sigma_table, const float* scale_up, const float* scale_down, uint64_t seed, int32_t* slot,
                       int32_t* holder, int32_t* slot_log_row, uint8_t* accept_log_row, int64_t* counters) {
  if (!md_ws || !ex_ws || !vel || !sigma || !epot_row || !beta || !sigma_table || !scale_up || !scale_down || !slot || !holder)
    return TMDNET_ERR_INVALID;
  if (ladder < 2 || n_mol < 1 || n_mol > INT32_MAX / 16 || n_mol % ladder != 0) return TMDNET_ERR_INVALID;
  if (n_atoms < 0 || n_atoms > INT32_MAX / 4 || n_atoms % n_mol != 0 || exchange_every < 1) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RemdArgs a;
  a.N = (int)n_atoms;
  a.n = (int)(n_atoms / n_mol);
  a.R = ladder;
  a.G = (int)(n_mol / ladder);
  a.every = (uint64_t)exchange_every;
  a.seed = seed;
  a.vel = vel;
  a.sigma = sigma;
  a.epot = epot_row;
  a.beta = beta;
  a.table = sigma_table;
  a.up = scale_up;
  a.down = scale_down;
  a.slot = slot;
  a.holder = holder;
  LoopCarver c(ex_ws);
  a.accept = remd_layout(c, a.G, a.R);
  a.slot_log = slot_log_row;
  a.accept_log = accept_log_row;
  a.counters = counters;
  a.counts = loop_graph(m, graph_ws, n_atoms, n_mol).counts;
  a.st = carve_md(md_ws, n_atoms, n_mol);
  const dim3 block(kThreads);
  hipLaunchKernelGGL(k_remd_decide, dim3(((int)n_mol + kThreads - 1) / kThreads), block, 0, s, a);
  if (a.N > 0) hipLaunchKernelGGL(k_remd_atoms, dim3((a.N + kThreads - 1) / kThreads), block, 0, s, a);
  return loop_launch_result(m, "tmdnet_md_exchange");
}

}  // extern "C"
