// Committee of M models: one pass over the members' energies and forces (tmdnet_committee_reduce; the arithmetic is
// tn_committee_math.h) and the gate that acts on it inside a captured MD step (tmdnet_committee_latch).  The M energy and M force
// pointers travel BY VALUE in the launch arguments: a captured loop has fresh output buffers for every step of a replay, their
// addresses are known on the host at capture time, and nothing is stacked or tabled in device memory.
//
// tmdnet_committee_reduce, two launches, no read-back, nothing allocated, capturable:
//   k_committee_atoms   one thread per atom: 3 M floats in, mean, std and deviation d_i out, and the molecule maximum as one 64-bit
//                       integer atomicMax on (bits(d_i) << 32) | (0xffffffff - i) - per WAVE when all its atoms belong to one
//                       molecule (a sorted batch: every wave but those that straddle a boundary), after a wave maximum by lane
//                       exchanges, per lane otherwise.  An integer maximum does not depend on the order of arrival: repeats are
//                       bit-identical and an unsorted batch is correct.  Thread 0 also folds the overflow flags of members 1..M-1
//                       into member 0's, the word the integrator reads (it writes that word and reads the others: no thread of
//                       this launch reads it).
//   k_committee_mols    one thread per molecule: mean and std of the M energies, D_m / a_m from the packed word - which it puts back
//                       to zero, so no memset node sits between two steps (k_prior_mol_sum does the same) -, the gate's decisions.
// Frozen loop (sticky status of the MD workspace) or an overflowed evaluation: nothing is logged and nothing is decided; the packed
// words are still put back.
//
// The gate.  flag: the first time !(D_m <= flag_above), molecule m's flagged_at / flagged_dev / flagged_atom are written by its
// thread of k_committee_mols, which also sets flag_now[m] for THIS step; the per-atom copy into flagged_pos is the next launch's
// (k_committee_latch), so no thread reads a flag that another thread of its launch writes.  stop: every molecule with
// !(D_m <= stop_above) enters (bits(D_m) << 32) | (0xffffffff - m) into one word by atomicMax; k_committee_latch, AFTER the closing
// launch of the integrator, turns a non-zero word into status 6 and the record {step, molecule, atom, value} and zeroes it.  The
// frozen state is therefore the completed step, closed with the committee mean.
#include <stdint.h>

#include "tmdnet_amd.h"
#include "tn_committee_math.h"
#include "tn_common.h"
#include "tn_md_state.h"
#include "tn_model.h"

namespace tn {

namespace {

constexpr int kMaxM = tn_committee::kMaxMembers;

struct CommitteeWs {  // views into the caller's workspace
  uint64_t* head;     // [0] the stop word, [1] stopped (0 / 1), [2] step, [3] molecule, [4] atom, [5] bits of the value
  uint64_t* packed;   // [B] the molecule maxima, zero between two passes
  int32_t* flag_now;  // [B] 1: the molecule was flagged by the pass before this latch
};

inline CommitteeWs committee_layout(LoopCarver& c, int64_t B) {
  const size_t b = (size_t)(B > 0 ? B : 0);
  CommitteeWs w;
  w.head = c.take<uint64_t>(kHeaderBytes / sizeof(uint64_t));
  w.packed = c.take<uint64_t>(b);
  w.flag_now = c.take<int32_t>(b);
  return w;
}

inline size_t committee_bytes(int64_t B) {
  return layout_bytes([&](LoopCarver& c) { committee_layout(c, B); });
}

inline CommitteeWs carve_committee(void* ws, int64_t B) {
  LoopCarver c(ws);
  return committee_layout(c, B);
}

struct CommitteeArgs {
  int N, B, flags;
  float flag_above, stop_above;
  const float* e[kMaxM];    // [B] each
  const float* f[kMaxM];    // [N, 3] each
  const int* counts[kMaxM];  // the members' graph counters, or NULL
  int* counts0;              // member 0's, the word the integrator reads
  const int64_t* batch;
  float* energy;      // [B]
  float* forces;      // [N, 3]
  float* energy_std;  // [B]
  float* forces_std;  // [N, 3]
  float* deviation;   // [N]
  float* max_dev;     // [B]
  int64_t* max_atom;  // [B]
  const uint32_t* md_head;  // the MD workspace's {step lo, step hi, status}, or NULL
  int64_t* flagged_at;
  float* flagged_dev;
  int64_t* flagged_atom;
  CommitteeWs ws;
};

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t w = __shfl_xor((unsigned long long)v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

template <int M>
__global__ __launch_bounds__(kThreads) void k_committee_atoms(CommitteeArgs a) {
  if (a.md_head && a.md_head[2]) return;  // frozen (uniform over the launch: the word is written by later launches only)
  const int i = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63;
  if (i == 0 && a.counts0) {
    int any = 0;
#pragma unroll
    for (int k = 1; k < M; ++k) any |= a.counts[k][2];
    if (any) a.counts0[2] = 1;
  }
  const bool live = i < a.N;
  int mol = -1;
  uint64_t key = 0;
  if (live) {
    double var[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float x[M], mean, sd;
#pragma unroll
      for (int k = 0; k < M; ++k) x[k] = a.f[k][(int64_t)i * 3 + c];
      var[c] = tn_committee::mean_std<M>(x, &mean, &sd);
      a.forces[(int64_t)i * 3 + c] = mean;
      a.forces_std[(int64_t)i * 3 + c] = sd;
    }
    const float d = tn_committee::deviation(var[0], var[1], var[2]);
    a.deviation[i] = d;
    const int64_t m = a.batch ? a.batch[i] : 0;
    if (m >= 0 && m < a.B) {
      mol = (int)m;
      key = tn_committee::pack(d, (uint32_t)i);
    }
  }
  // every lane of the wave is here: the exchanges below need them all
  const unsigned long long has = __ballot(mol >= 0);
  if (!has) return;
  const int first = __ffsll((long long)has) - 1;
  const int ref = __shfl(mol, first, 64);
  if (__all(mol < 0 || mol == ref)) {
    const uint64_t top = wave_max_u64(key);  // (lanes without a molecule carry 0, below every atom's word)
    if (lane == first) atomicMax(reinterpret_cast<unsigned long long*>(a.ws.packed + ref), (unsigned long long)top);
  } else if (mol >= 0) {
    atomicMax(reinterpret_cast<unsigned long long*>(a.ws.packed + mol), (unsigned long long)key);
  }
}

template <int M>
__global__ __launch_bounds__(kThreads) void k_committee_mols(CommitteeArgs a) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= a.B) return;
  const uint64_t w = a.ws.packed[m];
  a.ws.packed[m] = 0;  // this thread alone touches the word in this launch: the next pass finds it at zero
  const bool gated = a.flags != 0;
  if ((a.md_head && a.md_head[2]) || (a.counts0 && a.counts0[2])) {  // frozen, or this evaluation overflowed (folded by the launch before)
    if (gated) a.ws.flag_now[m] = 0;
    return;
  }
  float x[M], mean, sd, D;
  int64_t at;
#pragma unroll
  for (int k = 0; k < M; ++k) x[k] = a.e[k][m];
  tn_committee::mean_std<M>(x, &mean, &sd);
  tn_committee::unpack(w, &D, &at);
  a.energy[m] = mean;
  a.energy_std[m] = sd;
  a.max_dev[m] = D;
  a.max_atom[m] = at;
  if (!gated) return;
  int now = 0;
  if ((a.flags & TMDNET_COMMITTEE_FLAG) && a.flagged_at[m] < 0 && tn_committee::gate_fires(D, a.flag_above)) {
    // the step this evaluation closes: the counter is advanced by the closing launch, after this one
    const uint64_t step = loop_step(a.md_head) + 1;
    a.flagged_at[m] = (int64_t)step;
    a.flagged_dev[m] = D;
    a.flagged_atom[m] = at;
    now = 1;
  }
  a.ws.flag_now[m] = now;
  if ((a.flags & TMDNET_COMMITTEE_STOP) && tn_committee::gate_fires(D, a.stop_above))
    atomicMax(reinterpret_cast<unsigned long long*>(a.ws.head), (unsigned long long)tn_committee::pack(D, (uint32_t)m));
}

struct LatchArgs {
  int N, B, flags;
  const int64_t* batch;
  const float* pos;
  float* flagged_pos;
  const int64_t* max_atom;  // the row k_committee_mols wrote for this step
  uint32_t* md_head;
  CommitteeWs ws;
};

// after the closing launch of the step (which has advanced the counter, or latched an overflow - then the pass decided nothing).
// One thread per atom copies the atoms of the molecules flagged at this step; thread 0 latches a stop.  The closing launch does not
// move positions, so they are those of the evaluation the committee disagreed on.
__global__ __launch_bounds__(kThreads) void k_committee_latch(LatchArgs a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0 && (a.flags & TMDNET_COMMITTEE_STOP)) {
    const uint64_t w = a.ws.head[0];
    if (w) {
      a.ws.head[0] = 0;
      if (!a.md_head[2]) {
        float D;
        int64_t mol;
        tn_committee::unpack(w, &D, &mol);
        a.md_head[2] = 6u;  // (no other thread of this launch reads the status word)
        a.ws.head[1] = 1;
        a.ws.head[2] = loop_step(a.md_head);
        a.ws.head[3] = (uint64_t)mol;
        a.ws.head[4] = (uint64_t)a.max_atom[mol];
        a.ws.head[5] = tn_committee::float_bits(D);
      }
    }
  }
  if (i >= a.N || !(a.flags & TMDNET_COMMITTEE_FLAG)) return;
  const int64_t m = a.batch ? a.batch[i] : 0;
  if (m < 0 || m >= a.B || !a.ws.flag_now[m]) return;
#pragma unroll
  for (int d = 0; d < 3; ++d) a.flagged_pos[(int64_t)i * 3 + d] = a.pos[(int64_t)i * 3 + d];
}

template <int M>
void committee_launch_m(hipStream_t s, const CommitteeArgs& a) {
  if (a.N > 0) hipLaunchKernelGGL(k_committee_atoms<M>, dim3((a.N + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a);
  if (a.B > 0) hipLaunchKernelGGL(k_committee_mols<M>, dim3((a.B + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a);
}

void committee_launch(hipStream_t s, int M, const CommitteeArgs& a) {
  switch (M) {
#define TN_COMMITTEE_CASE(m) \
  case m:                    \
    return committee_launch_m<m>(s, a);
    TN_COMMITTEE_CASE(2)
    TN_COMMITTEE_CASE(3)
    TN_COMMITTEE_CASE(4)
    TN_COMMITTEE_CASE(5)
    TN_COMMITTEE_CASE(6)
    TN_COMMITTEE_CASE(7)
    TN_COMMITTEE_CASE(8)
    TN_COMMITTEE_CASE(9)
    TN_COMMITTEE_CASE(10)
    TN_COMMITTEE_CASE(11)
    TN_COMMITTEE_CASE(12)
    TN_COMMITTEE_CASE(13)
    TN_COMMITTEE_CASE(14)
    TN_COMMITTEE_CASE(15)
    TN_COMMITTEE_CASE(16)
#undef TN_COMMITTEE_CASE
  }
}

// what a gate may ask for; md_ws alone (flags 0) only freezes the pass with the loop
bool gate_ok(const tmdnet_committee_gate* g) {
  if (!g) return true;
  if (g->flags & ~(TMDNET_COMMITTEE_FLAG | TMDNET_COMMITTEE_STOP)) return false;
  if (g->flags && !g->md_ws) return false;
  if ((g->flags & TMDNET_COMMITTEE_FLAG) && (!g->flagged_at || !g->flagged_dev || !g->flagged_atom || !g->flagged_pos || g->flag_above != g->flag_above))
    return false;
  if ((g->flags & TMDNET_COMMITTEE_STOP) && g->stop_above != g->stop_above) return false;
  return true;
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_committee_workspace_bytes(int64_t n_atoms, int64_t n_mol, size_t* bytes) {
  if (!bytes || n_atoms < 0 || n_mol < 0 || n_atoms > INT32_MAX / 4 || n_mol > INT32_MAX / 16) return TMDNET_ERR_INVALID;
  *bytes = committee_bytes(n_mol);
  return TMDNET_OK;
}

int tmdnet_committee_reset(void* stream, void* ws, int64_t n_mol) {
  if (!ws || n_mol < 0 || n_mol > INT32_MAX / 16) return TMDNET_ERR_INVALID;
  char* p = reinterpret_cast<char*>(carve_committee(ws, n_mol).head);
  const size_t n = committee_bytes(n_mol) - 256;
  return hipMemsetAsync(p, 0, n, reinterpret_cast<hipStream_t>(stream)) == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_committee_reduce(void* stream, void* ws, size_t ws_bytes, int32_t n_members, const float* const* energies,
                            const float* const* forces, int64_t n_atoms, int64_t n_mol, const int64_t* batch, float* energy,
                            float* forces_mean, float* energy_std, float* forces_std, float* deviation, float* max_deviation,
                            int64_t* max_atom, tmdnet_model* const* members, void* const* graph_ws, const tmdnet_committee_gate* gate) {
  if (n_members < 2 || n_members > TMDNET_COMMITTEE_MAX_MEMBERS) return TMDNET_ERR_INVALID;
  if (n_atoms < 0 || n_mol < 0 || n_atoms > INT32_MAX / 4 || n_mol > INT32_MAX / 16) return TMDNET_ERR_INVALID;
  if (!ws || !energies || !forces || !gate_ok(gate)) return TMDNET_ERR_INVALID;
  if ((members == nullptr) != (graph_ws == nullptr)) return TMDNET_ERR_INVALID;
  if (n_mol && (!energy || !energy_std || !max_deviation || !max_atom)) return TMDNET_ERR_INVALID;
  if (n_atoms && (!forces_mean || !forces_std || !deviation)) return TMDNET_ERR_INVALID;
  for (int k = 0; k < n_members; ++k) {
    if ((n_mol && !energies[k]) || (n_atoms && !forces[k])) return TMDNET_ERR_INVALID;
    if (members && (!members[k] || !graph_ws[k])) return TMDNET_ERR_INVALID;
  }
  if (ws_bytes < committee_bytes(n_mol)) return TMDNET_ERR_WORKSPACE;
  CommitteeArgs a;
  a.N = (int)n_atoms, a.B = (int)n_mol;
  a.flags = gate ? gate->flags : 0;
  a.flag_above = gate ? gate->flag_above : 0.f;
  a.stop_above = gate ? gate->stop_above : 0.f;
  a.counts0 = nullptr;
  for (int k = 0; k < kMaxM; ++k) {
    const int j = k < n_members ? k : 0;  // (the unused slots repeat member 0: no kernel reads them)
    a.e[k] = energies[j];
    a.f[k] = forces[j];
    a.counts[k] = nullptr;
    if (members) {
      int* c = loop_graph(members[j], graph_ws[j], n_atoms, n_mol).counts;
      a.counts[k] = c;
      if (k == 0) a.counts0 = c;
    }
  }
  a.batch = batch;
  a.energy = energy, a.forces = forces_mean, a.energy_std = energy_std, a.forces_std = forces_std;
  a.deviation = deviation, a.max_dev = max_deviation, a.max_atom = max_atom;
  a.md_head = gate && gate->md_ws ? carve_md(gate->md_ws, 0, 0).head : nullptr;
  a.flagged_at = gate ? gate->flagged_at : nullptr;
  a.flagged_dev = gate ? gate->flagged_dev : nullptr;
  a.flagged_atom = gate ? gate->flagged_atom : nullptr;
  a.ws = carve_committee(ws, n_mol);
  committee_launch(reinterpret_cast<hipStream_t>(stream), n_members, a);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_committee_latch(void* stream, void* ws, int64_t n_atoms, int64_t n_mol, const int64_t* batch, const float* pos,
                           const int64_t* max_atom, const tmdnet_committee_gate* gate) {
  if (!ws || !gate || !gate_ok(gate) || !gate->md_ws) return TMDNET_ERR_INVALID;
  if (n_atoms < 0 || n_mol < 1 || n_atoms > INT32_MAX / 4 || n_mol > INT32_MAX / 16) return TMDNET_ERR_INVALID;
  if (!gate->flags) return TMDNET_OK;  // nothing to latch: no launch
  if ((gate->flags & TMDNET_COMMITTEE_STOP) && !max_atom) return TMDNET_ERR_INVALID;
  if ((gate->flags & TMDNET_COMMITTEE_FLAG) && n_atoms && !pos) return TMDNET_ERR_INVALID;
  LatchArgs a;
  a.N = (int)n_atoms, a.B = (int)n_mol, a.flags = gate->flags;
  a.batch = batch;
  a.pos = pos;
  a.flagged_pos = gate->flagged_pos;
  a.max_atom = max_atom;
  a.md_head = carve_md(gate->md_ws, 0, 0).head;
  a.ws = carve_committee(ws, n_mol);
  const int blocks = a.N > 0 && (a.flags & TMDNET_COMMITTEE_FLAG) ? (a.N + kThreads - 1) / kThreads : 1;
  hipLaunchKernelGGL(k_committee_latch, dim3(blocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_committee_status(void* stream, void* ws, uint64_t host[5]) {
  if (!ws || !host) return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint64_t head[6] = {0, 0, 0, 0, 0, 0};
  if (hipMemcpyAsync(head, carve_committee(ws, 0).head, sizeof(head), hipMemcpyDeviceToHost, s) != hipSuccess) return TMDNET_ERR_HIP;
  if (hipStreamSynchronize(s) != hipSuccess) return TMDNET_ERR_HIP;
  for (int k = 0; k < 5; ++k) host[k] = head[k + 1];
  return TMDNET_OK;
}

}  // extern "C"
