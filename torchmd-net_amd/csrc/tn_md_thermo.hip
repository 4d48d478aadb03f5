// Global thermostats of the device-resident MD loop: stochastic velocity rescaling (CSVR) and Nose-Hoover chains, one thermostat per
// molecule, between the closing half of a step and the opening half of the next (tmdnet_md_thermostat; the arithmetic is
// tn_md_thermo_math.h).  The protocol is the barostat's (tn_md.hip): one block computes every molecule's move in fp64 and, when all
// of them are usable, writes the fp32 factors, the thermostat's state and the log rows; one thread per atom then scales the
// velocities and, when another step follows, saves the scaled state and runs B, A of that step on the same registers.  An unusable
// move latches the sticky status 5 and writes nothing else.  k_md_scale of tn_md.hip with mu = 1 would give the same bits (a product
// with 1.0f is exact); the kernel below is its own because it has no position to scale - without OPEN it does not touch pos at all
// - and because an atom of infinite mass is left out of the scaling.
#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_md_state.h"
#include "tn_md_thermo_math.h"
#include "tn_model.h"

namespace tn {

namespace {

struct ThermoState {  // views into the caller's thermostat workspace
  float* alpha;       // [B]
  double* reservoir;  // [B]
  double* chain;      // [B, 2, M]
};

inline ThermoState thermo_layout(LoopCarver& c, int64_t B, int M) {
  const size_t b = (size_t)B;
  ThermoState t;
  t.alpha = c.take<float>(b);
  t.reservoir = c.take<double>(b);
  t.chain = c.take<double>(b * 2 * (size_t)M);
  return t;
}

inline size_t thermo_bytes(int64_t B, int M) {
  return layout_bytes([&](LoopCarver& c) { thermo_layout(c, B, M); });
}

inline ThermoState carve_thermo(void* ws, int64_t B, int M) {
  LoopCarver c(ws);
  return thermo_layout(c, B, M);
}

struct ThermoArgs {
  int B, kind, M, substeps;
  const float* ekin;    // [B]
  const int32_t* ndof;  // [B]
  double kT, tau, dt, c, force_scale;
  uint64_t seed;
  ThermoState th;
  float* scale_row;
  double* reservoir_row;
  const int* counts;  // the graph's counters, or NULL
  MdState st;
};

// ONE block, after the closing launch and its kinetic-energy reduction: per_molecule_move (tn_loop.h) with status 5.  Pass 1 runs
// every molecule's move on copies of its state; pass 2 runs it again, kept.
__device__ __forceinline__ int thermo_eval(const ThermoArgs& a, int m, uint64_t step, int keep, float* alpha) {
  return tn_md::thermo_move(a.kind, a.ekin[m], a.force_scale, a.ndof[m], a.kT, a.tau, a.dt, a.c, a.M, a.substeps, a.seed, step, (uint32_t)m,
                            a.th.chain + 2 * (int64_t)a.M * m, a.th.reservoir + m, keep, alpha);
}

__global__ __launch_bounds__(kThreads) void k_md_thermo_factor(ThermoArgs a) {
  float alpha;
  per_molecule_move(
      a.st, a.counts, a.B, 5u, [&](int m, uint64_t step) { return thermo_eval(a, m, step, 0, &alpha); },
      [&](int m, uint64_t step) {
        thermo_eval(a, m, step, 1, &alpha);
        a.th.alpha[m] = alpha;
        if (a.scale_row) a.scale_row[m] = alpha;
        if (a.reservoir_row) a.reservoir_row[m] = a.th.reservoir[m];
      });
}

struct ThermoScaleArgs {
  int N, B;
  float* pos;
  float* vel;
  const float* forces;
  const float* hk;
  float dt;
  const int64_t* batch;
  const float* alpha;
  MdState st;
};

// one thread per atom, after k_md_thermo_factor: v <- v alpha of the atom's molecule.  OPEN: then the opening half of the next step
// on the same registers - the saved state is the scaled one.
template <bool OPEN>
__global__ __launch_bounds__(kThreads) void k_md_thermo_scale(ThermoScaleArgs a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.N) return;
  if (a.st.head[2]) return;  // overflow (1) or an unusable move (5): k_md_thermo_factor wrote no factors
  const int64_t m = a.batch ? a.batch[i] : 0;
  if (m < 0 || m >= a.B) return;
  const float hk = a.hk[i];
  float v[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) v[d] = a.vel[i * 3 + d];
  tn_md::thermo_scale(v, hk, a.alpha[m]);
  if (OPEN) {
    float x[3], f[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      x[d] = a.pos[i * 3 + d];
      f[d] = a.forces[i * 3 + d];
    }
    md_save_and_open(a.st, i, x, v, f, hk, a.dt);
#pragma unroll
    for (int d = 0; d < 3; ++d) a.pos[i * 3 + d] = x[d];
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) a.vel[i * 3 + d] = v[d];
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_md_thermostat_workspace_bytes(int64_t n_mol, int32_t chain, size_t* bytes) {
  if (!bytes || n_mol < 0 || n_mol > INT32_MAX / 16 || chain < 0 || chain > tn_md::kThermoMaxChain) return TMDNET_ERR_INVALID;
  *bytes = thermo_bytes(n_mol, chain);
  return TMDNET_OK;
}

int tmdnet_md_thermostat(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* thermo_ws, int64_t n_atoms, int64_t n_mol,
                         int32_t kind, int32_t open_next, float* pos, float* vel, const float* forces, const float* hk, float dt,
                         const int64_t* batch, const float* ekin_row, const int32_t* ndof, double kT, double tau, int32_t chain,
                         int32_t substeps, double force_scale, uint64_t seed, float* scale_log_row, double* reservoir_log_row) {
  if (!md_ws || !thermo_ws || !vel || !hk || n_atoms < 0 || n_atoms > INT32_MAX / 4 || n_mol < 1 || n_mol > INT32_MAX / 16)
    return TMDNET_ERR_INVALID;
  if (!ekin_row || !ndof) return TMDNET_ERR_INVALID;
  if (kind != TMDNET_THERMOSTAT_CSVR && kind != TMDNET_THERMOSTAT_NHC) return TMDNET_ERR_INVALID;
  if (!(tau > 0.0) || !(kT > 0.0) || !(force_scale > 0.0)) return TMDNET_ERR_INVALID;
  if (kind == TMDNET_THERMOSTAT_NHC && (chain < 1 || chain > tn_md::kThermoMaxChain || substeps < 1)) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (open_next && (!pos || !forces)) return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n_atoms, B = (int)n_mol;
  ThermoArgs t;
  t.B = B;
  t.kind = kind;
  t.M = kind == TMDNET_THERMOSTAT_NHC ? chain : 0;
  t.substeps = substeps;
  t.ekin = ekin_row;
  t.ndof = ndof;
  t.kT = kT;
  t.tau = tau;
  t.dt = (double)dt;
  t.c = exp(-(double)dt / tau);
  t.force_scale = force_scale;
  t.seed = seed;
  t.th = carve_thermo(thermo_ws, n_mol, t.M);
  t.scale_row = scale_log_row;
  t.reservoir_row = reservoir_log_row;
  t.counts = loop_graph(m, graph_ws, n_atoms, n_mol).counts;
  t.st = carve_md(md_ws, n_atoms, n_mol);
  hipLaunchKernelGGL(k_md_thermo_factor, dim3(1), dim3(kThreads), 0, s, t);
  if (N > 0) {
    ThermoScaleArgs a;
    a.N = N;
    a.B = B;
    a.pos = pos;
    a.vel = vel;
    a.forces = forces;
    a.hk = hk;
    a.dt = dt;
    a.batch = batch;
    a.alpha = t.th.alpha;
    a.st = t.st;
    const dim3 grid((N + kThreads - 1) / kThreads), block(kThreads);
    if (open_next)
      hipLaunchKernelGGL((k_md_thermo_scale<true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((k_md_thermo_scale<false>), grid, block, 0, s, a);
  }
  return loop_launch_result(m, "tmdnet_md_thermostat");
}

}  // extern "C"
