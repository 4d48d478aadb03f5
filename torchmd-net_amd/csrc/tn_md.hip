// Device-resident molecular dynamics: the integrator kernels that sit between two energy+force evaluations of a captured step,
// so that K full MD steps replay as one HIP graph with no host work in between.
//
// One step (velocity Verlet; with a thermostat the BAOAB-like "B A [F] B O" splitting):
//   v <- v + hk F      (B)      hk_i = dt force_scale / (2 m_i), one value per atom
//   x <- x + dt v      (A)      unwrapped positions
//   F  = F(x)                   the engine's evaluation (any force buffer: the kernels take a plain pointer)
//   v <- v + hk F      (B)
//   v <- c1 v + c2 sigma_i xi   (O, only with a thermostat; xi from Philox4x32-10 keyed by (seed, step, caller's atom index))
// The launch that follows an evaluation closes step k (B, O, kinetic-energy term) and opens step k + 1 (B, A) for the same atom in
// the same thread - phase TMDNET_MD_MIDDLE -, so K steps are K evaluations and K + 1 per-atom launches (OPEN, K - 1 x MIDDLE, CLOSE),
// each closing launch followed by the per-molecule reduction of the kinetic energy.  The arithmetic is tn_md_math.h; every
// product and sum is one fp32 round-to-nearest operation in the order written there.
//
// State (tmdnet_md_workspace_bytes, caller-owned, device): a header {step lo, step hi, status}, the positions and velocities
// at the last completed step (written by the opening half before it moves the atoms), the per-atom kinetic-energy terms and the
// slice sums of large molecules.  Nothing allocates or synchronises; everything is capturable.
//
// Overflow.  The graph phase rebuilds its overflow flag counts[2] on every evaluation, and an overflowed evaluation leaves stale
// forces.  The launch after an evaluation reads the flag: when it is set, every atom goes back to the saved state of the last
// completed step, the reduction kernel sets the sticky status word, and from then on every launch returns at once - positions,
// velocities, logs and the step counter stay at the last valid step until tmdnet_md_reset.  The per-atom kernel never writes the
// status word (a block that saw it early would skip the restore); the reduction kernel, next in stream order, does.
//
// Kinetic energy per molecule: sum of 0.5 m v^2 at the full step, no floating-point atomics, fixed order - the two stages of
// tn_virial.hip: grid (B, S), slices of at most 1 024 atoms on average, the slice sums added in slice order by a second kernel
// when S > 1.  The terms are stored in the CALLER's atom order, which is the order of mstart..mend whenever those ranges are
// valid; when they are not (Graph::counts[3]: unsorted batch, or molecules interleaved by the cell list), or without a graph
// workspace, a slice is a range of all atoms filtered by `batch`.
#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_md_math.h"
#include "tn_md_state.h"
#include "tn_model.h"

namespace tn {

namespace {

struct MdArgs {
  int N;
  float* pos;
  float* vel;
  const float* forces;
  float* forces_keep;
  const float* hk;
  const float* mass;
  const float* sigma;
  float dt, c1, c2;
  uint64_t seed;
  int thermostat;
  const int* counts;  // the graph's counters, or NULL
  MdState st;
};

// one thread per atom.  CLOSE: B, O, kinetic term of the step that the evaluation before this launch belongs to; OPEN: save the
// state, B, A of the next step.  MIDDLE = CLOSE then OPEN on the same registers, with the same force.
template <bool CLOSE, bool OPEN>
__global__ __launch_bounds__(kThreads) void k_md_atoms(MdArgs a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.N) return;
  if (a.st.head[kHeadStatus]) return;  // frozen since an earlier overflow
  float x[3], v[3], f[3];
  if (CLOSE && a.counts && a.counts[2]) {  // this evaluation overflowed: back to the last completed step
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a.pos[i * 3 + d] = a.st.x_keep[i * 3 + d];
      a.vel[i * 3 + d] = a.st.v_keep[i * 3 + d];
    }
    return;
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    v[d] = a.vel[i * 3 + d];
    f[d] = a.forces[i * 3 + d];
  }
  const float hk = a.hk[i];
  if (CLOSE) {
    a.st.part[i] = tn_md::close_step(v, f, hk, a.mass[i], a.thermostat, a.c1, a.c2, a.thermostat ? a.sigma[i] : 0.f, a.seed,
                                     loop_step(a.st.head), (uint32_t)i);
    if (a.forces_keep)
#pragma unroll
      for (int d = 0; d < 3; ++d) a.forces_keep[i * 3 + d] = f[d];
  }
  if (OPEN) {
#pragma unroll
    for (int d = 0; d < 3; ++d) x[d] = a.pos[i * 3 + d];
    md_save_and_open(a.st, i, x, v, f, hk, a.dt);
#pragma unroll
    for (int d = 0; d < 3; ++d) a.pos[i * 3 + d] = x[d];
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) a.vel[i * 3 + d] = v[d];
}

__global__ void k_md_reset(MdState st, uint64_t step0) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    loop_set_step(st.head, step0);
    st.head[kHeadStatus] = 0u;
  }
}

// ---- barostat: isotropic stochastic cell rescaling, one per molecule (tn_md_math.h: baro_move) ------------------------------------
struct BaroArgs {
  int B;
  float* box;           // [B, 3, 3] (box_mode 1: B == 1, [3, 3])
  const float* virial;  // [B, 3, 3]
  const float* ekin;    // [B]
  double P0, kT, a, force_scale;
  uint64_t seed;
  float* factors;  // [2, B]: mu32 | nu32
  float* volume_row;
  float* pressure_row;
  float* scale_row;
  const int* counts;  // the graph's counters, or NULL
  MdState st;
};

// ONE block, after the closing launch and its kinetic-energy reduction: per_molecule_move (tn_loop.h) with status 2.  Pass 2 writes
// the factors for k_md_scale, the box and the log rows; the move is a function of what pass 1 read, so pass 2 evaluates it again
// instead of keeping it.
__global__ __launch_bounds__(kThreads) void k_md_baro(BaroArgs a) {
  double V, P;
  float mu, nu;
  const auto move = [&](int m, uint64_t step) {
    return tn_md::baro_move(a.box + 9 * (int64_t)m, a.virial + 9 * (int64_t)m, a.ekin[m], a.force_scale, a.P0, a.kT, a.a, a.seed, step,
                            (uint32_t)m, &V, &P, &mu, &nu);
  };
  per_molecule_move(a.st, a.counts, a.B, 2u, move, [&](int m, uint64_t step) {
    float* box = a.box + 9 * (int64_t)m;
    move(m, step);
    a.factors[m] = mu;
    a.factors[a.B + m] = nu;
#pragma unroll
    for (int r = 0; r < 3; ++r) tn_md::scale3(box + 3 * r, mu);
    if (a.volume_row) a.volume_row[m] = (float)V;
    if (a.pressure_row) a.pressure_row[m] = (float)P;
    if (a.scale_row) a.scale_row[m] = mu;
  });
}

// the barostat's scratch: mu32 | nu32
inline float* baro_layout(LoopCarver& c, int64_t B) { return c.take<float>((size_t)B * 2); }

struct ScaleArgs {
  int N, B;
  float* pos;
  float* vel;
  const float* forces;
  const float* hk;
  float dt;
  const int64_t* batch;
  const float* factors;
  MdState st;
};

// one thread per atom, after k_md_baro: x <- x mu, v <- v nu with the factors of the atom's molecule.  OPEN: then the opening half
// of the next step on the same registers - the saved state is the scaled one, consistent with the new box.
template <bool OPEN>
__global__ __launch_bounds__(kThreads) void k_md_scale(ScaleArgs a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.N) return;
  if (a.st.head[kHeadStatus]) return;  // overflow (1) or an unusable move (2): k_md_baro wrote no factors
  const int64_t m = a.batch ? a.batch[i] : 0;
  if (m < 0 || m >= a.B) return;
  const float mu = a.factors[m], nu = a.factors[a.B + m];
  float x[3], v[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    x[d] = a.pos[i * 3 + d];
    v[d] = a.vel[i * 3 + d];
  }
  tn_md::scale3(x, mu);
  tn_md::scale3(v, nu);
  if (OPEN) {
    float f[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) f[d] = a.forces[i * 3 + d];
    md_save_and_open(a.st, i, x, v, f, a.hk[i], a.dt);
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    a.pos[i * 3 + d] = x[d];
    a.vel[i * 3 + d] = v[d];
  }
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_md_workspace_bytes(int64_t n_atoms, int64_t n_mol, size_t* bytes) {
  if (!bytes || n_atoms < 0 || n_mol < 0 || n_atoms > INT32_MAX / 4) return TMDNET_ERR_INVALID;
  *bytes = md_bytes(n_atoms, n_mol);
  return TMDNET_OK;
}

int tmdnet_md_reset(void* stream, void* md_ws, uint64_t step0) {
  if (!md_ws) return TMDNET_ERR_INVALID;
  hipLaunchKernelGGL(k_md_reset, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), carve_md(md_ws, 0, 0), step0);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_md_advance(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, int64_t n_atoms, int64_t n_mol, int32_t phase,
                      float* pos, float* vel, const float* forces, const float* energy, const float* hk, const float* mass,
                      const float* sigma, float dt, float c1, float c2, uint64_t seed, const int64_t* batch, float* forces_keep,
                      float* epot_log_row, float* ekin_log_row) {
  if (!md_ws || !pos || !vel || !forces || !hk || n_atoms < 0 || n_atoms > INT32_MAX / 4 || n_mol < 1) return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MD_OPEN && phase != TMDNET_MD_MIDDLE && phase != TMDNET_MD_CLOSE) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MD_OPEN && !mass) return TMDNET_ERR_INVALID;
  if (n_atoms == 0) return TMDNET_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n_atoms, B = (int)n_mol;
  MdArgs a;
  a.N = N;
  a.pos = pos;
  a.vel = vel;
  a.forces = forces;
  a.forces_keep = forces_keep;
  a.hk = hk;
  a.mass = mass;
  a.sigma = sigma;
  a.dt = dt;
  a.c1 = c1;
  a.c2 = c2;
  a.seed = seed;
  a.thermostat = sigma != nullptr;
  const LoopGraph g = loop_graph(m, graph_ws, n_atoms, n_mol);
  a.counts = g.counts;
  a.st = carve_md(md_ws, n_atoms, n_mol);
  const dim3 grid((N + kThreads - 1) / kThreads), block(kThreads);
  if (phase == TMDNET_MD_OPEN)
    hipLaunchKernelGGL((k_md_atoms<false, true>), grid, block, 0, s, a);
  else if (phase == TMDNET_MD_MIDDLE)
    hipLaunchKernelGGL((k_md_atoms<true, true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((k_md_atoms<true, false>), grid, block, 0, s, a);
  if (phase != TMDNET_MD_OPEN) {
    const int S = mol_slices(n_atoms, n_mol);
    float* out = S == 1 ? ekin_log_row : a.st.slices;
    hipLaunchKernelGGL(k_md_ke_reduce<false>, dim3(B, S), block, 0, s, a.st, g.counts, g.mstart, g.mend, N, B, S, batch, energy, epot_log_row,
                       out, nullptr);
    if (S > 1 && ekin_log_row)
      hipLaunchKernelGGL(k_md_ke_finish, dim3((B + kThreads - 1) / kThreads), block, 0, s, a.st, a.counts, B, S, ekin_log_row);
  }
  return loop_launch_result(m, "tmdnet_md_advance");
}

int tmdnet_md_barostat_workspace_bytes(int64_t n_mol, size_t* bytes) {
  if (!bytes || n_mol < 0 || n_mol > INT32_MAX / 16) return TMDNET_ERR_INVALID;
  *bytes = layout_bytes([&](LoopCarver& c) { baro_layout(c, n_mol); });
  return TMDNET_OK;
}

int tmdnet_md_barostat(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* baro_ws, int64_t n_atoms, int64_t n_mol,
                       int32_t open_next, float* pos, float* vel, const float* forces, const float* hk, float dt, const int64_t* batch,
                       float* box, int32_t box_mode, const float* virial, const float* ekin_row, double pressure, double kT,
                       double compressibility, double tau, double force_scale, uint64_t seed, float* volume_log_row,
                       float* pressure_log_row, float* scale_log_row) {
  if (!md_ws || !baro_ws || !pos || !vel || n_atoms < 0 || n_atoms > INT32_MAX / 4 || n_mol < 1 || n_mol > INT32_MAX / 16)
    return TMDNET_ERR_INVALID;
  if (!box || !virial || !ekin_row) return TMDNET_ERR_INVALID;
  if (box_mode != 1 && box_mode != 2) return TMDNET_ERR_INVALID;
  if (box_mode == 1 && n_mol != 1) return TMDNET_ERR_INVALID;  // one barostat per molecule: a shared box has no single pressure
  if (!(tau > 0.0) || !(compressibility > 0.0) || !(kT >= 0.0) || !(force_scale > 0.0)) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (open_next && (!forces || !hk)) return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n_atoms, B = (int)n_mol;
  BaroArgs b;
  b.B = B;
  b.box = box;
  b.virial = virial;
  b.ekin = ekin_row;
  b.P0 = pressure;
  b.kT = kT;
  b.a = compressibility * (double)dt / tau;
  b.force_scale = force_scale;
  b.seed = seed;
  LoopCarver c(baro_ws);
  b.factors = baro_layout(c, n_mol);
  b.volume_row = volume_log_row;
  b.pressure_row = pressure_log_row;
  b.scale_row = scale_log_row;
  b.counts = loop_graph(m, graph_ws, n_atoms, n_mol).counts;
  b.st = carve_md(md_ws, n_atoms, n_mol);
  hipLaunchKernelGGL(k_md_baro, dim3(1), dim3(kThreads), 0, s, b);
  if (N > 0) {
    ScaleArgs a;
    a.N = N;
    a.B = B;
    a.pos = pos;
    a.vel = vel;
    a.forces = forces;
    a.hk = hk;
    a.dt = dt;
    a.batch = batch;
    a.factors = b.factors;
    a.st = b.st;
    const dim3 grid((N + kThreads - 1) / kThreads), block(kThreads);
    if (open_next)
      hipLaunchKernelGGL((k_md_scale<true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((k_md_scale<false>), grid, block, 0, s, a);
  }
  return loop_launch_result(m, "tmdnet_md_barostat");
}

int tmdnet_md_status(void* stream, void* md_ws, uint64_t host[2]) {
  if (!md_ws || !host) return TMDNET_ERR_INVALID;
  return loop_read_status(stream, carve_md(md_ws, 0, 0).head, 3, -1, host, 2);
}

}  // extern "C"
