// Anisotropic and semi-isotropic stochastic cell rescaling of the device-resident MD loop: the barostat move whose exponent is a
// 3 x 3 matrix (tn_md_cell_math.h), enqueued after the closing launch of a step as tmdnet_md_barostat (tn_md.hip) is.
//
//   k_md_ktensor_reduce / _finish   the six independent sums of 0.5 m v_a v_b per molecule, read from vel and mass (the scalar ekin
//                                   log of the CLOSE launch stays what it is).  The two stages of k_md_ke_reduce: grid (B, S),
//                                   slices of at most 1 024 atoms on average, fixed-order trees in fp64, no floating-point atomics,
//                                   bit-identical repeats; mstart..mend when those ranges are valid, else a filter on `batch`.
//   k_md_cell_move                  ONE block, two passes like k_md_baro: every molecule's move in fp64 and whether any is unusable;
//                                   then, only when none is, the matrices Mx | Mv | Mf, the new boxes and the log rows.
//   k_md_cell_scale<OPEN, DIAG>     one thread per atom: x <- x Mx, v <- v Mv, F <- F Mf, and with OPEN the opening half of the next
//                                   step on the same registers.  DIAG: the matrices are diagonal and the forces are left alone.
//
// All of them return at once on the status word or on the overflow flag of this step's evaluation (the CLOSE launch before has
// latched it), so box, positions and velocities stay those of the last completed step.
#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_md_cell_math.h"
#include "tn_md_state.h"
#include "tn_model.h"

namespace tn {

namespace {

struct CellWs {  // views into the caller's scratch
  float* M;        // [B, 27]  Mx | Mv | Mf of every molecule, row-major 3 x 3 each
  double* kt;      // [B, 6]   kinetic tensor xx, xy, xz, yy, yz, zz in the unit of m v^2
  double* slices;  // [B, S, 6] (S > 1 only)
};

inline CellWs cell_layout(LoopCarver& c, int64_t N, int64_t B) {
  const int S = mol_slices(N, B);
  CellWs w;
  w.M = c.take<float>((size_t)B * 27);
  w.kt = c.take<double>((size_t)B * 6);
  w.slices = c.take<double>(S > 1 ? (size_t)B * S * 6 : 0);
  return w;
}

inline size_t cell_bytes(int64_t N, int64_t B) {
  return layout_bytes([&](LoopCarver& c) { cell_layout(c, N, B); });
}

inline CellWs carve_cell(void* ws, int64_t N, int64_t B) {
  LoopCarver c(ws);
  return cell_layout(c, N, B);
}

// grid (B, S), after the closing launch and its reduction: slice s of molecule m -> out[(m S + s) 6 ..]
__global__ __launch_bounds__(kThreads) void k_md_ktensor_reduce(MdState st, const int* __restrict__ counts, const int* __restrict__ mstart,
                                                                const int* __restrict__ mend, int N, int S,
                                                                const int64_t* __restrict__ batch, const float* __restrict__ vel,
                                                                const float* __restrict__ mass, double* __restrict__ out) {
  __shared__ double sh[6][kThreads / 64];
  if (st.head[2]) return;
  if (counts && counts[2]) return;
  const int m = blockIdx.x, s = blockIdx.y;
  const SliceRange r = mol_slice_range(counts, mstart, mend, N, S, batch, m, s);
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = r.i0 + (int)threadIdx.x; i < r.i1; i += kThreads) {
    if (slice_skips(r, batch, i, m)) continue;
    const float v[3] = {vel[i * 3], vel[i * 3 + 1], vel[i * 3 + 2]};
    double t[6];
    tn_md::cell_ktensor_term(mass[i], v, t);
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[c] += t[c];
  }
  block_reduce_waves<6, 0u>(acc, sh);
  if (threadIdx.x < 6) out[((int64_t)m * S + s) * 6 + threadIdx.x] = block_reduce_row(sh[threadIdx.x], false);
}

// one thread per entry of a molecule's tensor: the slice sums in slice order
__global__ __launch_bounds__(kThreads) void k_md_ktensor_finish(MdState st, const int* __restrict__ counts, int B, int S,
                                                                const double* __restrict__ slices, double* __restrict__ kt) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= B * 6 || st.head[2] || (counts && counts[2])) return;
  const int m = j / 6, c = j - 6 * m;
  double v = 0.0;
  for (int s = 0; s < S; ++s) v += slices[((int64_t)m * S + s) * 6 + c];
  kt[j] = v;
}

struct CellArgs {
  int B;
  float* box;           // [B, 3, 3] (box_mode 1: B == 1, [3, 3])
  const float* virial;  // [B, 3, 3]
  const double* kt;     // [B, 6]
  double P0, kT, a, force_scale;
  uint64_t seed;
  int coupling, axis;
  float* M;  // [B, 27]
  float* volume_row;
  float* pressure_row;
  float* scale_row;
  const int* counts;  // the graph's counters, or NULL
  MdState st;
};

// ONE block: per_molecule_move (tn_loop.h) with status 2.  Pass 2 writes the matrices for k_md_cell_scale, the box and the log rows:
// with up to one molecule per thread what pass 1 left in the thread's registers, with more it evaluates the move again instead of
// keeping every one of them.
__global__ __launch_bounds__(kThreads) void k_md_cell_move(CellArgs a) {
  tn_md::CellMove mv;
  const auto move = [&](int m, uint64_t step) {
    return tn_md::cell_move(a.box + 9 * (int64_t)m, a.virial + 9 * (int64_t)m, a.kt + 6 * (int64_t)m, a.force_scale, a.P0, a.kT, a.a, a.seed,
                            step, (uint32_t)m, a.coupling, a.axis, &mv);
  };
  per_molecule_move(a.st, a.counts, a.B, 2u, move, [&](int m, uint64_t step) {
    float* box = a.box + 9 * (int64_t)m;
    if (a.B > kThreads) move(m, step);
#pragma unroll
    for (int i = 0; i < 27; ++i) a.M[27 * (int64_t)m + i] = mv.M[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) box[i] = mv.box[i];
    if (a.volume_row) a.volume_row[m] = (float)mv.V;
    if (a.pressure_row)
#pragma unroll
      for (int i = 0; i < 9; ++i) a.pressure_row[9 * (int64_t)m + i] = (float)mv.P[i];
    if (a.scale_row)
#pragma unroll
      for (int i = 0; i < 9; ++i) a.scale_row[9 * (int64_t)m + i] = mv.M[i];
  });
}

struct CellScaleArgs {
  int N, B;
  float* pos;
  float* vel;
  const float* forces;
  float* forces_keep;
  const float* hk;
  float dt;
  const int64_t* batch;
  const float* M;
  MdState st;
};

// one thread per atom, after k_md_cell_move: x <- x Mx, v <- v Mv with the matrices of the atom's molecule, and (not DIAG) the kept
// forces rotated by Mf.  OPEN: the forces of the evaluation are rotated in registers, stored as the kept forces, and the opening
// half of the next step runs on the same registers - the saved state is the scaled one, consistent with the new box.
template <bool OPEN, bool DIAG>
__global__ __launch_bounds__(kThreads) void k_md_cell_scale(CellScaleArgs a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.N) return;
  if (a.st.head[2]) return;  // overflow (1) or an unusable move (2): k_md_cell_move wrote no matrices
  const int64_t m = a.batch ? a.batch[i] : 0;
  if (m < 0 || m >= a.B) return;
  const float* Mp = a.M + 27 * m;
  float Mx[9], Mv[9], Mf[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    Mx[k] = Mp[k];
    Mv[k] = Mp[9 + k];
    if (!DIAG) Mf[k] = Mp[18 + k];
  }
  float x[3], v[3], f[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    x[d] = a.pos[i * 3 + d];
    v[d] = a.vel[i * 3 + d];
  }
  tn_md::cell_apply<DIAG>(x, Mx);
  tn_md::cell_apply<DIAG>(v, Mv);
  const float* fsrc = OPEN ? a.forces : a.forces_keep;
  if (OPEN || (!DIAG && fsrc)) {
#pragma unroll
    for (int d = 0; d < 3; ++d) f[d] = fsrc[i * 3 + d];
    if (!DIAG) {
      tn_md::cell_apply<false>(f, Mf);
      if (a.forces_keep)
#pragma unroll
        for (int d = 0; d < 3; ++d) a.forces_keep[i * 3 + d] = f[d];
    }
  }
  if (OPEN) {  // the opening half written out, not md_save_and_open: hk read after the saves keeps the rotating kernel's registers down
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a.st.x_keep[i * 3 + d] = x[d];
      a.st.v_keep[i * 3 + d] = v[d];
    }
    tn_md::open_step(x, v, f, a.hk[i], a.dt);
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

int tmdnet_md_barostat_cell_workspace_bytes(int64_t n_atoms, int64_t n_mol, size_t* bytes) {
  if (!bytes || n_atoms < 0 || n_atoms > INT32_MAX / 4 || n_mol < 0 || n_mol > INT32_MAX / 256) return TMDNET_ERR_INVALID;
  *bytes = cell_bytes(n_atoms, n_mol);
  return TMDNET_OK;
}

int tmdnet_md_barostat_cell(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* cell_ws, int64_t n_atoms, int64_t n_mol,
                            int32_t open_next, float* pos, float* vel, const float* forces, const float* hk, const float* mass, float dt,
                            const int64_t* batch, float* box, int32_t box_mode, const float* virial, double pressure, double kT,
                            double compressibility, double tau, double force_scale, uint64_t seed, int32_t coupling, int32_t axis,
                            float* forces_keep, float* volume_log_row, float* pressure_log_row, float* scale_log_row) {
  if (!md_ws || !cell_ws || !pos || !vel || !mass || n_atoms < 0 || n_atoms > INT32_MAX / 4 || n_mol < 1 || n_mol > INT32_MAX / 256)
    return TMDNET_ERR_INVALID;
  if (!box || !virial) return TMDNET_ERR_INVALID;
  if (box_mode != 1 && box_mode != 2) return TMDNET_ERR_INVALID;
  if (box_mode == 1 && n_mol != 1) return TMDNET_ERR_INVALID;  // one barostat per molecule: a shared box has no single pressure
  if (!(tau > 0.0) || !(compressibility > 0.0) || !(kT >= 0.0) || !(force_scale > 0.0)) return TMDNET_ERR_INVALID;
  if (coupling != TMDNET_CELL_ANISOTROPIC && coupling != TMDNET_CELL_DIAGONAL && coupling != TMDNET_CELL_SEMI_ISOTROPIC)
    return TMDNET_ERR_INVALID;
  if (axis < 0 || axis > 2) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (open_next && (!forces || !hk)) return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n_atoms, B = (int)n_mol;
  const MdState st = carve_md(md_ws, n_atoms, n_mol);
  const CellWs w = carve_cell(cell_ws, n_atoms, n_mol);
  const LoopGraph g = loop_graph(m, graph_ws, n_atoms, n_mol);
  const int* counts = g.counts;
  const dim3 block(kThreads);
  const int S = mol_slices(n_atoms, n_mol);
  hipLaunchKernelGGL(k_md_ktensor_reduce, dim3(B, S), block, 0, s, st, counts, g.mstart, g.mend, N, S, batch, vel, mass, S == 1 ? w.kt : w.slices);
  if (S > 1) hipLaunchKernelGGL(k_md_ktensor_finish, dim3((B * 6 + kThreads - 1) / kThreads), block, 0, s, st, counts, B, S, w.slices, w.kt);
  CellArgs c;
  c.B = B;
  c.box = box;
  c.virial = virial;
  c.kt = w.kt;
  c.P0 = pressure;
  c.kT = kT;
  c.a = compressibility * (double)dt / tau;
  c.force_scale = force_scale;
  c.seed = seed;
  c.coupling = coupling;
  c.axis = axis;
  c.M = w.M;
  c.volume_row = volume_log_row;
  c.pressure_row = pressure_log_row;
  c.scale_row = scale_log_row;
  c.counts = counts;
  c.st = st;
  hipLaunchKernelGGL(k_md_cell_move, dim3(1), block, 0, s, c);
  if (N > 0) {
    CellScaleArgs a;
    a.N = N;
    a.B = B;
    a.pos = pos;
    a.vel = vel;
    a.forces = forces;
    a.forces_keep = forces_keep;
    a.hk = hk;
    a.dt = dt;
    a.batch = batch;
    a.M = w.M;
    a.st = st;
    const dim3 grid((N + kThreads - 1) / kThreads);
    const bool diag = coupling != TMDNET_CELL_ANISOTROPIC;
    if (open_next && diag)
      hipLaunchKernelGGL((k_md_cell_scale<true, true>), grid, block, 0, s, a);
    else if (open_next)
      hipLaunchKernelGGL((k_md_cell_scale<true, false>), grid, block, 0, s, a);
    else if (diag)
      hipLaunchKernelGGL((k_md_cell_scale<false, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((k_md_cell_scale<false, false>), grid, block, 0, s, a);
  }
  return loop_launch_result(m, "tmdnet_md_barostat_cell");
}

}  // extern "C"
