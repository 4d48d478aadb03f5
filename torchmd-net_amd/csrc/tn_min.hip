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
//
// Cell relaxation (tmdnet_min_*_cell, the second half of this file): the same three launches on N + 3 rows per molecule.  The atoms
// are integrated in xt = x D^-T, the three rows of the deformation gradient D count as three more atoms with coordinates c D and
// force (W_s - p V I) D^-T / c from the step's virial, the controller's sums get their terms added, and the move rewrites the box
// H0 D^T the next evaluation reads.  The scheme is stated with the entries in include/tmdnet_amd.h; the reduction is one template
// (k_min_reduce<CELL>: the cell adds one statement), the controller and the per-atom kernel have siblings of their own, so the
// fixed-box path issues the launches and produces the bits it did before.
#include <cmath>

#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_loop.h"
#include "tn_min_math.h"
#include "tn_model.h"

namespace tn {

namespace {

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

// the cell relaxation's arrays sit behind MinState in the same workspace (see "cell relaxation" below)
struct MinCell {
  double* H0;       // [B, 9] the reference box
  double* D_keep;   // [B, 9] before the last move
  double* VD_keep;  // [B, 9]
  double* D_next;   // [B, 9] what the last control prepared
  double* VD_next;  // [B, 9]
  float* box_keep;  // [B, 9]
  float* box_next;  // [B, 9]
  float* d32;       // [B, 9]
  float* d32_prev;  // [B, 9]
  float* d32_next;  // [B, 9]
};

MinState min_layout(LoopCarver& c, int64_t N, int64_t B, MinCell* cell) {
  const size_t n = (size_t)(N > 0 ? N : 0), b = (size_t)(B > 0 ? B : 0);
  const size_t S = (size_t)mol_slices(N, B);
  MinState st;
  st.head = c.take<uint32_t>(kHeaderBytes / sizeof(uint32_t));
  st.start = reinterpret_cast<double*>(st.head + 4);
  st.dt = c.take<double>(b);
  st.alpha = c.take<double>(b);
  st.conv = c.take<int64_t>(b);
  st.n_pos = c.take<int32_t>(b);
  st.coef = c.take<float>(b * 3);
  st.x_keep = c.take<float>(n * 3);
  st.v_keep = c.take<float>(n * 3);
  st.slices = c.take<double>(b * S * 4);
  if (cell) {
    for (double** q : {&cell->H0, &cell->D_keep, &cell->VD_keep, &cell->D_next, &cell->VD_next}) *q = c.take<double>(b * 9);
    for (float** q : {&cell->box_keep, &cell->box_next, &cell->d32, &cell->d32_prev, &cell->d32_next}) *q = c.take<float>(b * 9);
  }
  return st;
}

size_t min_bytes(int64_t N, int64_t B, bool with_cell) {
  MinCell cell;
  return layout_bytes([&](LoopCarver& c) { min_layout(c, N, B, with_cell ? &cell : nullptr); });
}

MinState carve_min(void* ws, int64_t N, int64_t B) {
  LoopCarver c(ws);
  return min_layout(c, N, B, nullptr);
}

MinCell carve_min_cell(void* ws, int64_t N, int64_t B) {
  LoopCarver c(ws);
  MinCell cell;
  min_layout(c, N, B, &cell);
  return cell;
}

// grid (B, S): slice s of molecule m -> slices[m, s, 0..3].  Threads stride the atoms, lanes by the xor tree, waves in turn.  CELL: on
// the generalised forces Ft = F D32 of the D32 the positions were formed with (`d32`: [B, 9]).
template <bool CELL>
__global__ __launch_bounds__(kThreads) void k_min_reduce(MinState st, const float* __restrict__ d32, const int* __restrict__ counts,
                                                         const int* __restrict__ mstart, const int* __restrict__ mend, int N, int S,
                                                         const int64_t* __restrict__ batch, const float* __restrict__ vel,
                                                         const float* __restrict__ forces, const uint8_t* __restrict__ fixed) {
  __shared__ double sh[4][kThreads / 64];
  if (st.head[kHeadStatus]) return;           // frozen
  if (counts && counts[2]) return;  // overflowed: stale forces, the controller latches it
  const int m = blockIdx.x, s = blockIdx.y;
  const SliceRange r = mol_slice_range(counts, mstart, mend, N, S, batch, m, s);
  float D[9];
  if (CELL)
#pragma unroll
    for (int k = 0; k < 9; ++k) D[k] = d32[m * 9 + k];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = r.i0 + (int)threadIdx.x; i < r.i1; i += kThreads) {
    if (slice_skips(r, batch, i, m)) continue;
    float v[3], f[3], t[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      v[d] = vel[i * 3 + d];
      f[d] = forces[i * 3 + d];
    }
    if (CELL) {
      float ft[3];
      tn_min::cell_atom_force(f, D, ft);
      tn_min::atom_terms(v, ft, fixed && fixed[i], t);
    } else {
      tn_min::atom_terms(v, f, fixed && fixed[i], t);
    }
    acc[0] += (double)t[0];
    acc[1] += (double)t[1];
    acc[2] += (double)t[2];
    acc[3] = (double)t[1] > acc[3] ? (double)t[1] : acc[3];
  }
  block_reduce_waves<4, 8u>(acc, sh);
  if (threadIdx.x == 0) block_reduce_rows<4, 8u>(sh, st.slices + ((int64_t)m * S + s) * 4);
}

struct MinCtlArgs {
  int B, S;
  tn_min::FireParams p;
  const int* counts;  // the graph's counters, or NULL
  const float* energy;
  FireRows rows;
  MinState st;
};

// the sums of molecule m (slices in slice order) and its state (after a reset: the start values of the header)
__device__ __forceinline__ void min_load(const MinCtlArgs& a, int m, bool fresh, double sums[4], tn_min::FireState* s) {
  slice_sums<4, 8u>(a.st.slices + (int64_t)m * a.S * 4, a.S, 4, sums);
  fire_load(fire_units(a.st), m, fresh, s);
}

// ONE block striding the molecules, after k_min_reduce: optimiser_control (tn_loop.h) with FIRE's two passes
__global__ __launch_bounds__(kThreads) void k_min_control(MinCtlArgs a) {
  const auto control = [&](int m, bool fresh, uint64_t step, double sums[4], float coef[3], tn_min::FireState* s) {
    min_load(a, m, fresh, sums, s);
    return tn_min::fire_control(s, a.p, sums[0], sums[1], sums[2], sums[3], (int64_t)step, coef);
  };
  optimiser_control(
      a.st.head, a.counts, -1, true, a.B,
      [&](int m, bool fresh, uint64_t step) {
        double sums[4];
        float coef[3];
        tn_min::FireState s;
        return (int)(control(m, fresh, step, sums, coef, &s) == tn_min::FIRE_UNUSABLE);
      },
      [&](int m, bool fresh, uint64_t step) {
        double sums[4];
        float coef[3];
        tn_min::FireState s;
        control(m, fresh, step, sums, coef, &s);
        fire_store(fire_units(a.st), m, s, coef);
        a.rows.write(m, a.energy ? a.energy + m : nullptr, sums, sums[3], coef, s);
      });
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
__global__ __launch_bounds__(kThreads) void k_min_atoms(MinAtomArgs a) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.N) return;
  const uint32_t status = a.st.head[kHeadStatus], fresh = a.st.head[kHeadFresh];
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
    loop_head_reset(st.head, step0, -1);
    st.start[0] = dt0;
    st.start[1] = alpha0;
  }
}

// ---- cell relaxation: the same three launches with nine more degrees of freedom per molecule ------------------------------------
// The atoms' integrated state is xt = x D^-T and its velocity (`xt`, `vel`); `pos` is what the evaluation reads, x = xt D32^T.  D
// and V_D are the caller's fp64 buffers, the box is the buffer the evaluation reads.  The workspace adds, per molecule: H0, what the
// last move saved (D, V_D, the fp32 box), what the last control prepared (the next D, V_D, box and D32), and two D32: `d32`, which the
// current positions were formed with, and `d32_prev`, which the positions before the last move were formed with.  A move (the
// end of the controller in MIDDLE, k_min_cell_commit in OPEN) saves the current values, makes the prepared ones current and moves
// d32 to d32_prev; the per-atom kernel then forms the generalised force with d32_prev and the new position with d32.
// (MinCell and its layout: with MinState, above.)
constexpr int kMinCellCauseWord = 8;  // header byte 32: which sum or input was unusable when status 2 was latched (tn_min::CELL_BAD_*)

struct MinCellCtlArgs {
  MinCtlArgs base;
  MinCell cs;
  tn_min::CellParams cp;
  int move;                   // 1: MIDDLE, the move follows in this launch
  const float* virial;        // [B, 9] of the evaluation just made
  float* box;                 // [B, 9] the box the evaluation reads
  double* deform;             // [B, 9] D
  double* cell_vel;           // [B, 9] V_D
  const double* cell_factor;  // [B]
  double* stress_row;         // [B, 9] or NULL
  double* volume_row;         // [B] or NULL
  double* cell_force_row;     // [B, 9] or NULL: G / c
};

// the prepared values become the current ones, the current ones the saved ones (one thread per molecule)
__device__ __forceinline__ void min_cell_commit(const MinCell& cs, float* box, double* deform, double* cell_vel, int m) {
  for (int k = 0; k < 9; ++k) {
    const int j = m * 9 + k;
    cs.D_keep[j] = deform[j];
    cs.VD_keep[j] = cell_vel[j];
    cs.box_keep[j] = box[j];
    cs.d32_prev[j] = cs.d32[j];
    deform[j] = cs.D_next[j];
    cell_vel[j] = cs.VD_next[j];
    box[j] = cs.box_next[j];
    cs.d32[j] = cs.d32_next[j];
  }
}

struct MinCellOut {  // what one control of one molecule produces
  tn_min::FireState s;
  double atoms[4], sums[4], Gc[9], V, stress[9], Dn[9], VDn[9];  // atoms: the atoms' sums; sums: with the cell rows
  float coef[3], boxn[9], d32n[9];
  int ret, why;
};

__device__ __forceinline__ void min_cell_eval(const MinCellCtlArgs& a, int m, bool fresh, int64_t step, MinCellOut* o) {
  min_load(a.base, m, fresh, o->sums, &o->s);
  for (int k = 0; k < 4; ++k) o->atoms[k] = o->sums[k];
  float W[9], box[9], d32[9];
  double H0[9], D[9], VD[9];
  for (int k = 0; k < 9; ++k) {
    const int j = m * 9 + k;
    W[k] = a.virial[j];
    box[k] = a.box[j];
    d32[k] = a.cs.d32[j];
    H0[k] = a.cs.H0[j];
    D[k] = a.deform[j];
    VD[k] = a.cell_vel[j];
  }
  o->ret = tn_min::cell_control(&o->s, a.base.p, a.cp, a.cell_factor[m], o->sums, W, box, d32, H0, D, VD, step, o->coef, o->Gc, &o->V,
                                o->stress, o->Dn, o->VDn, o->boxn, o->d32n, &o->why);
}

// k_min_control with the cell rows: ONE block striding the molecules.  On an overflow it also puts D, V_D, the box and d32 back,
// before the skeleton latches it.
__global__ __launch_bounds__(kThreads) void k_min_control_cell(MinCellCtlArgs a) {
  const MinState& st = a.base.st;
  if (!st.head[kHeadStatus] && a.base.counts && a.base.counts[2]) {
    if (!st.head[kHeadFresh])  // nothing was saved before the first control
      for (int m = threadIdx.x; m < a.base.B; m += kThreads)
        for (int k = 0; k < 9; ++k) {
          const int j = m * 9 + k;
          a.deform[j] = a.cs.D_keep[j];
          a.cell_vel[j] = a.cs.VD_keep[j];
          a.box[j] = a.cs.box_keep[j];
          a.cs.d32[j] = a.cs.d32_prev[j];
        }
    __syncthreads();  // (every thread has read the status word)
  }
  optimiser_control(
      st.head, a.base.counts, kMinCellCauseWord, true, a.base.B,
      [&](int m, bool fresh, uint64_t step) {
        MinCellOut o;
        min_cell_eval(a, m, fresh, (int64_t)step, &o);
        return o.ret == tn_min::FIRE_UNUSABLE ? o.why : 0;
      },
      [&](int m, bool fresh, uint64_t step) {
        MinCellOut o;
        min_cell_eval(a, m, fresh, (int64_t)step, &o);
        fire_store(fire_units(st), m, o.s, o.coef);
        for (int k = 0; k < 9; ++k) {
          const int j = m * 9 + k;
          a.cs.D_next[j] = o.Dn[k];
          a.cs.VD_next[j] = o.VDn[k];
          a.cs.box_next[j] = o.boxn[k];
          a.cs.d32_next[j] = o.d32n[k];
          if (a.stress_row) a.stress_row[j] = o.stress[k];
          if (a.cell_force_row) a.cell_force_row[j] = o.Gc[k];
        }
        if (a.volume_row) a.volume_row[m] = o.V;
        a.base.rows.write(m, a.base.energy ? a.base.energy + m : nullptr, o.atoms, o.sums[3], o.coef, o.s);
        if (a.move) min_cell_commit(a.cs, a.box, a.deform, a.cell_vel, m);
      });
}

// OPEN: the cell's part of the move from what the last control prepared, before the per-atom kernel
__global__ __launch_bounds__(kThreads) void k_min_cell_commit(MinState st, MinCell cs, int B, float* box, double* deform,
                                                                  double* cell_vel) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= B || st.head[kHeadStatus] || st.head[kHeadFresh]) return;  // frozen, or straight after a reset: nothing is prepared yet
  min_cell_commit(cs, box, deform, cell_vel, m);
}

struct MinCellAtomArgs {
  MinAtomArgs base;  // vel is the velocity of xt
  MinCell cs;
  float* xt;
};

// k_min_atoms on xt: the generalised force from d32_prev, the update, then the position the evaluation reads from d32.  A fixed atom
// keeps xt and so follows the cell; an atom of a converged molecule is not touched at all (its D does not change either).
template <bool ACCEPT, bool MOVE>
__global__ __launch_bounds__(kThreads) void k_min_atoms_cell(MinCellAtomArgs c) {
  const MinAtomArgs& a = c.base;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.N) return;
  const uint32_t status = a.st.head[kHeadStatus], fresh = a.st.head[kHeadFresh];
  const int64_t m = a.batch ? a.batch[i] : 0;
  const bool mol_ok = m >= 0 && m < a.B;
  if (status) {
    // the evaluation before this launch overflowed: xt and its velocity as saved, and the position they gave with the D32 of then
    if (ACCEPT && status == 1u && !fresh && a.counts && a.counts[2] && mol_ok) {
      float xt[3], x[3], d32[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) d32[k] = c.cs.d32_prev[m * 9 + k];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        xt[d] = a.st.x_keep[i * 3 + d];
        c.xt[i * 3 + d] = xt[d];
        a.vel[i * 3 + d] = a.st.v_keep[i * 3 + d];
      }
      if (a.st.conv[m] < 0) {  // (an atom of a converged molecule was never moved)
        tn_min::cell_position(xt, d32, x);
#pragma unroll
        for (int d = 0; d < 3; ++d) a.pos[i * 3 + d] = x[d];
      }
    }
    return;
  }
  if (fresh) return;
  float x[3], xt[3], v[3], f[3], ft[3], d32[9];
#pragma unroll
  for (int d = 0; d < 3; ++d) f[d] = a.forces[i * 3 + d];
  if (ACCEPT && a.forces_keep)
#pragma unroll
    for (int d = 0; d < 3; ++d) a.forces_keep[i * 3 + d] = f[d];
  if (MOVE) {
    if (!mol_ok) return;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      xt[d] = c.xt[i * 3 + d];
      v[d] = a.vel[i * 3 + d];
      a.st.x_keep[i * 3 + d] = xt[d];
      a.st.v_keep[i * 3 + d] = v[d];
    }
    if (a.st.conv[m] >= 0) {
#pragma unroll
      for (int d = 0; d < 3; ++d) a.vel[i * 3 + d] = 0.f;
      return;
    }
    if (a.fixed && a.fixed[i]) {
#pragma unroll
      for (int d = 0; d < 3; ++d) a.vel[i * 3 + d] = 0.f;
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) d32[k] = c.cs.d32_prev[m * 9 + k];
      tn_min::cell_atom_force(f, d32, ft);
      tn_min::atom_move(xt, v, ft, a.st.coef[m * 3 + 0], a.st.coef[m * 3 + 1], a.st.coef[m * 3 + 2]);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        c.xt[i * 3 + d] = xt[d];
        a.vel[i * 3 + d] = v[d];
      }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) d32[k] = c.cs.d32[m * 9 + k];
    tn_min::cell_position(xt, d32, x);
#pragma unroll
    for (int d = 0; d < 3; ++d) a.pos[i * 3 + d] = x[d];
  }
}

// the header as k_min_reset; per molecule H0 = the box, D = I, V_D = 0, every saved and prepared value equal to the current one; per
// atom xt = x
__global__ __launch_bounds__(kThreads) void k_min_reset_cell(MinState st, MinCell cs, int N, int B, uint64_t step0, double dt0,
                                                                 double alpha0, const float* box, double* deform, double* cell_vel,
                                                                 const float* pos, float* xt) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) {
    loop_head_reset(st.head, step0, kMinCellCauseWord);
    st.start[0] = dt0;
    st.start[1] = alpha0;
  }
  if (i < B)
    for (int k = 0; k < 9; ++k) {
      const int j = i * 9 + k;
      const double e = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
      cs.H0[j] = (double)box[j];
      deform[j] = cs.D_keep[j] = cs.D_next[j] = e;
      cell_vel[j] = cs.VD_keep[j] = cs.VD_next[j] = 0.0;
      cs.box_keep[j] = cs.box_next[j] = box[j];
      cs.d32[j] = cs.d32_prev[j] = cs.d32_next[j] = (float)e;
    }
  if (i < 3 * N) xt[i] = pos[i];
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_min_workspace_bytes(int64_t n_atoms, int64_t n_mol, size_t* bytes) {
  if (!bytes || n_atoms < 0 || n_mol < 0 || n_atoms > INT32_MAX / 4 || n_mol > INT32_MAX / 16) return TMDNET_ERR_INVALID;
  *bytes = min_bytes(n_atoms, n_mol, false);
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
  const LoopGraph g = loop_graph(m, graph_ws, n_atoms, n_mol);
  const int* counts = g.counts;
  const dim3 block(kThreads);
  if (phase != TMDNET_MIN_OPEN) {
    const int S = mol_slices(n_atoms, n_mol);
    hipLaunchKernelGGL(k_min_reduce<false>, dim3(B, S), block, 0, s, st, nullptr, counts, g.mstart, g.mend, N, S, batch, vel, forces, fixed);
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
    c.rows = {epot_log_row, fmax_log_row, sums_log_row, coef_log_row, dt_log_row, alpha_log_row, converged_log_row};
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
    const dim3 grid((N + kThreads - 1) / kThreads);
    if (phase == TMDNET_MIN_OPEN)
      hipLaunchKernelGGL((k_min_atoms<false, true>), grid, block, 0, s, a);
    else if (phase == TMDNET_MIN_MIDDLE)
      hipLaunchKernelGGL((k_min_atoms<true, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((k_min_atoms<true, false>), grid, block, 0, s, a);
  }
  return loop_launch_result(m, "tmdnet_min_advance");
}

int tmdnet_min_status(void* stream, void* min_ws, uint64_t host[2]) {
  if (!min_ws || !host) return TMDNET_ERR_INVALID;
  return loop_read_status(stream, carve_min(min_ws, 0, 0).head, 3, -1, host, 2);
}

int tmdnet_min_workspace_bytes_cell(int64_t n_atoms, int64_t n_mol, size_t* bytes) {
  if (!bytes || n_atoms < 0 || n_mol < 0 || n_atoms > INT32_MAX / 4 || n_mol > INT32_MAX / 16) return TMDNET_ERR_INVALID;
  *bytes = min_bytes(n_atoms, n_mol, true);
  return TMDNET_OK;
}

int tmdnet_min_reset_cell(void* stream, void* min_ws, int64_t n_atoms, int64_t n_mol, uint64_t step0, double dt0, double alpha0,
                          const float* box, double* deform, double* cell_vel, const float* pos, float* xt) {
  if (!min_ws || !(dt0 > 0.0) || !(alpha0 >= 0.0) || !box || !deform || !cell_vel || n_atoms < 0 || n_atoms > INT32_MAX / 4 || n_mol < 1 ||
      n_mol > INT32_MAX / 16 || (n_atoms > 0 && (!pos || !xt)))
    return TMDNET_ERR_INVALID;
  const int64_t threads = 3 * n_atoms > n_mol ? 3 * n_atoms : n_mol;
  hipLaunchKernelGGL(k_min_reset_cell, dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), carve_min(min_ws, n_atoms, n_mol), carve_min_cell(min_ws, n_atoms, n_mol),
                     (int)n_atoms, (int)n_mol, step0, dt0, alpha0, box, deform, cell_vel, pos, xt);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_min_advance_cell(tmdnet_model* m, void* stream, void* graph_ws, void* min_ws, int64_t n_atoms, int64_t n_mol, int32_t phase,
                            float* pos, float* vel, const float* forces, const float* energy, const uint8_t* fixed, const int64_t* batch,
                            float* forces_keep, double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha0, double f_alpha,
                            double max_step, double fmax, float* epot_log_row, float* fmax_log_row, double* sums_log_row,
                            float* coef_log_row, double* dt_log_row, double* alpha_log_row, int64_t* converged_log_row, float* xt,
                            float* box, double* deform, double* cell_vel, const float* virial, const double* cell_factor,
                            const double* mask, int32_t flags, double pressure, double* stress_log_row, double* volume_log_row,
                            double* cell_force_log_row) {
  if (!min_ws || !pos || !vel || !forces || !xt || !box || !deform || !cell_vel || !cell_factor || !mask || n_atoms < 0 ||
      n_atoms > INT32_MAX / 4 || n_mol < 1 || n_mol > INT32_MAX / 16)
    return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MIN_OPEN && phase != TMDNET_MIN_MIDDLE && phase != TMDNET_MIN_CLOSE) return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MIN_OPEN && !virial) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (!(fmax > 0.0) || !(dt_max > 0.0) || !(max_step > 0.0) || !(f_inc > 0.0) || !(f_dec > 0.0) || !(f_alpha > 0.0) || !(alpha0 >= 0.0) ||
      n_min < 0 || !std::isfinite(pressure) || (flags & ~3) || (flags & 3) == 3)
    return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n_atoms, B = (int)n_mol;
  const MinState st = carve_min(min_ws, n_atoms, n_mol);
  const MinCell cs = carve_min_cell(min_ws, n_atoms, n_mol);
  const LoopGraph g = loop_graph(m, graph_ws, n_atoms, n_mol);
  const int* counts = g.counts;
  const dim3 block(kThreads);
  if (phase != TMDNET_MIN_OPEN) {
    const int S = mol_slices(n_atoms, n_mol);
    hipLaunchKernelGGL(k_min_reduce<true>, dim3(B, S), block, 0, s, st, cs.d32, counts, g.mstart, g.mend, N, S, batch, vel, forces, fixed);
    MinCellCtlArgs c;
    c.base.B = B;
    c.base.S = S;
    c.base.p.dt_max = dt_max;
    c.base.p.f_inc = f_inc;
    c.base.p.f_dec = f_dec;
    c.base.p.alpha0 = alpha0;
    c.base.p.f_alpha = f_alpha;
    c.base.p.max_step = max_step;
    c.base.p.fmax = fmax;
    c.base.p.n_min = n_min;
    c.base.counts = counts;
    c.base.energy = energy;
    c.base.rows = {epot_log_row, fmax_log_row, sums_log_row, coef_log_row, dt_log_row, alpha_log_row, converged_log_row};
    c.base.st = st;
    c.cs = cs;
    for (int k = 0; k < 9; ++k) c.cp.mask[k] = mask[k] != 0.0 ? 1.0 : 0.0;
    c.cp.pressure = pressure;
    c.cp.hydrostatic = flags & 1;
    c.cp.constant_volume = (flags >> 1) & 1;
    c.move = phase == TMDNET_MIN_MIDDLE;
    c.virial = virial;
    c.box = box;
    c.deform = deform;
    c.cell_vel = cell_vel;
    c.cell_factor = cell_factor;
    c.stress_row = stress_log_row;
    c.volume_row = volume_log_row;
    c.cell_force_row = cell_force_log_row;
    hipLaunchKernelGGL(k_min_control_cell, dim3(1), block, 0, s, c);
  } else {
    hipLaunchKernelGGL(k_min_cell_commit, dim3((B + kThreads - 1) / kThreads), block, 0, s, st, cs, B, box, deform, cell_vel);
  }
  if (N > 0) {
    MinCellAtomArgs a;
    a.base.N = N;
    a.base.B = B;
    a.base.pos = pos;
    a.base.vel = vel;
    a.base.forces = forces;
    a.base.forces_keep = forces_keep;
    a.base.fixed = fixed;
    a.base.batch = batch;
    a.base.counts = counts;
    a.base.st = st;
    a.cs = cs;
    a.xt = xt;
    const dim3 grid((N + kThreads - 1) / kThreads);
    if (phase == TMDNET_MIN_OPEN)
      hipLaunchKernelGGL((k_min_atoms_cell<false, true>), grid, block, 0, s, a);
    else if (phase == TMDNET_MIN_MIDDLE)
      hipLaunchKernelGGL((k_min_atoms_cell<true, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((k_min_atoms_cell<true, false>), grid, block, 0, s, a);
  }
  return loop_launch_result(m, "tmdnet_min_advance_cell");
}

int tmdnet_min_status_cell(void* stream, void* min_ws, uint64_t host[3]) {
  if (!min_ws || !host) return TMDNET_ERR_INVALID;
  return loop_read_status(stream, carve_min(min_ws, 0, 0).head, kMinCellCauseWord + 1, kMinCellCauseWord, host, 3);
}

}  // extern "C"
