// Device-resident minima hopping: the kernels that sit between two energy+force evaluations of a captured step, so that K steps of a
// conformer search replay as one HIP graph with no host work in between.  The B molecules of a batch are B independent walkers; each
// is in one of four phases - QUENCH (FIRE), COMPARE (is the fresh minimum new?), LAUNCH (remove momentum and angular momentum of the
// drawn velocities), MD (an NVE escape) - and walkers in different phases share the one evaluation of the step.  The arithmetic,
// the phase machine included, is tn_hop_math.h; the scheme is stated with the entries in include/tmdnet_amd.h.
//
// One step, after the energies E and forces F at pos are known - three launches (four when a molecule has more than one slice):
//   reduce    grid (walker, slice): the sums the walker's phase needs over the slice's atoms - FIRE's four, the escape's three, the
//             17 of a launch, or the 18 of every pair (fresh minimum, reference) of a comparison
//   finish    only with S > 1 slices: the slice sums added in slice order
//   control   ONE block, walkers strided: tn_hop::walker_control, the status word, the walkers' public state and the log rows
//   move      per atom: tn_hop::atom_apply with the walker's decision, after saving x and v
// Reductions are tn_loop.h's fixed-order ones.  No floating-point atomics: repeats are bit-identical.  Overflow and unusable sums
// follow the minimiser's protocol: the controller is the only kernel that writes the status word; an overflowed evaluation latches
// status 1 and the per-atom kernel puts back the x and v its last move saved; an energy or a sum that is not finite latches status 2
// before anything of that step is written.  From then on every launch returns at once until tmdnet_hop_reset.
// The fp64 statements of a walker must give the host checker's bits: no product is contracted into the sum that consumes it.
#pragma clang fp contract(off)
#include <cmath>

#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_hop_math.h"
#include "tn_loop.h"
#include "tn_model.h"

namespace tn {

namespace {

using namespace tn_hop;

struct HopState {  // views into the caller's workspace
  uint32_t* head;    // [0] step lo, [1] step hi, [2] status (sticky: 1 overflow, 2 an energy or a sum that is not finite)
  Walker* walker;    // [B]
  Decision* dec;     // [B]
  double* tot;       // [B, W] the sums of this step, W = 18 (capacity + 1)
  double* slices;    // [B, S, W] (S > 1 only)
  float* x_keep;     // [N, 3] positions before the last move
  float* v_keep;     // [N, 3]
};

inline int hop_width(int capacity) { return kPair * (capacity + 1); }

HopState hop_layout(LoopCarver& c, int64_t N, int64_t B, int capacity) {
  const size_t n = (size_t)(N > 0 ? N : 0), b = (size_t)(B > 0 ? B : 0), W = (size_t)hop_width(capacity);
  const size_t S = (size_t)mol_slices(N, B);
  HopState st;
  st.head = c.take<uint32_t>(kHeaderBytes / sizeof(uint32_t));
  st.walker = c.take<Walker>(b);
  st.dec = c.take<Decision>(b);
  st.tot = c.take<double>(b * W);
  st.slices = c.take<double>(S > 1 ? b * S * W : 0);
  st.x_keep = c.take<float>(n * 3);
  st.v_keep = c.take<float>(n * 3);
  return st;
}

size_t hop_bytes(int64_t N, int64_t B, int capacity) {
  return layout_bytes([&](LoopCarver& c) { hop_layout(c, N, B, capacity); });
}

HopState carve_hop(void* ws, int64_t N, int64_t B, int capacity) {
  LoopCarver c(ws);
  return hop_layout(c, N, B, capacity);
}

struct HopArgs {
  int N, B, S, W;
  HopParams p;
  tmdnet_hop_args a;  // the caller's buffers
  const int* counts;  // the graph's counters and molecule ranges, or NULL
  const int* mstart;
  const int* mend;
  HopState st;
};

__device__ __forceinline__ Ring hop_ring(const HopArgs& h, int m) {
  Ring r;
  r.energy = h.a.ring_energy + (int64_t)m * h.p.capacity;
  r.found_at = h.a.ring_found + (int64_t)m * h.p.capacity;
  r.visits = h.a.ring_visits + (int64_t)m * h.p.capacity;
  return r;
}

// grid (B, S): slice s of walker m -> tot[m] (S == 1) or slices[m, s].  Threads stride the atoms, lanes by the xor tree, waves in
// turn.  The accumulators of one reduction are at most 18 fp64 values per lane; the references of a comparison are taken one after
// the other through the same 18, so the kernel's register need does not grow with the capacity.
__global__ __launch_bounds__(kThreads) void k_hop_reduce(HopArgs h) {
  __shared__ double sh[kPair][kThreads / 64];
  if (h.st.head[kHeadStatus]) return;               // frozen
  if (h.counts && h.counts[2]) return;    // overflowed: stale forces, the controller latches it
  const int m = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
  const Walker& w = h.st.walker[m];
  const int phase = w.phase;
  const SliceRange r = mol_slice_range(h.counts, h.mstart, h.mend, h.N, h.S, h.a.batch, m, s);
  double* out = h.S == 1 ? h.st.tot + (int64_t)m * h.W : h.st.slices + ((int64_t)m * h.S + s) * h.W;
  if (phase == PH_QUENCH || phase == PH_MD) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = r.i0 + t; i < r.i1; i += kThreads) {
      if (slice_skips(r, h.a.batch, i, m)) continue;
      float v[3], f[3], tm[4];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v[k] = h.a.vel[i * 3 + k];
        f[k] = h.a.forces[i * 3 + k];
      }
      const int fx = h.a.fixed && h.a.fixed[i];
      if (phase == PH_QUENCH)
        quench_terms(v, f, fx, tm);
      else
        md_terms(v, f, h.a.hk[i], h.a.mass[i], fx, tm);
      acc[0] += (double)tm[0];
      acc[1] += (double)tm[1];
      acc[2] += (double)tm[2];
      acc[3] = (double)tm[3] > acc[3] ? (double)tm[3] : acc[3];
    }
    block_reduce_waves<4, 8u>(acc, sh);
    if (t == 0) block_reduce_rows<4, 8u>(sh, out);
    return;
  }
  if (phase == PH_LAUNCH) {
    const float cen[3] = {(float)w.cen[0], (float)w.cen[1], (float)w.cen[2]};
    double acc[kLaunch];
#pragma unroll
    for (int k = 0; k < kLaunch; ++k) acc[k] = 0.0;
    for (int i = r.i0 + t; i < r.i1; i += kThreads) {
      if (slice_skips(r, h.a.batch, i, m)) continue;
      float x[3], v[3], f[3];
      double tm[kLaunch];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        x[k] = h.a.pos[i * 3 + k];
        v[k] = h.a.vel[i * 3 + k];
        f[k] = h.a.forces[i * 3 + k];
      }
      launch_terms(x, v, f, h.a.mass[i], cen, h.a.fixed && h.a.fixed[i], tm);
#pragma unroll
      for (int k = 0; k < kLaunch; ++k) acc[k] += tm[k];
    }
    block_reduce_waves<kLaunch, 0u>(acc, sh);
    if (t == 0) block_reduce_rows<kLaunch, 0u>(sh, out);
    return;
  }
  // PH_COMPARE: one pass over the slice per reference that is looked at
  const double E = (double)h.a.energy[m];
  const double* ring_e = h.a.ring_energy + (int64_t)m * h.p.capacity;
  for (int ref = 0; ref <= h.p.capacity; ++ref) {
    if (!ref_considered(w, ring_e, h.p.capacity, ref, E, h.p.energy_tol)) continue;  // (the same answer in every thread)
    const float* b = ref == 0 ? (w.has_cur ? h.a.cur_pos : h.a.pos) : h.a.ring_pos + (int64_t)(ref - 1) * h.N * 3;
    double acc[kPair];
#pragma unroll
    for (int k = 0; k < kPair; ++k) acc[k] = 0.0;
    for (int i = r.i0 + t; i < r.i1; i += kThreads) {
      if (slice_skips(r, h.a.batch, i, m)) continue;
      float xa[3], xb[3];
      double tm[kPair];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        xa[k] = h.a.pos[i * 3 + k];
        xb[k] = b[i * 3 + k];
      }
      pair_terms(xa, xb, tm);
#pragma unroll
      for (int k = 0; k < kPair; ++k) acc[k] += tm[k];
    }
    block_reduce_waves<kPair, 0u>(acc, sh);
    if (t == 0) block_reduce_rows<kPair, 0u>(sh, out + ref * kPair);
    __syncthreads();  // (sh is written again by the next reference)
  }
}

// grid (B), S > 1 only: tot[m, j] = the slices' entries j in slice order; entry 3 of QUENCH and MD takes the maximum
__global__ __launch_bounds__(kThreads) void k_hop_finish(HopArgs h) {
  if (h.st.head[kHeadStatus]) return;
  if (h.counts && h.counts[2]) return;
  const int m = blockIdx.x;
  const Walker& w = h.st.walker[m];
  const int phase = w.phase;
  const int used = phase == PH_COMPARE ? h.W : phase_sums(phase);
  const double E = phase == PH_COMPARE ? (double)h.a.energy[m] : 0.0;
  const double* ring_e = h.a.ring_energy + (int64_t)m * h.p.capacity;
  for (int j = threadIdx.x; j < used; j += kThreads) {
    if (phase == PH_COMPARE && !ref_considered(w, ring_e, h.p.capacity, j / kPair, E, h.p.energy_tol)) continue;
    const bool mx = phase != PH_COMPARE && phase != PH_LAUNCH && j == 3;
    const double* sl = h.st.slices + (int64_t)m * h.S * h.W + j;
    double v = 0.0;
    for (int s = 0; s < h.S; ++s) {
      const double x = sl[(int64_t)s * h.W];
      v = mx ? (x > v ? x : v) : v + x;
    }
    h.st.tot[(int64_t)m * h.W + j] = v;
  }
}

// ONE block striding the walkers, after the reduction: optimiser_control (tn_loop.h) without a fresh word - the counter always
// advances - and without causes.  Pass 1: is any walker's step unusable?  Pass 2: every walker's state, decision, public state and
// log rows.
__global__ __launch_bounds__(kThreads) void k_hop_control(HopArgs h) {
  optimiser_control(
      h.st.head, h.counts, -1, false, h.B,
      [&](int m, bool, uint64_t) {
        return (int)!walker_usable(h.st.walker[m], hop_ring(h, m), h.p, h.st.tot + (int64_t)m * h.W, (double)h.a.energy[m]);
      },
      [&](int m, bool, uint64_t step) {
        Walker w = h.st.walker[m];
        Decision d;
        double log[kSumsLog];
        const double* tot = h.st.tot + (int64_t)m * h.W;
        const double E = (double)h.a.energy[m];
        walker_control(&w, hop_ring(h, m), h.p, tot, E, (int64_t)step, &d, log);
        h.st.walker[m] = w;
        h.st.dec[m] = d;
        h.a.kT[m] = w.kT;
        h.a.ediff[m] = w.ediff;
        h.a.cur_energy[m] = w.e_cur;
        h.a.best_energy[m] = w.e_best;
        h.a.phase[m] = w.phase;
#pragma unroll
        for (int k = 0; k < kCounters; ++k) h.a.counters[(int64_t)m * kCounters + k] = w.n[k];
        if (h.a.epot_row) h.a.epot_row[m] = h.a.energy[m];
        if (h.a.fmax_row) h.a.fmax_row[m] = d.phase == PH_QUENCH || d.phase == PH_MD ? (float)sqrt(tot[3]) : 0.f;
        if (h.a.ekin_row) h.a.ekin_row[m] = d.phase == PH_MD ? (float)tot[0] : 0.f;
        if (h.a.phase_row) h.a.phase_row[m] = d.phase;
        if (h.a.outcome_row) h.a.outcome_row[m] = d.outcome;
        if (h.a.sums_row)
#pragma unroll
          for (int k = 0; k < kSumsLog; ++k) h.a.sums_row[(int64_t)m * kSumsLog + k] = log[k];
        if (h.a.coef_row) {
          float* c = h.a.coef_row + (int64_t)m * kCoefLog;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            c[k] = d.coef[k];
            c[3 + k] = d.u[k];
            c[6 + k] = d.w[k];
          }
          c[9] = d.vscale;
        }
      });
}

// One thread per atom, the caller's atom order, after k_hop_control: keep the forces of the evaluation, save x and v, then
// tn_hop::atom_apply with the decision of the atom's walker; or, when the evaluation overflowed (the controller has just latched
// it), x and v back to what the last move saved.
__global__ __launch_bounds__(kThreads) void k_hop_move(HopArgs h) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= h.N) return;
  const uint32_t status = h.st.head[kHeadStatus];
  if (status) {
    if (status == 1u && h.counts && h.counts[2]) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        h.a.pos[i * 3 + k] = h.st.x_keep[i * 3 + k];
        h.a.vel[i * 3 + k] = h.st.v_keep[i * 3 + k];
      }
    }
    return;
  }
  const int64_t m = h.a.batch ? h.a.batch[i] : 0;
  if (m < 0 || m >= h.B) return;
  const Decision d = h.st.dec[m];
  float x[3], v[3], f[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    f[k] = h.a.forces[i * 3 + k];
    x[k] = h.a.pos[i * 3 + k];
    v[k] = h.a.vel[i * 3 + k];
    h.st.x_keep[i * 3 + k] = x[k];
    h.st.v_keep[i * 3 + k] = v[k];
  }
  if (h.a.forces_keep)
#pragma unroll
    for (int k = 0; k < 3; ++k) h.a.forces_keep[i * 3 + k] = f[k];
  float* ring = d.slot >= 0 ? h.a.ring_pos + ((int64_t)d.slot * h.N + i) * 3 : nullptr;
  atom_apply(d, h.p.dt, h.p.seed, (uint32_t)i, h.a.fixed && h.a.fixed[i], h.a.hk[i], h.a.sig[i], f, x, v, h.a.cur_pos + (int64_t)i * 3,
             ring, h.a.best_pos + (int64_t)i * 3);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    h.a.pos[i * 3 + k] = x[k];
    h.a.vel[i * 3 + k] = v[k];
  }
}

struct HopResetArgs {
  int N, B;
  HopParams p;
  HopState st;
  uint64_t step0;
  const double* kT0;
  const double* ediff0;
  int keep;
  const float* pos;
  const float* vel;
  double* kT;
  double* ediff;
  double* cur_energy;
  double* best_energy;
  int32_t* phase;
  int64_t* counters;
};

__global__ __launch_bounds__(kThreads) void k_hop_reset(HopResetArgs r) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) {
    loop_set_step(r.st.head, r.step0);
    r.st.head[kHeadStatus] = 0u;
  }
  if (i < r.B) {
    Walker w = r.st.walker[i];
    walker_reset(&w, r.p, r.kT0[i], r.ediff0[i], r.keep);
    r.st.walker[i] = w;
    r.st.dec[i].action = ACT_NONE;
    r.kT[i] = w.kT;
    r.ediff[i] = w.ediff;
    r.cur_energy[i] = w.e_cur;
    r.best_energy[i] = w.e_best;
    r.phase[i] = w.phase;
    for (int k = 0; k < kCounters; ++k) r.counters[(int64_t)i * kCounters + k] = w.n[k];
  }
  if (i < r.N)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r.st.x_keep[i * 3 + k] = r.pos[i * 3 + k];
      r.st.v_keep[i * 3 + k] = r.vel[i * 3 + k];
    }
}

bool hop_shape_ok(int64_t N, int64_t B, int64_t capacity) {
  if (N < 1 || B < 1 || B > INT32_MAX / 64 || N > INT32_MAX / 4) return false;
  if (capacity < 1 || capacity > kMaxCapacity) return false;
  return capacity <= (INT32_MAX / 4) / N;  // the rows of the ring stay below 2^31 floats
}

// the parameters, and the buffers a reset touches (`step`: also those only a step reads)
bool hop_args_ok(const tmdnet_hop_args* a, bool step) {
  if (!a) return false;
  if (!a->pos || !a->vel) return false;
  if (!a->kT || !a->ediff || !a->cur_energy || !a->best_energy || !a->phase || !a->counters) return false;
  if (step && (!a->forces || !a->energy || !a->hk || !a->mass || !a->sig)) return false;
  if (step && (!a->cur_pos || !a->best_pos || !a->ring_pos || !a->ring_energy || !a->ring_found || !a->ring_visits)) return false;
  if (!(a->fmax > 0.0) || !(a->dt_max > 0.0) || !(a->max_step > 0.0) || !(a->f_inc > 0.0) || !(a->f_dec > 0.0) || !(a->f_alpha > 0.0) ||
      !(a->alpha0 >= 0.0) || !(a->dt0 > 0.0) || a->n_min < 0)
    return false;
  if (!(a->beta1 > 0.0) || !(a->beta2 > 0.0) || !(a->beta3 > 0.0) || !(a->alpha1 > 0.0) || !(a->alpha2 > 0.0)) return false;
  if (!(a->rmsd_tol > 0.0) || !(a->energy_tol > 0.0) || !(a->dt > 0.f)) return false;
  if (a->mdmin < 1 || a->md_steps < 1 || a->opt_steps < 1) return false;
  return a->align == ALIGN_NONE || a->align == ALIGN_TRANSLATION || a->align == ALIGN_ROTATION;
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_hop_workspace_bytes(int64_t n_atoms, int64_t n_mol, int32_t capacity, size_t* bytes) {
  if (!bytes || !hop_shape_ok(n_atoms, n_mol, capacity)) return TMDNET_ERR_INVALID;
  *bytes = hop_bytes(n_atoms, n_mol, capacity);
  return TMDNET_OK;
}

int tmdnet_hop_reset(void* stream, void* hop_ws, int64_t n_atoms, int64_t n_mol, const tmdnet_hop_args* args, uint64_t step0,
                     const double* kT0, const double* ediff0, int32_t keep_history) {
  if (!hop_ws || !hop_args_ok(args, false) || !kT0 || !ediff0 || !hop_shape_ok(n_atoms, n_mol, args->capacity)) return TMDNET_ERR_INVALID;
  HopResetArgs r;
  r.N = (int)n_atoms;
  r.B = (int)n_mol;
  r.p = hop_params(*args);
  r.st = carve_hop(hop_ws, n_atoms, n_mol, args->capacity);
  r.step0 = step0;
  r.kT0 = kT0;
  r.ediff0 = ediff0;
  r.keep = keep_history != 0;
  r.pos = args->pos;
  r.vel = args->vel;
  r.kT = args->kT;
  r.ediff = args->ediff;
  r.cur_energy = args->cur_energy;
  r.best_energy = args->best_energy;
  r.phase = args->phase;
  r.counters = args->counters;
  const int64_t rows = n_atoms > n_mol ? n_atoms : n_mol;
  hipLaunchKernelGGL(k_hop_reset, dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), r);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_hop_advance(tmdnet_model* m, void* stream, void* graph_ws, void* hop_ws, int64_t n_atoms, int64_t n_mol,
                       const tmdnet_hop_args* args) {
  if (!hop_ws || !hop_args_ok(args, true) || !hop_shape_ok(n_atoms, n_mol, args->capacity)) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (n_mol > 1 && !args->batch) return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HopArgs h;
  h.N = (int)n_atoms;
  h.B = (int)n_mol;
  h.S = mol_slices(n_atoms, n_mol);
  h.W = hop_width(args->capacity);
  h.p = hop_params(*args);
  h.a = *args;
  const LoopGraph g = loop_graph(m, graph_ws, n_atoms, n_mol);
  h.counts = g.counts;
  h.mstart = g.mstart;
  h.mend = g.mend;
  h.st = carve_hop(hop_ws, n_atoms, n_mol, args->capacity);
  const dim3 block(kThreads);
  hipLaunchKernelGGL(k_hop_reduce, dim3((unsigned)h.B, (unsigned)h.S), block, 0, s, h);
  if (h.S > 1) hipLaunchKernelGGL(k_hop_finish, dim3((unsigned)h.B), block, 0, s, h);
  hipLaunchKernelGGL(k_hop_control, dim3(1), block, 0, s, h);
  hipLaunchKernelGGL(k_hop_move, dim3((unsigned)((h.N + kThreads - 1) / kThreads)), block, 0, s, h);
  return loop_launch_result(m, "tmdnet_hop_advance");
}

int tmdnet_hop_status(void* stream, void* hop_ws, uint64_t host[2]) {
  if (!hop_ws || !host) return TMDNET_ERR_INVALID;
  return loop_read_status(stream, carve_hop(hop_ws, 0, 0, 1).head, 3, -1, host, 2);
}

}  // extern "C"
