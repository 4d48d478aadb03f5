// Holonomic distance constraints |x_i - x_j| = d_c inside the device-resident MD loop: RATTLE in the splitting of tn_md.hip.
//   B   v <- v + hk F
//   A   x <- x + dt v
//   S   SHAKE: x <- x + Dx so that every constraint holds (reference directions: the saved x of the step's start), v <- v + Dx / dt
//       F = F(x)
//   B   v <- v + hk F
//  [O]  v <- c1 v + c2 sigma xi
//   R   RATTLE: v <- v + Dv so that (x_i - x_j).(v_i - v_j) = 0 for every constraint; kinetic energy of the projected v
// The connected components of the constraint graph (clusters: a heavy atom with its hydrogens, a rigid water) are independent, so
// one work item does a whole cluster's step: it closes step k (B, O, R, kinetic terms) and opens step k + 1 (save, B, A, S) on the
// same registers, and K constrained steps stay K + 1 integrator launches plus the kinetic-energy reductions.
//
// Geometry.  A group of 8 lanes per cluster, one lane per atom (8 clusters per wave); atoms in no constraint are packed 8 to a group
// with an empty table.  The cluster's table (a, b, d^2) in cluster-local indices is read uniformly by the group, the constraints
// are relaxed one after the other in table order, and a partner's coordinates come through a shuffle inside the group: every lane
// of a group evaluates the same multiplier from the same values, so all decisions are group-uniform without a reduction, there is
// no dynamically indexed register array and no scratch.  The result of a cluster does not depend on which group, wave or block it
// landed in.  B, A, O and the kinetic term are tn_md's own functions with the caller's atom index as the Philox counter: an atom in
// no constraint gets exactly the bits k_md_atoms gives it.  The constraint arithmetic is tn_md_cons_math.h (fp64).
//
// Failure.  A cluster that has not converged after max_iter sweeps, or that met a non-finite value, writes its atoms' saved state
// (x_keep, v_keep) back, ORs the fail word of the constraint workspace and does nothing else: unconverged positions are never
// written, so the evaluation that follows sees finite coordinates.  The next reduction kernel latches status 3; every cluster
// launch that finds the status word or the fail word set returns at once.  The fail word is read at entry while other clusters of
// the same launch may be setting it: which clusters of a FAILING launch still complete their half step depends on the scheduling,
// so the frozen state after a failure (finite, not a point of the trajectory) is not reproducible from run to run; the bit-identical
// repeats hold for runs in which no cluster fails.  The overflow protocol of tn_md.hip is unchanged.
#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_md_cons_math.h"
#include "tn_md_math.h"
#include "tn_md_state.h"
#include "tn_model.h"

namespace tn {

namespace {

constexpr int kGroup = tn_md_cons::kMaxAtoms;

// the constraint workspace: the word a cluster ORs when it gives up
inline uint32_t* cons_layout(LoopCarver& c) { return c.take<uint32_t>(1); }

struct ConsArgs {
  int N, n_clusters, n_cons;
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
  const int* counts;        // the graph's counters, or NULL
  const int* cl_atoms;      // [n_clusters, 8] caller's atom index, -1: no atom
  const int* cl_off;        // [n_clusters + 1] into the constraint table
  const int* cons_ab;       // [n_cons, 2] cluster-local ends
  const double* cons_d2;    // [n_cons]
  double tol;
  int max_iter;
  uint32_t* fail;
  MdState st;
};

__device__ __forceinline__ void fetch3(const double x[3], int src, double out[3]) {
#pragma unroll
  for (int d = 0; d < 3; ++d) out[d] = __shfl(x[d], src, kGroup);
}

// 1 when `ok` holds on every lane of this group (all lanes of a group are in the same control flow)
__device__ __forceinline__ int group_all(int ok) {
  const unsigned long long bad = __ballot(!ok);
  const int first = (int)(threadIdx.x & 63) & ~(kGroup - 1);
  return ((bad >> first) & 0xffull) == 0;
}

// SHAKE of constraints [c0, c1) on the group's positions x (fp64, one atom per lane); k: the saved positions, w = 1 / m.
// Group-uniform result: 1 converged.
__device__ __forceinline__ int group_shake(const ConsArgs& a, int c0, int c1, int l, double x[3], const double k[3], double w) {
  int moved = 0;
  for (int it = 0; it <= a.max_iter; ++it) {
    moved = 0;
    for (int c = c0; c < c1; ++c) {
      const int la = a.cons_ab[2 * c] & (kGroup - 1), lb = a.cons_ab[2 * c + 1] & (kGroup - 1);
      double xa[3], xb[3], ka[3], kb[3], g;
      fetch3(x, la, xa);
      fetch3(x, lb, xb);
      fetch3(k, la, ka);
      fetch3(k, lb, kb);
      const double wa = __shfl(w, la, kGroup), wb = __shfl(w, lb, kGroup);
      if (tn_md_cons::shake_one(xa, xb, ka, kb, wa, wb, a.cons_d2[c], a.tol, &g)) continue;
      moved = 1;
      if (it == a.max_iter) continue;  // the last sweep only tests
      if (l == la) tn_md_cons::move_along(x, g * wa, ka, kb);
      if (l == lb) tn_md_cons::move_along(x, -(g * wb), ka, kb);
    }
    if (!moved) break;
  }
  return !moved;
}

// RATTLE of constraints [c0, c1) on the group's velocities v (fp64) at the positions x.  Group-uniform result: 1 converged.
__device__ __forceinline__ int group_rattle(const ConsArgs& a, int c0, int c1, int l, const double x[3], double v[3], double w) {
  int moved = 0;
  for (int it = 0; it <= a.max_iter; ++it) {
    moved = 0;
    for (int c = c0; c < c1; ++c) {
      const int la = a.cons_ab[2 * c] & (kGroup - 1), lb = a.cons_ab[2 * c + 1] & (kGroup - 1);
      double xa[3], xb[3], va[3], vb[3], k;
      fetch3(x, la, xa);
      fetch3(x, lb, xb);
      fetch3(v, la, va);
      fetch3(v, lb, vb);
      const double wa = __shfl(w, la, kGroup), wb = __shfl(w, lb, kGroup);
      if (tn_md_cons::rattle_one(xa, xb, va, vb, wa, wb, a.cons_d2[c], (double)a.dt, a.tol, &k)) continue;
      moved = 1;
      if (it == a.max_iter) continue;
      if (l == la) tn_md_cons::move_along(v, k * wa, xa, xb);
      if (l == lb) tn_md_cons::move_along(v, -(k * wb), xa, xb);
    }
    if (!moved) break;
  }
  return !moved;
}

// a cluster gives up: its atoms go back to the saved state, one lane ORs the fail word
__device__ __forceinline__ void give_up(const ConsArgs& a, int i, int l, bool restore, unsigned bits) {
  if (restore && i >= 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a.pos[i * 3 + d] = a.st.x_keep[i * 3 + d];
      a.vel[i * 3 + d] = a.st.v_keep[i * 3 + d];
    }
  }
  if (l == 0) atomicOr(a.fail, bits);
}

// one lane per atom, one group of 8 lanes per cluster.  CLOSE / OPEN as in k_md_atoms, with R after the closing half and S after
// the opening one; neither: R alone (TMDNET_MD_PROJECT).
template <bool CLOSE, bool OPEN>
__global__ __launch_bounds__(kThreads) void k_md_clusters(ConsArgs a) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  const int cl = t / kGroup, l = t % kGroup;
  if (cl >= a.n_clusters) return;              // (whole groups)
  if (a.st.head[2] || a.fail[0]) return;       // frozen, or a cluster gave up since the last reduction
  int i = a.cl_atoms[cl * kGroup + l];
  if (i >= a.N) i = -1;
  const bool on = i >= 0;
  if (CLOSE && a.counts && a.counts[2]) {  // this evaluation overflowed: back to the last completed step
    if (on) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        a.pos[i * 3 + d] = a.st.x_keep[i * 3 + d];
        a.vel[i * 3 + d] = a.st.v_keep[i * 3 + d];
      }
    }
    return;
  }
  int c0 = a.cl_off[cl], c1 = a.cl_off[cl + 1];
  c0 = c0 < 0 ? 0 : c0;
  c1 = c1 > a.n_cons ? a.n_cons : c1;
  const bool bound = c1 > c0;  // a cluster with constraints: every atom of it is an end of one
  float x[3] = {0.f, 0.f, 0.f}, v[3] = {0.f, 0.f, 0.f}, f[3] = {0.f, 0.f, 0.f};
  float hk = 0.f, m = 1.f;
  if (on) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      v[d] = a.vel[i * 3 + d];
      if (CLOSE || OPEN) f[d] = a.forces[i * 3 + d];
    }
    if (CLOSE || OPEN) hk = a.hk[i];
    if (a.mass) m = a.mass[i];
  }
  const double w = tn_md_cons::inv_mass(m);
  if (bound || OPEN)
    if (on)
#pragma unroll
      for (int d = 0; d < 3; ++d) x[d] = a.pos[i * 3 + d];
  if (CLOSE) {
    float ke = 0.f;
    if (on)
      ke = tn_md::close_step(v, f, hk, m, a.thermostat, a.c1, a.c2, a.thermostat ? a.sigma[i] : 0.f, a.seed, loop_step(a.st.head),
                             (uint32_t)i);
    if (bound) {
      const double x64[3] = {(double)x[0], (double)x[1], (double)x[2]};
      double v64[3] = {(double)v[0], (double)v[1], (double)v[2]};
      int ok = group_rattle(a, c0, c1, l, x64, v64, w);
      if (ok) ok = group_all(tn_md_cons::rattle_finish(v64, v));
      if (!ok) {
        give_up(a, i, l, true, tn_md_cons::kFailRattle);
        return;
      }
      ke = tn_md::kinetic(m, v[0], v[1], v[2]);
    }
    if (on) {
      a.st.part[i] = ke;
      if (a.forces_keep)
#pragma unroll
        for (int d = 0; d < 3; ++d) a.forces_keep[i * 3 + d] = f[d];
    }
  }
  if (!CLOSE && !OPEN && bound) {  // the projection alone: nothing is saved yet, so a failure leaves the velocities as they are
    const double x64[3] = {(double)x[0], (double)x[1], (double)x[2]};
    double v64[3] = {(double)v[0], (double)v[1], (double)v[2]};
    int ok = group_rattle(a, c0, c1, l, x64, v64, w);
    if (ok) ok = group_all(tn_md_cons::rattle_finish(v64, v));
    if (!ok) {
      give_up(a, i, l, false, tn_md_cons::kFailRattle);
      return;
    }
  }
  if (OPEN) {
    const double k64[3] = {(double)x[0], (double)x[1], (double)x[2]};
    if (on) md_save_and_open(a.st, i, x, v, f, hk, a.dt);
    if (bound) {
      double x64[3] = {(double)x[0], (double)x[1], (double)x[2]};
      int ok = group_shake(a, c0, c1, l, x64, k64, w);
      if (ok) ok = group_all(tn_md_cons::shake_finish(x64, x, v, (double)a.dt));
      if (!ok) {
        give_up(a, i, l, true, tn_md_cons::kFailShake);
        return;
      }
    }
    if (on)
#pragma unroll
      for (int d = 0; d < 3; ++d) a.pos[i * 3 + d] = x[d];
  }
  if (on)
#pragma unroll
    for (int d = 0; d < 3; ++d) a.vel[i * 3 + d] = v[d];
}

// after the projection alone: no reduction follows, so the fail word is latched here
__global__ void k_md_cons_latch(MdState st, const uint32_t* __restrict__ fail) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && !st.head[2] && fail[0]) st.head[2] = 3u;
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_md_constraints_workspace_bytes(int64_t n_atoms, int64_t n_clusters, int64_t n_constraints, size_t* bytes) {
  if (!bytes || n_atoms < 0 || n_atoms > INT32_MAX / 4 || n_clusters < 0 || n_clusters > INT32_MAX / 16 || n_constraints < 0 ||
      n_constraints > (int64_t)tn_md_cons::kMaxCons * n_clusters)
    return TMDNET_ERR_INVALID;
  *bytes = layout_bytes([](LoopCarver& c) { cons_layout(c); });
  return TMDNET_OK;
}

int tmdnet_md_advance_constrained(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* cons_ws, int64_t n_atoms,
                                  int64_t n_mol, int32_t phase, float* pos, float* vel, const float* forces, const float* energy,
                                  const float* hk, const float* mass, const float* sigma, float dt, float c1, float c2, uint64_t seed,
                                  const int64_t* batch, float* forces_keep, float* epot_log_row, float* ekin_log_row,
                                  int64_t n_clusters, int64_t n_constraints, const int32_t* cluster_atoms,
                                  const int32_t* cluster_offsets, const int32_t* constraint_ends, const double* constraint_d2, double tol,
                                  int32_t max_iter) {
  if (!md_ws || !cons_ws || !pos || !vel || !mass || n_atoms < 0 || n_atoms > INT32_MAX / 4 || n_mol < 1) return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MD_OPEN && phase != TMDNET_MD_MIDDLE && phase != TMDNET_MD_CLOSE && phase != TMDNET_MD_PROJECT)
    return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MD_PROJECT && (!forces || !hk)) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (n_clusters < 0 || n_clusters > INT32_MAX / 16 || n_constraints < 0 || n_constraints > (int64_t)tn_md_cons::kMaxCons * n_clusters)
    return TMDNET_ERR_INVALID;
  if (n_clusters > 0 && (!cluster_atoms || !cluster_offsets)) return TMDNET_ERR_INVALID;
  if (n_constraints > 0 && (!constraint_ends || !constraint_d2)) return TMDNET_ERR_INVALID;
  if (!(tol > 0.0) || max_iter < 1) return TMDNET_ERR_INVALID;
  if (n_atoms == 0 || n_clusters == 0) return TMDNET_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N = (int)n_atoms, B = (int)n_mol;
  ConsArgs a;
  a.N = N;
  a.n_clusters = (int)n_clusters;
  a.n_cons = (int)n_constraints;
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
  a.cl_atoms = cluster_atoms;
  a.cl_off = cluster_offsets;
  a.cons_ab = constraint_ends;
  a.cons_d2 = constraint_d2;
  a.tol = tol;
  a.max_iter = max_iter;
  LoopCarver c(cons_ws);
  a.fail = cons_layout(c);
  a.st = carve_md(md_ws, n_atoms, n_mol);
  const LoopGraph g = loop_graph(m, graph_ws, n_atoms, n_mol);
  a.counts = g.counts;
  const int64_t lanes = n_clusters * kGroup;
  const dim3 grid((unsigned)((lanes + kThreads - 1) / kThreads)), block(kThreads);
  if (phase == TMDNET_MD_OPEN)
    hipLaunchKernelGGL((k_md_clusters<false, true>), grid, block, 0, s, a);
  else if (phase == TMDNET_MD_MIDDLE)
    hipLaunchKernelGGL((k_md_clusters<true, true>), grid, block, 0, s, a);
  else if (phase == TMDNET_MD_CLOSE)
    hipLaunchKernelGGL((k_md_clusters<true, false>), grid, block, 0, s, a);
  else {
    hipLaunchKernelGGL((k_md_clusters<false, false>), grid, block, 0, s, a);
    hipLaunchKernelGGL(k_md_cons_latch, dim3(1), dim3(64), 0, s, a.st, a.fail);
  }
  if (phase == TMDNET_MD_MIDDLE || phase == TMDNET_MD_CLOSE) {
    const int S = mol_slices(n_atoms, n_mol);
    float* out = S == 1 ? ekin_log_row : a.st.slices;
    hipLaunchKernelGGL(k_md_ke_reduce<true>, dim3(B, S), block, 0, s, a.st, g.counts, g.mstart, g.mend, N, B, S, batch, energy, epot_log_row,
                       out, a.fail);
    if (S > 1 && ekin_log_row)
      hipLaunchKernelGGL(k_md_ke_finish, dim3((B + kThreads - 1) / kThreads), block, 0, s, a.st, a.counts, B, S, ekin_log_row);
  }
  return loop_launch_result(m, "tmdnet_md_advance_constrained");
}

}  // extern "C"
