// Collective-variable restraints and metadynamics of the device-resident MD loop: ONE launch between the evaluation of a captured
// step and the integrator launch that closes it, which adds the bias force to the evaluation's force buffer in place.  The
// integrator, the evaluation and the neighbour search do not change: tmdnet_md_advance reads its forces from any buffer.
//
// A batch of B molecules is B walkers: kappa and the centres of the restraints are per walker (umbrella windows are one batch), and
// consecutive walkers form groups of W that share one list of hills (multiple-walker metadynamics).  The arithmetic is
// tn_bias_math.h, fp64 on the fp32 positions; the force on an atom is rounded to fp32 once and added with one md_add.
//
// One block of 256 threads per walker.  The first lanes compute the CVs, their gradients and the restraint terms into LDS; all four
// waves stride the group's hills and reduce V and dV/ds in a fixed order (a thread strides by 256, lanes add by the wave xor tree,
// waves add in turn: no floating-point atomics, bit-identical repeats); one lane per distinct atom of the walker then sums its
// (cv, slot) entries and writes the force.  No register array is indexed dynamically: what is indexed lives in LDS.
//
// Which hills exist is a function of the loop's step counter n, which only the closing launch that follows advances
// (tn_bias_math.h: hills_visible, hill_slot): a launch reads the slots below hill_base + ((n - step0) / pace) W and writes, on a
// deposit step, slots at or above that bound.  Hills are fp64 in a structure of arrays per group - centre 0 [H], centre 1 [H],
// height [H] - so a wave reads them coalesced.
//
// Frozen state: the kernel returns at once when the status word is set or the evaluation of this step overflowed (counts[2]; the
// closing launch then restores the state and latches status 1).  A walker that meets a value that is not finite leaves its forces
// alone, deposits nothing, writes no log row and stores status 4 (every writer stores the same constant); the closing launch, next
// in stream order, then returns at once, so the state stays where the opening half left it.
#include "tmdnet_amd.h"
#include "tn_bias_math.h"
#include "tn_common.h"
#include "tn_md_state.h"
#include "tn_model.h"

namespace tn {

namespace {

struct BiasArgs {
  int N, B, D, A, W, dm, mcv0, mcv1, deposit;
  const float* pos;
  float* forces;
  const int32_t* cv_kind;    // [D]
  const int32_t* cv_atoms;   // [D, 4] relative to the molecule's first atom
  const int32_t* mol_start;  // [B]
  const int32_t* atom_rel;   // [A]
  const int32_t* offsets;    // [A + 1]
  const int32_t* entries;    // [kMaxAtoms]
  const int32_t* res_kind;   // [D]
  const double* kappa;       // [B, D]
  const double* center;      // [B, D]
  double is0, is1, h0, kT, gamma;
  uint64_t pace;
  int64_t H;
  uint64_t* head;  // the bias workspace: step0, hill_base
  double* hills;   // [G, dm + 1, H]
  double* cv_row;
  double* res_row;
  double* bias_row;
  float* force_row;
  const int* counts;
  MdState st;
};

struct BiasWs {  // views into the caller's bias workspace
  uint64_t* head;  // [0] step0, [1] hill_base
  double* hills;   // [G, dm + 1, H] (dm > 0 only)
};

inline BiasWs bias_layout(LoopCarver& c, int64_t G, int dm, int64_t H) {
  BiasWs w;
  w.head = c.take<uint64_t>(kHeaderBytes / sizeof(uint64_t));
  w.hills = c.take<double>(dm > 0 ? (size_t)G * (size_t)(dm + 1) * (size_t)H : 0);
  return w;
}

__device__ __forceinline__ void load3(const float* pos, int64_t i, int N, double x[3]) {
  const bool ok = i >= 0 && i < N;  // an index outside the batch reads nothing: the CV is not finite, the walker reports status 4
#pragma unroll
  for (int d = 0; d < 3; ++d) x[d] = ok ? (double)pos[i * 3 + d] : (double)NAN;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void k_md_bias(BiasArgs a) {
  __shared__ double sh_s[tn_bias::kMaxCv], sh_er[tn_bias::kMaxCv], sh_dv[tn_bias::kMaxCv], sh_tot[tn_bias::kMaxCv];
  __shared__ double sh_grad[tn_bias::kMaxCv * 12];
  __shared__ double sh_red[4][3];
  __shared__ int sh_bad, sh_frozen;
  const int b = blockIdx.x, t = threadIdx.x;
  // one lane reads the status word for the block: another walker of this launch may store status 4 at any time, and the barriers
  // below need the whole block on one side.  Frozen: the status word is set, or this evaluation overflowed (the closing launch
  // restores the state and latches it).
  if (t == 0) {
    sh_frozen = a.st.head[2] != 0u || (a.counts && a.counts[2]);
    sh_bad = 0;
  }
  __syncthreads();
  if (sh_frozen) return;
  const uint64_t n = loop_step(a.st.head);
  const int64_t start = a.mol_start[b];
  if (t < a.D) {
    const int kind = a.cv_kind[t];
    double xi[3], xj[3], xk[3], xl[3], gi[3], gj[3], gk[3], gl[3];
    load3(a.pos, start + a.cv_atoms[t * 4 + 0], a.N, xi);
    load3(a.pos, start + a.cv_atoms[t * 4 + 1], a.N, xj);
    load3(a.pos, kind >= tn_bias::kAngle ? start + a.cv_atoms[t * 4 + 2] : start, a.N, xk);
    load3(a.pos, kind == tn_bias::kTorsion ? start + a.cv_atoms[t * 4 + 3] : start, a.N, xl);
    const double s = tn_bias::cv_eval(kind, xi, xj, xk, xl, gi, gj, gk, gl);
    double er = 0.0, dv = 0.0;
    const int rk = a.res_kind[t];
    if (rk != tn_bias::kNone)
      tn_bias::restraint(rk, a.kappa[(int64_t)b * a.D + t], tn_bias::diff(kind, s, a.center[(int64_t)b * a.D + t]), &er, &dv);
    bool ok = isfinite(s) && isfinite(er) && isfinite(dv);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      ok = ok && isfinite(gi[d]) && isfinite(gj[d]) && isfinite(gk[d]) && isfinite(gl[d]);
      sh_grad[t * 12 + d] = gi[d];
      sh_grad[t * 12 + 3 + d] = gj[d];
      sh_grad[t * 12 + 6 + d] = gk[d];
      sh_grad[t * 12 + 9 + d] = gl[d];
    }
    sh_s[t] = s;
    sh_er[t] = er;
    sh_dv[t] = dv;
    if (!ok) sh_bad = 1;
  }
  __syncthreads();
  double V = 0.0, d0 = 0.0, d1 = 0.0;
  if (a.dm > 0) {
    const int g = b / a.W;
    const uint64_t step0 = a.head[0], base = a.head[1];
    const int64_t nvis = tn_bias::hills_visible(n, step0, a.pace, a.W, base, a.H);
    const double* c0 = a.hills + (int64_t)g * (a.dm + 1) * a.H;
    const double* c1 = c0 + (a.dm == 2 ? a.H : 0);
    const double* hw = c0 + (int64_t)a.dm * a.H;
    const int k0 = a.cv_kind[a.mcv0], k1 = a.cv_kind[a.mcv1];
    const double s0 = sh_s[a.mcv0], s1 = sh_s[a.mcv1];
    for (int64_t h = t; h < nvis; h += kThreads) tn_bias::hill_term(a.dm, k0, k1, s0, s1, c0[h], c1[h], a.is0, a.is1, hw[h], &V, &d0, &d1);
    V = wave_sum_f64(V);
    d0 = wave_sum_f64(d0);
    d1 = wave_sum_f64(d1);
    if ((t & 63) == 0) {
      sh_red[t >> 6][0] = V;
      sh_red[t >> 6][1] = d0;
      sh_red[t >> 6][2] = d1;
    }
    __syncthreads();
    V = ((sh_red[0][0] + sh_red[1][0]) + sh_red[2][0]) + sh_red[3][0];
    d0 = ((sh_red[0][1] + sh_red[1][1]) + sh_red[2][1]) + sh_red[3][1];
    d1 = ((sh_red[0][2] + sh_red[1][2]) + sh_red[2][2]) + sh_red[3][2];
    if (t == 0 && !(isfinite(V) && isfinite(d0) && isfinite(d1))) sh_bad = 1;
  }
  if (t < a.D) {
    double tot = sh_dv[t];
    if (a.dm > 0 && t == a.mcv0) tot = tot + d0;
    if (a.dm == 2 && t == a.mcv1) tot = tot + d1;
    sh_tot[t] = tot;
  }
  __syncthreads();
  float f[3] = {0.f, 0.f, 0.f};
  int64_t i = -1;
  if (t < a.A) {
    int e0 = a.offsets[t], e1 = a.offsets[t + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > tn_bias::kMaxAtoms ? tn_bias::kMaxAtoms : e1;
    tn_bias::atom_force(a.entries, e0, e1, sh_tot, sh_grad, f);
    i = start + a.atom_rel[t];
    if (!(isfinite(f[0]) && isfinite(f[1]) && isfinite(f[2])) || i < 0 || i >= a.N) sh_bad = 1;
  }
  __syncthreads();
  if (sh_bad) {
    if (t == 0) a.st.head[2] = tn_bias::kStatusBias;
    return;
  }
  if (t < a.A) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a.forces[i * 3 + d] = tn_md::md_add(a.forces[i * 3 + d], f[d]);
      if (a.force_row) a.force_row[((int64_t)b * a.A + t) * 3 + d] = f[d];
    }
  }
  if (t < a.D && a.cv_row) a.cv_row[(int64_t)b * a.D + t] = sh_s[t];
  if (t == 0) {
    double er = 0.0;
    for (int c = 0; c < a.D; ++c) er = er + sh_er[c];
    if (a.res_row) a.res_row[b] = er;
    if (a.bias_row) a.bias_row[b] = V;
    if (a.dm > 0 && a.deposit) {
      const int g = b / a.W, w = b - g * a.W;
      const int64_t slot = tn_bias::hill_slot(n, a.head[0], a.pace, a.W, w, a.head[1], a.H);
      if (slot >= 0) {
        double* c0 = a.hills + (int64_t)g * (a.dm + 1) * a.H;
        c0[slot] = sh_s[a.mcv0];
        if (a.dm == 2) c0[a.H + slot] = sh_s[a.mcv1];
        c0[(int64_t)a.dm * a.H + slot] = tn_bias::hill_height(a.h0, V, a.kT, a.gamma);
      }
    }
  }
}

__global__ void k_md_bias_reset(uint64_t* head, uint64_t step0, uint64_t hill_base) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    head[0] = step0;
    head[1] = hill_base;
  }
}

inline bool bias_layout_ok(int64_t n_mol, int32_t n_cv, int32_t dm, int32_t W, int64_t H) {
  if (n_mol < 1 || n_mol > INT32_MAX / 16 || n_cv < 1 || n_cv > tn_bias::kMaxCv || dm < 0 || dm > 2 || dm > n_cv) return false;
  if (W < 1 || n_mol % W != 0) return false;
  if (dm > 0 && (H < W || H > (int64_t)1 << 40)) return false;
  return dm > 0 || H >= 0;
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_md_bias_workspace_bytes(int64_t n_mol, int32_t n_cv, int32_t n_metad_cv, int32_t walkers_per_group, int64_t capacity,
                                   size_t* bytes) {
  if (!bytes || !bias_layout_ok(n_mol, n_cv, n_metad_cv, walkers_per_group, capacity)) return TMDNET_ERR_INVALID;
  *bytes = layout_bytes([&](LoopCarver& c) { bias_layout(c, n_mol / walkers_per_group, n_metad_cv, capacity); });
  return TMDNET_OK;
}

int tmdnet_md_bias_reset(void* stream, void* bias_ws, uint64_t step0, uint64_t hill_base) {
  if (!bias_ws) return TMDNET_ERR_INVALID;
  LoopCarver c(bias_ws);
  hipLaunchKernelGGL(k_md_bias_reset, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), bias_layout(c, 0, 0, 0).head, step0,
                     hill_base);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_md_bias(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* bias_ws, int64_t n_atoms, int64_t n_mol,
                   int32_t deposit, const float* pos, float* forces, int32_t n_cv, const int32_t* cv_kind, const int32_t* cv_atoms,
                   const int32_t* mol_start, int32_t n_distinct, const int32_t* atom_rel, const int32_t* entry_offsets,
                   const int32_t* entries, const int32_t* restraint_kind, const double* kappa, const double* center,
                   int32_t n_metad_cv, int32_t metad_cv0, int32_t metad_cv1, double sigma0, double sigma1, double height, double kT,
                   double bias_factor, int64_t pace, int32_t walkers_per_group, int64_t capacity, double* cv_log_row,
                   double* restraint_log_row, double* bias_log_row, float* force_log_row) {
  if (!md_ws || !bias_ws || !pos || !forces || !cv_kind || !cv_atoms || !mol_start || !atom_rel || !entry_offsets || !entries ||
      !restraint_kind || !kappa || !center)
    return TMDNET_ERR_INVALID;
  if (n_atoms < 1 || n_atoms > INT32_MAX / 4) return TMDNET_ERR_INVALID;
  if (!bias_layout_ok(n_mol, n_cv, n_metad_cv, walkers_per_group, capacity)) return TMDNET_ERR_INVALID;
  if (n_distinct < 1 || n_distinct > tn_bias::kMaxAtoms) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  const int dm = n_metad_cv;
  if (dm > 0) {
    if (metad_cv0 < 0 || metad_cv0 >= n_cv || !(sigma0 > 0.0) || pace < 1 || !(height >= 0.0)) return TMDNET_ERR_INVALID;
    if (dm == 2 && (metad_cv1 < 0 || metad_cv1 >= n_cv || metad_cv1 == metad_cv0 || !(sigma1 > 0.0))) return TMDNET_ERR_INVALID;
    if (bias_factor != 0.0 && (!(bias_factor > 1.0) || !(kT > 0.0))) return TMDNET_ERR_INVALID;  // 0: plain metadynamics
  }
  BiasArgs a;
  a.N = (int)n_atoms;
  a.B = (int)n_mol;
  a.D = n_cv;
  a.A = n_distinct;
  a.W = walkers_per_group;
  a.dm = dm;
  a.mcv0 = dm > 0 ? metad_cv0 : 0;
  a.mcv1 = dm == 2 ? metad_cv1 : a.mcv0;
  a.deposit = deposit;
  a.pos = pos;
  a.forces = forces;
  a.cv_kind = cv_kind;
  a.cv_atoms = cv_atoms;
  a.mol_start = mol_start;
  a.atom_rel = atom_rel;
  a.offsets = entry_offsets;
  a.entries = entries;
  a.res_kind = restraint_kind;
  a.kappa = kappa;
  a.center = center;
  a.is0 = dm > 0 ? 1.0 / (sigma0 * sigma0) : 0.0;
  a.is1 = dm == 2 ? 1.0 / (sigma1 * sigma1) : 0.0;
  a.h0 = height;
  a.kT = kT;
  a.gamma = bias_factor;
  a.pace = dm > 0 ? (uint64_t)pace : 1u;
  a.H = capacity;
  LoopCarver c(bias_ws);
  const BiasWs w = bias_layout(c, n_mol / walkers_per_group, dm, capacity);
  a.head = w.head;
  a.hills = w.hills;
  a.cv_row = cv_log_row;
  a.res_row = restraint_log_row;
  a.bias_row = bias_log_row;
  a.force_row = force_log_row;
  a.counts = loop_graph(m, graph_ws, n_atoms, n_mol).counts;
  a.st = carve_md(md_ws, n_atoms, n_mol);
  hipLaunchKernelGGL(k_md_bias, dim3(a.B), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
  return loop_launch_result(m, "tmdnet_md_bias");
}

}  // extern "C"
