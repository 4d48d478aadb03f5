// The observer of the device-resident MD loop: sample frames, the pair-distance histogram g(r), the mean-square displacement and
// the velocity autocorrelation, recorded inside the captured graph.  It sits where the bias launch of tn_bias.hip sits - after the
// evaluation of a step, before the integrator launch that closes it - reads pos (x at the full step s = counter + 1), vel (the
// leapfrog velocity v(s - 1/2) the opening half stored) and the caller's static tables, and writes only into its own workspace: it
// cannot change a bit of the trajectory.  The arithmetic is tn_observe_math.h.
//
// The caller enqueues tmdnet_md_observe only at the sampling positions of a replay, so a step that is no sample costs nothing; the
// sample index j is computed from the loop's 64-bit step counter and the s0 in the workspace header.  No kernel counts samples:
// there is no last-block logic, and the only atomics are the integer adds of the histogram.
//
// At most three launches:
//   k_obs_atoms  one thread per atom: the frame slot j % F (positions, optionally velocities) and the velocity-ring slot j % L.
//   k_obs_rdf    one block of 256 threads per tile triple (molecule, i tile, j tile >= i tile) of the caller's table.  The j tile is
//                staged into LDS, 16 B per atom (position and selector mask); each thread holds one i atom and walks the tile
//                (every lane reads the same LDS address: a broadcast).  A pair's squared distance is tn_common.h's pair_geometry
//                with that molecule's box; the bin is tn_obs::rdf_bin.  Counts go into an LDS histogram of u32 (a tile pair adds at
//                most 65 536) and, after a barrier, the non-zero bins into the global u64 counts.  Integer adds commute: repeats
//                and different steps_per_replay give identical counts.
//   k_obs_mol    grid (B, 1 + L), after k_obs_atoms: block (m, 0) the MSD row of molecule m's groups, block (m, 1 + l) lag l of
//                the VACF from the ring.  fp64 sums, a thread strides by 256, then tn_loop.h's fixed-order block reduction; one
//                thread stores or accumulates.  No floating-point atomics.
//
// Frozen state: every kernel returns at once when the MD status word is set or this step's evaluation overflowed (counts[2]), as
// k_md_bias does: a frozen loop records nothing more.
#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_md_state.h"
#include "tn_model.h"
#include "tn_observe_math.h"

namespace tn {

namespace {

struct ObsWs {  // views into the caller's observer workspace
  uint64_t* head;       // [0] s0
  float* frame_pos;     // [F, N, 3]
  float* frame_vel;     // [F, N, 3] (frame_velocities only)
  uint64_t* counts;     // [B, P, bins]
  float* origin;        // [N, 3] positions at s0 (MSD only)
  double* msd;          // [T, B, Gm]
  float* ring;          // [L, N, 3]
  double* acc;          // [B, Gv, L]
};

inline ObsWs obs_layout(LoopCarver& c, int64_t N, int64_t B, const tmdnet_md_observe_spec& s) {
  const size_t n3 = (size_t)(N > 0 ? N : 0) * 3, b = (size_t)(B > 0 ? B : 0);
  ObsWs w;
  w.head = c.take<uint64_t>(kHeaderBytes / sizeof(uint64_t));
  w.frame_pos = c.take<float>((size_t)s.frame_capacity * n3);
  w.frame_vel = c.take<float>(s.frame_velocities ? (size_t)s.frame_capacity * n3 : 0);
  if (!s.frame_velocities) w.frame_vel = nullptr;  // (an array of no elements still has an address: the next array's)
  w.counts = c.take<uint64_t>(b * (size_t)s.n_pair_types * (size_t)s.bins);
  w.origin = c.take<float>(s.n_msd_groups > 0 ? n3 : 0);
  if (s.n_msd_groups == 0) w.origin = nullptr;
  w.msd = c.take<double>((size_t)s.msd_capacity * b * (size_t)s.n_msd_groups);
  w.ring = c.take<float>(s.n_vacf_groups > 0 ? (size_t)s.lags * n3 : 0);
  w.acc = c.take<double>(b * (size_t)s.n_vacf_groups * (size_t)s.lags);
  return w;
}

inline bool obs_spec_ok(int64_t N, int64_t B, const tmdnet_md_observe_spec* s) {
  if (!s || N < 1 || N > INT32_MAX / 4 || B < 1 || B > INT32_MAX / 16 || s->every < 1) return false;
  if (s->frame_capacity < 0 || s->frame_capacity > (1 << 24)) return false;
  if (s->n_pair_types < 0 || s->n_pair_types > tn_obs::kMaxTypes) return false;
  if (s->n_pair_types > 0 && (s->bins < 1 || s->bins > tn_obs::kMaxBins || !(s->r_max2 > 0.f) || !(s->inv_dr > 0.f))) return false;
  if (s->n_msd_groups < 0 || s->n_msd_groups > tn_obs::kMaxTypes) return false;
  if (s->n_msd_groups > 0 && (s->msd_capacity < 1 || s->msd_capacity > (int64_t)1 << 32)) return false;
  if (s->n_vacf_groups < 0 || s->n_vacf_groups > tn_obs::kMaxTypes) return false;
  if (s->n_vacf_groups > 0 && (s->lags < 1 || s->lags > tn_obs::kMaxLags)) return false;
  return s->frame_capacity > 0 || s->n_pair_types > 0 || s->n_msd_groups > 0 || s->n_vacf_groups > 0;
}

// the spec with the sizes of the observables that are off set to zero, so that the layout does not depend on what they hold
inline tmdnet_md_observe_spec obs_clean(const tmdnet_md_observe_spec& in) {
  tmdnet_md_observe_spec s = in;
  if (s.frame_capacity == 0) s.frame_velocities = 0;
  if (s.n_pair_types == 0) s.bins = 0;
  if (s.n_msd_groups == 0) s.msd_capacity = 0;
  if (s.n_vacf_groups == 0) s.lags = 0;
  return s;
}

struct ObsArgs {
  int N, B, S, F, P, bins, Gm, Gv, L, box_mode;
  int64_t T, n_tiles;
  float r_max2, inv_dr;
  const float* pos;
  const float* vel;
  const float* box;
  const int64_t* batch;
  const int32_t* mol_start;  // [B + 1]
  const uint32_t* mask;      // [N]
  const int32_t* tiles;      // [n_tiles, 3]
  const int* counts;
  const int* mstart;
  const int* mend;
  ObsWs w;
  MdState st;
};

// the sample this launch records, or -1: frozen, or (never, for a caller that enqueues at the sampling positions) no sample
__device__ __forceinline__ int64_t obs_sample(const ObsArgs& a) {
  if (a.st.head[2] != 0u || (a.counts && a.counts[2])) return -1;
  return tn_obs::sample_index(loop_step(a.st.head) + 1u, a.w.head[0], (uint64_t)a.S);
}

__global__ __launch_bounds__(kThreads) void k_obs_atoms(ObsArgs a) {
  const int64_t j = obs_sample(a);
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (j < 0 || i >= a.N) return;
  const size_t n3 = (size_t)a.N * 3;
  float x[3], v[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    x[d] = a.pos[(size_t)i * 3 + d];
    v[d] = a.vel[(size_t)i * 3 + d];
  }
  if (a.F > 0) {
    const size_t row = (size_t)tn_obs::ring_slot(j, a.F) * n3 + (size_t)i * 3;
#pragma unroll
    for (int d = 0; d < 3; ++d) a.w.frame_pos[row + d] = x[d];
    if (a.w.frame_vel)
#pragma unroll
      for (int d = 0; d < 3; ++d) a.w.frame_vel[row + d] = v[d];
  }
  if (a.Gv > 0) {
    const size_t row = (size_t)tn_obs::ring_slot(j, a.L) * n3 + (size_t)i * 3;
#pragma unroll
    for (int d = 0; d < 3; ++d) a.w.ring[row + d] = v[d];
  }
}

__global__ __launch_bounds__(kThreads) void k_obs_rdf(ObsArgs a) {
  __shared__ float4 sh_j[tn_obs::kTile];
  __shared__ uint32_t sh_hist[tn_obs::kMaxTypes * tn_obs::kMaxBins];
  if (obs_sample(a) < 0) return;  // (the same words for every thread of the launch, and no launch of the observer writes them)
  const int t = threadIdx.x;
  const int32_t* tr = a.tiles + (int64_t)blockIdx.x * 3;
  const int m = tr[0], it = tr[1], jt = tr[2];
  if (m < 0 || m >= a.B || it < 0 || jt < it) return;  // a row the caller's table should not hold: nothing is read through it
  int a0 = a.mol_start[m], a1 = a.mol_start[m + 1];
  a0 = a0 < 0 ? 0 : a0;
  a1 = a1 > a.N ? a.N : a1;
  const int64_t ib = (int64_t)a0 + (int64_t)it * tn_obs::kTile, jb = (int64_t)a0 + (int64_t)jt * tn_obs::kTile;
  if (jb >= a1) return;
  const int nj = (int)(a1 - jb < tn_obs::kTile ? a1 - jb : tn_obs::kTile);
  const int nh = a.P * a.bins;
  if (t < nj) {
    const int64_t g = jb + t;
    sh_j[t] = make_float4(a.pos[g * 3 + 0], a.pos[g * 3 + 1], a.pos[g * 3 + 2], __uint_as_float(a.mask[g] & tn_obs::kPairBits));
  }
  for (int k = t; k < nh; k += kThreads) sh_hist[k] = 0u;
  __syncthreads();
  const int64_t i = ib + t;
  const uint32_t mi = i < a1 ? a.mask[i] & tn_obs::kPairBits : 0u;
  if (mi) {
    float bx[9];
    const float* src = a.box ? a.box + (a.box_mode == 2 ? (int64_t)m * 9 : 0) : nullptr;
#pragma unroll
    for (int d = 0; d < 9; ++d) bx[d] = src ? src[d] : 0.f;
    float p[6];
#pragma unroll
    for (int d = 0; d < 3; ++d) p[3 + d] = a.pos[i * 3 + d];
    const bool diag = it == jt;
    for (int jj = 0; jj < nj; ++jj) {
      const float4 q = sh_j[jj];
      const uint32_t ty = tn_obs::pair_types(mi, __float_as_uint(q.w));
      if (!ty || (diag && jj <= t)) continue;
      p[0] = q.x;
      p[1] = q.y;
      p[2] = q.z;
      float dx, dy, dz;
      // hi = the j atom (the larger caller index: j > i in a diagonal tile, and jt > it otherwise), lo = the i atom
      const float d2 = pair_geometry(p, 0, 1, src ? bx : nullptr, dx, dy, dz);
      const int bin = tn_obs::rdf_bin(d2, a.r_max2, a.inv_dr, a.bins);
      if (bin < 0) continue;
#pragma unroll
      for (int ty_p = 0; ty_p < tn_obs::kMaxTypes; ++ty_p)
        if (ty_p < a.P && ((ty >> (2 * ty_p)) & 1u)) atomicAdd(&sh_hist[ty_p * a.bins + bin], 1u);
    }
  }
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(a.w.counts) + (size_t)m * (size_t)nh;
  for (int k = t; k < nh; k += kThreads) {
    const uint32_t c = sh_hist[k];
    if (c) atomicAdd(out + k, (unsigned long long)c);
  }
}

__global__ __launch_bounds__(kThreads) void k_obs_mol(ObsArgs a) {
  __shared__ double sh[tn_obs::kMaxTypes][kThreads / 64];
  const int64_t j = obs_sample(a);
  if (j < 0) return;
  const int m = blockIdx.x, y = blockIdx.y, t = threadIdx.x;
  const SliceRange r = mol_slice_range(a.counts, a.mstart, a.mend, a.N, 1, a.batch, m, 0);
  const size_t n3 = (size_t)a.N * 3;
  double acc[tn_obs::kMaxTypes] = {0.0, 0.0, 0.0, 0.0};
  if (y == 0) {  // MSD
    if (a.Gm == 0 || j >= a.T) return;
    for (int i = r.i0 + t; i < r.i1; i += kThreads) {
      if (slice_skips(r, a.batch, i, m)) continue;
      const uint32_t g = (a.mask[i] >> tn_obs::kMsdShift) & 0xfu;
      if (!g) continue;
      double d2 = 0.0;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const double e = (double)a.pos[(size_t)i * 3 + d] - (double)a.w.origin[(size_t)i * 3 + d];
        d2 += e * e;
      }
#pragma unroll
      for (int k = 0; k < tn_obs::kMaxTypes; ++k) acc[k] += ((g >> k) & 1u) ? d2 : 0.0;
    }
  } else {  // lag l of the VACF
    const int l = y - 1;
    if (a.Gv == 0 || l >= a.L || (int64_t)l > j) return;
    const float* now = a.w.ring + (size_t)tn_obs::ring_slot(j, a.L) * n3;
    const float* then = a.w.ring + (size_t)tn_obs::ring_slot(j - l, a.L) * n3;
    for (int i = r.i0 + t; i < r.i1; i += kThreads) {
      if (slice_skips(r, a.batch, i, m)) continue;
      const uint32_t g = (a.mask[i] >> tn_obs::kVacfShift) & 0xfu;
      if (!g) continue;
      double dot = 0.0;
#pragma unroll
      for (int d = 0; d < 3; ++d) dot += (double)now[(size_t)i * 3 + d] * (double)then[(size_t)i * 3 + d];
#pragma unroll
      for (int k = 0; k < tn_obs::kMaxTypes; ++k) acc[k] += ((g >> k) & 1u) ? dot : 0.0;
    }
  }
  block_reduce_waves<tn_obs::kMaxTypes, 0u>(acc, sh);
  if (t != 0) return;
  double out[tn_obs::kMaxTypes];
  block_reduce_rows<tn_obs::kMaxTypes, 0u>(sh, out);
  if (y == 0) {
    for (int k = 0; k < a.Gm; ++k) a.w.msd[((size_t)j * a.B + m) * a.Gm + k] = out[k];
  } else {
    for (int k = 0; k < a.Gv; ++k) a.w.acc[((size_t)m * a.Gv + k) * a.L + (y - 1)] += out[k];
  }
}

__global__ void k_obs_start(ObsWs w, uint64_t s0, const float* __restrict__ pos, int64_t n3) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) w.head[0] = s0;
  if (w.origin && i < n3) w.origin[i] = pos[i];
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_md_observe_workspace_bytes(int64_t n_atoms, int64_t n_mol, const tmdnet_md_observe_spec* spec, size_t* bytes) {
  if (!bytes || !obs_spec_ok(n_atoms, n_mol, spec)) return TMDNET_ERR_INVALID;
  const tmdnet_md_observe_spec s = obs_clean(*spec);
  *bytes = layout_bytes([&](LoopCarver& c) { obs_layout(c, n_atoms, n_mol, s); });
  return TMDNET_OK;
}

int tmdnet_md_observe_start(void* stream, void* obs_ws, int64_t n_atoms, int64_t n_mol, const tmdnet_md_observe_spec* spec, uint64_t s0,
                            const float* pos) {
  if (!obs_ws || !obs_spec_ok(n_atoms, n_mol, spec)) return TMDNET_ERR_INVALID;
  const tmdnet_md_observe_spec s = obs_clean(*spec);
  if (s.n_msd_groups > 0 && !pos) return TMDNET_ERR_INVALID;
  LoopCarver c(obs_ws);
  const ObsWs w = obs_layout(c, n_atoms, n_mol, s);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(w.head, 0, c.bytes(), st) != hipSuccess) return TMDNET_ERR_HIP;
  const int64_t n3 = n_atoms * 3;
  const int64_t blocks = w.origin ? (n3 + kThreads - 1) / kThreads : 1;
  hipLaunchKernelGGL(k_obs_start, dim3((unsigned)blocks), dim3(kThreads), 0, st, w, s0, pos, n3);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_md_observe(tmdnet_model* m, void* stream, void* graph_ws, void* md_ws, void* obs_ws, int64_t n_atoms, int64_t n_mol,
                      const tmdnet_md_observe_spec* spec, const float* pos, const float* vel, const int64_t* batch, const float* box,
                      int32_t box_mode, const uint32_t* atom_mask, const int32_t* mol_start, const int32_t* tiles, int64_t n_tiles) {
  if (!md_ws || !obs_ws || !pos || !vel || !atom_mask || !obs_spec_ok(n_atoms, n_mol, spec)) return TMDNET_ERR_INVALID;
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (n_mol > 1 && !batch) return TMDNET_ERR_INVALID;
  if (box ? (box_mode != 1 && box_mode != 2) : box_mode != 0) return TMDNET_ERR_INVALID;
  const tmdnet_md_observe_spec s = obs_clean(*spec);
  if (s.n_pair_types > 0 && (!mol_start || n_tiles < 0 || n_tiles > INT32_MAX || (n_tiles > 0 && !tiles))) return TMDNET_ERR_INVALID;
  ObsArgs a;
  a.N = (int)n_atoms;
  a.B = (int)n_mol;
  a.S = s.every;
  a.F = s.frame_capacity;
  a.P = s.n_pair_types;
  a.bins = s.bins;
  a.Gm = s.n_msd_groups;
  a.Gv = s.n_vacf_groups;
  a.L = s.lags;
  a.box_mode = box_mode;
  a.T = s.msd_capacity;
  a.n_tiles = n_tiles;
  a.r_max2 = s.r_max2;
  a.inv_dr = s.inv_dr;
  a.pos = pos;
  a.vel = vel;
  a.box = box;
  a.batch = batch;
  a.mol_start = mol_start;
  a.mask = atom_mask;
  a.tiles = tiles;
  const LoopGraph g = loop_graph(m, graph_ws, n_atoms, n_mol);
  a.counts = g.counts;
  a.mstart = g.mstart;
  a.mend = g.mend;
  LoopCarver c(obs_ws);
  a.w = obs_layout(c, n_atoms, n_mol, s);
  a.st = carve_md(md_ws, n_atoms, n_mol);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (a.F > 0 || a.Gv > 0)
    hipLaunchKernelGGL(k_obs_atoms, dim3((unsigned)((a.N + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a);
  if (a.P > 0 && n_tiles > 0) hipLaunchKernelGGL(k_obs_rdf, dim3((unsigned)n_tiles), dim3(kThreads), 0, st, a);
  if (a.Gm > 0 || a.Gv > 0) hipLaunchKernelGGL(k_obs_mol, dim3((unsigned)a.B, (unsigned)(1 + a.L)), dim3(kThreads), 0, st, a);
  return loop_launch_result(m, "tmdnet_md_observe");
}

}  // extern "C"
