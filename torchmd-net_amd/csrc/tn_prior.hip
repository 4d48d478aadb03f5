// Pair priors behind the engine call: ZBL and D2 (tn_prior_math.h) evaluated by brute force inside every molecule and ADDED to the
// energies, forces and virial the model's pass has written.  Row-owner scheme, no floating-point atomics, every sum in a fixed
// order: repeats are bit-identical.  Three launches on the caller's stream, no read-back, no synchronisation (capturable):
//
//   k_prior_ranges    per molecule [lo, hi), the smallest and one past the largest atom index with that batch id (integer atomicMax
//                     on two counters per molecule that the previous pass left at zero).  A sorted batch gives the tight range, an
//                     unsorted one a wider range that is still correct: the pair kernel tests batch[j] == batch[i] anyway.
//   k_prior_pairs     one wave owns atom i; the block (4 waves, 4 atoms) stages tiles of 256 j atoms into LDS as two float4 per atom
//                     (x, y, z, batch id | Z, Z^0.23, sqrt C6, Rr: 32 B, read with two conflict-free 16-byte reads per lane) over
//                     the union of its atoms' ranges, and every wave walks the tile, 64 pairs per step.  A lane evaluates both
//                     active priors from one pair vector (ZBL after the minimum image of the engine's neighbour search,
//                     tn_common.h pair_geometry; D2 never sees the box), each against its own cutoff, in fp32, and accumulates
//                     f_i, e_i = 1/2 sum_j u_ij and the six components of w_i = -1/2 sum_j (u'_ij / r) r_ij (x) r_ij in fp64.  The
//                     wave reduces with a butterfly (xor 32 .. 1); lane 0 rounds once, adds to forces[i], and writes e_i, w_i to
//                     the atom's scratch row (8 doubles).
//   k_prior_mol_sum   one wave per molecule sums the rows of its atoms over [lo, hi) (lane l takes lo + l, lo + l + 64, ...; then the
//                     butterfly), in fp64, rounds once, adds to energy[m] and virial[m], and puts the two range counters back to zero.
//
// Workspace: [2 n_mol int32 counters | n_atoms rows of 8 doubles].  The counters must be zero on entry - the caller zeroes the
// workspace once, and again whenever n_atoms or n_mol differ from the previous pass on it; every pass leaves them zero.  A counter
// that is not (a caller's mistake) is clamped to the atom count: wrong sums, no access out of bounds.
#include <string>

#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_model.h"
#include "tn_prior_math.h"

namespace tn {

namespace {

constexpr int kPriorThreads = 256, kPriorWaves = kPriorThreads / TN_WAVE, kPriorTile = 256, kPriorRow = 8;

struct PriorArgs {
  int N, B, flags, max_z, box_mode;
  tn_prior::ZblConst zbl;
  tn_prior::D2Const d2;
  const float* tab;  // [4][max_z]: Z, Z^0.23, sqrt C6, Rr
  const float* pos;
  const int64_t* z;
  const int64_t* batch;
  const float* box;
  int* rng;      // [B][2] counters: N - lo, hi
  double* rows;  // [N][kPriorRow]: e_i, w_xx, w_xy, w_xz, w_yy, w_yz, w_zz, 0
  float* energy;
  float* forces;
  float* virial;
};

__host__ __device__ inline size_t prior_rows_offset(int64_t B) { return (((size_t)B * 2 * sizeof(int)) + 255) & ~(size_t)255; }

__device__ __forceinline__ void prior_range(const int* __restrict__ rng, int m, int N, int& lo, int& hi) {
  const int a = rng[2 * m], h = rng[2 * m + 1];
  lo = N - min(max(a, 0), N);
  hi = min(max(h, 0), N);
}

__device__ __forceinline__ double wave_sum_f64(double v) {  // fixed order: xor 32, 16, 8, 4, 2, 1; the total in every lane
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_prior_ranges(int N, int B, const int64_t* __restrict__ batch, int* __restrict__ rng) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int64_t b = batch[i];
  if (b < 0 || b >= B) return;
  // only the ends of a run of equal ids can be a molecule's first or last atom
  if (i == 0 || batch[i - 1] != b) atomicMax(&rng[2 * b], N - i);
  if (i == N - 1 || batch[i + 1] != b) atomicMax(&rng[2 * b + 1], i + 1);
}

__global__ __launch_bounds__(256) void k_prior_pairs(PriorArgs a) {
  // one instantiation: the virial is a wave-uniform branch, so E and F have the same bits with and without it
  const bool vir = a.virial != nullptr;
  __shared__ float4 sA[kPriorTile], sB[kPriorTile];
  __shared__ int s_lo[kPriorWaves], s_hi[kPriorWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * kPriorWaves + wave;
  const int N = a.N;
  int bi = -1, lo = 0, hi = 0;
  if (i < N) {
    const int64_t b = a.batch[i];
    if (b >= 0 && b < a.B) {
      bi = (int)b;
      prior_range(a.rng, bi, N, lo, hi);
    }
  }
  if (lane == 0) {
    s_lo[wave] = hi > lo ? lo : N;
    s_hi[wave] = hi > lo ? hi : 0;
  }
  float xi = 0.f, yi = 0.f, zi = 0.f, Zi = 0.f, z23i = 0.f, c6i = 0.f, rri = 0.f;
  if (bi >= 0) {
    xi = a.pos[i * 3 + 0];
    yi = a.pos[i * 3 + 1];
    zi = a.pos[i * 3 + 2];
    const int64_t s = a.z[i];
    const bool known = s >= 0 && s < a.max_z;  // a species outside the tables poisons its atom's sums instead of reading past them
    Zi = known ? a.tab[s] : NAN;
    z23i = known ? a.tab[a.max_z + s] : NAN;
    c6i = known ? a.tab[2 * a.max_z + s] : NAN;
    rri = known ? a.tab[3 * a.max_z + s] : NAN;
  }
  float bx[9];
  const bool pbc = a.box && a.box_mode && bi >= 0;
  if (pbc) {
    const float* bp = a.box + (a.box_mode == 2 ? (size_t)bi * 9 : 0);
#pragma unroll
    for (int k = 0; k < 9; ++k) bx[k] = bp[k];
  }
  __syncthreads();
  int jlo = s_lo[0], jhi = s_hi[0];
#pragma unroll
  for (int w = 1; w < kPriorWaves; ++w) {
    jlo = min(jlo, s_lo[w]);
    jhi = max(jhi, s_hi[w]);
  }
  const bool zbl_on = a.flags & TMDNET_PRIOR_ZBL, d2_on = a.flags & TMDNET_PRIOR_D2;
  double fx = 0.0, fy = 0.0, fz = 0.0, e = 0.0, wxx = 0.0, wxy = 0.0, wxz = 0.0, wyy = 0.0, wyz = 0.0, wzz = 0.0;
  for (int t0 = jlo; t0 < jhi; t0 += kPriorTile) {  // block-uniform bounds: every wave reaches every barrier
    __syncthreads();
    {
      const int j = t0 + threadIdx.x;
      float4 pa = make_float4(0.f, 0.f, 0.f, __int_as_float(-2)), pb = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < jhi) {
        const int64_t b = a.batch[j], s = a.z[j];
        const bool known = s >= 0 && s < a.max_z;
        pa = make_float4(a.pos[j * 3 + 0], a.pos[j * 3 + 1], a.pos[j * 3 + 2], __int_as_float(b >= 0 && b < a.B ? (int)b : -2));
        pb = make_float4(known ? a.tab[s] : NAN, known ? a.tab[a.max_z + s] : NAN, known ? a.tab[2 * a.max_z + s] : NAN,
                         known ? a.tab[3 * a.max_z + s] : NAN);
      }
      sA[threadIdx.x] = pa;
      sB[threadIdx.x] = pb;
    }
    __syncthreads();
    if (bi < 0 || t0 + kPriorTile <= lo || t0 >= hi) continue;  // nothing of this atom's molecule in the tile (wave-uniform)
#pragma unroll
    for (int k = lane; k < kPriorTile; k += TN_WAVE) {
      const int j = t0 + k;
      const float4 pa = sA[k];
      if (__float_as_int(pa.w) != bi || j == i) continue;
      const float4 pb = sB[k];
      // pair vector r_ij = pos_i - pos_j; the minimum image is taken on pos[hi] - pos[lo] as the neighbour search takes it
      const float sg = i > j ? 1.0f : -1.0f;
      float dx, dy, dz, qx, qy, qz;
      {
#pragma clang fp contract(off)
        dx = sg * (xi - pa.x);
        dy = sg * (yi - pa.y);
        dz = sg * (zi - pa.z);
        qx = dx, qy = dy, qz = dz;  // the raw vector: D2 takes no image
        if (pbc) {
          const float s3 = -roundf(dz / bx[8]);
          dx = __builtin_fmaf(s3, bx[6], dx);
          dy = __builtin_fmaf(s3, bx[7], dy);
          dz = __builtin_fmaf(s3, bx[8], dz);
          const float s2 = -roundf(dy / bx[4]);
          dx = __builtin_fmaf(s2, bx[3], dx);
          dy = __builtin_fmaf(s2, bx[4], dy);
          const float s1 = -roundf(dx / bx[0]);
          dx = __builtin_fmaf(s1, bx[0], dx);
        }
      }
      if (zbl_on) {
        const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
        if (tn_prior::in_cutoff(d2, a.zbl.cutoff)) {
          const float r = sqrtf(d2);
          float u, du;
          tn_prior::zbl_pair(r, z23i + pb.y, Zi * pb.x, a.zbl, &u, &du);
          const float g = sg * du / r;  // d u / d r_ij = g * (dx, dy, dz) / sg^2
          const float gx = g * dx, gy = g * dy, gz = g * dz;
          e += (double)(0.5f * u);
          fx -= (double)gx;
          fy -= (double)gy;
          fz -= (double)gz;
          if (vir) {
            const float hx = -0.5f * sg * gx, hy = -0.5f * sg * gy, hz = -0.5f * sg * gz;
            wxx += (double)(hx * dx);
            wxy += (double)(hx * dy);
            wxz += (double)(hx * dz);
            wyy += (double)(hy * dy);
            wyz += (double)(hy * dz);
            wzz += (double)(hz * dz);
          }
        }
      }
      if (d2_on) {
        const float d2 = __builtin_fmaf(qz, qz, __builtin_fmaf(qy, qy, qx * qx));
        if (tn_prior::in_cutoff(d2, a.d2.cutoff)) {
          const float r = sqrtf(d2);
          float u, du;
          tn_prior::d2_pair(r, c6i * pb.z, rri + pb.w, a.d2, &u, &du);
          const float g = sg * du / r;
          const float gx = g * qx, gy = g * qy, gz = g * qz;
          e += (double)(0.5f * u);
          fx -= (double)gx;
          fy -= (double)gy;
          fz -= (double)gz;
          if (vir) {
            const float hx = -0.5f * sg * gx, hy = -0.5f * sg * gy, hz = -0.5f * sg * gz;
            wxx += (double)(hx * qx);
            wxy += (double)(hx * qy);
            wxz += (double)(hx * qz);
            wyy += (double)(hy * qy);
            wyz += (double)(hy * qz);
            wzz += (double)(hz * qz);
          }
        }
      }
    }
  }
  if (i >= N) return;  // (after the last barrier)
  e = wave_sum_f64(e);
  fx = wave_sum_f64(fx);
  fy = wave_sum_f64(fy);
  fz = wave_sum_f64(fz);
  if (vir) {
    wxx = wave_sum_f64(wxx);
    wxy = wave_sum_f64(wxy);
    wxz = wave_sum_f64(wxz);
    wyy = wave_sum_f64(wyy);
    wyz = wave_sum_f64(wyz);
    wzz = wave_sum_f64(wzz);
  }
  if (lane == 0) {
    if (a.forces && bi >= 0) {
      a.forces[i * 3 + 0] += (float)fx;
      a.forces[i * 3 + 1] += (float)fy;
      a.forces[i * 3 + 2] += (float)fz;
    }
    double* row = a.rows + (size_t)i * kPriorRow;
    row[0] = e;
    row[1] = wxx;
    row[2] = wxy;
    row[3] = wxz;
    row[4] = wyy;
    row[5] = wyz;
    row[6] = wzz;
    row[7] = 0.0;
  }
}

__global__ __launch_bounds__(256) void k_prior_mol_sum(PriorArgs a) {
  const int m = blockIdx.x * kPriorWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= a.B) return;
  int lo, hi;
  prior_range(a.rng, m, a.N, lo, hi);
  double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = lo + lane; i < hi; i += TN_WAVE) {
    if (a.batch[i] != m) continue;
    const double* row = a.rows + (size_t)i * kPriorRow;
#pragma unroll
    for (int c = 0; c < 7; ++c) s[c] += row[c];
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) s[c] = wave_sum_f64(s[c]);
  if (lane == 0) {
    a.energy[m] += (float)s[0];
    if (a.virial) {
      float* W = a.virial + (size_t)m * 9;
      const float xx = (float)s[1], xy = (float)s[2], xz = (float)s[3], yy = (float)s[4], yz = (float)s[5], zz = (float)s[6];
      W[0] += xx, W[1] += xy, W[2] += xz;
      W[3] += xy, W[4] += yy, W[5] += yz;
      W[6] += xz, W[7] += yz, W[8] += zz;
    }
    a.rng[2 * m] = 0;  // every lane has read the counters before the butterfly: the next pass finds them at zero
    a.rng[2 * m + 1] = 0;
  }
}

size_t prior_workspace_bytes(int64_t N, int64_t B) { return prior_rows_offset(B) + (size_t)N * kPriorRow * sizeof(double); }

int prior_check(tmdnet_model* m, void* ws, size_t ws_bytes, int64_t N, int64_t B, const float* pos, const int64_t* z, const int64_t* batch,
                const float* box, int32_t box_mode, const float* atom_weights, float* energy) {
  if (!m) return TMDNET_ERR_INVALID;
  if (!m->prior_flags) return fail(m, TMDNET_ERR_STATE, "no pair priors set (tmdnet_set_pair_priors)");
  if (atom_weights || m->atom_w) return fail(m, TMDNET_ERR_INVALID, "the pair priors are not implemented with atom weights (domain decomposition)");
  if (m->halo_fn) return fail(m, TMDNET_ERR_INVALID, "the pair priors are not implemented with the halo exchange (domain decomposition)");
  if (N < 0 || B < 0 || N > INT32_MAX / 16 || B > INT32_MAX / 16) return fail(m, TMDNET_ERR_INVALID, "pair priors: atom or molecule count out of range");
  if (B > 0 && N > (int64_t)tn_prior::kMaxMoleculeAtoms * B)
    return fail(m, TMDNET_ERR_INVALID, "pair priors: a molecule has more than " + std::to_string(tn_prior::kMaxMoleculeAtoms) +
                                           " atoms; the pass is brute force (a cell list is the follow-up)");
  if (box_mode < 0 || box_mode > 2 || (box_mode && !box)) return fail(m, TMDNET_ERR_INVALID, "pair priors: box_mode must be 0, 1 or 2, with a box for 1 and 2");
  if (N && B && (!ws || !pos || !z || !batch || !energy)) return fail(m, TMDNET_ERR_INVALID, "pair priors: null pointer");
  if (ws_bytes < prior_workspace_bytes(N, B))
    return fail(m, TMDNET_ERR_WORKSPACE, "pair prior workspace too small: need " + std::to_string(prior_workspace_bytes(N, B)));
  return TMDNET_OK;
}

void prior_launch(tmdnet_model* m, hipStream_t s, void* ws, int64_t N, int64_t B, const float* pos, const int64_t* z, const int64_t* batch,
                  const float* box, int32_t box_mode, float* energy, float* forces, float* virial) {
  PriorArgs a;
  a.N = (int)N, a.B = (int)B, a.flags = m->prior_flags, a.max_z = m->prior_max_z, a.box_mode = box ? box_mode : 0;
  a.zbl = m->prior_zbl, a.d2 = m->prior_d2;
  a.tab = m->prior_tab, a.pos = pos, a.z = z, a.batch = batch, a.box = box;
  a.rng = reinterpret_cast<int*>(ws);
  a.rows = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + prior_rows_offset(B));
  a.energy = energy, a.forces = forces, a.virial = virial;
  hipLaunchKernelGGL(k_prior_ranges, dim3((int)((N + 255) / 256)), dim3(256), 0, s, a.N, a.B, batch, a.rng);
  const dim3 grid((int)((N + kPriorWaves - 1) / kPriorWaves));
  hipLaunchKernelGGL(k_prior_pairs, grid, dim3(kPriorThreads), 0, s, a);
  hipLaunchKernelGGL(k_prior_mol_sum, dim3((int)((B + kPriorWaves - 1) / kPriorWaves)), dim3(kPriorThreads), 0, s, a);
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_set_pair_priors(tmdnet_model* m, const tmdnet_pair_priors* p) {
  if (!m) return TMDNET_ERR_INVALID;
  if (!p || !p->flags) {
    m->prior_flags = 0;
    return TMDNET_OK;
  }
  if (p->flags & ~(TMDNET_PRIOR_ZBL | TMDNET_PRIOR_D2)) return fail(m, TMDNET_ERR_INVALID, "tmdnet_set_pair_priors: unknown flag");
  if (p->max_z <= 0) return fail(m, TMDNET_ERR_INVALID, "tmdnet_set_pair_priors: max_z must be positive");
  const bool zbl = p->flags & TMDNET_PRIOR_ZBL, d2 = p->flags & TMDNET_PRIOR_D2;
  if (zbl && (!p->zbl_z || !p->zbl_z23 || !(p->zbl_cutoff > 0.0) || !(p->zbl_distance_scale > 0.0) || !(p->zbl_energy_scale > 0.0)))
    return fail(m, TMDNET_ERR_INVALID, "tmdnet_set_pair_priors: ZBL needs its two tables, a positive cutoff and positive unit scales");
  if (d2 && (!p->d2_sqrt_c6 || !p->d2_rr || !(p->d2_cutoff > 0.0) || !(p->d2_distance_scale > 0.0) || !(p->d2_energy_scale > 0.0)))
    return fail(m, TMDNET_ERR_INVALID, "tmdnet_set_pair_priors: D2 needs its two tables, a positive cutoff and positive unit scales");
  const size_t mz = (size_t)p->max_z;
  std::vector<float> host(4 * mz, 0.0f);
  for (size_t s = 0; s < mz; ++s) {
    if (zbl) host[s] = p->zbl_z[s], host[mz + s] = p->zbl_z23[s];
    if (d2) host[2 * mz + s] = p->d2_sqrt_c6[s], host[3 * mz + s] = p->d2_rr[s];
  }
  m->prior_flags = 0;
  if (m->prior_cap < 4 * mz) {  // (a grown table moves: captured graphs of the old one are stale, as after any re-upload)
    if (m->prior_tab) (void)hipFree(m->prior_tab);
    m->prior_tab = nullptr;
    m->prior_cap = 0;
    HIP_TRY(m, hipMalloc(&m->prior_tab, 4 * mz * sizeof(float)));
    m->prior_cap = 4 * mz;
  }
  HIP_TRY(m, hipMemcpy(m->prior_tab, host.data(), 4 * mz * sizeof(float), hipMemcpyHostToDevice));
  m->prior_max_z = p->max_z;
  if (zbl) m->prior_zbl = tn_prior::zbl_constants(p->zbl_cutoff, p->zbl_distance_scale, p->zbl_energy_scale);
  if (d2) m->prior_d2 = tn_prior::d2_constants(p->d2_cutoff, p->d2_distance_scale, p->d2_energy_scale);
  m->prior_flags = p->flags;
  return TMDNET_OK;
}

int tmdnet_pair_priors_workspace_bytes(const tmdnet_model* m, int64_t n_atoms, int64_t n_mol, size_t* bytes) {
  if (!m || !bytes || n_atoms < 0 || n_mol < 0) return TMDNET_ERR_INVALID;
  *bytes = prior_workspace_bytes(n_atoms, n_mol);
  return TMDNET_OK;
}

int tmdnet_pair_priors_add(tmdnet_model* m, void* stream, void* ws, size_t ws_bytes, int64_t n_atoms, int64_t n_mol, const float* pos,
                           const int64_t* z, const int64_t* batch, const float* box, int32_t box_mode, const float* atom_weights,
                           float* energy, float* forces, float* virial) {
  const int rc = prior_check(m, ws, ws_bytes, n_atoms, n_mol, pos, z, batch, box, box_mode, atom_weights, energy);
  if (rc != TMDNET_OK) return rc;
  if (!n_atoms || !n_mol) return TMDNET_OK;
  prior_launch(m, (hipStream_t)stream, ws, n_atoms, n_mol, pos, z, batch, box, box_mode, energy, forces, virial);
  HIP_TRY(m, hipGetLastError());
  return TMDNET_OK;
}

int tmdnet_debug_prior(tmdnet_model* m, void* stream, void* ws, size_t ws_bytes, int64_t n_atoms, int64_t n_mol, const float* pos,
                       const int64_t* z, const int64_t* batch, const float* box, int32_t box_mode, float* energy, float* forces,
                       float* virial, double* e_atom) {
  const int rc = prior_check(m, ws, ws_bytes, n_atoms, n_mol, pos, z, batch, box, box_mode, nullptr, energy);
  if (rc != TMDNET_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (n_mol) HIP_TRY(m, hipMemsetAsync(energy, 0, (size_t)n_mol * sizeof(float), s));
  if (forces && n_atoms) HIP_TRY(m, hipMemsetAsync(forces, 0, (size_t)n_atoms * 3 * sizeof(float), s));
  if (virial && n_mol) HIP_TRY(m, hipMemsetAsync(virial, 0, (size_t)n_mol * 9 * sizeof(float), s));
  if (!n_atoms || !n_mol) return TMDNET_OK;
  HIP_TRY(m, hipMemsetAsync(ws, 0, prior_rows_offset(n_mol), s));  // (a test's workspace: no contract on what it held)
  prior_launch(m, s, ws, n_atoms, n_mol, pos, z, batch, box, box_mode, energy, forces, virial);
  HIP_TRY(m, hipGetLastError());
  if (e_atom)
    HIP_TRY(m, hipMemcpy2DAsync(e_atom, sizeof(double), reinterpret_cast<char*>(ws) + prior_rows_offset(n_mol), kPriorRow * sizeof(double),
                                sizeof(double), (size_t)n_atoms, hipMemcpyDeviceToDevice, s));
  return TMDNET_OK;
}

}  // extern "C"
