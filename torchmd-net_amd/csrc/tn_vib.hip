// Hessians and normal-mode preparation assembled on the device.  R replicas of a batch, each seeded with (or displaced along) one
// coordinate of every molecule, give R Hessian columns of EVERY molecule in one evaluation of the replicated batch: analytically
// from the second-order pass (hv = H v of tmdnet_loss_param_grads), or as a central difference of the forces of two displaced
// evaluations.  This file holds what sits around those evaluations; the arithmetic is tn_vib_math.h and the scheme is stated with
// the entries in include/tmdnet_amd.h.
//
//   seed     one thread per replicated atom: the seed vector (SEED) or a displaced copy of the positions (PLUS / MINUS)
//   gather   one thread per (replica, free coordinate): the pass's columns into the padded row-major H [B, D, D]; every valid entry is
//            written exactly once over all passes, nothing else is touched, no atomics
//   finish   one block per molecule, fp64: diagnostics (largest entry, asymmetry, acoustic sum), S = (H + H^T) / 2, the mass
//            weighting, and the projection of translations / rotations.  Entries are strided over the block's threads and each is
//            computed by one thread in a fixed order; the three maxima go through a shared-memory tree (a maximum does not depend on
//            the order); the basis is built by lane 0.  Repeats are bit-identical.
//
// These launches are latency-sized next to the D column passes they serve; they are kept plain.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "tmdnet_amd.h"
#include "tn_vib_math.h"

namespace tn {

namespace {

constexpr int kVibThreads = 256;

// doubles of workspace per molecule: U [6, D], W = U^T A [6, D], G = U^T A U [6, 6]
__host__ __device__ inline size_t vib_ws_doubles(int64_t dim) { return (size_t)(2 * tn_vib::VIB_MAX_RANK) * (size_t)dim + tn_vib::VIB_MAX_RANK * tn_vib::VIB_MAX_RANK; }

bool vib_shape_ok(int64_t n_atoms, int64_t n_mol, int64_t dim, int64_t replicas) {
  if (n_atoms < 0 || n_mol < 0 || dim < 0 || replicas < 1) return false;
  if (dim % 3 != 0 || dim > 3 * n_atoms) return false;
  if (n_mol > INT32_MAX / 4 || dim > INT32_MAX / 4) return false;
  if (n_atoms > 0 && replicas > (INT32_MAX / 4) / n_atoms) return false;  // replicated rows, times three, stay below 2^31
  return true;
}

__global__ __launch_bounds__(kVibThreads) void k_vib_seed(int mode, int64_t N, int64_t B, int64_t R, int64_t col0, const float* __restrict__ pos,
                                                          const int64_t* __restrict__ batch, const int64_t* __restrict__ free_idx,
                                                          const int64_t* __restrict__ fstart, float delta, float* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * kVibThreads + threadIdx.x;
  if (row >= R * N) return;
  const int64_t r = row / N, a = row - r * N;
  const int64_t b = batch[a];
  const int comp = (b < 0 || b >= B) ? -1 : tn_vib::column_component(a, col0 + r, free_idx, fstart[b], fstart[b + 1]);
  float o[3];
  if (mode == tn_vib::VIB_SEED) {
    tn_vib::seed_row(comp, o);
  } else {
    const float x[3] = {pos[3 * a], pos[3 * a + 1], pos[3 * a + 2]};
    tn_vib::displace_row(x, comp, delta, mode, o);
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) out[3 * row + d] = o[d];
}

// thread t of replica r: free coordinate t (free atom t / 3 of the whole batch, component t % 3) is row i of its molecule
__global__ __launch_bounds__(kVibThreads) void k_vib_gather(int mode, int64_t N, int64_t B, int64_t n_free, int64_t D, int64_t R, int64_t col0,
                                                            const int64_t* __restrict__ batch, const int64_t* __restrict__ free_idx,
                                                            const int64_t* __restrict__ fstart, const float* __restrict__ a_in,
                                                            const float* __restrict__ f_minus, const float* __restrict__ x_plus,
                                                            const float* __restrict__ x_minus, float* __restrict__ H) {
  const int64_t t = (int64_t)blockIdx.x * kVibThreads + threadIdx.x;
  const int64_t r = blockIdx.y;
  if (t >= 3 * n_free || r >= R) return;
  const int64_t j = t / 3;
  const int d = (int)(t - 3 * j);
  const int64_t atom = free_idx[j];
  if (atom < 0 || atom >= N) return;  // (a malformed index list writes nothing)
  const int64_t b = batch[atom];
  if (b < 0 || b >= B) return;
  const int64_t f0 = fstart[b], Db = 3 * (fstart[b + 1] - f0);
  const int64_t k = col0 + r;
  if (k >= Db || Db > D) return;  // this replica carries no column of this molecule
  const int64_t i = 3 * (j - f0) + d;
  if (i < 0 || i >= Db) return;
  const int64_t src = 3 * (r * N + atom) + d;
  float h;
  if (mode == tn_vib::VIB_ANALYTIC) {
    h = a_in[src];
  } else {
    const int64_t moved = 3 * (r * N + free_idx[f0 + k / 3]) + k % 3;
    h = tn_vib::central_entry(a_in[src], f_minus[src], x_plus[moved], x_minus[moved]);
  }
  H[(b * D + i) * D + k] = h;
}

// block-wide maximum of three values (values >= 0; a maximum is independent of the order)
__device__ void block_max3(double v[3], double (*sh)[kVibThreads]) {
  for (int q = 0; q < 3; ++q) sh[q][threadIdx.x] = v[q];
  __syncthreads();
  for (int s = kVibThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int q = 0; q < 3; ++q) {
        const double o = sh[q][threadIdx.x + s];
        if (o > sh[q][threadIdx.x]) sh[q][threadIdx.x] = o;
      }
    __syncthreads();
  }
  for (int q = 0; q < 3; ++q) v[q] = sh[q][0];
  __syncthreads();
}

__global__ __launch_bounds__(kVibThreads) void k_vib_finish(int64_t D, int project, const float* __restrict__ Hall,
                                                            const float* __restrict__ pos, const float* __restrict__ mass,
                                                            const int64_t* __restrict__ free_idx, const int64_t* __restrict__ fstart,
                                                            const int64_t* __restrict__ mol_atoms, double* ws, double* Aall,
                                                            double* __restrict__ info) {
  __shared__ double sh[3][kVibThreads];
  __shared__ int sh_rank;
  const int64_t b = blockIdx.x;
  const int64_t f0 = fstart[b], nfree = fstart[b + 1] - f0, Db = 3 * nfree;
  const int64_t* idx = free_idx + f0;
  const float* H = Hall + b * D * D;
  double* A = Aall + b * D * D;
  double* U = ws + (size_t)b * vib_ws_doubles(D);
  double* W = U + tn_vib::VIB_MAX_RANK * D;
  double* G = W + tn_vib::VIB_MAX_RANK * D;
  const int mode = (mol_atoms && nfree < mol_atoms[b]) ? (int)tn_vib::VIB_PROJECT_NONE : project;
  const int tid = threadIdx.x;
  if (Db > D || Db < 0) {  // the index lists do not fit the padded block: nothing is computed, the rank says so
    if (tid == 0) info[b * tn_vib::VIB_INFO + 3] = -1.0;
    return;
  }

  // 1. diagnostics
  double mx[3] = {0.0, 0.0, 0.0};
  for (int64_t e = tid; e < Db * Db; e += kVibThreads) {
    const int64_t i = e / Db, j = e - i * Db;
    double h, a;
    tn_vib::diag_entry(H, D, i, j, &h, &a);
    if (h > mx[0]) mx[0] = h;
    if (a > mx[1]) mx[1] = a;
  }
  for (int64_t e = tid; e < 3 * Db; e += kVibThreads) {
    const double s = tn_vib::drift_entry(H, D, nfree, e / 3, (int)(e % 3));
    if (s > mx[2]) mx[2] = s;
  }
  block_max3(mx, sh);

  // 2. + 3. symmetrise and mass-weight; the padding of the block is written as zero
  for (int64_t e = tid; e < D * D; e += kVibThreads) {
    const int64_t i = e / D, j = e - i * D;
    A[e] = (i < Db && j < Db) ? tn_vib::weighted_entry(H, D, i, j, mass[idx[i / 3]], mass[idx[j / 3]]) : 0.0;
  }
  // 4. the basis, by one lane
  if (tid == 0) sh_rank = tn_vib::build_basis(pos, mass, idx, nfree, mode, U);
  __syncthreads();  // A and U are visible to the whole block
  const int rank = sh_rank;
  if (rank > 0) {
    for (int64_t e = tid; e < rank * Db; e += kVibThreads) W[e] = tn_vib::proj_w_entry(U, A, D, Db, (int)(e / Db), e % Db);
    __syncthreads();
    if (tid < rank * rank) G[(tid / rank) * tn_vib::VIB_MAX_RANK + tid % rank] = tn_vib::proj_g_entry(U, W, Db, tid / rank, tid % rank);
    __syncthreads();
    for (int64_t e = tid; e < Db * Db; e += kVibThreads) {
      const int64_t i = e / Db, j = e - i * Db;
      A[i * D + j] = tn_vib::proj_apply_entry(A[i * D + j], U, W, G, Db, rank, i, j);
    }
  }
  if (tid == 0) {
    double* o = info + b * tn_vib::VIB_INFO;
    o[0] = mx[0];
    o[1] = mx[1];
    o[2] = mx[2];
    o[3] = (double)rank;
    o[4] = (double)mode;
    o[5] = (double)Db;
    o[6] = o[7] = 0.0;
  }
}

inline int vib_done() { return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP; }

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_vib_workspace_bytes(int64_t n_mol, int64_t dim, size_t* bytes) {
  if (!bytes || n_mol < 0 || dim < 0 || dim % 3 != 0 || n_mol > INT32_MAX / 4 || dim > INT32_MAX / 4) return TMDNET_ERR_INVALID;
  *bytes = (size_t)n_mol * vib_ws_doubles(dim) * sizeof(double);
  return TMDNET_OK;
}

int tmdnet_vib_seed(void* stream, int32_t mode, int64_t n_atoms, int64_t n_mol, int64_t replicas, int64_t col0, const float* pos,
                    const int64_t* batch, const int64_t* free_idx, const int64_t* fstart, float delta, float* out) {
  if (mode != TMDNET_VIB_SEED && mode != TMDNET_VIB_PLUS && mode != TMDNET_VIB_MINUS) return TMDNET_ERR_INVALID;
  if (!vib_shape_ok(n_atoms, n_mol, 0, replicas) || col0 < 0 || !batch || !fstart || !out) return TMDNET_ERR_INVALID;
  if (mode != TMDNET_VIB_SEED && (!pos || !(delta > 0.f) || !std::isfinite(delta))) return TMDNET_ERR_INVALID;
  const int64_t rows = replicas * n_atoms;
  if (rows == 0) return TMDNET_OK;
  if (n_mol < 1 || !free_idx) return TMDNET_ERR_INVALID;
  hipLaunchKernelGGL(k_vib_seed, dim3((unsigned)((rows + kVibThreads - 1) / kVibThreads)), dim3(kVibThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), (int)mode, n_atoms, n_mol, replicas, col0, pos, batch, free_idx, fstart, delta, out);
  return vib_done();
}

int tmdnet_vib_gather(void* stream, int32_t mode, int64_t n_atoms, int64_t n_mol, int64_t n_free, int64_t dim, int64_t replicas,
                      int64_t col0, const int64_t* batch, const int64_t* free_idx, const int64_t* fstart, const float* hv_or_f_plus,
                      const float* f_minus, const float* pos_plus, const float* pos_minus, float* H) {
  if (mode != TMDNET_VIB_ANALYTIC && mode != TMDNET_VIB_CENTRAL) return TMDNET_ERR_INVALID;
  if (!vib_shape_ok(n_atoms, n_mol, dim, replicas) || col0 < 0 || n_free < 0 || n_free > n_atoms || replicas > 65535) return TMDNET_ERR_INVALID;
  if (n_free == 0 || dim == 0) return TMDNET_OK;
  if (!batch || !free_idx || !fstart || !hv_or_f_plus || !H) return TMDNET_ERR_INVALID;
  if (mode == TMDNET_VIB_CENTRAL && (!f_minus || !pos_plus || !pos_minus)) return TMDNET_ERR_INVALID;
  const dim3 grid((unsigned)((3 * n_free + kVibThreads - 1) / kVibThreads), (unsigned)replicas);
  hipLaunchKernelGGL(k_vib_gather, grid, dim3(kVibThreads), 0, reinterpret_cast<hipStream_t>(stream), (int)mode, n_atoms, n_mol, n_free, dim, replicas,
                     col0, batch, free_idx, fstart, hv_or_f_plus, f_minus, pos_plus, pos_minus, H);
  return vib_done();
}

int tmdnet_vib_finish(void* stream, void* vib_ws, size_t ws_bytes, int64_t n_atoms, int64_t n_mol, int64_t dim, int32_t project,
                      const float* H, const float* pos, const float* masses, const int64_t* free_idx, const int64_t* fstart,
                      const int64_t* mol_atoms, double* A, double* info) {
  if (project != TMDNET_VIB_PROJECT_NONE && project != TMDNET_VIB_PROJECT_TRANS && project != TMDNET_VIB_PROJECT_TRANS_ROT)
    return TMDNET_ERR_INVALID;
  if (!vib_shape_ok(n_atoms, n_mol, dim, 1) || !fstart || !info) return TMDNET_ERR_INVALID;
  if (n_mol == 0) return TMDNET_OK;
  if (dim > 0 && (!H || !A || !pos || !masses || !free_idx || !vib_ws)) return TMDNET_ERR_INVALID;
  if (dim > 0 && ws_bytes < (size_t)n_mol * vib_ws_doubles(dim) * sizeof(double)) return TMDNET_ERR_WORKSPACE;
  hipLaunchKernelGGL(k_vib_finish, dim3((unsigned)n_mol), dim3(kVibThreads), 0, reinterpret_cast<hipStream_t>(stream), dim, (int)project, H,
                     pos, masses, free_idx, fstart, mol_atoms, reinterpret_cast<double*>(vib_ws), A, info);
  return vib_done();
}

}  // extern "C"
