// Virial of the energy+force pass: minus the derivative of every molecule's energy with respect to a homogeneous strain,
//   pos -> pos (I + eps),  box -> box (I + eps)      (row vectors, one eps[3,3] per molecule)
//   W_m[a][b] = - d E_m / d eps_ab = - sum over the pairs p of molecule m of  pdelta_p[a] * g_delta_p[b]
// Why the pair form is exact: the energy depends on the geometry through the minimum-image pair vectors only,
// delta_p = pos_i - pos_j + n_p box with integer n_p, and box and positions are strained together, so delta_p -> delta_p (I + eps)
// with n_p fixed (the fractional coordinates do not move: no pair changes its image), and d E / d eps_ab = sum_p delta_p[a] dE/d delta_p[b].
// The reverse pass of every architecture ends with exactly that per-pair gradient, g_delta[P,3] (the forces are its signed sum over
// an atom's pairs), and the graph keeps pdelta[P,3].  Self pairs have no geometry and contribute nothing; mean / std / atomref enter
// through g_delta as they enter the forces.
//
// Two steps, no floating-point atomics, every sum in a fixed order (bit-identical repeats):
//   k_force_virial_gather   the force gather (tn_kernels.hip: k_force_gather, the same arithmetic on the same loads, so the forces
//                           are bit-identical) that also accumulates, over the edges of the row whose pair has this atom as its
//                           i end (esign > 0: every pair once), the nine products -> part [N, 9] in the engine's atom order
//   k_virial_reduce         per molecule: the atom range mstart..mend cut into S slices, one block per (molecule, slice);
//                           S == 1 (molecules of at most 1 024 atoms on average) writes W directly, otherwise k_virial_finish adds
//                           the slice sums in slice order.  256 molecules of 64 atoms: 256 blocks at once; one 10^6-atom system:
//                           256 blocks of ~3 900 atoms.  An unsorted batch, or several molecules interleaved by the cell list, has no
//                           ranges (Graph::counts[3]): a slice is then a range of ALL atoms filtered by the molecule index, O(N B)
//                           as in k_head_mol_sum.  A molecule index without atoms gets zeros.
// Static (capturable) mode: the kernels skip their work when the graph overflowed (counts[2]), like every other kernel of the step.
#include "tn_virial.h"

#include <string>

#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_model.h"

namespace tn {

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(256) void k_force_virial_gather(Graph g, int N, const float* __restrict__ g_delta, const int* __restrict__ perm,
                                                             float* __restrict__ forces, float* __restrict__ part) {
  const int i = blockIdx.x * 16 + (threadIdx.x >> 4), sub = threadIdx.x & 15;
  const bool live = i < N && !g.counts[2];
  float fx = 0.f, fy = 0.f, fz = 0.f;
  float w[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    const int e1 = g.rowptr[i + 1];
    for (int e = g.rowptr[i] + sub; e < e1; e += 16) {
      const float sg = g.esign[e];
      if (sg == 0.f) continue;
      const int p = g.epair[e];
      const float g0 = g_delta[p * 3], g1 = g_delta[p * 3 + 1], g2 = g_delta[p * 3 + 2];
      fx -= sg * g0;  // sg = +-1: the product is exact, so this is k_force_gather's sum whatever the contraction
      fy -= sg * g1;
      fz -= sg * g2;
      if (sg > 0.f) {
        const float d0 = g.pdelta[p * 3], d1 = g.pdelta[p * 3 + 1], d2 = g.pdelta[p * 3 + 2];
        w[0] -= d0 * g0; w[1] -= d0 * g1; w[2] -= d0 * g2;
        w[3] -= d1 * g0; w[4] -= d1 * g1; w[5] -= d1 * g2;
        w[6] -= d2 * g0; w[7] -= d2 * g1; w[8] -= d2 * g2;
      }
    }
  }
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    fx += __shfl_down(fx, off, 16);
    fy += __shfl_down(fy, off, 16);
    fz += __shfl_down(fz, off, 16);
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] += __shfl_down(w[k], off, 16);
  }
  if (live && sub == 0) {
    const int o = perm ? perm[i] : i;  // cell-list path: back to the caller's atom order
    forces[o * 3] = fx;
    forces[o * 3 + 1] = fy;
    forces[o * 3 + 2] = fz;
#pragma unroll
    for (int k = 0; k < 9; ++k) part[(int64_t)i * 9 + k] = w[k];  // engine order: the order of mstart..mend / of `batch`
  }
}

// sum of 9 values over the block (fixed order: lanes by the wave tree, waves in turn), result in every thread
__device__ __forceinline__ void block_sum9(float (&v)[9], float (*sh)[9]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 9; ++k) v[k] = wave_sum(v[k]);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 9; ++k) sh[wave][k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 9; ++k) v[k] = sh[0][k] + sh[1][k] + sh[2][k] + sh[3][k];
}

// grid (B, S): slice s of molecule m -> out[(m * S + s) * 9 ..]  (S == 1: out is the virial itself)
__global__ __launch_bounds__(kThreads) void k_virial_reduce(Graph g, int N, int S, const int64_t* __restrict__ batch,
                                                            const float* __restrict__ part, float* __restrict__ out) {
  __shared__ float sh[4][9];
  if (g.counts[2]) return;
  const int m = blockIdx.x, s = blockIdx.y;
  const bool filter = g.counts[3] != 0;  // no atom ranges: unsorted batch, or molecules interleaved in cell order
  int a = 0, b = N;
  if (!filter) {
    a = g.mstart[m];
    b = g.mend[m];
  }
  const int64_t len = b - a;
  const int i0 = a + (int)(len * s / S), i1 = a + (int)(len * (s + 1) / S);
  float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = i0 + (int)threadIdx.x; i < i1; i += kThreads) {
    if (filter && batch && batch[i] != m) continue;  // (no batch vector: one molecule)
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] += part[(int64_t)i * 9 + k];
  }
  block_sum9(v, sh);
  if (threadIdx.x < 9) out[((int64_t)m * S + s) * 9 + threadIdx.x] = v[threadIdx.x];
}

// one thread per (molecule, component): the slice sums in slice order
__global__ __launch_bounds__(kThreads) void k_virial_finish(Graph g, int B, int S, const float* __restrict__ slices,
                                                            float* __restrict__ virial) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (int64_t)B * 9 || g.counts[2]) return;
  const int64_t m = t / 9;
  const int k = (int)(t - m * 9);
  float v = 0.f;
  for (int s = 0; s < S; ++s) v += slices[(m * S + s) * 9 + k];
  virial[t] = v;
}

inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

}  // namespace

int virial_slices(int64_t N, int64_t B) {
  if (B <= 0 || N <= 1024 * B) return 1;
  const int64_t s = (N + 1024 * B - 1) / (1024 * B);
  return (int)(s > 256 ? 256 : s);
}

size_t virial_workspace_bytes(int64_t N, int64_t B) {
  const int S = virial_slices(N, B);
  size_t n = align256((size_t)(N > 0 ? N : 0) * 9 * sizeof(float));
  if (S > 1) n += align256((size_t)B * S * 9 * sizeof(float));
  return n + 256;  // room to align the caller's pointer
}

void launch_force_virial(const Graph& g, int N, int B, const float* g_delta, const int* perm, const int64_t* batch, float* forces,
                         float* virial, void* scratch, hipStream_t s) {
  if (B <= 0) return;
  if (N <= 0) {
    (void)hipMemsetAsync(virial, 0, (size_t)B * 9 * sizeof(float), s);
    return;
  }
  char* base = reinterpret_cast<char*>(align256(reinterpret_cast<size_t>(scratch)));
  float* part = reinterpret_cast<float*>(base);
  float* slices = reinterpret_cast<float*>(base + align256((size_t)N * 9 * sizeof(float)));
  const int S = virial_slices(N, B);
  hipLaunchKernelGGL(k_force_virial_gather, dim3((N + 15) / 16), dim3(256), 0, s, g, N, g_delta, perm, forces, part);
  hipLaunchKernelGGL(k_virial_reduce, dim3(B, S), dim3(kThreads), 0, s, g, N, S, batch, part, S == 1 ? virial : slices);
  if (S > 1)
    hipLaunchKernelGGL(k_virial_finish, dim3((int)(((int64_t)B * 9 + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, g, B, S, slices,
                       virial);
}

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_virial_workspace_bytes(const tmdnet_model* m, int64_t n_atoms, int64_t n_mol, size_t* bytes) {
  if (!m || !bytes || n_atoms < 0 || n_mol < 0) return TMDNET_ERR_INVALID;
  *bytes = virial_workspace_bytes(n_atoms, n_mol);
  return TMDNET_OK;
}

int tmdnet_energy_forces_virial(tmdnet_model* m, void* stream, void* graph_ws, void* ws, size_t ws_bytes, void* virial_ws,
                                size_t virial_ws_bytes, int64_t n_atoms, int64_t n_mol, int64_t n_pairs, const int64_t* z,
                                const int64_t* batch, const float* q, int32_t want_forces, float* energy, float* forces, float* virial) {
  (void)want_forces;  // the virial is a by-product of the force pass: always 1
  if (!m || !forces || !virial || !virial_ws) return TMDNET_ERR_INVALID;
  if (m->tn2)
    return fail(m, TMDNET_ERR_INVALID, "the virial is not implemented for TensorNet2 (the Coulomb head's forces do not come from the "
                                       "per-pair gradient)");
  if (m->head_kind) return fail(m, TMDNET_ERR_INVALID, "the virial is implemented for the scalar head only (tmdnet_set_output_head)");
  if (m->atom_w) return fail(m, TMDNET_ERR_INVALID, "the virial is not implemented with atom weights (tmdnet_set_atom_weights)");
  if (m->halo_fn) return fail(m, TMDNET_ERR_INVALID, "the virial is not implemented with the halo exchange (tmdnet_set_halo_exchange)");
  if (m->train) return fail(m, TMDNET_ERR_INVALID, "the virial is not implemented inside the parameter-gradient and second-order passes");
  if (virial_ws_bytes < virial_workspace_bytes(n_atoms, n_mol))
    return fail(m, TMDNET_ERR_WORKSPACE, "virial workspace too small: need " + std::to_string(virial_workspace_bytes(n_atoms, n_mol)));
  m->virial_out = virial;
  m->virial_ws = virial_ws;
  const int rc = tmdnet_energy_forces(m, stream, graph_ws, ws, ws_bytes, n_atoms, n_mol, n_pairs, z, batch, q, 1, energy, forces);
  m->virial_out = nullptr;
  m->virial_ws = nullptr;
  return rc;
}

}  // extern "C"
