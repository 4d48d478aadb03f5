// Property heads (reference output_modules.py:166-323): DipoleMoment and ElectronicSpatialExtent on TensorNet and on the
// Equivariant Transformer, EquivariantVectorOutput.
//
// The per-atom network is the Scalar head's MLP, so the head value q_i (times std) and its derivative d q_i / d ao come out of
// k_head_energy unchanged.  What these kernels add is the molecule side:
//   M = sum m_i,  c = sum m_i r_i / M,  d_i = r_i - c        (raw caller positions: no minimum image, as in the reference)
//   DipoleMoment:            y = || sum q_i d_i + mean ||      ElectronicSpatialExtent:  y = sum q_i ||d_i||^2 + mean
// and, for the forces, the reverse seed of every atom's head output plus the direct position term (centre of mass at fixed masses):
//   dipole: seed u . d_i,    d y / d r_j = u (q_j - m_j Q / M)              (u = mu / ||mu||, 0 where ||mu|| = 0; Q = sum q_i)
//   ESE:    seed ||d_i||^2,  d y / d r_j = 2 q_j d_j - 2 (m_j / M) sum_i q_i d_i
// The seed scales the rows of g_ao (d q_i / d ao from k_head_energy), after which the Scalar head's reverse pass runs unchanged;
// the direct term goes into the forces in k_force_gather.
//
// Reductions are two passes (centre of mass first, centred moments second: a one-pass sum q |r|^2 - ... cancels badly in fp32
// far from the origin), in fixed order and without atomics.  Molecules of at most 256 atoms on average: one block per molecule
// does both passes (k_heads_mol).  Fewer, larger molecules: S slices per molecule write partial sums (k_heads_pass1 / _pass2) and
// one thread per molecule adds them in slice order (k_heads_finish).  An unsorted batch (or several molecules interleaved in cell
// order) has no atom ranges: every block then scans all N atoms for its members, O(N B) work as in k_mol_sum / k_head_mol_sum.
//
// Equivariant Transformer: the dipole and vector heads keep the vector output v_i = gate_i (vq_i W22^T) of the second gated block
// (k_et_vout); sum std v_i joins the moment before the norm (dipole) or is the output (vector, y [B,3]).  Its reverse seeds enter
// g_pre2 through the gate channel (k_et_heads_seed) and g_vq through W22 (k_et_gvq_add).  EquivariantElectronicSpatialExtent is the
// Scalar MLP on the out_norm features, handled like TensorNet's.
//
// These heads take the general schedule only: the fused per-atom paths (tn_small.hip, tn_mid.hip) and k_head_mol_sum carry the
// Scalar head alone.  Nothing here allocates or synchronises (HIP-graph capture works as for the Scalar head).
#include "tn_heads.h"

#include "tn_common.h"
#include "tn_model.h"

namespace tn {

static inline int cdiv_h(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

namespace {

constexpr int kThreads = 256;

// atoms [i0, i1) of slice s of molecule m; `filter`: unsorted batch, the slice is a range of all atoms and membership is tested
__device__ __forceinline__ void slice_range(const Graph& g, int N, int S, int s, int m, int& i0, int& i1, bool& filter) {
  filter = g.counts[3] != 0;
  int a = 0, b = N;
  if (!filter) {
    a = g.mstart[m];
    b = g.mend[m];
  }
  const int64_t len = b - a;
  i0 = a + (int)(len * s / S);
  i1 = a + (int)(len * (s + 1) / S);
}

// sum of K values over the block (fixed order: waves in turn), result in every thread
template <int K>
__device__ __forceinline__ void block_sum(float (&v)[K], float (*sh)[K]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();  // sh may still be read from a previous call
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) sh[wave][k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = sh[0][k] + sh[1][k] + sh[2][k] + sh[3][k];
}

__device__ __forceinline__ void atom_geom(const float* __restrict__ pos, const int* __restrict__ perm, const int64_t* __restrict__ z,
                                          const float* __restrict__ mass, int n_mass, int i, float& mi, float r[3]) {
  const int o = perm ? perm[i] : i;
  r[0] = pos[(int64_t)o * 3];
  r[1] = pos[(int64_t)o * 3 + 1];
  r[2] = pos[(int64_t)o * 3 + 2];
  if (!mass) {  // vector output: no centre of mass
    mi = 1.0f;
    return;
  }
  int64_t zi = z[i];
  zi = zi < 0 ? 0 : (zi >= n_mass ? n_mass - 1 : zi);  // the host raises IndexError for z >= n_mass before the call
  mi = mass[zi];
}

// pass 1 over atoms [i0, i1): (sum m, sum m r)
__device__ __forceinline__ void acc_pass1(const float* pos, const int* perm, const int64_t* z, const float* mass, int n_mass,
                                          const int64_t* batch, int m, int i0, int i1, bool filter, float (&a)[4]) {
  for (int i = i0 + (int)threadIdx.x; i < i1; i += kThreads) {
    if (filter && batch[i] != m) continue;
    float mi, r[3];
    atom_geom(pos, perm, z, mass, n_mass, i, mi, r);
    a[0] += mi;
    a[1] += mi * r[0];
    a[2] += mi * r[1];
    a[3] += mi * r[2];
  }
}

// pass 2: (sum q d + sum std v, sum q |d|^2, sum q) around the centre c
__device__ __forceinline__ void acc_pass2(const float* pos, const int* perm, const float* q, const float* gate, const float* vq2s,
                                          const int64_t* batch, int m, int i0, int i1, bool filter, const float c[3], float (&a)[5]) {
  for (int i = i0 + (int)threadIdx.x; i < i1; i += kThreads) {
    if (filter && batch[i] != m) continue;
    const int o = perm ? perm[i] : i;
    const float dx = pos[(int64_t)o * 3] - c[0], dy = pos[(int64_t)o * 3 + 1] - c[1], dz = pos[(int64_t)o * 3 + 2] - c[2];
    const float qi = q ? q[i] : 0.f;
    a[0] += qi * dx;
    a[1] += qi * dy;
    a[2] += qi * dz;
    if (gate) {
      const float gi = gate[i];
      a[0] += gi * vq2s[(int64_t)i * 3];
      a[1] += gi * vq2s[(int64_t)i * 3 + 1];
      a[2] += gi * vq2s[(int64_t)i * 3 + 2];
    }
    a[3] += qi * (dx * dx + dy * dy + dz * dz);
    a[4] += qi;
  }
}

__device__ __forceinline__ void centre(const float (&a)[4], float c[3]) {
  const float M = a[0];
  // a molecule id without atoms: M = 0, nothing is centred (c = 0 keeps its output at the `mean` term instead of NaN)
  c[0] = M > 0.f ? a[1] / M : 0.f;
  c[1] = M > 0.f ? a[2] / M : 0.f;
  c[2] = M > 0.f ? a[3] / M : 0.f;
}

// y of molecule m and the state the seeds need: [M, cx, cy, cz, Q, vx, vy, vz] with v = u (dipole) or sum q d (ESE)
__device__ __forceinline__ void finish_mol(int kind, float mean, float M, const float c[3], const float (&b)[5], float* __restrict__ y,
                                           float* __restrict__ st) {
  float v0 = b[0], v1 = b[1], v2 = b[2];
  if (kind == TN_HEAD_VECTOR) {  // y [B,3]; every component seeds its atoms' vectors with 1
    y[0] = b[0] + mean;
    y[1] = b[1] + mean;
    y[2] = b[2] + mean;
    v0 = v1 = v2 = 1.f;
  } else if (kind == TN_HEAD_DIPOLE) {
    const float mx = b[0] + mean, my = b[1] + mean, mz = b[2] + mean;
    const float nrm = sqrtf(mx * mx + my * my + mz * mz);
    *y = nrm;
    const float inv = nrm > 0.f ? 1.0f / nrm : 0.f;  // torch.norm's backward: zero gradient at the origin
    v0 = mx * inv;
    v1 = my * inv;
    v2 = mz * inv;
  } else {
    *y = b[3] + mean;
  }
  if (st) {
    st[0] = M;
    st[1] = c[0];
    st[2] = c[1];
    st[3] = c[2];
    st[4] = b[4];
    st[5] = v0;
    st[6] = v1;
    st[7] = v2;
  }
}

// one block per molecule, both passes
__global__ __launch_bounds__(kThreads) void k_heads_mol(Graph g, HeadArgs h) {
  __shared__ float sh4[4][4];
  __shared__ float sh5[4][5];
  const int m = blockIdx.x;
  int i0, i1;
  bool filter;
  slice_range(g, h.N, 1, 0, m, i0, i1, filter);
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  acc_pass1(h.pos, h.perm, h.z, h.mass, h.n_mass, h.batch, m, i0, i1, filter, a);
  block_sum<4>(a, sh4);
  float c[3];
  centre(a, c);
  float b[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  acc_pass2(h.pos, h.perm, h.q, h.gate, h.vq2s, h.batch, m, i0, i1, filter, c, b);
  block_sum<5>(b, sh5);
  if (threadIdx.x == 0) finish_mol(h.kind, h.mean, a[0], c, b, h.y + (int64_t)m * (h.kind == TN_HEAD_VECTOR ? 3 : 1), h.state ? h.state + (int64_t)m * 8 : nullptr);
}

// slices: grid (S, B)
__global__ __launch_bounds__(kThreads) void k_heads_pass1(Graph g, HeadArgs h, int S, float* __restrict__ part1) {
  __shared__ float sh4[4][4];
  const int s = blockIdx.x, m = blockIdx.y;
  int i0, i1;
  bool filter;
  slice_range(g, h.N, S, s, m, i0, i1, filter);
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  acc_pass1(h.pos, h.perm, h.z, h.mass, h.n_mass, h.batch, m, i0, i1, filter, a);
  block_sum<4>(a, sh4);
  if (threadIdx.x == 0)
    for (int k = 0; k < 4; ++k) part1[((int64_t)m * S + s) * 4 + k] = a[k];
}

__device__ __forceinline__ void sum_slices1(const float* __restrict__ part1, int S, int m, float (&a)[4]) {
  for (int k = 0; k < 4; ++k) a[k] = 0.f;
  for (int s = 0; s < S; ++s)
    for (int k = 0; k < 4; ++k) a[k] += part1[((int64_t)m * S + s) * 4 + k];
}

__global__ __launch_bounds__(kThreads) void k_heads_pass2(Graph g, HeadArgs h, int S, const float* __restrict__ part1,
                                                         float* __restrict__ part2) {
  __shared__ float sh5[4][5];
  const int s = blockIdx.x, m = blockIdx.y;
  float a[4];
  sum_slices1(part1, S, m, a);  // every thread, same order: the same centre in all slices
  float c[3];
  centre(a, c);
  int i0, i1;
  bool filter;
  slice_range(g, h.N, S, s, m, i0, i1, filter);
  float b[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  acc_pass2(h.pos, h.perm, h.q, h.gate, h.vq2s, h.batch, m, i0, i1, filter, c, b);
  block_sum<5>(b, sh5);
  if (threadIdx.x == 0)
    for (int k = 0; k < 5; ++k) part2[((int64_t)m * S + s) * 5 + k] = b[k];
}

__global__ __launch_bounds__(kThreads) void k_heads_finish(HeadArgs h, int S, const float* __restrict__ part1,
                                                          const float* __restrict__ part2) {
  const int m = blockIdx.x * kThreads + threadIdx.x;
  if (m >= h.B) return;
  float a[4];
  sum_slices1(part1, S, m, a);
  float c[3];
  centre(a, c);
  float b[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < S; ++s)
    for (int k = 0; k < 5; ++k) b[k] += part2[((int64_t)m * S + s) * 5 + k];
  finish_mol(h.kind, h.mean, a[0], c, b, h.y + (int64_t)m * (h.kind == TN_HEAD_VECTOR ? 3 : 1), h.state ? h.state + (int64_t)m * 8 : nullptr);
}

// seeds: g_ao[i, :] *= d y / d q_i ; direct[i] = d y / d r_i at fixed head outputs (one wave per atom)
__global__ __launch_bounds__(kThreads) void k_heads_seed(HeadArgs h, int H, float* __restrict__ g_ao, float* __restrict__ direct) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= h.N) return;
  const int64_t bm = h.batch[i];
  float seed = 0.f, dr[3] = {0.f, 0.f, 0.f};
  if (bm >= 0 && bm < h.B) {  // out-of-range ids are reported by the graph phase; their atoms get no gradient
    const float* st = h.state + bm * 8;
    const float M = st[0];
    float mi, r[3];
    atom_geom(h.pos, h.perm, h.z, h.mass, h.n_mass, i, mi, r);
    const float d0 = r[0] - st[1], d1 = r[1] - st[2], d2 = r[2] - st[3];
    const float qi = h.q[i], w = M > 0.f ? mi / M : 0.f;
    if (h.kind == TN_HEAD_DIPOLE) {
      seed = st[5] * d0 + st[6] * d1 + st[7] * d2;
      const float t = qi - w * st[4];
      dr[0] = st[5] * t;
      dr[1] = st[6] * t;
      dr[2] = st[7] * t;
    } else {
      seed = d0 * d0 + d1 * d1 + d2 * d2;
      dr[0] = 2.f * (qi * d0 - w * st[5]);
      dr[1] = 2.f * (qi * d1 - w * st[6]);
      dr[2] = 2.f * (qi * d2 - w * st[7]);
    }
  }
  for (int k = lane; k < H; k += 64) g_ao[(int64_t)i * H + k] *= seed;
  if (lane < 3) direct[(int64_t)i * 3 + lane] = dr[lane];
}

// one wave per atom: gate_i = silu(pre2_i) . Wn2[1] + bn2[1], vq2s_i = std vq_i W22^T
__global__ __launch_bounds__(kThreads) void k_et_vout(int N, int F2, const float* __restrict__ pre2, const float* __restrict__ Wn2,
                                                     const float* __restrict__ bn2, const float* __restrict__ vq,
                                                     const float* __restrict__ W22, float std, float* __restrict__ gate,
                                                     float* __restrict__ vq2s) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= N) return;
  float g = 0.f, v0 = 0.f, v1 = 0.f, v2 = 0.f;
  const float* vr = vq + (int64_t)i * 3 * F2;
  for (int k = lane; k < F2; k += 64) {
    g += silu(pre2[(int64_t)i * F2 + k]) * Wn2[F2 + k];
    const float w = W22[k];
    v0 += vr[k] * w;
    v1 += vr[F2 + k] * w;
    v2 += vr[2 * F2 + k] * w;
  }
  g = wave_sum(g);
  v0 = wave_sum(v0);
  v1 = wave_sum(v1);
  v2 = wave_sum(v2);
  if (lane == 0) {
    gate[i] = g + bn2[1];
    vq2s[(int64_t)i * 3] = std * v0;
    vq2s[(int64_t)i * 3 + 1] = std * v1;
    vq2s[(int64_t)i * 3 + 2] = std * v2;
  }
}

// dipole: d y / d x_i = u . d_i (x_i: the scalar output, its std and Wn2[0] silu'(pre2) already in g_pre2), d y / d v_i = std u;
// vector: d y / d x_i = 0, d y / d v_i = std (1,1,1).  Through v_i = gate_i vq2_i: d y / d gate_i = std u . vq2_i and
// d y / d vq2_i = std u gate_i (-> gv, times W22 into g_vq by k_et_gvq_add)
__global__ __launch_bounds__(kThreads) void k_et_heads_seed(HeadArgs h, int F2, const float* __restrict__ pre2,
                                                           const float* __restrict__ Wn2, float* __restrict__ g_pre2,
                                                           float* __restrict__ gv, float* __restrict__ direct) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= h.N) return;
  const int64_t bm = h.batch[i];
  float seed = 0.f, u[3] = {0.f, 0.f, 0.f}, dr[3] = {0.f, 0.f, 0.f};
  if (bm >= 0 && bm < h.B) {
    const float* st = h.state + bm * 8;
    u[0] = st[5];
    u[1] = st[6];
    u[2] = st[7];
    if (h.kind == TN_HEAD_DIPOLE) {
      const float M = st[0];
      float mi, r[3];
      atom_geom(h.pos, h.perm, h.z, h.mass, h.n_mass, i, mi, r);
      const float d0 = r[0] - st[1], d1 = r[1] - st[2], d2 = r[2] - st[3];
      seed = u[0] * d0 + u[1] * d1 + u[2] * d2;
      const float t = h.q[i] - (M > 0.f ? mi / M : 0.f) * st[4];
      dr[0] = u[0] * t;
      dr[1] = u[1] * t;
      dr[2] = u[2] * t;
    }
  }
  const float* vs = h.vq2s + (int64_t)i * 3;
  const float g_gate = u[0] * vs[0] + u[1] * vs[1] + u[2] * vs[2];
  const bool has_x = h.kind == TN_HEAD_DIPOLE;
  for (int k = lane; k < F2; k += 64) {
    const int64_t o = (int64_t)i * F2 + k;
    const float gx = has_x ? seed * g_pre2[o] : 0.f;
    g_pre2[o] = gx + Wn2[F2 + k] * silu_grad(pre2[o]) * g_gate;
  }
  if (lane < 3) {
    gv[(int64_t)i * 3 + lane] = h.std * u[lane] * h.gate[i];
    direct[(int64_t)i * 3 + lane] = dr[lane];
  }
}

__global__ __launch_bounds__(kThreads) void k_et_gvq_add(int64_t n, int F2, const float* __restrict__ gv, const float* __restrict__ W22,
                                                        float* __restrict__ g_vq) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n) return;
  const int64_t row = e / F2;  // (atom, component)
  g_vq[e] += gv[row] * W22[e - row * F2];
}

}  // namespace

int heads_slices(int64_t N, int64_t B) {
  if (B <= 0 || N <= 256 * B) return 1;
  const int64_t s = (N + 1024 * B - 1) / (1024 * B);
  return (int)(s < 1 ? 1 : (s > 256 ? 256 : s));
}

void launch_et_vout(int N, int F2, const float* pre2, const float* Wn2, const float* bn2, const float* vq, const float* W22, float std,
                    float* gate, float* vq2s, hipStream_t s) {
  if (N <= 0) return;
  hipLaunchKernelGGL(k_et_vout, dim3(cdiv_h(N, 4)), dim3(kThreads), 0, s, N, F2, pre2, Wn2, bn2, vq, W22, std, gate, vq2s);
}

void launch_et_heads_seed(const HeadArgs& h, int F2, const float* pre2, const float* Wn2, float* g_pre2, float* gv, float* direct,
                          hipStream_t s) {
  if (h.N <= 0) return;
  hipLaunchKernelGGL(k_et_heads_seed, dim3(cdiv_h(h.N, 4)), dim3(kThreads), 0, s, h, F2, pre2, Wn2, g_pre2, gv, direct);
}

void launch_et_gvq_add(int N, int F2, const float* gv, const float* W22, float* g_vq, hipStream_t s) {
  const int64_t n = (int64_t)N * 3 * F2;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_et_gvq_add, dim3(cdiv_h(n, kThreads)), dim3(kThreads), 0, s, n, F2, gv, W22, g_vq);
}

HeadBuffers carve_heads(void* base, int64_t N, int64_t B, size_t* bytes) {
  Carver c(base);
  HeadBuffers hb{};
  const int S = heads_slices(N, B);
  hb.S = S;
  hb.state = c.take<float>(B * 8);
  hb.part1 = S > 1 ? c.take<float>(B * S * 4) : nullptr;
  hb.part2 = S > 1 ? c.take<float>(B * S * 5) : nullptr;
  hb.direct = c.take<float>(N * 3);
  hb.gate = c.take<float>(N);
  hb.vq2s = c.take<float>(N * 3);
  hb.gv = c.take<float>(N * 3);
  if (bytes) *bytes = c.off;
  return hb;
}

void launch_heads_reduce(const Graph& g, const HeadArgs& h, const HeadBuffers& hb, hipStream_t s) {
  if (h.B <= 0) return;
  if (hb.S == 1) {
    hipLaunchKernelGGL(k_heads_mol, dim3(h.B), dim3(kThreads), 0, s, g, h);
    return;
  }
  hipLaunchKernelGGL(k_heads_pass1, dim3(hb.S, h.B), dim3(kThreads), 0, s, g, h, hb.S, hb.part1);
  hipLaunchKernelGGL(k_heads_pass2, dim3(hb.S, h.B), dim3(kThreads), 0, s, g, h, hb.S, hb.part1, hb.part2);
  hipLaunchKernelGGL(k_heads_finish, dim3(cdiv_h(h.B, kThreads)), dim3(kThreads), 0, s, h, hb.S, hb.part1, hb.part2);
}

void launch_heads_seed(const HeadArgs& h, int H, float* g_ao, float* direct, hipStream_t s) {
  if (h.N <= 0) return;
  hipLaunchKernelGGL(k_heads_seed, dim3(cdiv_h(h.N, 4)), dim3(kThreads), 0, s, h, H, g_ao, direct);
}

}  // namespace tn
