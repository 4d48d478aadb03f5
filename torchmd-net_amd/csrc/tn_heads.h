// Property heads (DipoleMoment, ElectronicSpatialExtent on TensorNet and the Equivariant Transformer, EquivariantVectorOutput):
// molecule reductions and reverse seeds (tn_heads.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "tn_kernels.h"

namespace tn {

enum { TN_HEAD_SCALAR = 0, TN_HEAD_DIPOLE = 1, TN_HEAD_SPATIAL_EXTENT = 2, TN_HEAD_VECTOR = 3 };

struct HeadArgs {
  int kind;                 // TN_HEAD_DIPOLE, TN_HEAD_SPATIAL_EXTENT or TN_HEAD_VECTOR
  int N, B;
  const float* pos;         // [N,3] caller's positions, caller's atom order
  const int* perm;          // engine index -> caller index (cell list), or null
  const int64_t* z;         // [N] engine order
  const int64_t* batch;     // [N] engine order
  const float* mass;        // [n_mass] atomic masses (state-dict buffer output_model.atomic_mass); null: vector output (no masses)
  int n_mass;
  const float* q;           // [N] head output per atom, times std (k_head_energy), engine order; null: vector output
  const float* gate;        // [N] Equivariant Transformer, dipole / vector: gate of the second gated block, or null
  const float* vq2s;        // [N,3] ... and std * (its vec2_proj of the vector features): the atom's vector is gate * vq2s
  float mean, std;
  float* y;                 // [B] ([B,3] for the vector output)
  float* state;             // [B,8] M, c, Q, u (dipole; (1,1,1) vector) / sum q d (spatial extent); null: no forces
};

struct HeadBuffers {
  int S;                    // slices per molecule (1: one block per molecule)
  float *state, *part1, *part2, *direct;
  float *gate, *vq2s, *gv;  // Equivariant Transformer heads with a vector: [N], [N,3], [N,3] (d y / d v_i times the gate)
};

int heads_slices(int64_t N, int64_t B);
// sub-buffers of `base` (null: sizes only); *bytes = what they take
HeadBuffers carve_heads(void* base, int64_t N, int64_t B, size_t* bytes);
// y (and the per-molecule state when h.state is set)
void launch_heads_reduce(const Graph& g, const HeadArgs& h, const HeadBuffers& hb, hipStream_t s);
// g_ao [N,H] rows scaled by d y / d q_i; direct [N,3] = d y / d r_i at fixed q (engine order)
void launch_heads_seed(const HeadArgs& h, int H, float* g_ao, float* direct, hipStream_t s);
// Equivariant Transformer, second gated block of the dipole / vector heads: gate_i = silu(pre2_i) . Wn2[1] + bn2[1] and
// vq2s_i = std * vq_i W22^T ([N,3]) - the block's vector output is v_i = gate_i vq2s_i / std (reference utils.py GatedEquivariantBlock)
void launch_et_vout(int N, int F2, const float* pre2, const float* Wn2, const float* bn2, const float* vq, const float* W22, float std,
                    float* gate, float* vq2s, hipStream_t s);
// the seeds of the dipole / vector heads on the Equivariant Transformer: g_pre2 [N,F2] (in: std Wn2[0] silu'(pre2) for the dipole,
// from k_head_energy; out: d y / d pre2), gv [N,3] = d y / d v_i * gate_i, direct [N,3] as launch_heads_seed
void launch_et_heads_seed(const HeadArgs& h, int F2, const float* pre2, const float* Wn2, float* g_pre2, float* gv, float* direct,
                          hipStream_t s);
// g_vq[i, c, :] += gv[i, c] W22   (the vector output's path into block 1)
void launch_et_gvq_add(int N, int F2, const float* gv, const float* W22, float* g_vq, hipStream_t s);

}  // namespace tn
