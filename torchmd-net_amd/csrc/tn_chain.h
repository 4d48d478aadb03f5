// Per-atom MLP chains as single MFMA kernels over a tile of atoms that never leaves the CU (tn_chain.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tn {

// readout + head + their whole adjoint (forces only: the reverse seed of the head is a function of the atom's own row):
//   feat -> LayerNorm -> Lin, silu -> O1 -> head (e_n, g_ao) -> O1^T . silu'(al) -> Lin^T -> LayerNorm adjoint -> invariants' adjoint
struct ChainReadoutArgs {
  const float* feat;       // [N, 3F]    invariants of X (k_readout_feat / the update epilogue of k_tlin9)
  const float* X;          // [N, 9, F]  last layer's X
  float* G;                // [N, 9, F]  out: d E / d X
  float* x;                // [N, F]     out: silu(Lin(LayerNorm(feat)))  (debug tensor "x")
  float* ea;               // [N]        out: per-atom energies, atomref and atom weight applied (k_head_energy)
  const float *lnr_w, *lnr_b, *bLin, *bO1, *O2, *bO2;
  const uint16_t *Lin_fm, *LinT_fm, *O1_fm, *O1T_fm;  // fragment-major split images (split_weight_fm) of Lin [F][3F], LinT [3F][F], O1 [H][F], O1T [F][H]
  const float* atomref;    // [max_z] or null
  const int64_t* z;        // [N]
  const float* aw;         // atom weights (tmdnet_set_atom_weights) or null
  const int* perm;         // engine order -> caller order of aw, or null
  float std_;
  int N;
};

// gate MLP of the embedding, forward: s0n -> LayerNorm -> L1, silu -> L2, silu = gates.  Written: what the reverse pass and the gate
// epilogues of k_tlin9 read (x_hat and 1/sigma of the LayerNorm, both pre-activations, the gates); ln0 and h1 never reach memory
struct ChainGateFwdArgs {
  const float* s0n;        // [N, F]
  float *xh0, *rstd0;      // [N, F], [N]
  float *a1, *a2, *gates;  // [N, 2F], [N, 3F], [N, 3F]
  const float *ln_w, *ln_b, *bL1, *bL2;
  const uint16_t *L1_fm, *L2_fm;  // fragment-major split images of L1 [2F][F], L2 [3F][2F]
  int N;
};
// ... and its adjoint: g_a2 -> L2^T . silu'(a1) -> L1^T -> LayerNorm adjoint = g_s0n; g_a1 and g_ln0 never reach memory
struct ChainGateBwdArgs {
  const float *g_a2, *a1, *xh0, *rstd0, *ln_w;
  float* g_s0n;                     // [N, F]
  const uint16_t *L2T_fm, *L1T_fm;  // images of L2T [2F][3F], L1T [F][2F]
  int N;
};

bool chain_readout_shape_ok(int F, int H);  // shapes the kernels are instantiated for
bool chain_gate_shape_ok(int F);
int launch_chain_readout_fb(const ChainReadoutArgs& a, int F, int H, hipStream_t s);
int launch_chain_gate_fwd(const ChainGateFwdArgs& a, int F, hipStream_t s);
int launch_chain_gate_bwd(const ChainGateBwdArgs& a, int F, hipStream_t s);

}  // namespace tn
