// Per-atom MLP chains as single MFMA kernels (gfx950): a block owns a tile of 32 atoms, and the tile's activations go from one
// stage to the next through LDS - as the three bf16 planes of the exact 3-way split (tn_gemm_sb.hip), i.e. as the next stage's
// MFMA operand - instead of through [N, *] tensors in HBM between short launches.
//
// readout_fb: the readout, the head and their whole adjoint.  When forces are the only gradient wanted, the reverse seed of the
// head, g_ao[n, k] = w_n std O2[k] silu'(ao[n, k]), is a function of the atom's own row, so forward and reverse run back to back:
//
//   feat -> LayerNorm -> Lin, silu (= x) -> O1 -> head (e_n, g_ao) -> O1^T . silu'(al) -> Lin^T -> LayerNorm adjoint
//        -> adjoint of the invariants with X -> G
//
// (reference tensornet.py:398-402, models/utils.py:552-580, output_modules.py:43-73 and their autograd adjoints).  The seven
// launches it replaces (k_layernorm_fwd, two k_gemm_sb1 / k_gemm_sb1h each way, k_head_mol_sum, k_lnbwd_readout_bwd) moved nine
// intermediates through memory; here the kernel reads feat and X and writes G, x and the per-atom energies.
//
// gate_fwd / gate_bwd: the embedding's gate MLP (s0n -> LayerNorm -> L1, silu -> L2, silu = gates; tensornet.py:586-593) and its
// adjoint (g_a2 -> L2^T . silu'(a1) -> L1^T -> LayerNorm adjoint = g_s0n), each one launch instead of three.
//
// Arithmetic: every scalar formula is that of the kernel it replaces (two-pass LayerNorm, fast_silu in the GEMM epilogues, silu
// in the head, the LayerNorm adjoint and dquad of k_lnbwd_readout_bwd); every fp32 product is the six bf16 MFMA products of the
// 3-way split in the order 02 20 11 01 10 00.  Only summation orders differ.  All sums have a fixed order, no atomics.
//
// Layout of a product: the WEIGHTS are the MFMA's A operand (rows = output channels, read from the fragment-major image straight
// into registers, a few chunks ahead) and the ACTIVATIONS its B operand (columns = the 32 atoms, read from LDS), so an accumulator
// holds, per lane, ONE atom (lane & 31) and 4 x 4 consecutive output channels: four consecutive channels are half of a 16-byte
// operand piece of the next stage (one 8-byte LDS store per plane), and everything indexed by the atom (weight, atomref) is per lane.
#include <cstdlib>

#include "tn_chain.h"
#include "tn_common.h"
#include "tn_gemm_epi.h"
#include "tn_gemm_sb.h"

namespace tn {

constexpr int CH_RA = 32;         // atoms per tile
constexpr int CH_CS = 1024 + 32;  // bytes between the 16-channel chunks of a plane ([32 atoms][16 k] bf16 + 32: the 4-byte stores of
                                  // the LayerNorm stage - a wave = one atom, 64 lanes = 8 chunks - then hit 64 distinct banks)
constexpr int CH_D = 4;           // weight fragments in flight per wave (chunks ahead)

typedef float f2c __attribute__((ext_vector_type(2)));

// NACC accumulators (output channel blocks nb0 + j nbs of the image's nbt) over NKC chunks of 16 input channels
template <int NKC, int NACC>
struct ChainMma {
  static constexpr int STEPS = NKC * NACC;
  bf16x8 wr[CH_D][3];
  const uint16_t* wl;  // image + 8 * lane
  int nbt, nb0, nbs;
  __device__ __forceinline__ void fetch(int i) {
    const int kc = i / NACC, j = i % NACC;
    const uint16_t* p = wl + (int64_t)((kc * nbt + nb0 + j * nbs) * 3) * 512;
#pragma unroll
    for (int q = 0; q < 3; ++q) wr[i % CH_D][q] = *reinterpret_cast<const bf16x8*>(p + q * 512);
  }
  __device__ __forceinline__ void start(const uint16_t* img, int lane, int nbt_, int nb0_, int nbs_) {
    wl = img + lane * 8;
    nbt = nbt_;
    nb0 = nb0_;
    nbs = nbs_;
#pragma unroll
    for (int i = 0; i < CH_D; ++i)
      if (i < STEPS) fetch(i);
  }
  // act: plane 0 of the activations + this lane's piece (sb_piece(lane & 31, lane >> 5)); pstride: bytes between the planes
  __device__ __forceinline__ void run(const unsigned char* act, int pstride, floatx16 (&acc)[NACC]) {
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    // the scheduler is kept from moving anything across the end of a step (one chunk, one accumulator): left alone it sinks every
    // weight request down to its first use, and each step then waits for a whole round trip to the L2
    bf16x8 af[2][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) af[0][q] = *reinterpret_cast<const bf16x8*>(act + q * pstride);
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc) {
      if (kc + 1 < NKC) {
#pragma unroll
        for (int q = 0; q < 3; ++q) af[(kc + 1) & 1][q] = *reinterpret_cast<const bf16x8*>(act + q * pstride + (kc + 1) * CH_CS);
      }
#pragma unroll
      for (int j = 0; j < NACC; ++j) {
        const int i = kc * NACC + j;
#define CH_MMA(pa_, pw_) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wr[i % CH_D][pw_], af[kc & 1][pa_], acc[j], 0, 0, 0);
        CH_MMA(0, 2) CH_MMA(2, 0) CH_MMA(1, 1) CH_MMA(0, 1) CH_MMA(1, 0) CH_MMA(0, 0)
#undef CH_MMA
        if (i + CH_D < STEPS) fetch(i + CH_D);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
};

// four consecutive channels k .. k + 3 (k % 4 == 0) of atom r -> the three planes at `base`
__device__ __forceinline__ void chain_put4(unsigned char* base, int pstride, int r, int k, float v0, float v1, float v2, float v3) {
  uint32_t h0, m0, l0, h1, m1, l1;
  split2(v0, v1, h0, m0, l0);
  split2(v2, v3, h1, m1, l1);
  unsigned char* p = base + (k >> 4) * CH_CS + sb_piece(r, (k >> 3) & 1) + (k & 4) * 2;
  *reinterpret_cast<uint2*>(p) = make_uint2(h0, h1);
  *reinterpret_cast<uint2*>(p + pstride) = make_uint2(m0, m1);
  *reinterpret_cast<uint2*>(p + 2 * pstride) = make_uint2(l0, l1);
}

template <int F, int H>
__global__ __launch_bounds__(256, 2) void k_chain_readout_fb(ChainReadoutArgs a) {
  static_assert(F == 128, "a lane holds channels 2 lane, 2 lane + 1 of each of the three invariants");
  static_assert(H % 32 == 0 && H <= 128, "one wave per 32 head channels");
  constexpr int R = 3 * F, NKL = R / 16, NKF = F / 16, NKH = H / 16;
  constexpr int PL = NKL * CH_CS, PF = NKF * CH_CS, PH = NKH * CH_CS;  // plane sizes for 3F / F / H channels
  // LDS: the LayerNorm output's planes [0, 3 PL) are dead after the first product; x, g_ao and g_al follow one another inside that
  // range, and the fp32 rows of g_ln (the last product's output) alias its start once g_al has been read
  constexpr int O_X = 0, O_GAO = 3 * PF, O_GAL = O_GAO + 3 * PH, GLN_LD = R + 4, O_ES = 3 * PL;
  static_assert(O_GAL + 3 * PF <= 3 * PL && CH_RA * GLN_LD * 4 <= 3 * PL, "stage buffers alias the first stage's planes");
  __shared__ __attribute__((aligned(16))) unsigned char sm[3 * PL + CH_RA * 4];
  float* const gln = reinterpret_cast<float*>(sm);
  float* const es = reinterpret_cast<float*>(sm + O_ES);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = a.N, m0 = blockIdx.x * CH_RA;
  const int ra = lane & 31, hi = lane >> 5;      // product stages: this lane's atom of the tile, half of the lanes
  const int na = m0 + ra < N ? m0 + ra : N - 1;  // rows past the end: any valid row (their outputs are not stored)
  const bool oka = m0 + ra < N;
  const int frag = sb_piece(ra, hi);

  // ---------------------------------------------------------------- LayerNorm (a wave = one atom at a time, 8 atoms per wave)
  f2c fx[8][3];  // feat, then x_hat: kept for the adjoint
  float rs[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int n = m0 + wave * 8 + i;
    const float* p = a.feat + (int64_t)(n < N ? n : N - 1) * R + 2 * lane;
#pragma unroll
    for (int t = 0; t < 3; ++t) fx[i][t] = *reinterpret_cast<const f2c*>(p + t * F);
  }
  f2c lw[3], lb[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    lw[t] = *reinterpret_cast<const f2c*>(a.lnr_w + t * F + 2 * lane);
    lb[t] = *reinterpret_cast<const f2c*>(a.lnr_b + t * F + 2 * lane);
  }
  ChainMma<NKL, 1> mm1;
  mm1.start(a.Lin_fm, lane, F / 32, wave, 0);  // on their way while the rows are normalised
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 3; ++t) s += fx[i][t][0] + fx[i][t][1];
    const float mean = wave_sum(s) / R;
    float var = 0.f;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const float d0 = fx[i][t][0] - mean, d1 = fx[i][t][1] - mean;
      var += d0 * d0 + d1 * d1;
    }
    var = wave_sum(var) / R;
    rs[i] = 1.0f / sqrtf(var + 1e-5f);
    const int r = wave * 8 + i;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      fx[i][t] = (fx[i][t] - mean) * rs[i];
      const f2c y = fx[i][t] * lw[t] + lb[t];
      uint32_t h, m, l;
      split2(y[0], y[1], h, m, l);
      unsigned char* p = sm + (t * NKF + (lane >> 3)) * CH_CS + sb_piece(r, (lane >> 2) & 1) + (lane & 3) * 4;
      *reinterpret_cast<uint32_t*>(p) = h;
      *reinterpret_cast<uint32_t*>(p + PL) = m;
      *reinterpret_cast<uint32_t*>(p + 2 * PL) = l;
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- al = Lin(ln) + b, x = silu(al): wave = 32 of the F channels
  float al[16];
  {
    floatx16 acc[1];
    mm1.run(sm + frag, PL, acc);
    __syncthreads();  // every wave is done with the LayerNorm planes: x goes over them
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int k = 32 * wave + 8 * g + 4 * hi;
      const float4 b4 = *reinterpret_cast<const float4*>(a.bLin + k);
      const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
      float xv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        al[4 * g + e] = acc[0][4 * g + e] + bb[e];
        xv[e] = fast_silu(al[4 * g + e]);
      }
      if (oka) *reinterpret_cast<float4*>(a.x + (int64_t)na * F + k) = make_float4(xv[0], xv[1], xv[2], xv[3]);
      chain_put4(sm + O_X, PF, ra, k, xv[0], xv[1], xv[2], xv[3]);
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- ao = O1 x + b, head: e_n and g_ao = d e_n / d ao
  const float wgt = a.aw ? a.aw[a.perm ? a.perm[na] : na] : 1.0f;  // weight of this atom in the energy sum (tmdnet_set_atom_weights)
  float esum = 0.f;
  if (wave < H / 32) {
    ChainMma<NKF, 1> mm2;
    mm2.start(a.O1_fm, lane, H / 32, wave, 0);
    floatx16 acc[1];
    mm2.run(sm + O_X + frag, PF, acc);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int k = 32 * wave + 8 * g + 4 * hi;
      const float4 b4 = *reinterpret_cast<const float4*>(a.bO1 + k), o4 = *reinterpret_cast<const float4*>(a.O2 + k);
      const float bb[4] = {b4.x, b4.y, b4.z, b4.w}, oo[4] = {o4.x, o4.y, o4.z, o4.w};
      float gv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ao = acc[0][4 * g + e] + bb[e];
        esum += silu(ao) * oo[e];
        gv[e] = wgt * a.std_ * oo[e] * silu_grad(ao);
      }
      chain_put4(sm + O_GAO, PH, ra, k, gv[0], gv[1], gv[2], gv[3]);
    }
    esum += __shfl_xor(esum, 32, 64);  // the two halves of the lanes hold the two halves of the wave's 32 channels
    if (wave > 0 && lane < 32) es[(wave - 1) * CH_RA + ra] = esum;
  }
  ChainMma<NKH, 1> mm3;
  mm3.start(a.O1T_fm, lane, F / 32, wave, 0);
  __syncthreads();
  if (wave == 0 && lane < 32 && oka) {
    float s = esum;
#pragma unroll
    for (int w = 1; w < H / 32; ++w) s += es[(w - 1) * CH_RA + ra];
    float e = (s + a.bO2[0]) * a.std_;
    if (a.atomref) e += a.atomref[a.z[na]];
    a.ea[na] = wgt * e;
  }

  // ---------------------------------------------------------------- g_al = (O1^T g_ao) silu'(al)
  {
    floatx16 acc[1];
    mm3.run(sm + O_GAO + frag, PH, acc);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float gv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = acc[0][4 * g + e] * fast_silu_grad(al[4 * g + e]);
      chain_put4(sm + O_GAL, PF, ra, 32 * wave + 8 * g + 4 * hi, gv[0], gv[1], gv[2], gv[3]);
    }
  }
  f2c xr[3][9];  // ring of the rows of X of the last stage
  auto load_x = [&](int i) __attribute__((always_inline)) {
    const int n = m0 + wave * 8 + i;
    const float* p = a.X + (int64_t)(n < N ? n : N - 1) * 9 * F + 2 * lane;
#pragma unroll
    for (int c = 0; c < 9; ++c) xr[i % 3][c] = *reinterpret_cast<const f2c*>(p + c * F);
  };
  ChainMma<NKF, 3> mm4;
  mm4.start(a.LinT_fm, lane, R / 32, wave, 4);
  __syncthreads();

  // ---------------------------------------------------------------- g_ln = Lin^T g_al: wave = channel blocks w, w + 4, w + 8 of 3F
  {
    floatx16 acc[3];
    mm4.run(sm + O_GAL + frag, PF, acc);
    load_x(0);  // (not before the product: with them the kernel does not fit its registers)
    load_x(1);
    __syncthreads();  // every wave is done with g_al: the fp32 rows go over it
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(gln + ra * GLN_LD + 32 * (wave + 4 * j) + 8 * g + 4 * hi) =
            make_float4(acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]);
  }
  load_x(2);
  __syncthreads();

  // ---------------------------------------------------------------- LayerNorm adjoint, adjoint of the invariants (a wave = one atom)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = wave * 8 + i, n = m0 + r;
    f2c gw[3];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      gw[t] = *reinterpret_cast<const f2c*>(gln + r * GLN_LD + t * F + 2 * lane) * lw[t];
      s1 += gw[t][0] + gw[t][1];
      s2 += gw[t][0] * fx[i][t][0] + gw[t][1] * fx[i][t][1];
    }
    s1 = wave_sum(s1) / R;
    s2 = wave_sum(s2) / R;
    f2c gf[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) gf[t] = (gw[t] - s1 - fx[i][t] * s2) * rs[i];
    f2c o[9];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float u[9], dq[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) u[c] = xr[i % 3][c][j];
      dquad(u, dq);
#pragma unroll
      for (int c = 0; c < 9; ++c) o[c][j] = dq[c] * gf[type_of(c)][j];
    }
    if (i + 3 < 8) load_x(i + 3);
    if (n < N) {
      float* p = a.G + (int64_t)n * 9 * F + 2 * lane;
#pragma unroll
      for (int c = 0; c < 9; ++c) *reinterpret_cast<f2c*>(p + c * F) = o[c];
    }
  }
}

// ---- gate MLP of the embedding (reference tensornet.py:586-593): s0n -> LayerNorm -> L1, silu -> L2, silu
template <int F>
__global__ __launch_bounds__(256, 2) void k_chain_gate_fwd(ChainGateFwdArgs a) {
  static_assert(F == 128, "a lane holds channels 2 lane, 2 lane + 1 of the row");
  constexpr int NK1 = F / 16, NK2 = 2 * F / 16;
  constexpr int P1 = NK1 * CH_CS, P2 = NK2 * CH_CS, O_H = 3 * P1;  // planes of ln0 (F channels), then of h1 (2F)
  __shared__ __attribute__((aligned(16))) unsigned char sm[3 * P1 + 3 * P2];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = a.N, m0 = blockIdx.x * CH_RA;
  const int ra = lane & 31, hi = lane >> 5;
  const int na = m0 + ra < N ? m0 + ra : N - 1;
  const bool oka = m0 + ra < N;
  const int frag = sb_piece(ra, hi);

  // ---------------------------------------------------------------- LayerNorm (a wave = one atom at a time)
  f2c v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int n = m0 + wave * 8 + i;
    v[i] = *reinterpret_cast<const f2c*>(a.s0n + (int64_t)(n < N ? n : N - 1) * F + 2 * lane);
  }
  const f2c lw = *reinterpret_cast<const f2c*>(a.ln_w + 2 * lane), lb = *reinterpret_cast<const f2c*>(a.ln_b + 2 * lane);
  ChainMma<NK1, 2> mm1;
  mm1.start(a.L1_fm, lane, 2 * F / 32, wave, 4);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = wave * 8 + i, n = m0 + r;
    const float mean = wave_sum(v[i][0] + v[i][1]) / F;
    const float d0 = v[i][0] - mean, d1 = v[i][1] - mean;
    const float var = wave_sum(d0 * d0 + d1 * d1) / F;
    const float rs = 1.0f / sqrtf(var + 1e-5f);
    const f2c xh = (v[i] - mean) * rs;
    if (n < N) {
      *reinterpret_cast<f2c*>(a.xh0 + (int64_t)n * F + 2 * lane) = xh;
      if (lane == 0) a.rstd0[n] = rs;
    }
    const f2c y = xh * lw + lb;
    uint32_t h, m, l;
    split2(y[0], y[1], h, m, l);
    unsigned char* p = sm + (lane >> 3) * CH_CS + sb_piece(r, (lane >> 2) & 1) + (lane & 3) * 4;
    *reinterpret_cast<uint32_t*>(p) = h;
    *reinterpret_cast<uint32_t*>(p + P1) = m;
    *reinterpret_cast<uint32_t*>(p + 2 * P1) = l;
  }
  __syncthreads();

  // ---------------------------------------------------------------- a1 = L1 ln0 + b, h1 = silu(a1): wave = channel blocks w, w + 4 of 2F
  ChainMma<NK2, 3> mm2;
  {
    floatx16 acc[2];
    mm1.run(sm + frag, P1, acc);
    mm2.start(a.L2_fm, lane, 3 * F / 32, wave, 4);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k = 32 * (wave + 4 * j) + 8 * g + 4 * hi;
        const float4 b4 = *reinterpret_cast<const float4*>(a.bL1 + k);
        const float p0 = acc[j][4 * g] + b4.x, p1 = acc[j][4 * g + 1] + b4.y, p2 = acc[j][4 * g + 2] + b4.z, p3 = acc[j][4 * g + 3] + b4.w;
        if (oka) *reinterpret_cast<float4*>(a.a1 + (int64_t)na * 2 * F + k) = make_float4(p0, p1, p2, p3);
        chain_put4(sm + O_H, P2, ra, k, fast_silu(p0), fast_silu(p1), fast_silu(p2), fast_silu(p3));
      }
  }
  __syncthreads();

  // ---------------------------------------------------------------- a2 = L2 h1 + b, gates = silu(a2): wave = blocks w, w + 4, w + 8 of 3F
  {
    floatx16 acc[3];
    mm2.run(sm + O_H + frag, P2, acc);
    if (oka) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int k = 32 * (wave + 4 * j) + 8 * g + 4 * hi;
          const float4 b4 = *reinterpret_cast<const float4*>(a.bL2 + k);
          const float p0 = acc[j][4 * g] + b4.x, p1 = acc[j][4 * g + 1] + b4.y, p2 = acc[j][4 * g + 2] + b4.z, p3 = acc[j][4 * g + 3] + b4.w;
          *reinterpret_cast<float4*>(a.a2 + (int64_t)na * 3 * F + k) = make_float4(p0, p1, p2, p3);
          *reinterpret_cast<float4*>(a.gates + (int64_t)na * 3 * F + k) = make_float4(fast_silu(p0), fast_silu(p1), fast_silu(p2), fast_silu(p3));
        }
    }
  }
}

// ---- adjoint of the gate MLP: g_a2 -> L2^T . silu'(a1) -> L1^T -> LayerNorm adjoint (k_layernorm_bwd)
template <int F>
__global__ __launch_bounds__(256, 2) void k_chain_gate_bwd(ChainGateBwdArgs a) {
  static_assert(F == 128, "a lane holds channels 2 lane, 2 lane + 1 of the row");
  constexpr int NK3 = 3 * F / 16, NK2 = 2 * F / 16;
  constexpr int P3 = NK3 * CH_CS, P2 = NK2 * CH_CS;
  // LDS: the planes of g_a2 (3F channels); g_a1's (2F) go over their start once they have been read, the fp32 rows of g_ln0 behind
  constexpr int GL_LD = F + 4, O_GL = 3 * P2;
  static_assert(O_GL + CH_RA * GL_LD * 4 <= 3 * P3, "stage buffers alias the first stage's planes");
  __shared__ __attribute__((aligned(16))) unsigned char sm[3 * P3];
  float* const gl = reinterpret_cast<float*>(sm + O_GL);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = a.N, m0 = blockIdx.x * CH_RA;
  const int ra = lane & 31, hi = lane >> 5;
  const int na = m0 + ra < N ? m0 + ra : N - 1;
  const int frag = sb_piece(ra, hi);

  // ---------------------------------------------------------------- g_a2 -> planes (a wave = one atom at a time)
  ChainMma<NK3, 2> mm1;
  mm1.start(a.L2T_fm, lane, 2 * F / 32, wave, 4);
  {
    f2c v[8][3];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int n = m0 + wave * 8 + i;
      const float* p = a.g_a2 + (int64_t)(n < N ? n : N - 1) * 3 * F + 2 * lane;
#pragma unroll
      for (int t = 0; t < 3; ++t) v[i][t] = *reinterpret_cast<const f2c*>(p + t * F);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        uint32_t h, m, l;
        split2(v[i][t][0], v[i][t][1], h, m, l);
        unsigned char* p = sm + (t * (F / 16) + (lane >> 3)) * CH_CS + sb_piece(wave * 8 + i, (lane >> 2) & 1) + (lane & 3) * 4;
        *reinterpret_cast<uint32_t*>(p) = h;
        *reinterpret_cast<uint32_t*>(p + P3) = m;
        *reinterpret_cast<uint32_t*>(p + 2 * P3) = l;
      }
  }
  // this lane's part of a1 (the epilogue's operand): requested before the product
  float4 a1v[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) a1v[j][g] = *reinterpret_cast<const float4*>(a.a1 + (int64_t)na * 2 * F + 32 * (wave + 4 * j) + 8 * g + 4 * hi);
  __syncthreads();

  // ---------------------------------------------------------------- g_a1 = (L2^T g_a2) silu'(a1): wave = channel blocks w, w + 4 of 2F
  ChainMma<NK2, 1> mm2;
  {
    floatx16 acc[2];
    mm1.run(sm + frag, P3, acc);
    mm2.start(a.L1T_fm, lane, F / 32, wave, 0);
    __syncthreads();  // every wave is done with g_a2's planes: g_a1's go over them
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 p = a1v[j][g];
        chain_put4(sm, P2, ra, 32 * (wave + 4 * j) + 8 * g + 4 * hi, acc[j][4 * g] * fast_silu_grad(p.x), acc[j][4 * g + 1] * fast_silu_grad(p.y),
                   acc[j][4 * g + 2] * fast_silu_grad(p.z), acc[j][4 * g + 3] * fast_silu_grad(p.w));
      }
  }
  // operands of the LayerNorm adjoint: requested before the last product
  f2c xh[8];
  float rs[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int n = m0 + wave * 8 + i, nc = n < N ? n : N - 1;
    xh[i] = *reinterpret_cast<const f2c*>(a.xh0 + (int64_t)nc * F + 2 * lane);
    rs[i] = a.rstd0[nc];
  }
  const f2c lw = *reinterpret_cast<const f2c*>(a.ln_w + 2 * lane);
  __syncthreads();

  // ---------------------------------------------------------------- g_ln0 = L1^T g_a1: wave = 32 of the F channels
  {
    floatx16 acc[1];
    mm2.run(sm + frag, P2, acc);
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(gl + ra * GL_LD + 32 * wave + 8 * g + 4 * hi) =
          make_float4(acc[0][4 * g], acc[0][4 * g + 1], acc[0][4 * g + 2], acc[0][4 * g + 3]);
  }
  __syncthreads();

  // ---------------------------------------------------------------- LayerNorm adjoint (a wave = one atom at a time)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = wave * 8 + i, n = m0 + r;
    const f2c gw = *reinterpret_cast<const f2c*>(gl + r * GL_LD + 2 * lane) * lw;
    const float s1 = wave_sum(gw[0] + gw[1]) / F;
    const float s2 = wave_sum(gw[0] * xh[i][0] + gw[1] * xh[i][1]) / F;
    if (n < N) *reinterpret_cast<f2c*>(a.g_s0n + (int64_t)n * F + 2 * lane) = (gw - s1 - xh[i] * s2) * rs[i];
  }
}

static bool chain_off() {
  static const bool off = getenv("TMDNET_NO_SPLIT_BF16") != nullptr;  // developer switch: fp32 MFMA everywhere, no split-bf16 kernel
  return off;
}
bool chain_gate_shape_ok(int F) { return !chain_off() && F == 128; }

int launch_chain_gate_fwd(const ChainGateFwdArgs& a, int F, hipStream_t s) {
  if (!chain_gate_shape_ok(F)) return (int)hipErrorInvalidValue;
  if (a.N <= 0) return 0;
  hipLaunchKernelGGL((k_chain_gate_fwd<128>), dim3((a.N + CH_RA - 1) / CH_RA), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}
int launch_chain_gate_bwd(const ChainGateBwdArgs& a, int F, hipStream_t s) {
  if (!chain_gate_shape_ok(F)) return (int)hipErrorInvalidValue;
  if (a.N <= 0) return 0;
  hipLaunchKernelGGL((k_chain_gate_bwd<128>), dim3((a.N + CH_RA - 1) / CH_RA), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

bool chain_readout_shape_ok(int F, int H) {
  return !chain_off() && F == 128 && H == 64;
}

int launch_chain_readout_fb(const ChainReadoutArgs& a, int F, int H, hipStream_t s) {
  if (!chain_readout_shape_ok(F, H)) return (int)hipErrorInvalidValue;
  if (a.N <= 0) return 0;
  hipLaunchKernelGGL((k_chain_readout_fb<128, 64>), dim3((a.N + CH_RA - 1) / CH_RA), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace tn
