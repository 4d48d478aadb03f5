// Per-atom arithmetic of the device-resident MD loop (tn_md.hip): velocity-Verlet half-kick and drift, the Langevin O step, the
// kinetic-energy term, and the Philox4x32-10 / Box-Muller noise.  __host__ __device__: tests/md_host.hip compiles this header
// host-only, so the statements a GPU lane runs are the statements the host checker runs.
//
// Rounding contract.  Every product and every sum below is ONE round-to-nearest-even fp32 operation, in the order written:
// md_mul / md_add wrap __fmul_rn / __fadd_rn.  The HIP headers define those intrinsics as plain `x * y` / `x + y`, which the
// device compiler (-ffp-contract=fast, applied after inlining whatever pragma the body carries) fuses into an FMA with the
// addition that consumes the product - so on the device md_mul passes its result through an empty asm statement, which the
// optimiser cannot see through: the product exists, rounded, in a register before anything adds to it.  (It emits no
// instruction.)  No reassociation: nothing here is compiled with fast-math.  A trajectory without a thermostat is therefore a fixed
// sequence of IEEE operations that any fp32 mirror which multiplies, rounds, adds, rounds reproduces bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MD_FN __host__ __device__ inline
#else
#define MD_FN inline
#endif

namespace tn_md {

MD_FN float md_mul(float a, float b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
  float p = __fmul_rn(a, b);
  asm volatile("" : "+v"(p));
  return p;
#else
  return a * b;
#endif
}

MD_FN float md_add(float a, float b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(a, b);
#else
  return a + b;
#endif
}

// B: v <- v + hk * F      (hk = dt force_scale / (2 m); m = inf: hk = 0 and the atom keeps its velocity bit for bit)
MD_FN float kick(float v, float hk, float f) { return md_add(v, md_mul(hk, f)); }

// A: x <- x + dt * v      (unwrapped positions)
MD_FN float drift(float x, float dt, float v) { return md_add(x, md_mul(dt, v)); }

// O: v <- c1 * v + (c2 * sigma) * xi      (c1 = exp(-gamma dt), c2 = sqrt(1 - c1^2), sigma = sqrt(kT force_scale / m))
MD_FN float ou(float v, float c1, float c2, float sigma, float xi) { return md_add(md_mul(c1, v), md_mul(md_mul(c2, sigma), xi)); }

// kinetic energy of one atom, (0.5 m) * ((vx vx + vy vy) + vz vz), in the unit of m v^2.  An atom of infinite mass is frozen
// (hk = sigma = 0) and contributes nothing, whatever velocity it was given.
MD_FN float kinetic(float m, float vx, float vy, float vz) {
  if (isinf(m)) return 0.f;
  const float s = md_add(md_add(md_mul(vx, vx), md_mul(vy, vy)), md_mul(vz, vz));
  return md_mul(md_mul(0.5f, m), s);
}

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) -------------------------
// counter c[4], key k[2] -> four 32-bit words.  Ten rounds; the key is bumped by the Weyl constants between rounds.
MD_FN void philox4x32_10(const uint32_t c[4], const uint32_t k[2], uint32_t out[4]) {
  uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 32 random bits -> u = ((r >> 8) + 0.5) 2^-24 evaluated in fp32.  Below one half ((r >> 8) < 2^23) the sum has at most 24
// significant bits and u is the exact real number; above, the half is the 25th bit and the sum rounds to nearest even, so u lies
// in [2^-25, 1]: never 0 (the logarithm is finite, |xi| <= 5.89), and 1 only for r >> 8 = 2^24 - 1, where the radius is 0.
MD_FN float uniform_open(uint32_t r) { return md_mul(md_add((float)(r >> 8), 0.5f), 5.9604644775390625e-08f); }

// Box-Muller on the four words of one Philox call: words 0 / 1 -> (xi_x, xi_y), words 2 / 3 -> xi_z (its sine partner is
// dropped).  The accurate logf / cosf / sinf, not the fast intrinsics.
MD_FN void normals3(const uint32_t w[4], float xi[3]) {
  const float two_pi = 6.283185307179586f;
  const float r0 = sqrtf(md_mul(-2.f, logf(uniform_open(w[0])))), a0 = md_mul(two_pi, uniform_open(w[1]));
  const float r1 = sqrtf(md_mul(-2.f, logf(uniform_open(w[2])))), a1 = md_mul(two_pi, uniform_open(w[3]));
  xi[0] = md_mul(r0, cosf(a0));
  xi[1] = md_mul(r0, sinf(a0));
  xi[2] = md_mul(r1, cosf(a1));
}

// the noise of atom `atom` (the CALLER's index) in the O step that follows `step` completed steps:
// key = the 64-bit seed, counter = (step lo, step hi, atom, 0)
MD_FN void langevin_noise(uint64_t seed, uint64_t step, uint32_t atom, float xi[3]) {
  const uint32_t c[4] = {(uint32_t)step, (uint32_t)(step >> 32), atom, 0u};
  const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  philox4x32_10(c, k, w);
  normals3(w, xi);
}

// The closing half of a step for one atom: B, then O when `thermostat`, then the kinetic-energy term.  v[3] in / out.
MD_FN float close_step(float v[3], const float f[3], float hk, float m, int thermostat, float c1, float c2, float sigma, uint64_t seed,
                       uint64_t step, uint32_t atom) {
  for (int d = 0; d < 3; ++d) v[d] = kick(v[d], hk, f[d]);
  if (thermostat) {
    float xi[3];
    langevin_noise(seed, step, atom, xi);
    for (int d = 0; d < 3; ++d) v[d] = ou(v[d], c1, c2, sigma, xi[d]);
  }
  return kinetic(m, v[0], v[1], v[2]);
}

// The opening half of a step for one atom: B, A.  The fused launch of tn_md.hip runs close_step and then this, with the same
// force: the two kicks stay two additions.
MD_FN void open_step(float x[3], float v[3], const float f[3], float hk, float dt) {
  for (int d = 0; d < 3; ++d) {
    v[d] = kick(v[d], hk, f[d]);
    x[d] = drift(x[d], dt, v[d]);
  }
}

// ---- isotropic stochastic cell rescaling (Bernetti, Bussi: J. Chem. Phys. 153, 114107, 2020), one barostat per molecule ---------
// First order in the log-volume: d = -a (P0 - P) + sqrt(2 kT a / V) xi with a = compressibility dt / tau; the box and the positions
// are scaled by mu = exp(d / 3), the velocities by nu = exp(-d / 3).  Everything up to mu and nu is fp64, in the order written; the
// two factors are rounded to fp32 once, and every scaling is then ONE md_mul, subject to the rounding contract above.

// V = |det box| of a row-major 3 x 3 box, fp32 entries widened
MD_FN double box_volume(const float b[9]) {
  const double b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3], b4 = b[4], b5 = b[5], b6 = b[6], b7 = b[7], b8 = b[8];
  return fabs((b0 * (b4 * b8 - b5 * b7) - b1 * (b3 * b8 - b5 * b6)) + b2 * (b3 * b7 - b4 * b6));
}

// P = (2 K + tr W) / (3 V): K the kinetic energy in the unit of the potential energy, W = -dE/d eps (tr W = -3 V dE/dV)
MD_FN double baro_pressure(double V, double K, const float W[9]) {
  return (2.0 * K + (((double)W[0] + (double)W[4]) + (double)W[8])) / (3.0 * V);
}

// the noise of molecule `mol` in the barostat move that follows `step` completed steps: xi[0] of normals3 on one Philox call,
// key = the 64-bit seed, counter = (step lo, step hi, mol, 1) - word 3 keeps the stream apart from the atoms' (langevin_noise: 0)
MD_FN double baro_noise(uint64_t seed, uint64_t step, uint32_t mol) {
  const uint32_t c[4] = {(uint32_t)step, (uint32_t)(step >> 32), mol, 1u};
  const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  float xi[3];
  philox4x32_10(c, k, w);
  normals3(w, xi);
  return (double)xi[0];
}

// One barostat move of one molecule.  ekin = sum of 0.5 m v^2 in the unit of m v^2 (the kinetic-energy log row).  Writes the volume
// before the move, the pressure and the two fp32 factors; returns 0 when the move is usable, 1 when it is not (V = 0, or anything
// not finite on the way: a NaN in the virial, a box about to vanish or explode).  kT = 0: no Philox call, weak coupling.
MD_FN int baro_move(const float box[9], const float W[9], float ekin, double force_scale, double P0, double kT, double a,
                    uint64_t seed, uint64_t step, uint32_t mol, double* V_out, double* P_out, float* mu32, float* nu32) {
  const double V = box_volume(box);
  const double P = baro_pressure(V, (double)ekin / force_scale, W);
  double d = -a * (P0 - P);
  if (kT > 0.0) d = d + sqrt(2.0 * kT * a / V) * baro_noise(seed, step, mol);
  const double mu = exp(d / 3.0), nu = exp(-d / 3.0);
  *V_out = V;
  *P_out = P;
  *mu32 = (float)mu;
  *nu32 = (float)nu;
  return !(V > 0.0) || !isfinite(d) || !isfinite(*mu32) || !isfinite(*nu32) || !(*mu32 > 0.f) || !(*nu32 > 0.f);
}

// scale the nine entries of a box, or the position / velocity of one atom: one rounded product each
MD_FN void scale3(float x[3], float s) {
  for (int d = 0; d < 3; ++d) x[d] = md_mul(x[d], s);
}

}  // namespace tn_md
