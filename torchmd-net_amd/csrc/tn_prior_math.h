// Pair priors (tn_prior.hip): the ZBL screened nuclear repulsion and the DFT-D2 dispersion tail, parameter-free pair potentials of
// pos, z, batch and box that are ADDED to the model's energies, forces and virial behind the engine call.  __host__ __device__:
// tests/prior_host.hip compiles this header host-only, so the statements a GPU lane runs are the statements the host checker runs.
//
//   ZBL  (Ziegler, Biersack, Littmark 1985, eqs. 9, 10; reference priors/zbl.py:83-112), r in the caller's length unit:
//            a   = 0.8854 a_0 / (Z_i^0.23 + Z_j^0.23),   a_0 = 5.29177210903e-11 m
//            d   = r distance_scale / a
//            phi = 0.1818 e^{-3.2 d} + 0.5099 e^{-0.9423 d} + 0.2802 e^{-0.4029 d} + 0.02817 e^{-0.2016 d}
//            u   = (2.30707755e-28 / energy_scale / distance_scale) phi C(r) Z_i Z_j / r,   C = cosine cutoff on [0, cutoff)
//   D2   (Grimme 2006; reference priors/d2.py:163-201), R = r distance_scale 1e9 in nm:
//            u   = - s_6 sqrt(C6_i C6_j) / R^6 / (1 + e^{-d (R / (Rr_i + Rr_j) - 1)}) / (energy_scale N_A),   d = 20, s_6 = 1
//        The cutoff is hard: du/dr carries no term from it.
//
// The constants that depend on the unit scales only are derived ONCE in fp64 (zbl_constants / d2_constants) and rounded to fp32;
// the per-species values Z, Z^0.23, sqrt(C6), Rr arrive as fp32 tables.  Everything per pair is fp32 in the order written.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PRIOR_FN __host__ __device__ inline
#else
#define PRIOR_FN inline
#endif

namespace tn_prior {

constexpr int kMaxMoleculeAtoms = 32768;  // the pass is brute force inside a molecule: larger molecules wait for a cell list
constexpr double kBohr = 5.29177210903e-11, kZblEnergy = 2.30707755e-28, kAvogadro = 6.02214076e23;
constexpr float kD2Steepness = 20.0f, kD2S6 = 1.0f;

struct ZblConst {
  float cutoff;  // caller's length unit
  float ka;      // distance_scale / (0.8854 a_0):  d = r ka (Z_i^0.23 + Z_j^0.23)
  float ke;      // 2.30707755e-28 / energy_scale / distance_scale
};
struct D2Const {
  float cutoff;  // caller's length unit
  float snm;     // distance_scale 1e9:  R = r snm
  float ke;      // s_6 / (energy_scale N_A)
};

PRIOR_FN ZblConst zbl_constants(double cutoff, double distance_scale, double energy_scale) {
  ZblConst c;
  c.cutoff = (float)cutoff;
  c.ka = (float)(distance_scale / (0.8854 * kBohr));
  c.ke = (float)(kZblEnergy / energy_scale / distance_scale);
  return c;
}
PRIOR_FN D2Const d2_constants(double cutoff, double distance_scale, double energy_scale) {
  D2Const c;
  c.cutoff = (float)cutoff;
  c.snm = (float)(distance_scale * 1e9);
  c.ke = (float)((double)kD2S6 / (energy_scale * kAvogadro));
  return c;
}

// u(r) and du/dr of one ZBL pair, 0 < r < cutoff.  z23 = Z_i^0.23 + Z_j^0.23, zz = Z_i Z_j.
PRIOR_FN void zbl_pair(float r, float z23, float zz, const ZblConst& c, float* u, float* du) {
  const float PI = 3.14159265358979323846f;
  const float s = c.ka * z23;  // d = r s
  const float d = r * s;
  const float e0 = 0.1818f * expf(-3.2f * d), e1 = 0.5099f * expf(-0.9423f * d), e2 = 0.2802f * expf(-0.4029f * d),
              e3 = 0.02817f * expf(-0.2016f * d);
  const float phi = e0 + e1 + e2 + e3;
  const float dphi = -(3.2f * e0 + 0.9423f * e1 + 0.4029f * e2 + 0.2016f * e3) * s;  // d phi / d r
  const float k = PI / c.cutoff;
  const float cut = 0.5f * (cosf(r * k) + 1.0f), dcut = -0.5f * sinf(r * k) * k;
  const float ir = 1.0f / r, pre = c.ke * zz * ir;
  *u = pre * phi * cut;
  *du = pre * (dphi * cut + phi * dcut - phi * cut * ir);
}

// u(r) and du/dr of one D2 pair, 0 < r < cutoff.  c6 = sqrt(C6_i) sqrt(C6_j) [J/mol nm^6], rr = Rr_i + Rr_j [nm].
PRIOR_FN void d2_pair(float r, float c6, float rr, const D2Const& c, float* u, float* du) {
  const float R = r * c.snm;
  const float iR = 1.0f / R, iR2 = iR * iR, iR6 = iR2 * iR2 * iR2;
  const float irr = 1.0f / rr;
  const float t = expf(-kD2Steepness * (R * irr - 1.0f));  // f = 1 / (1 + t),  df/dR = d t / (rr (1 + t)^2)
  const float f = 1.0f / (1.0f + t);
  const float df = kD2Steepness * irr * t * f * f;
  const float pre = -c.ke * c6 * iR6;
  *u = pre * f;
  *du = pre * (df - 6.0f * iR * f) * c.snm;
}

// the pair test of both priors, on the squared distance
PRIOR_FN bool in_cutoff(float d2, float cutoff) { return d2 > 0.0f && d2 < cutoff * cutoff; }

}  // namespace tn_prior
