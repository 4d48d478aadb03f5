// Global thermostats of the device-resident MD loop (tn_md_thermo.hip): one thermostat per molecule acts on the molecule's kinetic
// energy through ONE scale factor alpha, after the closing kick of every step, for the full dt.  __host__ __device__:
// tests/md_thermo_host.hip compiles this header host-only, so the statements a GPU lane runs are the statements the host checker runs.
//
//   CSVR  stochastic velocity rescaling (Bussi, Donadio, Parrinello: J. Chem. Phys. 126, 014101, 2007; eq. A7), with
//         c = exp(-dt / tau), N = ndof, r = (N kT / 2) / (N K):
//             alpha^2 = (sqrt(c) + R1 sqrt(r (1 - c)))^2 + r (1 - c) S        (a sum of two squares: rounding cannot make it negative)
//         R1 a standard normal, S chi-square with N - 1 degrees of freedom: 2 Gamma((N - 1) / 2) for N - 1 even,
//         2 Gamma((N - 2) / 2) + R2^2 for N - 1 odd, R2^2 alone for N - 1 = 1 and 0 for N - 1 = 0.  The gamma deviate of shape a >= 1 is
//         Marsaglia and Tsang's (ACM TOMS 26, 363, 2000).
//   NHC   Nose-Hoover chain of length M (Martyna, Klein, Tuckerman: J. Chem. Phys. 97, 2635, 1992), propagated by the routine of
//         Martyna, Tuckerman, Tobias, Klein (Mol. Phys. 87, 1117, 1996) = Frenkel and Smit, Algorithm 30, whose delt / 2 is the h
//         below: `substeps` applications of U(h), h = dt / substeps.  Q_1 = N kT tau^2, Q_j = kT tau^2.
//
// K is the kinetic energy in the unit of the potential energy, ekin / force_scale.  Everything up to alpha is fp64 in the order
// written; alpha is rounded to fp32 ONCE, and every velocity scaling is then one md_mul under the rounding contract of tn_md_math.h.
//
// Random numbers: Philox4x32-10, key = the thermostat's seed, counter = (step lo, step hi, molecule, 3 + 256 draw).  Word 3 keeps the
// stream apart from the atoms' (0), the barostat's (1) and the exchange's (2).  Draw 0: R1 = xi_x, R2 = xi_y of normals3.  Draw
// j >= 1 is attempt j of the gamma deviate: x = xi_x, u = uniform_open(word 2) - word 2 does not enter xi_x.
#pragma once
#include "tn_md_math.h"

namespace tn_md {

constexpr int kThermoCsvr = 0, kThermoNhc = 1;  // TMDNET_THERMOSTAT_* of include/tmdnet_amd.h
constexpr int kThermoMaxChain = 8;
constexpr int kThermoGammaAttempts = 64;  // the method rejects under 5 % of its attempts: the bound never binds

// the four words of draw `draw` of molecule `mol` in the move that follows `step` completed steps
MD_FN void thermo_words(uint64_t seed, uint64_t step, uint32_t mol, uint32_t draw, uint32_t w[4]) {
  const uint32_t c[4] = {(uint32_t)step, (uint32_t)(step >> 32), mol, 3u + 256u * draw};
  const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  philox4x32_10(c, k, w);
}

// Gamma(a, 1), a >= 1, from draws 1, 2, ...  Returns 0 and the deviate, or 1 when every attempt was rejected.
MD_FN int thermo_gamma(double a, uint64_t seed, uint64_t step, uint32_t mol, double* out) {
  const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  for (int j = 1; j <= kThermoGammaAttempts; ++j) {
    uint32_t w[4];
    float xi[3];
    thermo_words(seed, step, mol, (uint32_t)j, w);
    normals3(w, xi);
    const double x = (double)xi[0], u = (double)uniform_open(w[2]);
    const double t = 1.0 + c * x, v = t * t * t;
    if (v > 0.0 && log(u) < 0.5 * x * x + d - d * v + d * log(v)) {
      *out = d * v;
      return 0;
    }
  }
  *out = 0.0;
  return 1;
}

// chi-square with n degrees of freedom, the sum of noises of Bussi's resamplekin; r2 is the second normal of draw 0
MD_FN int thermo_chi2(int64_t n, double r2, uint64_t seed, uint64_t step, uint32_t mol, double* out) {
  double g = 0.0;
  int bad = 0;
  if (n <= 0) {
    *out = 0.0;
  } else if (n == 1) {
    *out = r2 * r2;
  } else if (n % 2 == 0) {
    bad = thermo_gamma(0.5 * (double)n, seed, step, mol, &g);
    *out = 2.0 * g;
  } else {
    bad = thermo_gamma(0.5 * (double)(n - 1), seed, step, mol, &g);
    *out = 2.0 * g + r2 * r2;
  }
  return bad;
}

// One CSVR move of one molecule.  ekin = the kinetic-energy log row's entry (unit of m v^2), c = exp(-dt / tau).  Writes alpha^2 and K
// (fp64: the reservoir loses (alpha^2 - 1) K) and the fp32 factor; returns 0 when the move is usable, 1 when it is not.  A molecule
// without degrees of freedom or without kinetic energy is not scaled: alpha = 1, no Philox call.
MD_FN int csvr_move(float ekin, double force_scale, int32_t ndof, double kT, double c, uint64_t seed, uint64_t step, uint32_t mol,
                    double* a2_out, double* K_out, float* alpha32) {
  const double K = (double)ekin / force_scale;
  *K_out = K;
  if (ndof <= 0 || K == 0.0) {
    *a2_out = 1.0;
    *alpha32 = 1.f;
    return 0;
  }
  const double N = (double)ndof, Kbar = N * kT / 2.0, r = Kbar / (N * K);
  uint32_t w[4];
  float xi[3];
  thermo_words(seed, step, mol, 0u, w);
  normals3(w, xi);
  const double R1 = (double)xi[0], R2 = (double)xi[1];
  double S;
  const int bad = thermo_chi2((int64_t)ndof - 1, R2, seed, step, mol, &S);
  const double g = r * (1.0 - c);
  const double t = sqrt(c) + R1 * sqrt(g);
  const double a2 = t * t + g * S;
  const double alpha = sqrt(a2);
  *a2_out = a2;
  *alpha32 = (float)alpha;
  return bad || !isfinite(K) || !isfinite(a2) || !isfinite(*alpha32) || !(*alpha32 > 0.f);
}

// the force on thermostat j (0-based) of the chain: the particles' kinetic energy drives the first, thermostat j - 1 the others
MD_FN double nhc_force(int j, double K, double N, double kT, double Q1, double Qj, const double* v) {
  return j == 0 ? (2.0 * K - N * kT) / Q1 : ((j == 1 ? Q1 : Qj) * v[j - 1] * v[j - 1] - kT) / Qj;
}

// One Nose-Hoover-chain move of one molecule: `substeps` times U(h) on xi[M], v[M] (in place) and on K; alpha is the accumulated
// scale s.  Writes the energy the chain holds afterwards.  Returns 0 when the move is usable, 1 when it is not; the caller passes
// copies, so an unusable move leaves no trace.  ndof = 0 or K = 0: nothing is touched, alpha = 1, *reservoir is not written.
MD_FN int nhc_move(float ekin, double force_scale, int32_t ndof, double kT, double tau, double dt, int M, int substeps, double* xi,
                   double* v, double* reservoir, float* alpha32) {
  double K = (double)ekin / force_scale;
  if (ndof <= 0 || K == 0.0) {
    *alpha32 = 1.f;
    return 0;
  }
  const double N = (double)ndof, Qj = kT * tau * tau, Q1 = N * Qj, h = dt / (double)substeps;
  double s = 1.0;
  for (int n = 0; n < substeps; ++n) {
    v[M - 1] += nhc_force(M - 1, K, N, kT, Q1, Qj, v) * h / 2.0;
    for (int j = M - 2; j >= 0; --j) {
      const double e = exp(-v[j + 1] * h / 4.0);
      v[j] = (v[j] * e + nhc_force(j, K, N, kT, Q1, Qj, v) * h / 2.0) * e;
    }
    s = s * exp(-v[0] * h);
    K = K * exp(-2.0 * v[0] * h);
    for (int j = 0; j < M; ++j) xi[j] += v[j] * h;
    for (int j = 0; j < M - 1; ++j) {
      const double e = exp(-v[j + 1] * h / 4.0);
      v[j] = (v[j] * e + nhc_force(j, K, N, kT, Q1, Qj, v) * h / 2.0) * e;
    }
    v[M - 1] += nhc_force(M - 1, K, N, kT, Q1, Qj, v) * h / 2.0;
  }
  double E = 0.0;
  int bad = !isfinite(K) || !isfinite(s);
  for (int j = 0; j < M; ++j) {
    E += 0.5 * (j == 0 ? Q1 : Qj) * v[j] * v[j];
    bad |= !isfinite(xi[j]) || !isfinite(v[j]);
  }
  E += N * kT * xi[0];
  for (int j = 1; j < M; ++j) E += kT * xi[j];
  *reservoir = E;
  *alpha32 = (float)s;
  return bad || !isfinite(E) || !isfinite(*alpha32) || !(*alpha32 > 0.f);
}

// One move of either kind for molecule `mol`, on the molecule's own state: chain = (xi[M] | v[M]) and *reservoir are read, and
// written only when `commit` - pass 1 of k_md_thermo_factor asks whether the move is usable, pass 2 runs it again and keeps it.
MD_FN int thermo_move(int kind, float ekin, double force_scale, int32_t ndof, double kT, double tau, double dt, double c, int M,
                      int substeps, uint64_t seed, uint64_t step, uint32_t mol, double* chain, double* reservoir, int commit,
                      float* alpha32) {
  if (kind == kThermoCsvr) {
    double a2, K;
    const int bad = csvr_move(ekin, force_scale, ndof, kT, c, seed, step, mol, &a2, &K, alpha32);
    if (commit && !bad && a2 != 1.0) *reservoir = *reservoir - (a2 - 1.0) * K;
    return bad;
  }
  double x[kThermoMaxChain], v[kThermoMaxChain], E = *reservoir;
  for (int j = 0; j < M; ++j) {
    x[j] = chain[j];
    v[j] = chain[M + j];
  }
  const int bad = nhc_move(ekin, force_scale, ndof, kT, tau, dt, M, substeps, x, v, &E, alpha32);
  if (commit && !bad) {
    for (int j = 0; j < M; ++j) {
      chain[j] = x[j];
      chain[M + j] = v[j];
    }
    *reservoir = E;
  }
  return bad;
}

// v <- v alpha for one atom: one rounded product per component.  An atom of infinite mass (hk = 0) is no degree of freedom of the
// thermostat - it carries no kinetic energy - and keeps its velocity bit for bit.
MD_FN void thermo_scale(float v[3], float hk, float alpha) {
  if (hk == 0.f) return;
  for (int d = 0; d < 3; ++d) v[d] = md_mul(v[d], alpha);
}

}  // namespace tn_md
