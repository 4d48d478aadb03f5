// Anisotropic and semi-isotropic stochastic cell rescaling of the device-resident MD loop (tn_md_cell.hip), one barostat per
// molecule: the move of the isotropic barostat of tn_md_math.h with a 3 x 3 matrix in the exponent.  __host__ __device__:
// tests/md_cell_host.hip compiles this header host-only, so the statements a GPU lane runs are the statements the host checker runs.
//
// After the closing half of a step (B, [O]), in fp64, row vectors (x -> x mu, box -> box mu), h = box_m:
//     V   = |det h|
//     Kt  = sum over the atoms of 0.5 m v_a v_b / force_scale                   (3 x 3, symmetric)
//     P   = (2 Kt + W) / V                                                      (W as the evaluation returns it, not symmetrised)
//     a   = compressibility dt / tau
//     D_f = -(a / 3) (P0 I - P) + sqrt(2 kT a / (3 V)) Xi                       (Xi: nine independent standard normals)
//     D   = Pi(D_f);    mu = exp(D);    nu = exp(-D^T)                          (matrix exponentials)
// Pi is the Frobenius-orthogonal projection onto the coupling's subspace: the identity (kCellAnisotropic), the diagonal
// (kCellDiagonal), or the diagonal with the two entries other than `axis` replaced by their mean (kCellSemiIsotropic).  This is
// the anisotropic scheme of Bernetti and Bussi (J. Chem. Phys. 153, 114107, 2020) written in the exponent: the Ito term of exp
// cancels the paper's + kT / V, so -(a / 3) (P0 - P) is all the drift.  In every mode tr D is distributed as the d of baro_move.
//
// Lower-triangular box (kCellAnisotropic only; the neighbour search and the minimum image read one).  h' = h mu is factored by
// Gram-Schmidt on its rows, top down, q2 = q0 x q1: h' = L Q, L lower triangular with a positive diagonal, and the whole system is
// rotated by Q^T: box <- L, x <- x (mu Q^T), v <- v (nu Q^T), F <- F Q^T.  In the two diagonal modes Q = I by construction: no
// factorisation, the matrices are diagonal (their entries are scalar exponentials) and the forces are left alone.
//
// Rounding contract.  Mx = mu Q^T, Mv = nu Q^T, Mf = Q^T and the new box are rounded to fp32 ONCE; every per-atom component is then
// ((x0 M0b) + (x1 M1b)) + (x2 M2b), each product and each sum one rounded fp32 operation (md_mul / md_add of tn_md_math.h) in that
// order - ONE product x_b M_bb in the diagonal modes.
//
// Random numbers: three Philox4x32-10 calls per molecule and step, key = the barostat's seed, counter = (step lo, step hi,
// molecule, 4 + r); row r of Xi is normals3 of call r.  Word 3 = 4, 5, 6 keeps the streams apart from the atoms' (0), the isotropic
// barostat's (1), the exchange's (2) and the global thermostats' (3 + 256 draw: tn_md_thermo_math.h).
#pragma once
#include "tn_md_math.h"

namespace tn_md {

constexpr int kCellAnisotropic = 0, kCellDiagonal = 1, kCellSemiIsotropic = 2;  // TMDNET_CELL_* of include/tmdnet_amd.h
constexpr uint32_t kCellNoiseTag = 4u;  // counter word 3 of row r of Xi: kCellNoiseTag + r

// C = A B, row-major 3 x 3 (C must not alias A or B)
MD_FN void mat3_mul(const double A[9], const double B[9], double C[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

MD_FN double mat3_det(const double b[9]) {
  return (b[0] * (b[4] * b[8] - b[5] * b[7]) - b[1] * (b[3] * b[8] - b[5] * b[6])) + b[2] * (b[3] * b[7] - b[4] * b[6]);
}

// E = exp(A): A is scaled by 2^-s so that its max-row-sum norm is at most 2^-4, a Taylor series to degree 8 in Horner form
// (truncation about (2^-4)^9 / 9! = 4e-17), then s squarings.  s is bounded, so a norm that is not finite ends the loop too (the
// caller has flagged the move by then).
MD_FN void mat3_exp(const double A[9], double E[9]) {
  double norm = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double r = (fabs(A[3 * i]) + fabs(A[3 * i + 1])) + fabs(A[3 * i + 2]);
    norm = r > norm ? r : norm;
  }
  int s = 0;
  double scale = 1.0;
  while (norm > 0.0625 && s < 64) {
    norm *= 0.5;
    scale *= 0.5;
    ++s;
  }
  double B[9], T[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    B[i] = A[i] * scale;
    E[i] = (i % 4 == 0) ? 1.0 : 0.0;
  }
  for (int k = 8; k >= 1; --k) {  // E <- I + B E / k
    mat3_mul(B, E, T);
    const double inv = 1.0 / (double)k;
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = ((i % 4 == 0) ? 1.0 : 0.0) + T[i] * inv;
  }
  for (int k = 0; k < s; ++k) {
    mat3_mul(E, E, T);
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = T[i];
  }
}

// the kinetic-tensor term of one atom in fp64, the six independent entries xx, xy, xz, yy, yz, zz of 0.5 m v_a v_b in the unit of
// m v^2.  An atom of infinite mass is frozen and contributes nothing (as tn_md_math.h: kinetic).
MD_FN void cell_ktensor_term(float m, const float v[3], double t[6]) {
  const double hm = isinf(m) ? 0.0 : 0.5 * (double)m;
  const double x = isinf(m) ? 0.0 : (double)v[0], y = isinf(m) ? 0.0 : (double)v[1], z = isinf(m) ? 0.0 : (double)v[2];
  t[0] = hm * (x * x);
  t[1] = hm * (x * y);
  t[2] = hm * (x * z);
  t[3] = hm * (y * y);
  t[4] = hm * (y * z);
  t[5] = hm * (z * z);
}

// row r of Xi of molecule `mol` in the move that follows `step` completed steps
MD_FN void cell_noise_row(uint64_t seed, uint64_t step, uint32_t mol, uint32_t r, float xi[3]) {
  const uint32_t c[4] = {(uint32_t)step, (uint32_t)(step >> 32), mol, kCellNoiseTag + r};
  const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  philox4x32_10(c, k, w);
  normals3(w, xi);
}

// what one move yields.  V, P, D, mu, nu, L, Q are fp64 (L, Q: the factorisation of h mu; the identity rotation and h mu itself in
// the diagonal modes); Mx | Mv | Mf and box are the four fp32 objects of the rounding contract.
struct CellMove {
  double V, P[9], D[9], mu[9], nu[9], L[9], Q[9];
  float M[27], box[9];
};

// One move of one molecule.  kt[6] = the sums of cell_ktensor_term over the molecule's atoms.  Returns 0 when the move is usable,
// 1 when it is not: V = 0, anything not finite on the way (a NaN in the virial, a box about to vanish or explode), or
// det (h mu) <= 0 (a left-handed box has no factorisation with a positive diagonal).  kT = 0: no Philox call, weak coupling.
MD_FN int cell_move(const float box[9], const float W[9], const double kt[6], double force_scale, double P0, double kT, double a,
                    uint64_t seed, uint64_t step, uint32_t mol, int coupling, int axis, CellMove* o) {
  double h[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) h[i] = (double)box[i];
  const double V = fabs(mat3_det(h));
  o->V = V;
  const double K[9] = {kt[0] / force_scale, kt[1] / force_scale, kt[2] / force_scale, kt[1] / force_scale, kt[3] / force_scale,
                       kt[4] / force_scale, kt[2] / force_scale, kt[4] / force_scale, kt[5] / force_scale};
  const double drift = -(a / 3.0), amp = kT > 0.0 ? sqrt(2.0 * kT * a / (3.0 * V)) : 0.0;
  double Df[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    o->P[i] = (2.0 * K[i] + (double)W[i]) / V;
    Df[i] = drift * (((i % 4 == 0) ? P0 : 0.0) - o->P[i]);
  }
  if (kT > 0.0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      float xi[3];
      cell_noise_row(seed, step, mol, (uint32_t)r, xi);
#pragma unroll
      for (int c = 0; c < 3; ++c) Df[3 * r + c] = Df[3 * r + c] + amp * (double)xi[c];
    }
  }
  int bad = !(V > 0.0);
  // the projection, as selects on values (stores into D from two branches end up behind a pointer chosen at run time: scratch)
  const bool full = coupling == kCellAnisotropic, semi = coupling == kCellSemiIsotropic;
  const double m12 = 0.5 * (Df[4] + Df[8]), m02 = 0.5 * (Df[0] + Df[8]), m01 = 0.5 * (Df[0] + Df[4]);
  const double d0 = !semi || axis == 0 ? Df[0] : (axis == 1 ? m02 : m01);
  const double d1 = !semi || axis == 1 ? Df[4] : (axis == 0 ? m12 : m01);
  const double d2 = !semi || (axis != 0 && axis != 1) ? Df[8] : (axis == 0 ? m12 : m02);
  double D[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) D[i] = full ? Df[i] : 0.0;
  D[0] = d0;
  D[4] = d1;
  D[8] = d2;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    o->D[i] = D[i];
    bad |= !isfinite(D[i]);
  }
  double hp[9];
  if (coupling == kCellAnisotropic) {
    double Dm[9];  // -D^T
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Dm[3 * i + j] = -D[3 * j + i];
    mat3_exp(D, o->mu);
    mat3_exp(Dm, o->nu);
    mat3_mul(h, o->mu, hp);
    // Gram-Schmidt on the rows of h mu, top down: L[i][j] = r_i . q_j (j <= i), q2 = q0 x q1, so det Q = 1
    double* L = o->L;
    double* Q = o->Q;
    const double l00 = sqrt((hp[0] * hp[0] + hp[1] * hp[1]) + hp[2] * hp[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) Q[c] = hp[c] / l00;
    const double l10 = (hp[3] * Q[0] + hp[4] * Q[1]) + hp[5] * Q[2];
    double u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = hp[3 + c] - l10 * Q[c];
    const double l11 = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) Q[3 + c] = u[c] / l11;
    Q[6] = Q[1] * Q[5] - Q[2] * Q[4];
    Q[7] = Q[2] * Q[3] - Q[0] * Q[5];
    Q[8] = Q[0] * Q[4] - Q[1] * Q[3];
    L[0] = l00; L[1] = 0.0; L[2] = 0.0;
    L[3] = l10; L[4] = l11; L[5] = 0.0;
    L[6] = (hp[6] * Q[0] + hp[7] * Q[1]) + hp[8] * Q[2];
    L[7] = (hp[6] * Q[3] + hp[7] * Q[4]) + hp[8] * Q[5];
    L[8] = (hp[6] * Q[6] + hp[7] * Q[7]) + hp[8] * Q[8];
    bad |= !(l00 > 0.0) || !(l11 > 0.0) || !(L[8] > 0.0);
    double Qt[9], Mx[9], Mv[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Qt[3 * i + j] = Q[3 * j + i];
    mat3_mul(o->mu, Qt, Mx);
    mat3_mul(o->nu, Qt, Mv);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      o->M[i] = (float)Mx[i];
      o->M[9 + i] = (float)Mv[i];
      o->M[18 + i] = (float)Qt[i];
      o->box[i] = (float)L[i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      o->mu[i] = 0.0;
      o->nu[i] = 0.0;
      o->Q[i] = (i % 4 == 0) ? 1.0 : 0.0;
    }
    // (six calls written out: a loop over the diagonal keeps D in an array indexed at run time, which lives in scratch)
    o->mu[0] = exp(D[0]);
    o->mu[4] = exp(D[4]);
    o->mu[8] = exp(D[8]);
    o->nu[0] = exp(-D[0]);
    o->nu[4] = exp(-D[4]);
    o->nu[8] = exp(-D[8]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) hp[3 * i + j] = h[3 * i + j] * o->mu[4 * j];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      o->L[i] = hp[i];
      o->M[i] = (float)o->mu[i];
      o->M[9 + i] = (float)o->nu[i];
      o->M[18 + i] = (i % 4 == 0) ? 1.f : 0.f;
      o->box[i] = (float)hp[i];
    }
  }
  bad |= !(mat3_det(hp) > 0.0);
#pragma unroll
  for (int i = 0; i < 9; ++i) bad |= !isfinite(o->M[i]) || !isfinite(o->M[9 + i]) || !isfinite(o->M[18 + i]) || !isfinite(o->box[i]);
  return bad;
}

// x <- x M for one atom: component b = ((x0 M0b) + (x1 M1b)) + (x2 M2b), or the one product x_b M_bb when the matrix is diagonal
template <bool DIAG>
MD_FN void cell_apply(float x[3], const float M[9]) {
  if (DIAG) {
#pragma unroll
    for (int b = 0; b < 3; ++b) x[b] = md_mul(x[b], M[4 * b]);
  } else {
    const float x0 = x[0], x1 = x[1], x2 = x[2];
#pragma unroll
    for (int b = 0; b < 3; ++b) x[b] = md_add(md_add(md_mul(x0, M[b]), md_mul(x1, M[3 + b])), md_mul(x2, M[6 + b]));
  }
}

}  // namespace tn_md
