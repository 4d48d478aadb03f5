// Arithmetic of the Hessian assembly and the normal-mode preparation (tn_vib.hip): which column a replica of the batch carries, the
// seed and the displacement of a replicated atom, one entry of the central difference quotient, and the fp64 steps that turn a
// per-molecule Hessian into the mass-weighted, projected matrix whose eigenvalues are the squared frequencies.  Projection of the
// translations and rotations in mass-weighted coordinates: Wilson, Decius and Cross, Molecular Vibrations (1955), ch. 2; the
// projector P = 1 - U U^T over an orthonormalised Eckart basis is what ASE's and Gaussian's frequency analyses apply.
// __host__ __device__: tests/vib_host.hip compiles this header host-only, so the statements a GPU lane runs are the statements the
// host checker runs.
//
// Numbering.  Molecule b has nfree_b free atoms, free_idx[fstart[b] .. fstart[b+1]) in the caller's order, and D_b = 3 nfree_b
// coordinates; coordinate i is component i % 3 of free atom i / 3.  Replica r of a pass that starts at column col0 carries column
// k = col0 + r of every molecule with k < D_b.
//
// Rounding.  A displacement is ONE rounded fp32 addition (md_add, the contract of tn_md_math.h).  Everything else is fp64 in the
// order written, sums in index order, no atomics.  (The device compiler may contract an fp64 product into the sum that consumes it.)
#pragma once
#include "tn_md_math.h"

namespace tn_vib {

using tn_md::md_add;

enum { VIB_SEED = 0, VIB_PLUS = 1, VIB_MINUS = 2 };       // what tmdnet_vib_seed writes
enum { VIB_ANALYTIC = 0, VIB_CENTRAL = 1 };               // what tmdnet_vib_gather reads
enum { VIB_PROJECT_NONE = 0, VIB_PROJECT_TRANS = 1, VIB_PROJECT_TRANS_ROT = 2 };
enum { VIB_INFO = 8 };  // doubles per molecule: hmax, asym, drift, rank, mode, D_b, 0, 0
enum { VIB_MAX_RANK = 6 };

// The component (0..2) of atom `a` of molecule b that column k seeds or displaces, or -1: k is beyond the molecule's columns, or
// belongs to another atom.
MD_FN int column_component(int64_t a, int64_t k, const int64_t* free_idx, int64_t f0, int64_t f1) {
  if (k < 0 || k >= 3 * (f1 - f0)) return -1;
  return free_idx[f0 + k / 3] == a ? (int)(k % 3) : -1;
}

// one replicated atom of the seed vector: 1.0 at the carried component
MD_FN void seed_row(int comp, float v[3]) {
  for (int d = 0; d < 3; ++d) v[d] = d == comp ? 1.f : 0.f;
}

// one replicated atom of a displaced geometry: the carried component moved by sign * delta in one rounded addition, the rest the
// caller's bits
MD_FN void displace_row(const float x[3], int comp, float delta, int mode, float out[3]) {
  for (int d = 0; d < 3; ++d) out[d] = d == comp ? md_add(x[d], mode == VIB_PLUS ? delta : -delta) : x[d];
}

// H_ik = - (F+_i - F-_i) / den with den = the ACTUAL difference of the two rounded positions of coordinate k (not 2 delta): the
// difference and the quotient in fp64, rounded once
MD_FN float central_entry(float f_plus, float f_minus, float x_plus, float x_minus) {
  const double den = (double)x_plus - (double)x_minus;
  return (float)(-((double)f_plus - (double)f_minus) / den);
}

// ---- finish: one molecule, H the molecule's padded fp32 block with leading dimension ld, Db its coordinates -------------------------

// |H_ij| and |H_ij - H_ji| of one entry
MD_FN void diag_entry(const float* H, int64_t ld, int64_t i, int64_t j, double* habs, double* asym) {
  const double a = (double)H[i * ld + j], b = (double)H[j * ld + i];
  *habs = fabs(a);
  *asym = fabs(a - b);
}

// the acoustic sum of row i, component beta: | sum_j H[i, 3 j + beta] |, the atoms in index order
MD_FN double drift_entry(const float* H, int64_t ld, int64_t nfree, int64_t i, int beta) {
  double s = 0.0;
  for (int64_t j = 0; j < nfree; ++j) s += (double)H[i * ld + 3 * j + beta];
  return fabs(s);
}

// A_ij = (H_ij + H_ji) / 2 / sqrt(m_i m_j), the masses of the two coordinates' atoms widened
MD_FN double weighted_entry(const float* H, int64_t ld, int64_t i, int64_t j, float mi, float mj) {
  const double s = 0.5 * ((double)H[i * ld + j] + (double)H[j * ld + i]);
  return s / sqrt((double)mi * (double)mj);
}

// The orthonormal basis U [rank, Db] (row p at U + p * Db) of the molecule's translations (mode 1) or translations and rotations (mode
// 2) in mass-weighted coordinates, run by ONE lane.  Candidates in the order t_x, t_y, t_z, r_x, r_y, r_z:
//   t_alpha[3 j + beta] = sqrt(m_j) delta_alpha,beta        r_alpha[3 j ..] = sqrt(m_j) (e_alpha x (x_j - c))
// c the centre of mass from the fp32 positions widened.  Each is orthogonalised against the kept ones by modified Gram-Schmidt,
// twice, and kept when |w|^2 > 1e-12 |w0|^2.  pos, mass: the caller's [N, 3] and [N]; idx the molecule's nfree free atoms.
// Returns the rank.
MD_FN int build_basis(const float* pos, const float* mass, const int64_t* idx, int64_t nfree, int mode, double* U) {
  if (mode == VIB_PROJECT_NONE || nfree <= 0) return 0;
  const int64_t Db = 3 * nfree;
  double c[3] = {0.0, 0.0, 0.0}, mt = 0.0;
  for (int64_t j = 0; j < nfree; ++j) {
    const double m = (double)mass[idx[j]];
    mt += m;
    for (int d = 0; d < 3; ++d) c[d] += m * (double)pos[3 * idx[j] + d];
  }
  for (int d = 0; d < 3; ++d) c[d] /= mt;
  int rank = 0;
  const int n_cand = mode == VIB_PROJECT_TRANS ? 3 : 6;
  for (int cand = 0; cand < n_cand; ++cand) {
    double* w = U + (int64_t)rank * Db;
    double n0 = 0.0;
    for (int64_t j = 0; j < nfree; ++j) {
      const double sm = sqrt((double)mass[idx[j]]);
      double e[3] = {0.0, 0.0, 0.0};
      if (cand < 3) {
        e[cand] = sm;
      } else {
        const int a = cand - 3, a1 = (a + 1) % 3, a2 = (a + 2) % 3;
        // e_a x d: component a1 = - d[a2], component a2 = d[a1]
        e[a1] = -sm * ((double)pos[3 * idx[j] + a2] - c[a2]);
        e[a2] = sm * ((double)pos[3 * idx[j] + a1] - c[a1]);
      }
      for (int d = 0; d < 3; ++d) {
        w[3 * j + d] = e[d];
        n0 += e[d] * e[d];
      }
    }
    for (int pass = 0; pass < 2; ++pass)
      for (int p = 0; p < rank; ++p) {
        const double* u = U + (int64_t)p * Db;
        double dot = 0.0;
        for (int64_t i = 0; i < Db; ++i) dot += u[i] * w[i];
        for (int64_t i = 0; i < Db; ++i) w[i] -= dot * u[i];
      }
    double n1 = 0.0;
    for (int64_t i = 0; i < Db; ++i) n1 += w[i] * w[i];
    if (!(n1 > 1e-12 * n0)) continue;
    const double inv = 1.0 / sqrt(n1);
    for (int64_t i = 0; i < Db; ++i) w[i] *= inv;
    ++rank;
  }
  return rank;
}

// W = U^T A, one entry: W[p, j] = sum_i U[p, i] A[i, j]   (A with leading dimension ld)
MD_FN double proj_w_entry(const double* U, const double* A, int64_t ld, int64_t Db, int p, int64_t j) {
  double s = 0.0;
  for (int64_t i = 0; i < Db; ++i) s += U[(int64_t)p * Db + i] * A[i * ld + j];
  return s;
}

// G = U^T A U, one entry: G[p, q] = sum_j W[p, j] U[q, j]
MD_FN double proj_g_entry(const double* U, const double* W, int64_t Db, int p, int q) {
  double s = 0.0;
  for (int64_t j = 0; j < Db; ++j) s += W[(int64_t)p * Db + j] * U[(int64_t)q * Db + j];
  return s;
}

// (P A P)_ij = A_ij - sum_p U_pi W_pj - sum_p W_pi U_pj + sum_pq U_pi G_pq U_qj
MD_FN double proj_apply_entry(double a, const double* U, const double* W, const double* G, int64_t Db, int rank, int64_t i, int64_t j) {
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int p = 0; p < rank; ++p) {
    s1 += U[(int64_t)p * Db + i] * W[(int64_t)p * Db + j];
    s2 += W[(int64_t)p * Db + i] * U[(int64_t)p * Db + j];
    double t = 0.0;
    for (int q = 0; q < rank; ++q) t += G[p * VIB_MAX_RANK + q] * U[(int64_t)q * Db + j];
    s3 += U[(int64_t)p * Db + i] * t;
  }
  return ((a - s1) - s2) + s3;
}

}  // namespace tn_vib
