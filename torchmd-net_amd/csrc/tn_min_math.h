// Arithmetic of the device-resident FIRE minimiser (tn_min.hip): the per-atom terms of the three scalar products, the
// per-molecule controller and the per-atom update.  FIRE: Bitzek, Koskinen, Gaehler, Moseler, Gumbsch, Phys. Rev. Lett. 97, 170201
// (2006), in the form ASE ships (unit masses, the whole-molecule step clamp), one controller per molecule.  __host__ __device__:
// tests/min_host.hip compiles this header host-only, so the statements a GPU lane runs are the statements the host checker runs.
//
// Rounding.  The per-atom terms and the per-atom update are fp32 under the contract of tn_md_math.h: every product is one md_mul,
// every sum one md_add, in the order written.  The controller is fp64 in the order written; its three outputs c_v, c_f, d are
// rounded to fp32 once.  (The device compiler may contract an fp64 product into the sum that consumes it; every state update -
// dt, alpha - is a single operation and does not depend on that.)
//
// Cell relaxation (the second half of this file; tests/min_cell_host.hip compiles it host-only): the box relaxes with the atoms by
// ASE's UnitCellFilter scheme.  The per-atom products with D32 follow the same fp32 contract; everything per molecule is fp64 in
// the order written, and the box and D32 are rounded to fp32 once.
#pragma once
#include "tn_md_math.h"

namespace tn_min {

using tn_md::md_add;
using tn_md::md_mul;

struct FireParams {  // the caller's parameters (dt0 and alpha0 also live in the workspace header: tmdnet_min_reset)
  double dt_max, f_inc, f_dec, alpha0, f_alpha, max_step, fmax;
  int32_t n_min;
};

struct FireState {  // per molecule
  double dt, alpha;
  int32_t n_pos;
  int64_t converged_at;  // -1 until the molecule converges
};

enum { FIRE_MOVING = 0, FIRE_FROZEN = 1, FIRE_UNUSABLE = 2 };

// (ax bx + ay by) + az bz
MD_FN float dot3(const float a[3], const float b[3]) { return md_add(md_add(md_mul(a[0], b[0]), md_mul(a[1], b[1])), md_mul(a[2], b[2])); }

// t[0] = v.f, t[1] = f.f, t[2] = v.v of one atom; a fixed atom contributes nothing
MD_FN void atom_terms(const float v[3], const float f[3], int fixed, float t[3]) {
  if (fixed) {
    t[0] = t[1] = t[2] = 0.f;
    return;
  }
  t[0] = dot3(f, v);
  t[1] = dot3(f, f);
  t[2] = dot3(v, v);
}

// One controller move of one molecule from its sums vf, ff, vv and fmax2 = max_i |f_i|^2 after `step` steps.  Updates *s, writes
// coef = {c_v, c_f, d}.  FIRE_FROZEN: the molecule had converged before (nothing is written but coef = 0) or converges now;
// FIRE_UNUSABLE: a sum is not finite - *s is untouched, coef = 0, and the caller latches status 2.
MD_FN int fire_control(FireState* s, const FireParams& p, double vf, double ff, double vv, double fmax2, int64_t step, float coef[3]) {
  coef[0] = coef[1] = coef[2] = 0.f;
  if (s->converged_at >= 0) return FIRE_FROZEN;
  if (!isfinite(vf) || !isfinite(ff) || !isfinite(vv) || !isfinite(fmax2)) return FIRE_UNUSABLE;
  if (sqrt(fmax2) < p.fmax) {
    s->converged_at = step;
    return FIRE_FROZEN;
  }
  double c_v, mix;
  if (vf > 0.0) {
    c_v = 1.0 - s->alpha;
    mix = (ff > 0.0 && vv > 0.0) ? s->alpha * sqrt(vv / ff) : 0.0;
    if (s->n_pos > p.n_min) {
      const double grown = s->dt * p.f_inc;
      s->dt = grown < p.dt_max ? grown : p.dt_max;
      s->alpha = s->alpha * p.f_alpha;
    }
    s->n_pos += 1;
  } else {
    c_v = 0.0;
    mix = 0.0;
    s->alpha = p.alpha0;
    s->dt = s->dt * p.f_dec;
    s->n_pos = 0;
  }
  const double dt = s->dt;
  const double c_f = mix + dt;
  // |v_new|^2 of v_new = c_v v + c_f f from the sums: the whole-molecule step clamp needs no second reduction
  const double n2 = ((c_v * c_v) * vv + ((2.0 * c_v) * c_f) * vf) + (c_f * c_f) * ff;
  const double len = dt * sqrt(n2 > 0.0 ? n2 : 0.0);
  const double d = len > p.max_step ? dt * (p.max_step / len) : dt;
  coef[0] = (float)c_v;
  coef[1] = (float)c_f;
  coef[2] = (float)d;
  return FIRE_MOVING;
}

// v <- c_v v + c_f f, then x <- x + d v, of one atom of a moving molecule
MD_FN void atom_move(float x[3], float v[3], const float f[3], float c_v, float c_f, float d) {
  for (int k = 0; k < 3; ++k) {
    v[k] = md_add(md_mul(c_v, v[k]), md_mul(c_f, f[k]));
    x[k] = md_add(x[k], md_mul(d, v[k]));
  }
}

// ---- cell relaxation (tmdnet_min_advance_cell): ASE's UnitCellFilter, one deformation gradient per molecule ----------------------
// Row vectors.  State per molecule, fp64: the reference box H0, the deformation gradient D (I after a reset), its FIRE velocity V_D,
// c = cell_factor.  The box is H = H0 D^T, rounded to fp32 once; D32 = fp32(D).  State per atom, fp32: xt = x D^-T and its velocity.
// The three rows of D count as three more atoms with coordinates c D and forces G / c, where
//   G = (W_s - pressure V I) D^-T,  W_s = (W + W^T) / 2,  V = |det box|        (- d(E + p V) / dD at fixed xt; W = - dE / d eps)
// then `hydrostatic` (G <- (tr G / 3) I) or `constant_volume` (G <- G - (tr G / 3) I), then the mask, entry by entry.

struct CellParams {
  double mask[9];  // 0 / 1
  double pressure;
  int32_t hydrostatic, constant_volume;
};

enum { CELL_OK = 0, CELL_BAD_SUMS = 1, CELL_BAD_VIRIAL = 2, CELL_BAD_VOLUME = 3 };  // the detail of status 2

// x_a = (xt_0 D32[a][0] + xt_1 D32[a][1]) + xt_2 D32[a][2]: the position handed to the evaluation
MD_FN void cell_position(const float xt[3], const float D32[9], float x[3]) {
  for (int a = 0; a < 3; ++a)
    x[a] = md_add(md_add(md_mul(xt[0], D32[3 * a + 0]), md_mul(xt[1], D32[3 * a + 1])), md_mul(xt[2], D32[3 * a + 2]));
}

// Ft_b = (F_0 D32[0][b] + F_1 D32[1][b]) + F_2 D32[2][b]: the force on xt, with the D32 the positions were formed with
MD_FN void cell_atom_force(const float F[3], const float D32[9], float Ft[3]) {
  for (int b = 0; b < 3; ++b) Ft[b] = md_add(md_add(md_mul(F[0], D32[b]), md_mul(F[1], D32[3 + b])), md_mul(F[2], D32[6 + b]));
}

MD_FN double det3(const double m[9]) {
  return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// inverse of a 3 x 3 matrix: cofactors over the determinant
MD_FN void inv3(const double m[9], double det, double inv[9]) {
  inv[0] = (m[4] * m[8] - m[5] * m[7]) / det;
  inv[1] = (m[2] * m[7] - m[1] * m[8]) / det;
  inv[2] = (m[1] * m[5] - m[2] * m[4]) / det;
  inv[3] = (m[5] * m[6] - m[3] * m[8]) / det;
  inv[4] = (m[0] * m[8] - m[2] * m[6]) / det;
  inv[5] = (m[2] * m[3] - m[0] * m[5]) / det;
  inv[6] = (m[3] * m[7] - m[4] * m[6]) / det;
  inv[7] = (m[1] * m[6] - m[0] * m[7]) / det;
  inv[8] = (m[0] * m[4] - m[1] * m[3]) / det;
}

// The cell rows' force G / c of one molecule from the step's virial W, the fp32 box the evaluation read and D.  Writes the volume
// and the stress -W_s / V as well.  CELL_BAD_VIRIAL: an entry of W is not finite; CELL_BAD_VOLUME: V or det D is zero or not finite.
MD_FN int cell_force(const float W[9], const float box[9], const double D[9], const CellParams& p, double c, double Gc[9], double* V_out,
                     double stress[9]) {
  for (int i = 0; i < 9; ++i) {
    Gc[i] = 0.0;
    stress[i] = 0.0;
  }
  *V_out = 0.0;
  for (int i = 0; i < 9; ++i)
    if (!isfinite(W[i])) return CELL_BAD_VIRIAL;
  const double V = tn_md::box_volume(box), det = det3(D);
  if (!(V > 0.0) || !isfinite(V) || !isfinite(det) || det == 0.0) return CELL_BAD_VOLUME;
  *V_out = V;
  double A[9], inv[9], G[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      A[3 * a + b] = 0.5 * ((double)W[3 * a + b] + (double)W[3 * b + a]);
      stress[3 * a + b] = -A[3 * a + b] / V;
    }
  const double pV = p.pressure * V;
  A[0] = A[0] - pV;
  A[4] = A[4] - pV;
  A[8] = A[8] - pV;
  inv3(D, det, inv);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b)  // (A D^-T)[a][b] = sum_k A[a][k] inv[b][k]
      G[3 * a + b] = (A[3 * a + 0] * inv[3 * b + 0] + A[3 * a + 1] * inv[3 * b + 1]) + A[3 * a + 2] * inv[3 * b + 2];
  if (p.hydrostatic || p.constant_volume) {
    const double t = ((G[0] + G[4]) + G[8]) / 3.0;
    if (p.hydrostatic) {
      for (int i = 0; i < 9; ++i) G[i] = 0.0;
      G[0] = G[4] = G[8] = t;
    } else {
      G[0] = G[0] - t;
      G[4] = G[4] - t;
      G[8] = G[8] - t;
    }
  }
  for (int i = 0; i < 9; ++i) Gc[i] = (p.mask[i] != 0.0 ? G[i] : 0.0) / c;
  return CELL_OK;
}

// the three cell rows' terms added to the sums of the atoms: sums = vf, ff, vv, fmax2
MD_FN void cell_sums(const double VD[9], const double Gc[9], double sums[4]) {
  for (int a = 0; a < 3; ++a) {
    const double *v = VD + 3 * a, *g = Gc + 3 * a;
    const double t_vf = (g[0] * v[0] + g[1] * v[1]) + g[2] * v[2];
    const double t_ff = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    const double t_vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    sums[0] = sums[0] + t_vf;
    sums[1] = sums[1] + t_ff;
    sums[2] = sums[2] + t_vv;
    sums[3] = t_ff > sums[3] ? t_ff : sums[3];
  }
}

// The cell rows' move with the coefficients the atoms use (fp32, widened): V_D <- c_v V_D + c_f G / c, D <- D + d V_D / c, in fp64;
// then the box H0 D^T and D, each entry rounded to fp32 once.  Returns 0 when the new box is usable (finite, volume > 0), 1 when not.
MD_FN int cell_move(const double D[9], const double VD[9], const double Gc[9], const float coef[3], double c, const double H0[9],
                    double Dn[9], double VDn[9], float boxn[9], float d32n[9]) {
  const double c_v = (double)coef[0], c_f = (double)coef[1], d = (double)coef[2];
  int bad = 0;
  for (int i = 0; i < 9; ++i) {
    VDn[i] = c_v * VD[i] + c_f * Gc[i];
    Dn[i] = D[i] + (d * VDn[i]) / c;
    d32n[i] = (float)Dn[i];
    bad |= !isfinite(d32n[i]);
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {  // (H0 D^T)[a][b] = sum_k H0[a][k] D[b][k]
      const double h = (H0[3 * a + 0] * Dn[3 * b + 0] + H0[3 * a + 1] * Dn[3 * b + 1]) + H0[3 * a + 2] * Dn[3 * b + 2];
      boxn[3 * a + b] = (float)h;
      bad |= !isfinite(boxn[3 * a + b]);
    }
  const double V = tn_md::box_volume(boxn);
  return bad || !(V > 0.0) || !isfinite(V);
}

// One molecule's control with its cell rows: the atoms' sums (vf, ff, vv, fmax2; on return with the cell rows' terms added), the
// step's virial, the box it was evaluated with, D and V_D.  Writes Gc = G / c, the volume, the stress, the coefficients and the next
// D, V_D, box and D32 (a frozen molecule: D and the box as they are, V_D = 0).  Returns FIRE_MOVING / FIRE_FROZEN, or FIRE_UNUSABLE
// with *why = CELL_BAD_*: then *s is untouched.  A molecule that had converged looks at nothing.
MD_FN int cell_control(FireState* s, const FireParams& p, const CellParams& cp, double c, double sums[4], const float W[9],
                       const float box[9], const float d32[9], const double H0[9], const double D[9], const double VD[9], int64_t step,
                       float coef[3], double Gc[9], double* V_out, double stress[9], double Dn[9], double VDn[9], float boxn[9],
                       float d32n[9], int* why) {
  *why = CELL_OK;
  for (int i = 0; i < 9; ++i) {
    Dn[i] = D[i];
    VDn[i] = 0.0;
    boxn[i] = box[i];
    d32n[i] = d32[i];
  }
  if (s->converged_at >= 0) {
    for (int i = 0; i < 9; ++i) Gc[i] = stress[i] = 0.0;
    *V_out = 0.0;
    return fire_control(s, p, sums[0], sums[1], sums[2], sums[3], step, coef);
  }
  const int bad = cell_force(W, box, D, cp, c, Gc, V_out, stress);
  if (bad) {
    coef[0] = coef[1] = coef[2] = 0.f;
    *why = bad;
    return FIRE_UNUSABLE;
  }
  cell_sums(VD, Gc, sums);
  const FireState before = *s;
  const int ret = fire_control(s, p, sums[0], sums[1], sums[2], sums[3], step, coef);
  if (ret == FIRE_UNUSABLE) *why = CELL_BAD_SUMS;
  if (ret == FIRE_MOVING && cell_move(D, VD, Gc, coef, c, H0, Dn, VDn, boxn, d32n)) {
    *s = before;
    coef[0] = coef[1] = coef[2] = 0.f;
    for (int i = 0; i < 9; ++i) {
      Dn[i] = D[i];
      VDn[i] = 0.0;
      boxn[i] = box[i];
      d32n[i] = d32[i];
    }
    *why = CELL_BAD_VOLUME;
    return FIRE_UNUSABLE;
  }
  return ret;
}

}  // namespace tn_min
