// TEST INFRASTRUCTURE ONLY: the anisotropic cell-rescaling arithmetic of the device-resident MD loop
// (torchmd-net_amd/csrc/tn_md_cell_math.h) compiled for the host (hipcc --cuda-host-only), one plain loop per kernel body, loaded
// through ctypes by tests/md_cell_host_mirror.py.  The statements are the ones a GPU lane runs; tests/test_md_cell_host.py compares
// them with tests/md_cell_oracle.py without a GPU.  With -DMD_CELL_HOST_MAIN the file is a program of its own (for the host
// sanitizers).
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../torchmd-net_amd/csrc/tn_md_cell_math.h"

extern "C" {

// Xi [n, 9] of mols[0..n) at `step`
void cell_noise(int64_t n, uint64_t seed, uint64_t step, const uint32_t* mols, double* out) {
  for (int64_t i = 0; i < n; ++i)
    for (uint32_t r = 0; r < 3; ++r) {
      float xi[3];
      tn_md::cell_noise_row(seed, step, mols[i], r, xi);
      for (int c = 0; c < 3; ++c) out[9 * i + 3 * r + c] = (double)xi[c];
    }
}

void cell_expm(const double* A, double* E) { tn_md::mat3_exp(A, E); }

// k_md_ktensor_reduce as one loop: kt[n_mol, 6] in the unit of m v^2
void cell_ktensor(int64_t n_atoms, int64_t n_mol, const int64_t* batch, const float* mass, const float* vel, double* kt) {
  for (int64_t j = 0; j < 6 * n_mol; ++j) kt[j] = 0.0;
  for (int64_t i = 0; i < n_atoms; ++i) {
    double t[6];
    tn_md::cell_ktensor_term(mass[i], vel + 3 * i, t);
    for (int c = 0; c < 6; ++c) kt[6 * batch[i] + c] += t[c];
  }
}

// one move per molecule (pass 1 of k_md_cell_move): box, W [n, 9], kt [n, 6] -> everything of CellMove and the flag
void cell_move(int64_t n, const float* box, const float* W, const double* kt, double force_scale, double P0, double kT, double a,
               uint64_t seed, uint64_t step, int32_t coupling, int32_t axis, double* V, double* P, double* D, double* mu, double* nu,
               double* L, double* Q, float* M, float* newbox, int32_t* flag) {
  for (int64_t m = 0; m < n; ++m) {
    tn_md::CellMove o;
    flag[m] = tn_md::cell_move(box + 9 * m, W + 9 * m, kt + 6 * m, force_scale, P0, kT, a, seed, step, (uint32_t)m, coupling, axis, &o);
    V[m] = o.V;
    for (int i = 0; i < 9; ++i) {
      P[9 * m + i] = o.P[i];
      D[9 * m + i] = o.D[i];
      mu[9 * m + i] = o.mu[i];
      nu[9 * m + i] = o.nu[i];
      L[9 * m + i] = o.L[i];
      Q[9 * m + i] = o.Q[i];
      newbox[9 * m + i] = o.box[i];
    }
    for (int i = 0; i < 27; ++i) M[27 * m + i] = o.M[i];
  }
}

// k_md_cell_scale<false, diag>: x, v and (not diag) f of every atom by Mx, Mv, Mf of its molecule, in place
void cell_scale(int64_t n_atoms, const int64_t* batch, const float* M, int32_t diag, float* x, float* v, float* f) {
  for (int64_t i = 0; i < n_atoms; ++i) {
    const float* Mp = M + 27 * batch[i];
    if (diag) {
      tn_md::cell_apply<true>(x + 3 * i, Mp);
      tn_md::cell_apply<true>(v + 3 * i, Mp + 9);
    } else {
      tn_md::cell_apply<false>(x + 3 * i, Mp);
      tn_md::cell_apply<false>(v + 3 * i, Mp + 9);
      tn_md::cell_apply<false>(f + 3 * i, Mp + 18);
    }
  }
}

// The ideal gas (F = 0) under Langevin + the cell barostat, the launch sequence of a captured replay written as loops: OPEN, then
// per step CLOSE (B, O), the kinetic tensor per replica, the move, the scaling and the opening half of the next step.  R replicas of
// n atoms each (atom i belongs to replica i / n), in place on box [R, 9], x, v [R n, 3].  The virial is 0, or with kappa > 0 the
// synthetic W_aa = -kappa (ln box_aa - eps0) of the exactly solvable per-axis ensemble.  volumes [steps, R] and lengths
// [steps, R, 3] (the box's diagonal) are those before each move.  Returns the number of unusable moves (0 expected).
int64_t cell_ideal_gas(int64_t R, int64_t n, int64_t steps, float* box, float* x, float* v, const float* hk, const float* mass,
                       const float* sigma, float dt, float c1, float c2, uint64_t seed, double force_scale, double P0, double kT,
                       double compressibility, double tau, uint64_t baro_seed, int32_t coupling, int32_t axis, double kappa, double eps0,
                       float* volumes, float* lengths) {
  const float zero[3] = {0.f, 0.f, 0.f};
  const double a = compressibility * (double)dt / tau;
  const bool diag = coupling != tn_md::kCellAnisotropic;
  int64_t bad = 0;
  for (int64_t i = 0; i < R * n; ++i) tn_md::open_step(x + 3 * i, v + 3 * i, zero, hk[i], dt);
  for (int64_t s = 0; s < steps; ++s) {
    for (int64_t m = 0; m < R; ++m) {
      double kt[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int64_t i = m * n; i < (m + 1) * n; ++i) {
        tn_md::close_step(v + 3 * i, zero, hk[i], mass[i], 1, c1, c2, sigma[i], seed, (uint64_t)s, (uint32_t)i);
        double t[6];
        tn_md::cell_ktensor_term(mass[i], v + 3 * i, t);
        for (int c = 0; c < 6; ++c) kt[c] += t[c];
      }
      float W[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (kappa > 0.0)
        for (int d = 0; d < 3; ++d) W[4 * d] = (float)(-kappa * (log((double)box[9 * m + 4 * d]) - eps0));
      tn_md::CellMove o;
      if (tn_md::cell_move(box + 9 * m, W, kt, force_scale, P0, kT, a, baro_seed, (uint64_t)s, (uint32_t)m, coupling, axis, &o)) {
        ++bad;
        continue;
      }
      volumes[s * R + m] = (float)o.V;
      for (int d = 0; d < 3; ++d) lengths[(s * R + m) * 3 + d] = box[9 * m + 4 * d];
      for (int i = 0; i < 9; ++i) box[9 * m + i] = o.box[i];
      for (int64_t i = m * n; i < (m + 1) * n; ++i) {
        if (diag) {
          tn_md::cell_apply<true>(x + 3 * i, o.M);
          tn_md::cell_apply<true>(v + 3 * i, o.M + 9);
        } else {
          tn_md::cell_apply<false>(x + 3 * i, o.M);
          tn_md::cell_apply<false>(v + 3 * i, o.M + 9);
        }
        tn_md::open_step(x + 3 * i, v + 3 * i, zero, hk[i], dt);
      }
    }
  }
  return bad;
}

}  // extern "C"

#ifdef MD_CELL_HOST_MAIN
// every entry of the mirror on heap arrays of exact size: moves in the three couplings, the scaling, a short ideal gas
int main() {
  const int64_t nm = 3, na = 12;
  std::vector<float> box(9 * nm), W(9 * nm), M(27 * nm), nb(9 * nm), x(3 * na), v(3 * na), f(3 * na), mass(na);
  std::vector<double> kt(6 * nm), V(nm), P(9 * nm), D(9 * nm), mu(9 * nm), nu(9 * nm), L(9 * nm), Q(9 * nm), xi(9 * nm), E(9);
  std::vector<int64_t> batch(na);
  std::vector<int32_t> flag(nm);
  std::vector<uint32_t> mols(nm);
  for (int64_t m = 0; m < nm; ++m) {
    mols[m] = (uint32_t)m;
    for (int i = 0; i < 9; ++i) {
      box[9 * m + i] = (i % 4 == 0) ? 6.f + (float)m + 0.5f * (float)(i / 4) : (i == 3 || i == 6 || i == 7) ? 0.4f * (float)(m + 1) : 0.f;
      W[9 * m + i] = 0.3f * sinf((float)(7 * m + i));
    }
  }
  for (int64_t i = 0; i < na; ++i) {
    batch[i] = i / 4;
    mass[i] = 1.f + (float)(i % 3);
    for (int d = 0; d < 3; ++d) {
      x[3 * i + d] = 0.7f * (float)((5 * i + 3 * d) % 11);
      v[3 * i + d] = 0.05f * cosf((float)(3 * i + d));
      f[3 * i + d] = sinf((float)(i + 2 * d));
    }
  }
  cell_noise(nm, 77, 5, mols.data(), xi.data());
  cell_ktensor(na, nm, batch.data(), mass.data(), v.data(), kt.data());
  int bad = 0;
  for (int32_t coupling = 0; coupling < 3; ++coupling)
    for (int32_t axis = 0; axis < 3; ++axis) {
      cell_move(nm, box.data(), W.data(), kt.data(), 1.0, 1e-3, 0.025, 0.5, 77, 5, coupling, axis, V.data(), P.data(), D.data(), mu.data(),
                nu.data(), L.data(), Q.data(), M.data(), nb.data(), flag.data());
      for (int64_t m = 0; m < nm; ++m) bad += flag[m];
      cell_scale(na, batch.data(), M.data(), coupling != 0, x.data(), v.data(), f.data());
    }
  cell_expm(D.data(), E.data());
  const int64_t R = 4, n = 8, steps = 50;
  std::vector<float> gbox(9 * R, 0.f), gx(3 * R * n), gv(3 * R * n, 0.01f), hk(R * n, 0.5f), gm(R * n, 1.f), sg(R * n, 0.158f);
  std::vector<float> vol(steps * R), len(steps * R * 3);
  for (int64_t m = 0; m < R; ++m)
    for (int d = 0; d < 3; ++d) gbox[9 * m + 4 * d] = 7.f;
  for (size_t i = 0; i < gx.size(); ++i) gx[i] = 0.1f * (float)(i % 70);
  for (int32_t coupling = 0; coupling < 3; ++coupling)
    bad += (int)cell_ideal_gas(R, n, steps, gbox.data(), gx.data(), gv.data(), hk.data(), gm.data(), sg.data(), 1.f, 0.9f, 0.43f, 3, 1.0, 1e-3,
                               0.025, 1e3, 20.0, 9, coupling, 2, coupling == 1 ? 10.0 : 0.0, 1.9, vol.data(), len.data());
  printf("moves done, bad %d, V %.6f, E00 %.6f, last volume %.4f\n", bad, V[0], E[0], (double)vol[steps * R - 1]);
  return bad != 0;
}
#endif
