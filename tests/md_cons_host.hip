// TEST INFRASTRUCTURE ONLY: the constraint arithmetic of the device-resident MD loop (torchmd-net_amd/csrc/tn_md_cons_math.h, with
// tn_md_math.h for B, A, O and the kinetic term) compiled for the host (hipcc --cuda-host-only), loaded through ctypes by
// tests/md_cons_host_mirror.py.  One plain loop over the clusters stands for the groups of lanes of tn_md_cons.hip: a cluster's
// eight lanes become arrays of eight, a shuffle becomes an index, and the per-constraint statements are the header's own.
// MD_CONS_HOST_MAIN adds a main() that runs every entry once on a small system (the sanitizer build of tests/test_md_constraints_host.py).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../torchmd-net_amd/csrc/tn_md_cons_math.h"

namespace {

using namespace tn_md_cons;

int cluster_shake(int nc, const int32_t* ab, const double* d2, double x[kMaxAtoms][3], const double k[kMaxAtoms][3],
                  const double w[kMaxAtoms], double tol, int max_iter) {
  int moved = 0;
  for (int it = 0; it <= max_iter; ++it) {
    moved = 0;
    for (int c = 0; c < nc; ++c) {
      const int la = ab[2 * c] & (kMaxAtoms - 1), lb = ab[2 * c + 1] & (kMaxAtoms - 1);
      double g;
      if (shake_one(x[la], x[lb], k[la], k[lb], w[la], w[lb], d2[c], tol, &g)) continue;
      moved = 1;
      if (it == max_iter) continue;
      move_along(x[la], g * w[la], k[la], k[lb]);
      move_along(x[lb], -(g * w[lb]), k[la], k[lb]);
    }
    if (!moved) break;
  }
  return !moved;
}

int cluster_rattle(int nc, const int32_t* ab, const double* d2, const double x[kMaxAtoms][3], double v[kMaxAtoms][3],
                   const double w[kMaxAtoms], double dt, double tol, int max_iter) {
  int moved = 0;
  for (int it = 0; it <= max_iter; ++it) {
    moved = 0;
    for (int c = 0; c < nc; ++c) {
      const int la = ab[2 * c] & (kMaxAtoms - 1), lb = ab[2 * c + 1] & (kMaxAtoms - 1);
      double k;
      if (rattle_one(x[la], x[lb], v[la], v[lb], w[la], w[lb], d2[c], dt, tol, &k)) continue;
      moved = 1;
      if (it == max_iter) continue;
      move_along(v[la], k * w[la], x[la], x[lb]);
      move_along(v[lb], -(k * w[lb]), x[la], x[lb]);
    }
    if (!moved) break;
  }
  return !moved;
}

void widen(const float a[kMaxAtoms][3], double b[kMaxAtoms][3]) {
  for (int l = 0; l < kMaxAtoms; ++l)
    for (int d = 0; d < 3; ++d) b[l][d] = (double)a[l][d];
}

}  // namespace

extern "C" {

// One launch of k_md_clusters<CLOSE, OPEN> (neither: the projection alone) without the overflow and status tests.  pos, vel [N,3] in
// place; x_keep, v_keep [N,3] and part [N] as the MD workspace holds them.  Returns the fail word.
uint32_t md_cons_advance(int close, int open, int64_t n_atoms, int64_t n_clusters, const int32_t* cl_atoms, const int32_t* cl_off,
                         const int32_t* cons_ab, const double* cons_d2, float* pos, float* vel, const float* forces, const float* hk,
                         const float* mass, const float* sigma, float dt, float c1, float c2, uint64_t seed, uint64_t step, double tol,
                         int max_iter, float* x_keep, float* v_keep, float* part) {
  uint32_t fail = 0;
  for (int64_t cl = 0; cl < n_clusters; ++cl) {
    int idx[kMaxAtoms];
    float x[kMaxAtoms][3], v[kMaxAtoms][3], f[kMaxAtoms][3], h[kMaxAtoms], m[kMaxAtoms], ke[kMaxAtoms];
    double w[kMaxAtoms], x64[kMaxAtoms][3], v64[kMaxAtoms][3], k64[kMaxAtoms][3];
    memset(x, 0, sizeof(x));
    memset(v, 0, sizeof(v));
    memset(f, 0, sizeof(f));
    const int c0 = cl_off[cl], nc = cl_off[cl + 1] - c0;
    const int32_t* ab = cons_ab + 2 * (int64_t)c0;
    const double* d2 = cons_d2 + c0;
    for (int l = 0; l < kMaxAtoms; ++l) {
      int i = cl_atoms[cl * kMaxAtoms + l];
      if (i >= n_atoms) i = -1;
      idx[l] = i;
      h[l] = 0.f;
      m[l] = 1.f;
      ke[l] = 0.f;
      if (i >= 0) {
        for (int d = 0; d < 3; ++d) {
          x[l][d] = pos[i * 3 + d];
          v[l][d] = vel[i * 3 + d];
          if (close || open) f[l][d] = forces[i * 3 + d];
        }
        if (close || open) h[l] = hk[i];
        m[l] = mass[i];
      }
      w[l] = inv_mass(m[l]);
    }
    int ok = 1;
    uint32_t bits = 0;
    bool restore = true;
    if (close) {
      for (int l = 0; l < kMaxAtoms; ++l)
        if (idx[l] >= 0)
          ke[l] = tn_md::close_step(v[l], f[l], h[l], m[l], sigma != nullptr, c1, c2, sigma ? sigma[idx[l]] : 0.f, seed, step,
                                    (uint32_t)idx[l]);
    }
    if ((close || !open) && nc > 0) {
      widen(x, x64);
      widen(v, v64);
      ok = cluster_rattle(nc, ab, d2, x64, v64, w, (double)dt, tol, max_iter);
      if (ok)
        for (int l = 0; l < kMaxAtoms; ++l) ok &= rattle_finish(v64[l], v[l]);
      if (!ok) {
        bits = kFailRattle;
        restore = close;
      } else if (close) {
        for (int l = 0; l < kMaxAtoms; ++l) ke[l] = tn_md::kinetic(m[l], v[l][0], v[l][1], v[l][2]);
      }
    }
    if (ok && close)
      for (int l = 0; l < kMaxAtoms; ++l)
        if (idx[l] >= 0) part[idx[l]] = ke[l];
    if (ok && open) {
      widen(x, k64);
      for (int l = 0; l < kMaxAtoms; ++l) {
        const int i = idx[l];
        if (i < 0) continue;
        for (int d = 0; d < 3; ++d) {
          x_keep[i * 3 + d] = x[l][d];
          v_keep[i * 3 + d] = v[l][d];
        }
        tn_md::open_step(x[l], v[l], f[l], h[l], dt);
      }
      if (nc > 0) {
        widen(x, x64);
        ok = cluster_shake(nc, ab, d2, x64, k64, w, tol, max_iter);
        if (ok)
          for (int l = 0; l < kMaxAtoms; ++l) ok &= shake_finish(x64[l], x[l], v[l], (double)dt);
        if (!ok) bits = kFailShake;
      }
    }
    fail |= bits;
    for (int l = 0; l < kMaxAtoms; ++l) {
      const int i = idx[l];
      if (i < 0) continue;
      for (int d = 0; d < 3; ++d) {
        if (ok) {
          if (open) pos[i * 3 + d] = x[l][d];
          vel[i * 3 + d] = v[l][d];
        } else if (restore) {
          pos[i * 3 + d] = x_keep[i * 3 + d];
          vel[i * 3 + d] = v_keep[i * 3 + d];
        }
      }
    }
  }
  return fail;
}

}  // extern "C"

#ifdef MD_CONS_HOST_MAIN
// two rigid waters, a diatomic with one end of infinite mass and five free atoms: OPEN, MIDDLE, CLOSE and the projection, with and
// without a thermostat, and one run that fails (max_iter = 1)
int main() {
  const int N = 13;
  const int32_t cl_atoms[4 * 8] = {0, 1, 2, -1, -1, -1, -1, -1, 3, 4, 5, -1, -1, -1, -1, -1, 6, 7, -1, -1, -1, -1, -1, -1, 8, 9, 10, 11, 12, -1, -1, -1};
  const int32_t cl_off[5] = {0, 3, 6, 7, 7};
  const int32_t ab[7 * 2] = {0, 1, 0, 2, 1, 2, 0, 1, 0, 2, 1, 2, 0, 1};
  float pos[N * 3], vel[N * 3], frc[N * 3], hk[N], mass[N], sigma[N], xk[N * 3], vk[N * 3], part[N];
  double d2[7];
  uint32_t seed = 12345u;
  auto rnd = [&seed]() {
    seed = seed * 1664525u + 1013904223u;
    return (float)(seed >> 8) * (1.0f / 16777216.0f) - 0.5f;
  };
  const float water[9] = {0.f, 0.f, 0.f, 0.9572f, 0.f, 0.f, -0.24f, 0.9266f, 0.f};
  for (int i = 0; i < N; ++i) {
    for (int d = 0; d < 3; ++d) {
      pos[i * 3 + d] = (i < 6 ? water[(i % 3) * 3 + d] : 2.f * rnd()) + 3.f * (float)(i / 3);
      vel[i * 3 + d] = 0.02f * rnd();
      frc[i * 3 + d] = 2.f * rnd();
    }
    mass[i] = (i % 3 == 0) ? 15.999f : 1.008f;
    if (i == 6) mass[i] = INFINITY;
    hk[i] = (float)(0.5 * 2.0 * 9.648533e-3 / (double)mass[i]);
    sigma[i] = (float)sqrt(0.025 * 9.648533e-3 / (double)mass[i]);
  }
  for (int c = 0; c < 7; ++c) {
    const int base = c < 3 ? 0 : c < 6 ? 3 : 6;
    const int i = base + ab[2 * c], j = base + ab[2 * c + 1];
    double s = 0;
    for (int d = 0; d < 3; ++d) s += ((double)pos[i * 3 + d] - pos[j * 3 + d]) * ((double)pos[i * 3 + d] - pos[j * 3 + d]);
    d2[c] = s;
  }
  uint32_t fail = 0;
  for (int th = 0; th < 2; ++th) {
    const float* sg = th ? sigma : nullptr;
    fail |= md_cons_advance(0, 0, N, 4, cl_atoms, cl_off, ab, d2, pos, vel, frc, hk, mass, sg, 2.f, 0.98f, 0.199f, 7, 0, 1e-6, 64, xk, vk, part);
    fail |= md_cons_advance(0, 1, N, 4, cl_atoms, cl_off, ab, d2, pos, vel, frc, hk, mass, sg, 2.f, 0.98f, 0.199f, 7, 0, 1e-6, 64, xk, vk, part);
    for (int k = 0; k < 3; ++k)
      fail |= md_cons_advance(1, 1, N, 4, cl_atoms, cl_off, ab, d2, pos, vel, frc, hk, mass, sg, 2.f, 0.98f, 0.199f, 7, k, 1e-6, 64, xk, vk, part);
    fail |= md_cons_advance(1, 0, N, 4, cl_atoms, cl_off, ab, d2, pos, vel, frc, hk, mass, sg, 2.f, 0.98f, 0.199f, 7, 3, 1e-6, 64, xk, vk, part);
  }
  for (int i = 0; i < N * 3; ++i) frc[i] *= 50.f;
  const uint32_t fail1 = md_cons_advance(0, 1, N, 4, cl_atoms, cl_off, ab, d2, pos, vel, frc, hk, mass, nullptr, 2.f, 1.f, 0.f, 7, 0, 1e-6, 1, xk, vk, part);
  double worst = 0;
  for (int c = 0; c < 7; ++c) {
    const int base = c < 3 ? 0 : c < 6 ? 3 : 6;
    const int i = base + ab[2 * c], j = base + ab[2 * c + 1];
    double s = 0;
    for (int d = 0; d < 3; ++d) s += ((double)pos[i * 3 + d] - pos[j * 3 + d]) * ((double)pos[i * 3 + d] - pos[j * 3 + d]);
    const double e = fabs(sqrt(s) - sqrt(d2[c])) / sqrt(d2[c]);
    worst = e > worst ? e : worst;
  }
  printf("md_cons_host: fail %u, forced fail %u, worst residual %.3e\n", fail, fail1, worst);
  return (fail == 0 && fail1 == kFailShake && worst < 1e-5) ? 0 : 1;
}
#endif
