// TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident L-BFGS minimiser (torchmd-net_amd/csrc/tn_lbfgs_math.h) compiled for
// the host (hipcc --cuda-host-only), one plain loop per kernel body, loaded through ctypes by tests/lbfgs_host_mirror.py.  The statements
// are the ones a GPU wave runs, with one lane; tests/test_lbfgs_host.py compares them with tests/lbfgs_oracle.py without a GPU.  With
// -DLBFGS_HOST_MAIN the file is a stand-alone program (for the sanitizers).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../torchmd-net_amd/csrc/tn_lbfgs_math.h"

namespace {

tn_lbfgs::MolState mol(int64_t m, int32_t memory, int32_t* h, int32_t* order, int64_t* conv, double* SS, double* SY, double* YY) {
  const int64_t M1 = memory + 1;
  tn_lbfgs::MolState st;
  st.h = h + m;
  st.order = order + m * M1;
  st.conv = conv + m;
  st.SS = SS + m * M1 * M1;
  st.SY = SY + m * M1 * M1;
  st.YY = YY + m * M1 * M1;
  return st;
}

tn_lbfgs::Params params(int32_t memory, double alpha, double max_step, double damping, double fmax) {
  tn_lbfgs::Params p;
  p.memory = memory;
  p.alpha = alpha;
  p.max_step = max_step;
  p.damping = damping;
  p.fmax = fmax;
  return p;
}

}  // namespace

extern "C" {

// the state a reset leaves
void lb_init(int64_t n_mol, int32_t memory, int32_t* h, int32_t* order, int64_t* conv) {
  for (int64_t m = 0; m < n_mol; ++m) {
    h[m] = 0;
    conv[m] = -1;
    for (int32_t q = 0; q <= memory; ++q) order[m * (memory + 1) + q] = q;
  }
}

// the candidate of every atom: s, y [n, 3]
void lb_candidate(int64_t n, const float* x, const float* x_prev, const float* f, const float* f_prev, const uint8_t* fixed, float* s,
                  float* y) {
  for (int64_t i = 0; i < n; ++i)
    tn_lbfgs::candidate(x + 3 * i, x_prev + 3 * i, f + 3 * i, f_prev + 3 * i, fixed && fixed[i], s + 3 * i, y + 3 * i);
}

// k_lbfgs_dots and the slice loop of the controller, the atoms in index order: the candidate of every molecule that moved into its spare
// slot of the rings S, Y [memory + 1, n_atoms, 3], and tot [n_mol, 6 (memory + 1) + 4]
void lb_sums(int64_t n_mol, int64_t n_atoms, const int64_t* batch, int32_t memory, int32_t fresh, const int32_t* h, const int32_t* order,
             const int64_t* conv, const float* x, const float* x_prev, const float* f, const float* f_prev, const uint8_t* fixed, float* S,
             float* Y, double* tot) {
  const int64_t M1 = memory + 1, NP = 6 * M1 + 4;
  for (int64_t e = 0; e < n_mol * NP; ++e) tot[e] = 0.0;
  for (int64_t i = 0; i < n_atoms; ++i) {
    const int64_t m = batch[i];
    const bool moved = !fresh && conv[m] < 0;
    const int fx = fixed && fixed[i];
    double* t = tot + m * NP;
    float g[3], sc[3] = {0.f, 0.f, 0.f}, yc[3] = {0.f, 0.f, 0.f};
    for (int d = 0; d < 3; ++d) g[d] = fx ? 0.f : -f[3 * i + d];
    if (moved) {
      tn_lbfgs::candidate(x + 3 * i, x_prev + 3 * i, f + 3 * i, f_prev + 3 * i, fx, sc, yc);
      const int32_t* ord = order + m * M1;
      for (int32_t q = 0; q < h[m]; ++q) {
        const int64_t a = ord[q];
        const float* sa = S + (a * n_atoms + i) * 3;
        const float* ya = Y + (a * n_atoms + i) * 3;
        t[6 * a + 0] += tn_lbfgs::dot3w(sc, sa);
        t[6 * a + 1] += tn_lbfgs::dot3w(sc, ya);
        t[6 * a + 2] += tn_lbfgs::dot3w(yc, sa);
        t[6 * a + 3] += tn_lbfgs::dot3w(yc, ya);
        t[6 * a + 4] += tn_lbfgs::dot3w(g, sa);
        t[6 * a + 5] += tn_lbfgs::dot3w(g, ya);
      }
      const int64_t c = ord[h[m]];
      for (int d = 0; d < 3; ++d) {
        S[(c * n_atoms + i) * 3 + d] = sc[d];
        Y[(c * n_atoms + i) * 3 + d] = yc[d];
      }
      t[6 * c + 0] += tn_lbfgs::dot3w(sc, sc);
      t[6 * c + 1] += tn_lbfgs::dot3w(sc, yc);
      t[6 * c + 3] += tn_lbfgs::dot3w(yc, yc);
      t[6 * c + 4] += tn_lbfgs::dot3w(g, sc);
      t[6 * c + 5] += tn_lbfgs::dot3w(g, yc);
      t[6 * c + 2] = t[6 * c + 1];
      t[6 * M1 + 2] = t[6 * c + 0];
      t[6 * M1 + 3] = t[6 * c + 3];
    }
    const double t_ff = tn_lbfgs::dot3w(g, g);
    t[6 * M1] += t_ff;
    t[6 * M1 + 1] = t_ff > t[6 * M1 + 1] ? t_ff : t[6 * M1 + 1];
  }
}

// the controller of every molecule, the state in place: -> delta [n_mol, 2 (memory + 1) + 1], accepted, gp, ret [n_mol] (0 moving, 1
// frozen, 2 unusable: then nothing of that molecule was written)
void lb_control(int64_t n_mol, int32_t memory, double alpha, double max_step, double damping, double fmax, int32_t fresh, int64_t step,
                int32_t* h, int32_t* order, int64_t* conv, double* SS, double* SY, double* YY, const double* tot, double* delta,
                int32_t* accepted, double* gp, int32_t* ret) {
  const tn_lbfgs::Params p = params(memory, alpha, max_step, damping, fmax);
  const int64_t M1 = memory + 1, NP = 6 * M1 + 4;
  std::vector<double> av(M1);
  std::vector<int32_t> ord(M1);
  for (int64_t m = 0; m < n_mol; ++m) {
    const tn_lbfgs::MolState st = mol(m, memory, h, order, conv, SS, SY, YY);
    const int moved = !fresh && conv[m] < 0;
    accepted[m] = 0;
    gp[m] = 0.0;
    if (!tn_lbfgs::usable(conv[m], memory, tot + m * NP, moved)) {
      ret[m] = tn_lbfgs::LBFGS_UNUSABLE;
      continue;
    }
    ret[m] = tn_lbfgs::control(st, p, tot + m * NP, moved, step, delta + m * (2 * M1 + 1), av.data(), ord.data(), accepted + m, gp + m);
  }
}

// k_lbfgs_direction: p [n_atoms, 3] (the rows of a converged molecule are left alone) and longest2 [n_mol] = max |p_i|^2
void lb_direction(int64_t n_mol, int64_t n_atoms, const int64_t* batch, int32_t memory, const int32_t* h, const int32_t* order,
                  const int64_t* conv, const double* delta, const float* f, const uint8_t* fixed, const float* S, const float* Y, float* p,
                  double* longest2) {
  const int64_t M1 = memory + 1;
  for (int64_t m = 0; m < n_mol; ++m) longest2[m] = 0.0;
  for (int64_t i = 0; i < n_atoms; ++i) {
    const int64_t m = batch[i];
    if (conv[m] >= 0) continue;
    float q[3] = {0.f, 0.f, 0.f};
    if (!(fixed && fixed[i])) tn_lbfgs::atom_direction(f + 3 * i, h[m], order + m * M1, (int)M1, delta + m * (2 * M1 + 1), S, Y, n_atoms, i, q);
    for (int d = 0; d < 3; ++d) p[3 * i + d] = q[d];
    const double n2 = tn_lbfgs::dot3w(q, q);
    longest2[m] = n2 > longest2[m] ? n2 : longest2[m];
  }
}

// k_lbfgs_move (MOVE): x_prev, f_prev saved, x <- x + c p; scale [n_mol] = c (0 for a converged molecule)
void lb_move(int64_t n_mol, int64_t n_atoms, const int64_t* batch, const int64_t* conv, const uint8_t* fixed, const double* longest2,
             double max_step, double damping, float* x, const float* p, const float* f, float* x_prev, float* f_prev, float* scale) {
  for (int64_t m = 0; m < n_mol; ++m) scale[m] = conv[m] >= 0 ? 0.f : tn_lbfgs::clamp(longest2[m], max_step, damping);
  for (int64_t i = 0; i < n_atoms; ++i) {
    const int64_t m = batch[i];
    for (int d = 0; d < 3; ++d) {
      x_prev[3 * i + d] = x[3 * i + d];
      f_prev[3 * i + d] = f[3 * i + d];
    }
    if (conv[m] >= 0 || (fixed && fixed[i])) continue;
    tn_lbfgs::atom_step(x + 3 * i, scale[m], p + 3 * i);
  }
}

// Spring wells (tests/lbfgs_oracle.py: well_forces, in fp32), the launch sequence of the minimiser written as loops: the control of the
// start geometry, then per step move, forces, sums, control, direction, until every molecule has converged or max_steps is reached.
// In place on x; h_log, acc_log [max_steps + 1, n_mol] = pairs held and the accepted flag after every control.  Returns the number of
// steps taken, or -1 when a sum was not finite.
int64_t lb_wells(int64_t n_mol, int64_t n_atoms, const int64_t* batch, const float* kspring, const float* x0, float* x, const uint8_t* fixed,
                 float anharmonic, int32_t memory, double alpha, double max_step, double damping, double fmax, int64_t max_steps,
                 int64_t* conv, int32_t* h_log, int32_t* acc_log) {
  const int64_t M1 = memory + 1, NP = 6 * M1 + 4;
  std::vector<int32_t> h(n_mol), order(n_mol * M1), accepted(n_mol), ret(n_mol);
  std::vector<double> SS(n_mol * M1 * M1), SY(n_mol * M1 * M1), YY(n_mol * M1 * M1), tot(n_mol * NP), delta(n_mol * (2 * M1 + 1)), gp(n_mol),
      longest2(n_mol);
  std::vector<float> f(3 * n_atoms), x_prev(3 * n_atoms), f_prev(3 * n_atoms), p(3 * n_atoms), S(M1 * n_atoms * 3), Y(M1 * n_atoms * 3),
      scale(n_mol);
  lb_init(n_mol, memory, h.data(), order.data(), conv);
  for (int64_t step = 0;; ++step) {
    if (step > 0)
      lb_move(n_mol, n_atoms, batch, conv, fixed, longest2.data(), max_step, damping, x, p.data(), f.data(), x_prev.data(), f_prev.data(),
              scale.data());
    for (int64_t i = 0; i < n_atoms; ++i) {
      float d[3], u = 0.f;
      for (int k = 0; k < 3; ++k) {
        d[k] = x[3 * i + k] - x0[3 * i + k];
        u += d[k] * d[k];
      }
      const float w = anharmonic == 0.f ? 1.f : 1.f - 1.8f * anharmonic * u + (anharmonic * anharmonic) * (u * u);
      for (int k = 0; k < 3; ++k) f[3 * i + k] = -(kspring[i] * d[k] * w);
    }
    lb_sums(n_mol, n_atoms, batch, memory, step == 0, h.data(), order.data(), conv, x, x_prev.data(), f.data(), f_prev.data(), fixed, S.data(),
            Y.data(), tot.data());
    lb_control(n_mol, memory, alpha, max_step, damping, fmax, step == 0, step, h.data(), order.data(), conv, SS.data(), SY.data(), YY.data(),
               tot.data(), delta.data(), accepted.data(), gp.data(), ret.data());
    int64_t open = 0;
    for (int64_t m = 0; m < n_mol; ++m) {
      if (ret[m] == tn_lbfgs::LBFGS_UNUSABLE) return -1;
      h_log[step * n_mol + m] = h[m];
      acc_log[step * n_mol + m] = accepted[m];
      open += conv[m] < 0;
    }
    if (open == 0 || step == max_steps) return step;
    lb_direction(n_mol, n_atoms, batch, memory, h.data(), order.data(), conv, delta.data(), f.data(), fixed, S.data(), Y.data(), p.data(),
                 longest2.data());
  }
}

}  // extern "C"

#ifdef LBFGS_HOST_MAIN
// one non-convex well problem on heap arrays of exact size: three molecules, interleaved, a fixed atom, memory 3 so the ring wraps
int main() {
  const int64_t n_mol = 3, n = 47, max_steps = 400;
  std::vector<int64_t> batch(n), conv(n_mol);
  std::vector<float> k(n), x0(3 * n), x(3 * n);
  std::vector<uint8_t> fixed(n, 0);
  std::vector<int32_t> h_log((max_steps + 1) * n_mol), acc_log((max_steps + 1) * n_mol);
  uint32_t r = 12345u;
  auto rnd = [&r]() {
    r = r * 1664525u + 1013904223u;
    return (float)(r >> 8) / 16777216.f - 0.5f;
  };
  for (int64_t i = 0; i < n; ++i) {
    batch[i] = i % 7 == 0 ? 0 : (i % 2 ? 1 : 2);
    k[i] = 1.f + (float)batch[i];
    for (int d = 0; d < 3; ++d) {
      x0[3 * i + d] = 8.f * rnd();
      x[3 * i + d] = x0[3 * i + d] + 1.2f * rnd();
    }
  }
  fixed[5] = 1;
  const int64_t steps = lb_wells(n_mol, n, batch.data(), k.data(), x0.data(), x.data(), fixed.data(), 2.0f, 3, 70.0, 0.2, 1.0, 1e-3, max_steps,
                                 conv.data(), h_log.data(), acc_log.data());
  int64_t rejected = 0;
  for (int64_t s = 1; s <= steps; ++s)
    for (int64_t m = 0; m < n_mol; ++m) rejected += (conv[m] < 0 || s < conv[m]) && !acc_log[s * n_mol + m];
  printf("steps %lld converged_at %lld %lld %lld rejected %lld\n", (long long)steps, (long long)conv[0], (long long)conv[1], (long long)conv[2],
         (long long)rejected);
  return steps > 0 && conv[0] >= 0 && conv[1] >= 0 && conv[2] >= 0 ? 0 : 1;
}
#endif
