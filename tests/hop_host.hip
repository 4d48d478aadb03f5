// TEST INFRASTRUCTURE ONLY: the arithmetic of the device-resident minima hopping (torchmd-net_amd/csrc/tn_hop_math.h) compiled for the
// host (hipcc --cuda-host-only), one plain loop per kernel body, loaded through ctypes by tests/hop_host_mirror.py.  The statements
// are the ones a GPU lane runs, and the sums are added in the device's order: in a slice thread t of 256 takes atoms i0 + t,
// i0 + t + 256, ... in turn; the 64 lanes of a wave by the xor tree 1, 2, ... 32; the four waves left to right; the slices in slice
// order.  A walker's atoms are those with batch[i] = b among all atoms, as on the device without a graph workspace.
#pragma clang fp contract(off)
#include <stdint.h>

#include <vector>

#include "../include/tmdnet_amd.h"
#include "../torchmd-net_amd/csrc/tn_hop_math.h"

namespace {

using namespace tn_hop;

struct Host {
  int N, B, cap, W, S;
  std::vector<Walker> w;
  std::vector<Decision> d;
  std::vector<double> tot;
  std::vector<float> xk, vk;
  uint64_t step;
  uint32_t status;
};

int slices(int64_t N, int64_t B) {  // tn_loop.h's mol_slices
  if (B <= 0 || N <= 1024 * B) return 1;
  const int64_t s = (N + 1024 * B - 1) / (1024 * B);
  return (int)(s > 256 ? 256 : s);
}

Ring ring_of(const tmdnet_hop_args& a, int cap, int m) {
  Ring r;
  r.energy = a.ring_energy + (int64_t)m * cap;
  r.found_at = a.ring_found + (int64_t)m * cap;
  r.visits = a.ring_visits + (int64_t)m * cap;
  return r;
}

// K sums of walker m over all its atoms in the device's order.  term(i, t[K]); entry k of `maxmask` takes the maximum.
template <int K, class Term>
void tree_sums(const Host& h, const int64_t* batch, int m, unsigned maxmask, Term term, double* out) {
  static double acc[256][K];
  double total[K];
  for (int k = 0; k < K; ++k) total[k] = 0.0;
  for (int s = 0; s < h.S; ++s) {
    const int i0 = (int)((int64_t)h.N * s / h.S), i1 = (int)((int64_t)h.N * (s + 1) / h.S);
    for (int t = 0; t < 256; ++t) {
      for (int k = 0; k < K; ++k) acc[t][k] = 0.0;
      for (int i = i0 + t; i < i1; i += 256) {
        if (batch && batch[i] != m) continue;
        double tm[K];
        term(i, tm);
        for (int k = 0; k < K; ++k) {
          if ((maxmask >> k) & 1u)
            acc[t][k] = tm[k] > acc[t][k] ? tm[k] : acc[t][k];
          else
            acc[t][k] += tm[k];
        }
      }
    }
    double wave[4][K];
    for (int w = 0; w < 4; ++w) {
      for (int o = 1; o < 64; o <<= 1) {
        double nxt[64][K];
        for (int l = 0; l < 64; ++l)
          for (int k = 0; k < K; ++k) {
            const double mine = acc[w * 64 + l][k], other = acc[w * 64 + (l ^ o)][k];
            nxt[l][k] = ((maxmask >> k) & 1u) ? (other > mine ? other : mine) : mine + other;
          }
        for (int l = 0; l < 64; ++l)
          for (int k = 0; k < K; ++k) acc[w * 64 + l][k] = nxt[l][k];
      }
      for (int k = 0; k < K; ++k) wave[w][k] = acc[w * 64][k];
    }
    double slice[K];
    for (int k = 0; k < K; ++k) {
      if ((maxmask >> k) & 1u) {
        double mx = wave[0][k];
        for (int w = 1; w < 4; ++w) mx = wave[w][k] > mx ? wave[w][k] : mx;
        slice[k] = mx;
      } else {
        slice[k] = ((wave[0][k] + wave[1][k]) + wave[2][k]) + wave[3][k];
      }
    }
    for (int k = 0; k < K; ++k) {
      if (h.S == 1)
        total[k] = slice[k];
      else if ((maxmask >> k) & 1u)
        total[k] = slice[k] > total[k] ? slice[k] : total[k];
      else
        total[k] = total[k] + slice[k];
    }
  }
  for (int k = 0; k < K; ++k) out[k] = total[k];
}

// k_hop_reduce (+ k_hop_finish) for walker m
void reduce(Host& h, const HopParams& p, const tmdnet_hop_args& a, int m) {
  const Walker& w = h.w[m];
  double* out = h.tot.data() + (int64_t)m * h.W;
  if (w.phase == PH_QUENCH || w.phase == PH_MD) {
    tree_sums<4>(h, a.batch, m, 8u, [&](int i, double* t) {
      float tm[4];
      const int fx = a.fixed && a.fixed[i];
      if (w.phase == PH_QUENCH)
        quench_terms(a.vel + 3 * i, a.forces + 3 * i, fx, tm);
      else
        md_terms(a.vel + 3 * i, a.forces + 3 * i, a.hk[i], a.mass[i], fx, tm);
      for (int k = 0; k < 4; ++k) t[k] = (double)tm[k];
    }, out);
    return;
  }
  if (w.phase == PH_LAUNCH) {
    const float cen[3] = {(float)w.cen[0], (float)w.cen[1], (float)w.cen[2]};
    tree_sums<kLaunch>(h, a.batch, m, 0u, [&](int i, double* t) {
      launch_terms(a.pos + 3 * i, a.vel + 3 * i, a.forces + 3 * i, a.mass[i], cen, a.fixed && a.fixed[i], t);
    }, out);
    return;
  }
  const double E = (double)a.energy[m];
  for (int ref = 0; ref <= p.capacity; ++ref) {
    if (!ref_considered(w, a.ring_energy + (int64_t)m * p.capacity, p.capacity, ref, E, p.energy_tol)) continue;
    const float* b = ref == 0 ? (w.has_cur ? a.cur_pos : a.pos) : a.ring_pos + (int64_t)(ref - 1) * h.N * 3;
    tree_sums<kPair>(h, a.batch, m, 0u, [&](int i, double* t) { pair_terms(a.pos + 3 * i, b + 3 * i, t); }, out + ref * kPair);
  }
}

}  // namespace

extern "C" {

void* hop_host_create(int64_t N, int64_t B, int32_t capacity) {
  Host* h = new Host;
  h->N = (int)N;
  h->B = (int)B;
  h->cap = capacity;
  h->W = kPair * (capacity + 1);
  h->S = slices(N, B);
  h->w.assign(B, Walker());
  h->d.assign(B, Decision());
  h->tot.assign((size_t)B * h->W, 0.0);
  h->xk.assign((size_t)N * 3, 0.f);
  h->vk.assign((size_t)N * 3, 0.f);
  h->step = 0;
  h->status = 0;
  return h;
}

void hop_host_destroy(void* hp) { delete static_cast<Host*>(hp); }

// k_hop_reset
void hop_host_reset(void* hp, const tmdnet_hop_args* a, uint64_t step0, const double* kT0, const double* ediff0, int32_t keep) {
  Host& h = *static_cast<Host*>(hp);
  const HopParams p = hop_params(*a);
  h.step = step0;
  h.status = 0;
  for (int m = 0; m < h.B; ++m) {
    Walker& w = h.w[m];
    walker_reset(&w, p, kT0[m], ediff0[m], keep);
    h.d[m].action = ACT_NONE;
    a->kT[m] = w.kT;
    a->ediff[m] = w.ediff;
    a->cur_energy[m] = w.e_cur;
    a->best_energy[m] = w.e_best;
    a->phase[m] = w.phase;
    for (int k = 0; k < kCounters; ++k) a->counters[(int64_t)m * kCounters + k] = w.n[k];
  }
  for (int64_t i = 0; i < (int64_t)h.N * 3; ++i) {
    h.xk[i] = a->pos[i];
    h.vk[i] = a->vel[i];
  }
}

// the launches of tmdnet_hop_advance as loops.  `overflowed`: what counts[2] would say of this step's evaluation.
void hop_host_advance(void* hp, const tmdnet_hop_args* ap, int32_t overflowed) {
  Host& h = *static_cast<Host*>(hp);
  const tmdnet_hop_args& a = *ap;
  const HopParams p = hop_params(a);
  if (h.status) return;
  if (overflowed) {
    h.status = 1;
    for (int64_t i = 0; i < (int64_t)h.N * 3; ++i) {
      a.pos[i] = h.xk[i];
      a.vel[i] = h.vk[i];
    }
    return;
  }
  for (int m = 0; m < h.B; ++m) reduce(h, p, a, m);
  const uint64_t step = h.step + 1;
  for (int m = 0; m < h.B; ++m)
    if (!walker_usable(h.w[m], ring_of(a, h.cap, m), p, h.tot.data() + (int64_t)m * h.W, (double)a.energy[m])) {
      h.status = 2;
      return;
    }
  for (int m = 0; m < h.B; ++m) {
    Walker& w = h.w[m];
    Decision& d = h.d[m];
    double log[kSumsLog];
    const double* tot = h.tot.data() + (int64_t)m * h.W;
    walker_control(&w, ring_of(a, h.cap, m), p, tot, (double)a.energy[m], (int64_t)step, &d, log);
    a.kT[m] = w.kT;
    a.ediff[m] = w.ediff;
    a.cur_energy[m] = w.e_cur;
    a.best_energy[m] = w.e_best;
    a.phase[m] = w.phase;
    for (int k = 0; k < kCounters; ++k) a.counters[(int64_t)m * kCounters + k] = w.n[k];
    if (a.epot_row) a.epot_row[m] = a.energy[m];
    if (a.fmax_row) a.fmax_row[m] = d.phase == PH_QUENCH || d.phase == PH_MD ? (float)sqrt(tot[3]) : 0.f;
    if (a.ekin_row) a.ekin_row[m] = d.phase == PH_MD ? (float)tot[0] : 0.f;
    if (a.phase_row) a.phase_row[m] = d.phase;
    if (a.outcome_row) a.outcome_row[m] = d.outcome;
    if (a.sums_row)
      for (int k = 0; k < kSumsLog; ++k) a.sums_row[(int64_t)m * kSumsLog + k] = log[k];
    if (a.coef_row) {
      float* c = a.coef_row + (int64_t)m * kCoefLog;
      for (int k = 0; k < 3; ++k) {
        c[k] = d.coef[k];
        c[3 + k] = d.u[k];
        c[6 + k] = d.w[k];
      }
      c[9] = d.vscale;
    }
  }
  h.step = step;
  for (int i = 0; i < h.N; ++i) {
    const int64_t m = a.batch ? a.batch[i] : 0;
    if (m < 0 || m >= h.B) continue;
    const Decision& d = h.d[m];
    for (int k = 0; k < 3; ++k) {
      h.xk[3 * i + k] = a.pos[3 * i + k];
      h.vk[3 * i + k] = a.vel[3 * i + k];
      if (a.forces_keep) a.forces_keep[3 * i + k] = a.forces[3 * i + k];
    }
    float* ring = d.slot >= 0 ? a.ring_pos + ((int64_t)d.slot * h.N + i) * 3 : nullptr;
    atom_apply(d, p.dt, p.seed, (uint32_t)i, a.fixed && a.fixed[i], a.hk[i], a.sig[i], a.forces + 3 * i, a.pos + 3 * i, a.vel + 3 * i,
               a.cur_pos + 3 * i, ring, a.best_pos + 3 * i);
  }
}

void hop_host_status(void* hp, uint64_t out[2]) {
  const Host& h = *static_cast<Host*>(hp);
  out[0] = h.step;
  out[1] = h.status;
}

// the 18 sums of a pair of n atoms (fp32), added in index order
void hop_host_pair_sums(int64_t n, const float* a, const float* b, double* out) {
  for (int k = 0; k < kPair; ++k) out[k] = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    double t[kPair];
    pair_terms(a + 3 * i, b + 3 * i, t);
    for (int k = 0; k < kPair; ++k) out[k] += t[k];
  }
}

double hop_host_rmsd2(const double* sums, int32_t align) { return pair_rmsd2(sums, align); }

void hop_host_launch_solve(const double* t, int32_t align, float* u, float* w, int32_t* singular) {
  int s;
  launch_solve(t, align, u, w, &s);
  *singular = s;
}

// the launch draw of `n` atoms: v[n, 3] = (vscale sig_i) xi
void hop_host_noise(uint64_t seed, uint64_t hop, int64_t n, float* xi) {
  for (int64_t i = 0; i < n; ++i) launch_noise(seed, (uint32_t)hop, (uint32_t)(hop >> 32), (uint32_t)i, xi + 3 * i);
}

}  // extern "C"
