// TEST INFRASTRUCTURE ONLY: the committee reduction (torchmd-net_amd/csrc/tn_committee_math.h) compiled for the host
// (hipcc --cuda-host-only), one plain loop per kernel, loaded through ctypes by tests/committee_host_mirror.py.  The statements are the
// ones a GPU lane runs; tests/test_committee_host.py compares them with tests/committee_oracle.py without a GPU.  With
// -DCOMMITTEE_HOST_MAIN the file is a program of its own (for the host sanitizers).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../torchmd-net_amd/csrc/tn_committee_math.h"

namespace {

// E [M, B], F [M, N, 3] stacked (the test's layout; the device pass takes M pointers).  The atoms are visited from the LAST to the
// first: the integer maximum does not depend on the order.
template <int M>
void reduce_m(const float* E, const float* F, int64_t N, int64_t B, const int64_t* batch, float* energy, float* forces, float* energy_std,
              float* forces_std, float* deviation, float* max_dev, int64_t* max_atom) {
  std::vector<uint64_t> packed((size_t)B, 0);
  for (int64_t i = N - 1; i >= 0; --i) {
    double var[3];
    for (int c = 0; c < 3; ++c) {
      float x[M];
      for (int k = 0; k < M; ++k) x[k] = F[((int64_t)k * N + i) * 3 + c];
      var[c] = tn_committee::mean_std<M>(x, forces + i * 3 + c, forces_std + i * 3 + c);
    }
    const float d = tn_committee::deviation(var[0], var[1], var[2]);
    deviation[i] = d;
    const int64_t m = batch ? batch[i] : 0;
    if (m < 0 || m >= B) continue;
    const uint64_t key = tn_committee::pack(d, (uint32_t)i);
    if (key > packed[(size_t)m]) packed[(size_t)m] = key;
  }
  for (int64_t m = 0; m < B; ++m) {
    float x[M];
    for (int k = 0; k < M; ++k) x[k] = E[(int64_t)k * B + m];
    tn_committee::mean_std<M>(x, energy + m, energy_std + m);
    tn_committee::unpack(packed[(size_t)m], max_dev + m, max_atom + m);
  }
}

}  // namespace

extern "C" {

int32_t committee_reduce(int32_t M, const float* E, const float* F, int64_t N, int64_t B, const int64_t* batch, float* energy, float* forces,
                         float* energy_std, float* forces_std, float* deviation, float* max_dev, int64_t* max_atom) {
  switch (M) {
#define CASE(m) \
  case m:       \
    reduce_m<m>(E, F, N, B, batch, energy, forces, energy_std, forces_std, deviation, max_dev, max_atom); \
    return 0;
    CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#undef CASE
  }
  return 1;
}

int32_t committee_gate_fires(float D, float threshold) { return tn_committee::gate_fires(D, threshold) ? 1 : 0; }

int32_t committee_max_members() { return tn_committee::kMaxMembers; }

}  // extern "C"

#ifdef COMMITTEE_HOST_MAIN
int main() {
  const int M = 5, N = 70, B = 4;
  std::vector<float> E(M * B), F(M * N * 3), e(B), es(B), f(N * 3), fs(N * 3), d(N), D(B);
  std::vector<int64_t> batch(N), a(B);
  for (int k = 0; k < M * B; ++k) E[k] = 1e5f + 0.01f * (float)(k % 7);
  for (int k = 0; k < M * N * 3; ++k) F[k] = 0.001f * (float)((k * 37) % 101) - 0.05f;
  F[3 * 11 + 1] = NAN;                                           // member 0, atom 11
  for (int i = 0; i < N; ++i) batch[i] = i % 5 == 4 ? -1 : i % 3;  // unsorted, some atoms in no molecule, molecule 3 empty
  if (committee_reduce(M, E.data(), F.data(), N, B, batch.data(), e.data(), f.data(), es.data(), fs.data(), d.data(), D.data(), a.data())) return 1;
  if (committee_reduce(17, E.data(), F.data(), N, B, batch.data(), e.data(), f.data(), es.data(), fs.data(), d.data(), D.data(), a.data()) != 1) return 1;
  double s = 0.0;
  for (int m = 0; m < B; ++m) s += (double)e[m] + (double)es[m] + (double)a[m];
  printf("committee_host ok %.6e %d %d %d\n", s, (int)a[3], committee_gate_fires(D[11 % 3], 1e30f), committee_gate_fires(0.5f, 1.0f));
  return 0;
}
#endif
