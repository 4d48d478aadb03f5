// TEST INFRASTRUCTURE ONLY: the host parts of the captured loops' shared device layer (torchmd-net_amd/csrc/tn_loop.h) compiled for
// the host (hipcc --cuda-host-only) and loaded through ctypes by tests/loop_host_mirror.py.  The statements are the header's own;
// tests/test_loop_host.py compares them with a Python spec without a GPU.
#include <stdint.h>

#include "../torchmd-net_amd/csrc/tn_dimer_math.h"
#include "../torchmd-net_amd/csrc/tn_irc_math.h"
#include "../torchmd-net_amd/csrc/tn_loop.h"

extern "C" {

int loop_mol_slices(int64_t N, int64_t B) { return tn::mol_slices(N, B); }

// out = {i0, i1, filter} of slice s of molecule m; member[i] = 1 for every atom of the slice that the reduction would add
void loop_slice_range(const int* counts, const int* mstart, const int* mend, int N, int S, const int64_t* batch, int m, int s, int* out,
                      uint8_t* member) {
  const tn::SliceRange r = tn::mol_slice_range(counts, mstart, mend, N, S, batch, m, s);
  out[0] = r.i0;
  out[1] = r.i1;
  out[2] = r.filter;
  for (int i = r.i0; i < r.i1; ++i) member[i] = !tn::slice_skips(r, batch, i, m);
}

// walks n arrays of count[k] elements of elem[k] bytes (1, 4 or 8) from `ws`: where each starts, what was handed out, and what the
// size entry of such a workspace answers
void loop_carve(uint64_t ws, int64_t n, const int64_t* count, const int32_t* elem, uint64_t* starts, uint64_t* handed_out, uint64_t* entry) {
  const auto walk = [&](tn::LoopCarver& c, uint64_t* at) {
    for (int64_t k = 0; k < n; ++k) {
      const void* p = elem[k] == 8 ? (void*)c.take<double>(count[k]) : elem[k] == 4 ? (void*)c.take<float>(count[k]) : (void*)c.take<char>(count[k]);
      if (at) at[k] = (uint64_t)(uintptr_t)p;
    }
  };
  tn::LoopCarver c(reinterpret_cast<void*>((uintptr_t)ws));
  walk(c, starts);
  *handed_out = c.bytes();
  *entry = tn::layout_bytes([&](tn::LoopCarver& z) { walk(z, nullptr); });
}

uint64_t loop_step_roundtrip(uint64_t step, uint32_t* head) {
  tn::loop_set_step(head, step);
  return tn::loop_step(head);
}

// the three shapes slice_sums is called with: 0 FIRE's four sums (the last a maximum), 1 the IRC's six, 2 the dimer's FIRE and
// partner sums in one row; -> K
int loop_slice_sums(int shape, const double* slices, int S, int stride, double* out) {
  constexpr int kDimer = 4 + tn_dimer::N_PART;
  if (shape == 0) tn::slice_sums<4, 8u>(slices, S, stride, out);
  if (shape == 1) tn::slice_sums<tn_irc::N_SUMS, tn_irc::kMaxMask>(slices, S, stride, out);
  if (shape == 2) tn::slice_sums<kDimer, 8u>(slices, S, stride, out);
  return shape == 0 ? 4 : shape == 1 ? (int)tn_irc::N_SUMS : kDimer;
}

void loop_head_reset(uint32_t* head, uint64_t step0, int cause_word) { tn::loop_head_reset(head, step0, cause_word); }

int loop_status_result(const uint32_t* head, int cause_word, uint64_t* host, int n_host) {
  return tn::loop_status_result(head, cause_word, host, n_host);
}

// fire_load of `unit` -> state = {dt, alpha}, counts = {n_pos, converged_at}
void loop_fire_load(double* dt, double* alpha, int64_t* conv, int32_t* n_pos, float* coef, const double* start, int unit, int fresh,
                    double* state, int64_t* counts) {
  tn_min::FireState s;
  tn::fire_load(tn::FireUnits{dt, alpha, conv, n_pos, coef, start}, unit, fresh != 0, &s);
  state[0] = s.dt;
  state[1] = s.alpha;
  counts[0] = s.n_pos;
  counts[1] = s.converged_at;
}

// fire_store of `unit` from state / counts (as above) and coef3, then FireRows::write on the seven rows (each may be NULL)
void loop_fire_store(double* dt, double* alpha, int64_t* conv, int32_t* n_pos, float* coef, int unit, const double* state,
                     const int64_t* counts, const float* coef3, const float* energy, const double* sums4, double fmax2, float* epot_row,
                     float* fmax_row, double* sums_row, float* coef_row, double* dt_row, double* alpha_row, int64_t* conv_row) {
  tn_min::FireState s;
  s.dt = state[0];
  s.alpha = state[1];
  s.n_pos = (int32_t)counts[0];
  s.converged_at = counts[1];
  tn::fire_store(tn::FireUnits{dt, alpha, conv, n_pos, coef, nullptr}, unit, s, coef3);
  const tn::FireRows rows = {epot_row, fmax_row, sums_row, coef_row, dt_row, alpha_row, conv_row};
  rows.write(unit, energy, sums4, fmax2, coef3, s);
}

}  // extern "C"
