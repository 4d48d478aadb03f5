// TEST INFRASTRUCTURE ONLY: the host parts of the captured loops' shared device layer (torchmd-net_amd/csrc/tn_loop.h) compiled for
// the host (hipcc --cuda-host-only) and loaded through ctypes by tests/loop_host_mirror.py.  The statements are the header's own;
// tests/test_loop_host.py compares them with a Python spec without a GPU.
#include <stdint.h>

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

}  // extern "C"
