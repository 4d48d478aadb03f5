// Virial of the energy+force pass (tn_virial.hip): W_m[a][b] = - sum over the pairs p of molecule m of pdelta_p[a] * g_delta_p[b].
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "tn_kernels.h"

namespace tn {

// slices a molecule's atom range is cut into by the reduction (1: one block per molecule does it all)
int virial_slices(int64_t N, int64_t B);
// scratch of one call: the per-atom partials [N, 9] and, with more than one slice, the slice sums [B, S, 9]
size_t virial_workspace_bytes(int64_t N, int64_t B);
// launch_force_gather (same forces, bit for bit; `direct` is not taken: the property heads are refused) that also leaves the nine
// products of every row's pairs in the scratch, then the per-molecule reduction into virial [B, 9] (row-major a * 3 + b).
// `batch`: the molecule index in the engine's atom order (read only when the graph says the ranges are not contiguous).
void launch_force_virial(const Graph& g, int N, int B, const float* g_delta, const int* perm, const int64_t* batch, float* forces,
                         float* virial, void* scratch, hipStream_t s);

}  // namespace tn
