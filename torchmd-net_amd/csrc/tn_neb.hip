// Device-resident nudged elastic band: the kernels that sit between two energy+force evaluations of a captured step, so that K band
// steps replay as one HIP graph with no host work in between.  A band is M images of the same n atoms, a call has G bands; rows are
// image-major, atom a of image i of band g is row (g M + i) n + a, and the evaluation sees G M molecules of n atoms.  Images 0 and
// M - 1 of every band never move.  The arithmetic is tn_neb_math.h (tangents, band force) and tn_min_math.h (FIRE, one controller per
// band).  The scheme is stated with the entries in include/tmdnet_amd.h.
//
// One step, after the energies E and forces F at the current positions are known - four launches:
//   path      grid (image, slice): the five path sums a, b, c, p, q of every interior image   (fp32 terms, fp64 sums, fixed order),
//             and the number of atoms that are not fixed (none: the image has no degree of freedom and needs no tangent)
//   project   grid (image, slice): every block derives its image's weights and its two coefficients from the slice sums and the band's
//             energies itself (every block of an image computes the same bits), writes F_neb into the workspace and reduces the
//             FIRE terms v.F_neb, F_neb.F_neb, v.v, max |F_neb|^2 per image
//   control   ONE block, bands strided: the images' sums added in image order, tn_min::fire_control, the status word, the logs
//   atoms     per atom: accept (F_neb -> forces_keep, or the saved state back after an overflow) and, in MIDDLE, the move
// CLOSE omits the move, OPEN is the move alone from the coefficients the workspace holds and the kept F_neb.
//
// Reductions are tn_loop.h's, as in k_min_reduce: threads stride the atoms of a slice, lanes add by the wave's xor tree, waves in
// turn, slices in slice order.  No floating-point atomics: repeats are bit-identical.
//
// Overflow, non-finite sums and unusable tangents follow the minimiser's protocol: the controller is the only kernel that writes
// the status word; an overflowed evaluation latches status 1 and the per-atom kernel puts x and v back; a band that still moves
// and has an energy that is not finite, a tangent of length zero or a sum that is not finite latches status 2 (the cause in header
// word 5) before anything of that step is written.  From then on every launch returns at once until tmdnet_neb_reset.
#include <cmath>

#include "tmdnet_amd.h"
#include "tn_common.h"
#include "tn_loop.h"
#include "tn_model.h"
#include "tn_neb_math.h"

namespace tn {

namespace {

// The header: six uint32 words, then two doubles.  Words 0 / 1 the step counter (lo / hi), 2 the status, 3 "reset, not yet controlled",
constexpr int kNebClimbWord = 4;       // 1: the climbing image is on
constexpr int kNebCauseWord = 5;       // which input was unusable when status 2 was latched (tn_neb::NEB_*)
constexpr int kNebHeadWords = 6;       // words the status entry reads back
constexpr size_t kNebStartByte = 32;   // dt0, alpha0 (fp64)
static_assert(kNebClimbWord > 3 && kNebCauseWord != kNebClimbWord && kNebCauseWord < kNebHeadWords, "header words must not overlap");
static_assert(kNebHeadWords * sizeof(uint32_t) <= kNebStartByte && kNebStartByte % sizeof(double) == 0 &&
                  kNebStartByte + 2 * sizeof(double) <= kHeaderBytes,
              "the start values lie behind the header words, aligned, inside the header");

struct NebState {  // views into the caller's workspace
  uint32_t* head;       // [0] step lo, [1] step hi, [2] status, [3] 1 = reset, not yet controlled, [4] climb, [5] cause of status 2
  double* start;        // [0] dt0, [1] alpha0 (header bytes 32..47, behind the six words)
  double* dt;           // [G]
  double* alpha;        // [G]
  int64_t* conv;        // [G] converged_at
  int32_t* n_pos;       // [G]
  float* coef;          // [G, 3] c_v, c_f, d of the next move
  double* img_sums;     // [G M, 5] a, b, c, p, q
  double* img_w;        // [G M, 2] w+, w-
  float* img_s;         // [G M, 2] s+, s-
  int32_t* img_why;     // [G M] tn_neb::NEB_*
  double* path_slices;  // [G M, S, 6] a, b, c, p, q and the number of atoms that are not fixed
  double* fire_slices;  // [G M, S, 4]
  float* x_keep;        // [N, 3] positions before the last move
  float* v_keep;        // [N, 3]
  float* f_neb;         // [N, 3] F_neb of the evaluation being controlled
};

NebState neb_layout(LoopCarver& c, int64_t n, int64_t M, int64_t G) {
  const size_t g = (size_t)(G > 0 ? G : 0), gm = g * (size_t)(M > 0 ? M : 0), N = gm * (size_t)(n > 0 ? n : 0);
  const size_t S = (size_t)mol_slices(n, 1);  // slices per image: one image is the molecule
  NebState st;
  st.head = c.take<uint32_t>(kHeaderBytes / sizeof(uint32_t));
  st.start = reinterpret_cast<double*>(reinterpret_cast<char*>(st.head) + kNebStartByte);
  st.dt = c.take<double>(g);
  st.alpha = c.take<double>(g);
  st.conv = c.take<int64_t>(g);
  st.n_pos = c.take<int32_t>(g);
  st.coef = c.take<float>(g * 3);
  st.img_sums = c.take<double>(gm * 5);
  st.img_w = c.take<double>(gm * 2);
  st.img_s = c.take<float>(gm * 2);
  st.img_why = c.take<int32_t>(gm);
  st.path_slices = c.take<double>(gm * S * 6);
  st.fire_slices = c.take<double>(gm * S * 4);
  st.x_keep = c.take<float>(N * 3);
  st.v_keep = c.take<float>(N * 3);
  st.f_neb = c.take<float>(N * 3);
  return st;
}

size_t neb_bytes(int64_t n, int64_t M, int64_t G) {
  return layout_bytes([&](LoopCarver& c) { neb_layout(c, n, M, G); });
}

NebState carve_neb(void* ws, int64_t n, int64_t M, int64_t G) {
  LoopCarver c(ws);
  return neb_layout(c, n, M, G);
}

struct NebGeom {
  int n, M, G, S;
};

// d+ and d- of atom a of interior image `img` (rows img n + a and its two neighbours' n rows away)
__device__ __forceinline__ void neb_load_diff(const float* __restrict__ pos, int64_t row, int n, float dp[3], float dm[3]) {
  float xp[3], x[3], xn[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    xp[d] = pos[(row - n) * 3 + d];
    x[d] = pos[row * 3 + d];
    xn[d] = pos[(row + n) * 3 + d];
  }
  tn_neb::path_diff(xp, x, xn, dp, dm);
}

// grid (G M, S): slice s of interior image img -> path_slices[img, s, 0..5]
__global__ __launch_bounds__(kThreads) void k_neb_path(NebState st, NebGeom g, const int* __restrict__ counts,
                                                          const float* __restrict__ pos, const float* __restrict__ forces,
                                                          const uint8_t* __restrict__ fixed) {
  __shared__ double sh[6][kThreads / 64];
  if (st.head[kHeadStatus]) return;           // frozen
  if (counts && counts[2]) return;  // overflowed: stale forces, the controller latches it
  const int img = blockIdx.x, s = blockIdx.y, i = img % g.M;
  if (i == 0 || i == g.M - 1) return;  // an endpoint has no tangent
  const int a0 = (int)((int64_t)g.n * s / g.S), a1 = (int)((int64_t)g.n * (s + 1) / g.S);
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int a = a0 + (int)threadIdx.x; a < a1; a += kThreads) {
    const int64_t row = (int64_t)img * g.n + a;
    const int fx = fixed && fixed[a];
    float dp[3], dm[3], f[3], t[5];
    neb_load_diff(pos, row, g.n, dp, dm);
#pragma unroll
    for (int d = 0; d < 3; ++d) f[d] = forces[row * 3 + d];
    tn_neb::path_terms(dp, dm, f, fx, t);
#pragma unroll
    for (int k = 0; k < 5; ++k) acc[k] += (double)t[k];
    acc[5] += fx ? 0.0 : 1.0;  // (a count: exact)
  }
  block_reduce_waves<6, 0u>(acc, sh);
  if (threadIdx.x == 0) block_reduce_rows<6, 0u>(sh, st.path_slices + ((int64_t)img * g.S + s) * 6);
}

// grid (G M, S), after k_neb_path: the image's coefficients (every block of the image computes the same bits; the block of slice 0
// records them), F_neb of the slice's atoms into the workspace, fire_slices[img, s, 0..3] = v.F_neb, F_neb.F_neb, v.v, max |F_neb|^2
__global__ __launch_bounds__(kThreads) void k_neb_project(NebState st, NebGeom g, const int* __restrict__ counts,
                                                             const float* __restrict__ pos, const float* __restrict__ vel,
                                                             const float* __restrict__ forces, const float* __restrict__ energy,
                                                             const uint8_t* __restrict__ fixed, double spring_k) {
  __shared__ double sh[4][kThreads / 64];
  if (st.head[kHeadStatus]) return;
  if (counts && counts[2]) return;
  const int img = blockIdx.x, s = blockIdx.y, i = img % g.M;
  const int a0 = (int)((int64_t)g.n * s / g.S), a1 = (int)((int64_t)g.n * (s + 1) / g.S);
  if (i == 0 || i == g.M - 1) {  // an endpoint feels no band force
    for (int a = a0 + (int)threadIdx.x; a < a1; a += kThreads) {
      const int64_t row = (int64_t)img * g.n + a;
#pragma unroll
      for (int d = 0; d < 3; ++d) st.f_neb[row * 3 + d] = 0.f;
    }
    return;
  }
  double S5[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w[2];  // [5]: the number of atoms that are not fixed
  float sc[2];
  const double* sl = st.path_slices + (int64_t)img * g.S * 6;
  for (int k = 0; k < g.S; ++k)
#pragma unroll
    for (int j = 0; j < 6; ++j) S5[j] += sl[k * 6 + j];
  const int why = tn_neb::image_control(energy + (int64_t)(img - i), g.M, i, S5, spring_k, st.head[kNebClimbWord] != 0, S5[5] > 0.0, w, sc);
  if (s == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < 5; ++j) st.img_sums[(int64_t)img * 5 + j] = S5[j];
    st.img_w[img * 2 + 0] = w[0];
    st.img_w[img * 2 + 1] = w[1];
    st.img_s[img * 2 + 0] = sc[0];
    st.img_s[img * 2 + 1] = sc[1];
    st.img_why[img] = why;
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int a = a0 + (int)threadIdx.x; a < a1; a += kThreads) {
    const int64_t row = (int64_t)img * g.n + a;
    const int fx = fixed && fixed[a];
    float dp[3], dm[3], f[3], v[3], fn[3], t[3];
    neb_load_diff(pos, row, g.n, dp, dm);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      f[d] = forces[row * 3 + d];
      v[d] = vel[row * 3 + d];
    }
    if (fx) {  // a fixed atom is outside the band: it keeps the force of the evaluation
#pragma unroll
      for (int d = 0; d < 3; ++d) fn[d] = f[d];
    } else {
      tn_neb::project(f, dp, dm, sc[0], sc[1], fn);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) st.f_neb[row * 3 + d] = fn[d];
    tn_min::atom_terms(v, fn, fx, t);
    acc[0] += (double)t[0];
    acc[1] += (double)t[1];
    acc[2] += (double)t[2];
    acc[3] = (double)t[1] > acc[3] ? (double)t[1] : acc[3];
  }
  block_reduce_waves<4, 8u>(acc, sh);
  if (threadIdx.x == 0) block_reduce_rows<4, 8u>(sh, st.fire_slices + ((int64_t)img * g.S + s) * 4);
}

struct NebCtlArgs {
  NebGeom g;
  tn_min::FireParams p;
  const int* counts;  // the graph's counters, or NULL
  const float* energy;
  float* epot_row;      // [G, M]
  FireRows rows;        // [G, ...]; its epot is NULL: the band's energy row is epot_row
  double* path_row;     // [G, M, 5]
  double* weights_row;  // [G, M, 2]
  float* tcoef_row;     // [G, M, 2]
  int32_t* climber_row; // [G]
  NebState st;
};

// the FIRE sums of band b (per image the slices in slice order, then the images in image order), its state (after a reset: the
// start values of the header) and the largest cause among its interior images
__device__ __forceinline__ int neb_load(const NebCtlArgs& a, int b, bool fresh, double sums[4], tn_min::FireState* s) {
  sums[0] = sums[1] = sums[2] = sums[3] = 0.0;
  int why = 0;
  for (int i = 1; i < a.g.M - 1; ++i) {
    const int img = b * a.g.M + i;
    double t[4];
    slice_sums<4, 8u>(a.st.fire_slices + (int64_t)img * a.g.S * 4, a.g.S, 4, t);
    sums[0] += t[0];
    sums[1] += t[1];
    sums[2] += t[2];
    sums[3] = t[3] > sums[3] ? t[3] : sums[3];
    why = a.st.img_why[img] > why ? a.st.img_why[img] : why;
  }
  fire_load(fire_units(a.st), b, fresh, s);
  return why;
}

// ONE block striding the bands, after k_neb_project: optimiser_control (tn_loop.h) with FIRE's two passes and the tangents' causes
__global__ __launch_bounds__(kThreads) void k_neb_control(NebCtlArgs a) {
  optimiser_control(
      a.st.head, a.counts, kNebCauseWord, true, a.g.G,
      [&](int b, bool fresh, uint64_t step) {
        double sums[4];
        float coef[3];
        tn_min::FireState s;
        int c = neb_load(a, b, fresh, sums, &s);
        if (s.converged_at >= 0) return 0;  // a band that has converged looks at nothing
        if (!c && tn_min::fire_control(&s, a.p, sums[0], sums[1], sums[2], sums[3], (int64_t)step, coef) == tn_min::FIRE_UNUSABLE)
          c = tn_neb::NEB_BAD_SUMS;
        return c;
      },
      [&](int b, bool fresh, uint64_t step) {
        const int M = a.g.M;
        double sums[4];
        float coef[3];
        tn_min::FireState s;
        neb_load(a, b, fresh, sums, &s);
        tn_min::fire_control(&s, a.p, sums[0], sums[1], sums[2], sums[3], (int64_t)step, coef);
        fire_store(fire_units(a.st), b, s, coef);
        if (a.epot_row)
          for (int i = 0; i < M; ++i) a.epot_row[b * M + i] = a.energy[b * M + i];
        a.rows.write(b, nullptr, sums, sums[3], coef, s);
        if (a.climber_row) a.climber_row[b] = tn_neb::climber(a.energy + (int64_t)b * M, M);
        for (int i = 0; i < M; ++i) {  // an endpoint's rows are zero
          const int64_t img = (int64_t)b * M + i;
          const bool inner = i > 0 && i < M - 1;
          if (a.path_row)
#pragma unroll
            for (int k = 0; k < 5; ++k) a.path_row[img * 5 + k] = inner ? a.st.img_sums[img * 5 + k] : 0.0;
          if (a.weights_row)
#pragma unroll
            for (int k = 0; k < 2; ++k) a.weights_row[img * 2 + k] = inner ? a.st.img_w[img * 2 + k] : 0.0;
          if (a.tcoef_row)
#pragma unroll
            for (int k = 0; k < 2; ++k) a.tcoef_row[img * 2 + k] = inner ? a.st.img_s[img * 2 + k] : 0.f;
        }
      });
}

struct NebAtomArgs {
  NebGeom g;
  int64_t N;
  float* pos;
  float* vel;
  const float* forces;  // OPEN: the kept F_neb
  float* forces_keep;
  const uint8_t* fixed;
  const int* counts;  // the graph's counters, or NULL
  NebState st;
};

// one thread per row.  ACCEPT (after k_neb_control): keep F_neb of the evaluation, or, when it overflowed, go back to the state the
// last move saved.  MOVE: save x and v, then the update with the band's coefficients (ACCEPT: on the F_neb just made, else on `forces`).
template <bool ACCEPT, bool MOVE>
__global__ __launch_bounds__(kThreads) void k_neb_atoms(NebAtomArgs a) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.N) return;
  const uint32_t status = a.st.head[kHeadStatus], fresh = a.st.head[kHeadFresh];
  if (status) {
    if (ACCEPT && status == 1u && !fresh && a.counts && a.counts[2]) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        a.pos[r * 3 + d] = a.st.x_keep[r * 3 + d];
        a.vel[r * 3 + d] = a.st.v_keep[r * 3 + d];
      }
    }
    return;
  }
  if (fresh) return;  // (OPEN straight after a reset: there are no coefficients yet)
  float x[3], v[3], f[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) f[d] = ACCEPT ? a.st.f_neb[r * 3 + d] : a.forces[r * 3 + d];
  if (ACCEPT && a.forces_keep)
#pragma unroll
    for (int d = 0; d < 3; ++d) a.forces_keep[r * 3 + d] = f[d];
  if (MOVE) {
    const int img = (int)(r / a.g.n), atom = (int)(r - (int64_t)img * a.g.n);
    const int b = img / a.g.M, i = img - b * a.g.M;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      x[d] = a.pos[r * 3 + d];
      v[d] = a.vel[r * 3 + d];
      a.st.x_keep[r * 3 + d] = x[d];
      a.st.v_keep[r * 3 + d] = v[d];
    }
    if (i == 0 || i == a.g.M - 1 || a.st.conv[b] >= 0 || (a.fixed && a.fixed[atom])) {  // a branch: x keeps its bits
#pragma unroll
      for (int d = 0; d < 3; ++d) a.vel[r * 3 + d] = 0.f;
      return;
    }
    tn_min::atom_move(x, v, f, a.st.coef[b * 3 + 0], a.st.coef[b * 3 + 1], a.st.coef[b * 3 + 2]);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a.pos[r * 3 + d] = x[d];
      a.vel[r * 3 + d] = v[d];
    }
  }
}

__global__ void k_neb_reset(NebState st, uint64_t step0, double dt0, double alpha0, uint32_t climb) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    loop_head_reset(st.head, step0, kNebCauseWord);
    st.head[kNebClimbWord] = climb;
    st.start[0] = dt0;
    st.start[1] = alpha0;
  }
}

bool neb_shape_ok(int64_t n, int64_t M, int64_t G) {
  if (n < 0 || M < 3 || G < 1 || M > INT32_MAX / 16 || G > INT32_MAX / 16) return false;
  if (G * M > INT32_MAX / 16) return false;
  return n == 0 || G * M <= (INT32_MAX / 4) / n;
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tmdnet_neb_workspace_bytes(int64_t n_atoms_per_image, int64_t n_images, int64_t n_bands, size_t* bytes) {
  if (!bytes || !neb_shape_ok(n_atoms_per_image, n_images, n_bands)) return TMDNET_ERR_INVALID;
  *bytes = neb_bytes(n_atoms_per_image, n_images, n_bands);
  return TMDNET_OK;
}

int tmdnet_neb_reset(void* stream, void* neb_ws, uint64_t step0, double dt0, double alpha0, int32_t climb) {
  if (!neb_ws || !(dt0 > 0.0) || !(alpha0 >= 0.0) || (climb != 0 && climb != 1)) return TMDNET_ERR_INVALID;
  hipLaunchKernelGGL(k_neb_reset, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), carve_neb(neb_ws, 0, 0, 0), step0, dt0,
                     alpha0, (uint32_t)climb);
  return hipGetLastError() == hipSuccess ? TMDNET_OK : TMDNET_ERR_HIP;
}

int tmdnet_neb_advance(tmdnet_model* m, void* stream, void* graph_ws, void* neb_ws, int64_t n_atoms_per_image, int64_t n_images,
                       int64_t n_bands, int32_t phase, float* pos, float* vel, const float* forces, const float* energy,
                       const uint8_t* fixed, float* forces_keep, double dt_max, int32_t n_min, double f_inc, double f_dec, double alpha0,
                       double f_alpha, double max_step, double fmax, double spring_k, float* epot_log_row, float* fmax_log_row,
                       double* sums_log_row, float* coef_log_row, double* dt_log_row, double* alpha_log_row,
                       int64_t* converged_log_row, double* path_sums_log_row, double* weights_log_row, float* tangent_coef_log_row,
                       int32_t* climber_log_row) {
  if (!neb_ws || !pos || !vel || !forces || !neb_shape_ok(n_atoms_per_image, n_images, n_bands)) return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MIN_OPEN && phase != TMDNET_MIN_MIDDLE && phase != TMDNET_MIN_CLOSE) return TMDNET_ERR_INVALID;
  if (phase != TMDNET_MIN_OPEN && !energy) return TMDNET_ERR_INVALID;  // the tangents need the energies
  if (graph_ws && !m) return TMDNET_ERR_INVALID;
  if (!(fmax > 0.0) || !(dt_max > 0.0) || !(max_step > 0.0) || !(f_inc > 0.0) || !(f_dec > 0.0) || !(f_alpha > 0.0) || !(alpha0 >= 0.0) ||
      n_min < 0 || !(spring_k > 0.0) || !std::isfinite(spring_k))
    return TMDNET_ERR_INVALID;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  NebGeom g;
  g.n = (int)n_atoms_per_image;
  g.M = (int)n_images;
  g.G = (int)n_bands;
  g.S = mol_slices(n_atoms_per_image, 1);
  const int64_t n_img = n_images * n_bands, N = n_img * n_atoms_per_image;
  const NebState st = carve_neb(neb_ws, n_atoms_per_image, n_images, n_bands);
  const int* counts = loop_graph(m, graph_ws, N, n_img).counts;
  const dim3 block(kThreads);
  if (phase != TMDNET_MIN_OPEN) {
    const dim3 grid((unsigned)n_img, (unsigned)g.S);
    hipLaunchKernelGGL(k_neb_path, grid, block, 0, s, st, g, counts, pos, forces, fixed);
    hipLaunchKernelGGL(k_neb_project, grid, block, 0, s, st, g, counts, pos, vel, forces, energy, fixed, spring_k);
    NebCtlArgs c;
    c.g = g;
    c.p.dt_max = dt_max;
    c.p.f_inc = f_inc;
    c.p.f_dec = f_dec;
    c.p.alpha0 = alpha0;
    c.p.f_alpha = f_alpha;
    c.p.max_step = max_step;
    c.p.fmax = fmax;
    c.p.n_min = n_min;
    c.counts = counts;
    c.energy = energy;
    c.epot_row = epot_log_row;
    c.rows = {nullptr, fmax_log_row, sums_log_row, coef_log_row, dt_log_row, alpha_log_row, converged_log_row};
    c.path_row = path_sums_log_row;
    c.weights_row = weights_log_row;
    c.tcoef_row = tangent_coef_log_row;
    c.climber_row = climber_log_row;
    c.st = st;
    hipLaunchKernelGGL(k_neb_control, dim3(1), block, 0, s, c);
  }
  if (N > 0) {
    NebAtomArgs a;
    a.g = g;
    a.N = N;
    a.pos = pos;
    a.vel = vel;
    a.forces = forces;
    a.forces_keep = forces_keep;
    a.fixed = fixed;
    a.counts = counts;
    a.st = st;
    const dim3 grid((unsigned)((N + kThreads - 1) / kThreads));
    if (phase == TMDNET_MIN_OPEN)
      hipLaunchKernelGGL((k_neb_atoms<false, true>), grid, block, 0, s, a);
    else if (phase == TMDNET_MIN_MIDDLE)
      hipLaunchKernelGGL((k_neb_atoms<true, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((k_neb_atoms<true, false>), grid, block, 0, s, a);
  }
  return loop_launch_result(m, "tmdnet_neb_advance");
}

int tmdnet_neb_status(void* stream, void* neb_ws, uint64_t host[3]) {
  if (!neb_ws || !host) return TMDNET_ERR_INVALID;
  return loop_read_status(stream, carve_neb(neb_ws, 0, 0, 0).head, kNebHeadWords, kNebCauseWord, host, 3);
}

}  // extern "C"
