// LDS-staged message sweeps with 16 bytes per lane (reference tensornet.py:757-806 and its adjoint), gfx950.
//
//     acc[i, c, f] = sum_{e in row(i)} w[pair(e), type(c), f] * src[col(e), c, f]
//
// Same tiling as tn_message_tile.hip - a block owns 64 consecutive rows x 32 channels and stages the rows of its
// column window [<= 64][9][32] (72 KB) in LDS once - but a different thread layout.  There a half-wave owned a row
// with one channel per lane: every edge cost a wave 3 dword loads, 9 ds_read_b32 and 9 v_fma for 2 rows x 32 channels, and
// the sweep was bound by instruction issue (4 cycles per wave64 VALU / LDS instruction), not by HBM or LDS bandwidth
// (profiles/r02_notes.md: 113 us of the 200 us remained with the weight loads removed, against 29 us of LDS time).
// Here EIGHT lanes own a row and each lane carries FOUR channels: an edge costs a wave 3 global_load_dwordx4,
// 9 ds_read_b128 and 18 v_pk_fma_f32 for 8 rows x 32 channels - a quarter of the instructions per channel - and all 64
// rows of the tile advance together (8 waves), so the two reads of a pair's weights (by its row i and by its row j) fall
// within the few microseconds a tile takes instead of being spread over a long block lifetime.
//
// The tile's slice of the adjacency (col / epair of rows r0 .. r1, contiguous) sits in LDS next to the window: the (column,
// pair id) record of a trip is an LDS broadcast read, fetched one step ahead; weights are loaded two edges ahead.  The rows of
// a tile are balanced: the k-th longest row hands the tail of its list to the group of the k-th shortest (see "Balanced
// walk" below).  Deterministic, no atomics; the summation order of a long row differs from the other sweeps' by that
// one split.  A tile whose column window is wider than 64 rows (large systems in cell order, ragged molecules straddling
// the tile) gathers its sources from global memory instead of LDS, one whose slice exceeds 4096 entries walks it from global
// memory with the 8 lanes of a row fetching 8 records at a time; both choices are block-uniform.
//
// In-kernel timestamps (round 4, C2: 1024 blocks in 4 rounds): window + slice staging 5.7 us, edge loop 20.9 us (27.9 before
// the slice was staged and the rows balanced), epilogue 2.1 us per block; with the weight loads removed the loop still took
// 13 us, with the window reads removed as well the same - the loop moves ~590 KB of weight pieces per block, 7.2 TB/s over all
// CUs while it runs, the rate tools/microbench/gather_bw.hip measures for random 128-byte pieces.
//
// Three kernels share this layout: the forward sweep k_message_rows8 (message + group product + normalisation -> Mi, Ch), the
// reverse sweep k_message_adjoint_rows8 and the reverse sweep with the group-product adjoint in its prologue,
// k_message_adjoint_rows8_fold.  The tile prologue, the balanced walk and the nine-component accumulation are written once, as
// force-inlined helpers in front of the kernels; the two reverse kernels are one body (adjoint_tile_body) behind two prologues.
// (A reverse mode of this layout existed in round 2 and again, with the symmetric walk order, in round 4: 216 VGPRs, one block
// per CU, 325 us against 283 for the row kernel k_message_adjoint_gd; removed, profiles/r04_notes.md, profiles/r04_experiments/.)
#include <cstdlib>

#include "tn_common.h"
#include "tn_kernels.h"

namespace tn {

constexpr int MP_TA = 64;        // rows per tile
constexpr int MP_FC = 32;  // channels per block
constexpr int MP_W = 64;   // source-window capacity (rows staged in LDS)
constexpr int MP_E = 4096;  // adjacency entries of a tile kept in LDS (32 KB)
constexpr int MP_U = 2;    // edges whose weights are loaded ahead of their use
constexpr int MP_WAVES = 8;  // waves of a reverse sweep's block
constexpr int MP_SLOT_PAIRS = MP_TA * (MP_TA - 1) / 2;  // pairs of a closed tile: 2016
constexpr int MP_SLOTS = 2 * MP_SLOT_PAIRS;             // their slots (pair, direction) of one channel chunk, kept in LDS (16 KB)

typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
template <int VW> struct VecOf;
template <> struct VecOf<4> { typedef f4v T; };
template <> struct VecOf<2> { typedef f2v T; };

__device__ __forceinline__ f4v ldg4(const float* p) { return *reinterpret_cast<const f4v*>(p); }

// A pointer into LDS carries its address space in its type.  The helpers below see the kernels' __shared__ arrays as pointers;
// as plain pointers an "LDS or global memory" choice of theirs compiles to ONE flat load from a selected address (seen: 18
// flat_load_dwordx4 in the reverse sweep's edge loop), typed it stays a ds_read and a global_load.
#define TN_LDS __attribute__((address_space(3)))
template <typename T>
__device__ __forceinline__ TN_LDS T* lds_ptr(T* p) { return (TN_LDS T*)p; }
template <typename vf>
__device__ __forceinline__ vf ldv_of(const float* p) { return *reinterpret_cast<const vf*>(p); }
template <typename vf>
__device__ __forceinline__ vf ldv_of(const TN_LDS float* p) { return *reinterpret_cast<const TN_LDS vf*>(p); }

// Order in which a row walks its (ascending) neighbour list.  Both rows of a pair read the pair's weight row; in list order
// the two reads are up to a tile lifetime apart and the second one misses the 4 MB L2 two times out of three (PMC: 1.30x the
// algorithmic bytes).  Walking in the order of the symmetric key (i + j) mod 64 - a ROTATION of the ascending list: start at the
// first neighbour j >= J, J = -i (mod 64), wrap at the end - puts the pair (i, j) at about the same trip of both rows, so the
// second read finds the line in L2.  Any rotation is a valid order; molecules wider than 64 atoms only lose the symmetry.
// The start is the position of the smallest key in the row; the LPR lanes of a row look at every LPR-th entry (independent
// loads, one round trip for rows of up to 8 LPR entries) and combine with a min over the group.  Group-uniform result.
template <int LPR>
__device__ __forceinline__ int row_rotation(const Graph& g, int i, int e0, int len, int ql) {
  unsigned best = 0xffffffffu;  // (key << 16) | position
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int pos = ql + m * LPR;
    if (pos < len) best = min(best, ((unsigned)((i + g.col[e0 + pos]) & 63) << 16) | (unsigned)pos);
  }
  for (int pos = ql + 8 * LPR; pos < len; pos += LPR)
    best = min(best, ((unsigned)((i + g.col[e0 + pos]) & 63) << 16) | (unsigned)pos);
#pragma unroll
  for (int off = 1; off < LPR; off <<= 1) best = min(best, (unsigned)__shfl_xor((int)best, off, 64));
  return len > 0 ? (int)(best & 0xffffu) : 0;
}
__device__ __forceinline__ int walk_edge(int e0, int len, int rot, int t) {  // edge of trip t (clamped to the last trip)
  int pos = rot + min(t, len - 1);
  if (pos >= len) pos -= len;
  return e0 + max(pos, 0);
}

// ================================================================================================ the tile, shared by the sweeps
// Every helper below is force-inlined into a kernel that owns the LDS arrays (the layout per kernel is the kernel's); acc, s9 and
// y travel as references to arrays of nine and are indexed with unrolled constants only, so they stay in registers.
struct TileLds {
  TN_LDS float* win;                     // source window [MP_W][9][32]
  TN_LDS float* help;                    // helper partial sums of the long rows [MP_TA / 2][9][32]
  TN_LDS int *col, *pair;                // the tile's slice of col / epair [MP_E]
  TN_LDS int *rp, *len, *rank, *byrank;  // row table [MP_TA]: start within the slice, length, rank by length, row of a rank
  // reverse sweeps only (see "Slots of a tile" below)
  TN_LDS int* prange;                    // per wave of the block: smallest / largest pair id and count of the slice's non-self entries [3][MP_WAVES]
  TN_LDS float* slot;                    // the tile's slots [MP_SLOTS]
};
struct Tile {
  TileLds lds;
  const int *gcol, *gpair;  // the graph's col / epair
  int chunk, c0;            // channel chunk of the block and its first channel
  int r0, r1;               // rows of the tile
  int eT0, nE;              // its slice of the adjacency: first entry, entries
};
__device__ __forceinline__ Tile tile_of_block(const Graph& g, int N, int nchunks, const TileLds& lds) {
  Tile T;
  T.lds = lds;
  T.gcol = g.col;
  T.gpair = g.epair;
  const int b = xcd_chunk(blockIdx.x, gridDim.x);
  const int tile = b / nchunks;
  T.chunk = b - tile * nchunks;
  T.c0 = T.chunk * MP_FC;
  T.r0 = tile * MP_TA;
  T.r1 = min(N, T.r0 + MP_TA);
  T.eT0 = g.rowptr[T.r0];
  T.nE = g.rowptr[T.r1] - T.eT0;
  return T;
}

// ---- the tile's slice of the adjacency -> LDS.  Timestamps inside the kernel (round 4) showed the edge loop at 0.35 us per
// trip with the weight loads AND the window reads removed: it waited for the (column, pair id) records, a dependent global
// load in front of every eight trips' weight loads.  Rows r0 .. r1 are one contiguous range of col / epair (~1500 entries
// for 64-atom molecules); it is requested together with the row table (and, with WINDOW, the column bounds of the thread's row:
// rows are sorted ascending, first / last entry) and read from LDS afterwards.  in_lds: the slice fits (block-uniform).
//
// Slots of a tile.  The engine numbers the pairs of rows r0 .. r1 of a closed tile contiguously, and both directions of each lie
// in the tile: it owns the slots [2 pmin, 2 pmax + 2) of its channel chunk and nothing else touches them.  While the slice is on
// its way every wave reduces the smallest and largest pair id and the count of the non-self entries (pair id != self_pair =
// counts[0]) it staged; the barrier that publishes the slice publishes them (slot_range reads them).  A slice left in global
// memory counts nothing.
template <int THREADS, bool WINDOW>
__device__ __forceinline__ void stage_slice(const Graph& g, const Tile& T, bool in_lds, int tid, int& lo, int& hi, int self_pair) {
  static_assert(THREADS == 64 * MP_WAVES, "one entry of prange per wave");
  int cbuf[MP_E / THREADS], pbuf[MP_E / THREADS];
  if (in_lds) {
#pragma unroll
    for (int k = 0; k < MP_E / THREADS; ++k) {
      const int idx = tid + k * THREADS;
      if (idx < T.nE) {
        cbuf[k] = g.col[T.eT0 + idx];
        pbuf[k] = g.epair[T.eT0 + idx];
      }
    }
  }
  if (tid < MP_TA) {
    const int rr = min(T.r0 + tid, T.r1);
    const int a0 = g.rowptr[rr], a1 = g.rowptr[min(rr + 1, T.r1)];
    T.lds.rp[tid] = a0 - T.eT0;
    T.lds.len[tid] = a1 - a0;
    if (WINDOW && a1 > a0) {
      lo = g.col[a0];
      hi = g.col[a1 - 1];
    }
  }
  int pmin = 0x7fffffff, pmax = -1, pcnt = 0;
  if (in_lds) {
#pragma unroll
    for (int k = 0; k < MP_E / THREADS; ++k) {
      const int idx = tid + k * THREADS;
      if (idx < T.nE) {
        T.lds.col[idx] = cbuf[k];
        T.lds.pair[idx] = pbuf[k];
        if (pbuf[k] != self_pair) {
          pmin = min(pmin, pbuf[k]);
          pmax = max(pmax, pbuf[k]);
          ++pcnt;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    pmin = min(pmin, __shfl_xor(pmin, off, 64));
    pmax = max(pmax, __shfl_xor(pmax, off, 64));
    pcnt += __shfl_xor(pcnt, off, 64);
  }
  if ((tid & 63) == 0) {
    T.lds.prange[tid >> 6] = pmin;
    T.lds.prange[MP_WAVES + (tid >> 6)] = pmax;
    T.lds.prange[2 * MP_WAVES + (tid >> 6)] = pcnt;
  }
}

// The tile's slot range from what stage_slice left (after the barrier behind it; block-uniform): the first pair id and the
// number of slots when the tile takes its slots through LDS, 0 slots when it stores them directly.  Through LDS when the pair
// ids of the slice's non-self entries span at most MP_SLOT_PAIRS ids and there are exactly two entries per id of the span: an
// entry is one (pair, direction) and no two entries are the same one, so every slot of the span is then written exactly once by
// this tile and nothing uninitialised leaves LDS.
__device__ __forceinline__ int slot_range(const TileLds& s, int& pmin) {
  int lo = s.prange[0], hi = s.prange[MP_WAVES], cnt = s.prange[2 * MP_WAVES];
#pragma unroll
  for (int k = 1; k < MP_WAVES; ++k) {
    lo = min(lo, s.prange[k]);
    hi = max(hi, s.prange[MP_WAVES + k]);
    cnt += s.prange[2 * MP_WAVES + k];
  }
  pmin = lo;
  const int span = hi - lo + 1;
  return (cnt > 0 && span <= MP_SLOT_PAIRS && cnt == 2 * span) ? 2 * span : 0;
}

// column window of the tile: min / max of the rows' bounds over the block (one barrier; it also publishes slice and row table)
template <int THREADS>
__device__ __forceinline__ void window_bounds(int& lo, int& hi, TN_LDS int* s_lo, TN_LDS int* s_hi, int tid) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    lo = min(lo, __shfl_xor(lo, off, 64));
    hi = max(hi, __shfl_xor(hi, off, 64));
  }
  if ((tid & 63) == 0) {
    s_lo[tid >> 6] = lo;
    s_hi[tid >> 6] = hi;
  }
  __syncthreads();
  lo = s_lo[0];
  hi = s_hi[0];
#pragma unroll
  for (int k = 1; k < THREADS / 64; ++k) {
    lo = min(lo, s_lo[k]);
    hi = max(hi, s_hi[k]);
  }
}

// rank of every row by length (0 = longest; ties by row), one wave; placed where a kernel has loads in flight
__device__ __forceinline__ void rank_rows(const TN_LDS int* s_len, TN_LDS int* s_rank, TN_LDS int* s_byrank, int tid) {
  if (tid < MP_TA) {
    const int mylen = s_len[tid];
    int rank = 0;
    for (int r = 0; r < MP_TA; ++r) {
      const int l = s_len[r];
      rank += (l > mylen || (l == mylen && r < tid)) ? 1 : 0;
    }
    s_rank[tid] = rank;
    s_byrank[rank] = tid;
  }
}

// rows lo .. lo + wn - 1 of src -> LDS window as [row][9][FC]: 8 lanes x 16 B cover 32 channels of one (row, component).
// All of a thread's pieces are requested before the first one is stored: as a plain loop (trip count unknown to the
// compiler) this was nine dependent load -> store round trips, 9 of the 44 us a block lives.  The rows are ranked while the
// window is on its way.  wn = 0: nothing staged (rank only).  Ends with the barrier that publishes window and ranks.
template <int THREADS, int FC>
__device__ __forceinline__ void stage_window(const float* __restrict__ src, int F, const Tile& T, int lo, int wn, int tid) {
  constexpr int PIECES = FC / 4, NIT = (MP_W * 9 * PIECES + THREADS - 1) / THREADS;
  const int pieces = wn * 9 * PIECES, F9 = 9 * F;
  f4v tmp[NIT];
#pragma unroll
  for (int k = 0; k < NIT; ++k) {
    const int idx = tid + k * THREADS;
    if (idx < pieces) {
      const int rc = idx / PIECES, f4 = (idx % PIECES) << 2;
      const int row = rc / 9, c = rc - row * 9;
      tmp[k] = ldg4(src + (int64_t)(lo + row) * F9 + c * F + T.c0 + f4);
    }
  }
  rank_rows(T.lds.len, T.lds.rank, T.lds.byrank, tid);
#pragma unroll
  for (int k = 0; k < NIT; ++k) {
    const int idx = tid + k * THREADS;
    if (idx < pieces) {
      const int rc = idx / PIECES, f4 = (idx % PIECES) << 2;
      *reinterpret_cast<TN_LDS f4v*>(&T.lds.win[rc * FC + f4]) = tmp[k];
    }
  }
  __syncthreads();
}

// ---- Balanced walk.  The 8 rows of a wave advance together and the block lives as long as its longest row: 45 trips at
// C2 against a mean row length of 24.  The k-th longest row hands the last h = (len_long - len_short) / 2 entries of its
// list to the group of the k-th shortest row, which sums them FIRST (segment A), parks that partial sum in LDS and then walks
// its own row (segment B, the head of the row when this row is a long one); the long row's group adds the parked sum to its
// own in the epilogue.  Fixed order, one writer per slot: deterministic (the order differs from the one-lane-per-channel
// sweeps' by that one split).
struct TileWalk {
  int baseA, lenA, rowA;  // segment A: first entry within the slice, entries, the row they belong to
  int baseB, lenB;        // segment B
  int slotA;              // where segment A's sum is parked
  int help_slot;          // >= 0: this row is a long row, the partial sum of its last entries is parked there
  int rotA, rotB;         // rotation of each segment (see row_rotation)
  int ntrip, nmax;        // trips of this row; of the longest row of the wave (past its end a row adds zeros)
};
// where the (column, pair id) records are read from
enum SliceSrc {
  SLICE_LDS,            // forward sweep, on its LDS branch
  SLICE_LDS_OR_GLOBAL,  // reverse sweep: a slice that did not fit is read from global memory
  SLICE_LDS_GUARDED,    // folded reverse sweep: LDS, and a tile without entries reads none
};

template <SliceSrc SRC, int LPR>
__device__ __forceinline__ TileWalk walk_of_row(const Tile& T, bool in_lds, bool balance, int rl, int ql, int rowA0) {
  const TileLds& s = T.lds;
  const int rank = s.rank[rl], partner = s.byrank[MP_TA - 1 - rank];
  const int mylen = s.len[rl], plen = s.len[partner];
  TileWalk k;
  k.baseA = 0, k.lenA = 0, k.rowA = rowA0, k.baseB = s.rp[rl], k.lenB = mylen, k.slotA = 0, k.help_slot = -1;
  if (balance) {
    if (rank < MP_TA / 2) {
      const int h = ((mylen - plen) / 2) & ~(MP_U - 1);
      k.lenB = mylen - h;
      if (h > 0) k.help_slot = rank;
    } else {
      const int h = ((plen - mylen) / 2) & ~(MP_U - 1);
      k.lenA = h;
      k.baseA = s.rp[partner] + plen - h;
      k.rowA = T.r0 + partner;
      k.slotA = MP_TA - 1 - rank;
    }
  }
  // rotation of a segment (see row_rotation): position of its smallest key (row + column) mod 64
  auto seg_rot = [&](int base, int len, int row) __attribute__((always_inline)) {
    unsigned best = 0xffffffffu;
    if (SRC != SLICE_LDS_OR_GLOBAL || in_lds)
      for (int pos = ql; pos < len; pos += LPR) best = min(best, ((unsigned)((row + s.col[base + pos]) & 63) << 16) | (unsigned)pos);
    else
      for (int pos = ql; pos < len; pos += LPR) best = min(best, ((unsigned)((row + T.gcol[T.eT0 + base + pos]) & 63) << 16) | (unsigned)pos);
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) best = min(best, (unsigned)__shfl_xor((int)best, off, 64));
    return len > 0 ? (int)(best & 0xffffu) : 0;
  };
  k.rotA = seg_rot(k.baseA, k.lenA, k.rowA);
  k.rotB = seg_rot(k.baseB, k.lenB, T.r0 + rl);
  k.ntrip = k.lenA + k.lenB;
  k.nmax = k.ntrip;  // the 8 rows of a wave advance together: trip count = the longest of them
#pragma unroll
  for (int off = LPR; off <= 32; off <<= 1) k.nmax = max(k.nmax, __shfl_xor(k.nmax, off, 64));
  return k;
}

// (column, pair id) of trip t (clamped past the end): every lane of a row reads one address, an LDS broadcast
template <SliceSrc SRC>
__device__ __forceinline__ void walk_record(const TileWalk& k, const Tile& T, bool in_lds, int t, int& j, int& p) {
  const bool inA = t < k.lenA;
  const int tt = inA ? t : t - k.lenA, L = inA ? k.lenA : k.lenB;
  int pos = (inA ? k.rotA : k.rotB) + min(tt, L - 1);
  if (pos >= L) pos -= L;
  const int entry = L > 0 ? (inA ? k.baseA : k.baseB) + pos : 0;  // a row without entries: entry 0 of the slice, masked
  if (SRC == SLICE_LDS_GUARDED) {
    j = T.nE > 0 ? T.lds.col[entry] : T.r0;  // a tile without entries (never with self edges): its own first row, masked
    p = T.nE > 0 ? T.lds.pair[entry] : 0;
  } else if (SRC == SLICE_LDS || in_lds) {
    j = T.lds.col[entry];
    p = T.lds.pair[entry];
  } else {
    j = T.nE > 0 ? T.gcol[T.eT0 + entry] : 0;
    p = T.nE > 0 ? T.gpair[T.eT0 + entry] : 0;
  }
}

// segment A is done: its sum goes to LDS, the own row starts from zero
template <typename vf>
__device__ __forceinline__ void walk_park(vf (&acc)[9], const TileWalk& k, const TileLds& s, int vq) {
  TN_LDS float* hp = s.help + k.slotA * (9 * MP_FC) + vq;
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    *reinterpret_cast<TN_LDS vf*>(hp + c * MP_FC) = acc[c];
    acc[c] = (vf)(0.f);
  }
}
// a long row adds what its helper parked (after the barrier that follows the walk)
template <typename vf>
__device__ __forceinline__ void walk_add_parked(vf (&acc)[9], const TileWalk& k, const TileLds& s, int vq) {
  if (k.help_slot >= 0) {
    const TN_LDS float* hp = s.help + k.help_slot * (9 * MP_FC) + vq;
#pragma unroll
    for (int c = 0; c < 9; ++c) acc[c] += ldv_of<vf>(hp + c * MP_FC);
  }
}

// nine pieces, a stride apart, from LDS or from global memory
template <typename vf, typename P>
__device__ __forceinline__ void load9(vf (&v)[9], P p, int stride) {
#pragma unroll
  for (int c = 0; c < 9; ++c) v[c] = ldv_of<vf>(p + c * stride);
}
// the nine pieces of source row j: from window row wrow when the window is staged, else from global memory
template <typename vf>
__device__ __forceinline__ void load9_window_or_global(vf (&v)[9], bool staged, const TN_LDS float* win, int wrow, int vq,
                                                       const float* __restrict__ src, int j, int F, int f) {
  if (__builtin_expect(staged, true))  // the LDS reads are the fall-through of the edge loops
    load9(v, win + wrow * (9 * MP_FC) + vq, MP_FC);
  else
    load9(v, src + (int64_t)j * (9 * F) + f, F);
}
// acc += w (x) s9 with the weight of each component's irreducible part (1 + 3 + 5), masked past the row's end
template <typename vf>
__device__ __forceinline__ void message_fma9(vf (&acc)[9], const vf (&wv)[3], float msk, const vf (&s9)[9]) {
  const vf w0 = wv[0] * msk, w1 = wv[1] * msk, w2 = wv[2] * msk;
  acc[0] += w0 * s9[0];
  acc[1] += w1 * s9[1];
  acc[2] += w1 * s9[2];
  acc[3] += w1 * s9[3];
  acc[4] += w2 * s9[4];
  acc[5] += w2 * s9[5];
  acc[6] += w2 * s9[6];
  acc[7] += w2 * s9[7];
  acc[8] += w2 * s9[8];
}

// The distance-gradient half of one edge (adjoint_tile_body):
//     dv0 * (s0 y0) + dv1 * (s1 y1 + s2 y2 + s3 y3) + dv2 * (s4 y4 + s5 y5 + s6 y6 + s7 y7 + s8 y8)
// Of a sum of two products a b + c d one is rounded and the other fused into the add, and WHICH was the compiler's choice: it
// depended on the code around the expression.  The two reverse kernels happened to agree while they were two copies and stopped
// agreeing in the last bits of the slots when they became one body - and the engine switches between them per batch.  The product
// that has always been the rounded one is computed with contraction off, which leaves one way to fuse the sum; the rest stays
// with the compiler.  The expression itself stands in the edge loop: as a helper that takes dv, s9 and y it cost four registers.
__device__ __forceinline__ f4v mul_rounded(f4v a, f4v b) {
#pragma clang fp contract(off)
  return a * b;
}

// ================================================================================================ forward sweep
// LPR lanes own a row, VW channels per lane (LPR * VW = 32 channels per block).  8 x 4: 512 threads, 16-byte accesses, the
// fewest instructions per channel - but the reverse sweep's per-lane state (two 9-vectors, weights and their derivatives
// two edges ahead) is then 216 VGPRs = two waves per SIMD, too few to cover the loads.  16 x 2: 1024 threads, 8-byte
// accesses, half the state per lane (four waves per SIMD in one block per CU).
template <int LPR, int VW>
__global__ __launch_bounds__(64 * LPR) void k_message_rows8(Graph g, int N, int F, const float* __restrict__ w,
                                                                const float* __restrict__ src, const float* __restrict__ q,
                                                                const int64_t* __restrict__ batch, int o3,
                                                                float* __restrict__ Mi, float* __restrict__ out, int nchunks,
                                                                int balance) {
  constexpr int MP_THREADS = 64 * LPR, U = MP_U;
  static_assert(VW * LPR == MP_FC && MP_TA == 64 && MP_E % MP_THREADS == 0, "32 channels per block; one wave ranks the tile's rows");
  typedef typename VecOf<VW>::T vf;
  __shared__ __attribute__((aligned(16))) float win[MP_W * 9 * MP_FC];
  __shared__ __attribute__((aligned(16))) float s_help[(MP_TA / 2) * 9 * MP_FC];  // helper partial sums of the long rows
  __shared__ int s_col[MP_E], s_pair[MP_E];                                          // the tile's slice of col / epair
  __shared__ int s_lo[MP_THREADS / 64], s_hi[MP_THREADS / 64], s_rp[MP_TA], s_len[MP_TA], s_rank[MP_TA], s_byrank[MP_TA];
  if (g.counts[2]) return;  // pair overflow: the adjacency was not filled (the host reports the error)
  const Tile T = tile_of_block(g, N, nchunks, {lds_ptr(win), lds_ptr(s_help), lds_ptr(s_col), lds_ptr(s_pair), lds_ptr(s_rp),
                                               lds_ptr(s_len), lds_ptr(s_rank), lds_ptr(s_byrank)});
  const int r0 = T.r0, r1 = T.r1, c0 = T.c0;
  const int tid = threadIdx.x, lane = tid & 63;
  const int F9 = 9 * F, F3 = 3 * F;

  // The slice staging (stage_slice) stays written out here: through the helper the compiler schedules the staging differently (the
  // LDS stores of a record wait for both of its loads) and this kernel - the shortest of the three - was 1 % slower per launch,
  // 158.1 against 156.8 us at C2, with every other helper in place (profiles/message_tile_walk.json).
  const int eT0 = T.eT0, nE = T.nE;
  const bool csr_lds = nE <= MP_E;  // block-uniform
  int lo = 0x7fffffff, hi = -1;
  {
    int cbuf[MP_E / MP_THREADS], pbuf[MP_E / MP_THREADS];
    if (csr_lds) {
#pragma unroll
      for (int k = 0; k < MP_E / MP_THREADS; ++k) {
        const int idx = tid + k * MP_THREADS;
        if (idx < nE) {
          cbuf[k] = g.col[eT0 + idx];
          pbuf[k] = g.epair[eT0 + idx];
        }
      }
    }
    // column window of the tile (rows are sorted ascending: first / last entry of each row)
    if (tid < MP_TA) {
      const int rr = min(r0 + tid, r1);
      const int a0 = g.rowptr[rr], a1 = g.rowptr[min(rr + 1, r1)];
      s_rp[tid] = a0 - eT0;
      s_len[tid] = a1 - a0;
      if (a1 > a0) {
        lo = g.col[a0];
        hi = g.col[a1 - 1];
      }
    }
    if (csr_lds) {
#pragma unroll
      for (int k = 0; k < MP_E / MP_THREADS; ++k) {
        const int idx = tid + k * MP_THREADS;
        if (idx < nE) {
          s_col[idx] = cbuf[k];
          s_pair[idx] = pbuf[k];
        }
      }
    }
  }
  window_bounds<MP_THREADS>(lo, hi, lds_ptr(s_lo), lds_ptr(s_hi), tid);
  const int wn = hi - lo + 1;
  const bool staged = hi >= lo && wn <= MP_W;  // block-uniform
  stage_window<MP_THREADS, MP_FC>(src, F, T, lo, staged ? wn : 0, tid);

  const int rl = tid / LPR, i = r0 + rl, ql = tid & (LPR - 1), f = c0 + VW * ql;  // row, lane within the row's group, first channel
  const bool live = i < r1;
  vf acc[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) acc[c] = (vf)(0.f);
  TileWalk wk;
  wk.help_slot = -1;

  if (csr_lds) {
    wk = walk_of_row<SLICE_LDS, LPR>(T, true, balance, rl, ql, 0);
    bool parked = wk.lenA == 0;
    int jn[U], pn[U];
#pragma unroll
    for (int u = 0; u < U; ++u) walk_record<SLICE_LDS>(wk, T, true, u, jn[u], pn[u]);
    for (int t = 0; t < wk.nmax; t += U) {
      if (!parked && t == wk.lenA) {  // lenA is a multiple of U
        walk_park(acc, wk, T.lds, VW * ql);
        parked = true;
      }
      int jj[U];
      vf wv[U][3];
      float msk[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        jj[u] = jn[u];
        msk[u] = (t + u < wk.ntrip) ? 1.0f : 0.0f;
        const float* wp = w + (int64_t)pn[u] * F3 + f;
        wv[u][0] = ldv_of<vf>(wp);
        wv[u][1] = ldv_of<vf>(wp + F);
        wv[u][2] = ldv_of<vf>(wp + 2 * F);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) walk_record<SLICE_LDS>(wk, T, true, t + U + u, jn[u], pn[u]);  // the next step's records
#pragma unroll
      for (int u = 0; u < U; ++u) {
        vf s9[9];
        load9_window_or_global(s9, staged, T.lds.win, jj[u] - lo, VW * ql, src, jj[u], F, f);
        message_fma9(acc, wv[u], msk[u], s9);
      }
    }
    if (!parked) walk_park(acc, wk, T.lds, VW * ql);  // a helper whose own row is empty
  } else {
    // the slice did not fit: every row is walked by its own group, which fetches LPR records at a time and hands them round
    const int e0 = live ? g.rowptr[i] : 0, e1 = live ? g.rowptr[i + 1] : 0;
    const int grp = lane & ~(LPR - 1);  // first lane of this row's group within the wave
    const int len = e1 - e0, rot = row_rotation<LPR>(g, i, e0, len, ql);
    int nmax = e1 - e0;
#pragma unroll
    for (int off = LPR; off <= 32; off <<= 1) nmax = max(nmax, __shfl_xor(nmax, off, 64));
    for (int eb = 0; eb < nmax; eb += LPR) {
      const int me = walk_edge(e0, len, rot, eb + ql);  // clamped: lanes past the row's end repeat its last edge with zero weights
      const int myc = (e1 > e0) ? g.col[me] : 0, myp = (e1 > e0) ? g.epair[me] : 0;
      const int n = min(LPR, nmax - eb);
      for (int k = 0; k < n; k += MP_U) {
        int jj[MP_U], pp[MP_U];
        vf wv[MP_U][3];
        float msk[MP_U];
#pragma unroll
        for (int u = 0; u < MP_U; ++u) {
          const bool valid = e0 + eb + k + u < e1;
          const int srcl = grp + min(k + u, LPR - 1);
          jj[u] = __shfl(myc, srcl, 64);
          pp[u] = __shfl(myp, srcl, 64);
          msk[u] = valid ? 1.0f : 0.0f;
          const float* wp = w + (int64_t)pp[u] * F3 + f;
          wv[u][0] = ldv_of<vf>(wp);
          wv[u][1] = ldv_of<vf>(wp + F);
          wv[u][2] = ldv_of<vf>(wp + 2 * F);
        }
#pragma unroll
        for (int u = 0; u < MP_U; ++u) {
          vf s9[9];
          load9_window_or_global(s9, staged, T.lds.win, jj[u] - lo, VW * ql, src, jj[u], F, f);
          message_fma9(acc, wv[u], msk[u], s9);
        }
      }
    }
  }
  __syncthreads();  // the parked sums are complete
  if (!live) return;
  walk_add_parked(acc, wk, T.lds, VW * ql);

  float* o = out + (int64_t)i * F9 + f;
  vf yy[9];  // the row's own source row; overwritten component by component with the result
  // the row's own source row is in its window whenever it has a self edge
  load9_window_or_global(yy, staged && i >= lo && i <= hi, T.lds.win, i - lo, VW * ql, src, i, F, f);
  float* mo = Mi + (int64_t)i * F9 + f;
#pragma unroll
  for (int c = 0; c < 9; ++c) *reinterpret_cast<vf*>(mo + c * F) = acc[c];
  const float kap = q ? (batch ? 1.0f + 0.1f * q[batch[i]] : q[i]) : 1.0f;
#pragma unroll
  for (int t = 0; t < VW; ++t) {
    float m9[9], y9[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      m9[c] = acc[c][t];
      y9[c] = yy[c][t];
    }
    const M3 Y = compose(y9), M = compose(m9);
    M3 Cm = o3 ? scale(add(matmul(Y, M), matmul(M, Y)), kap) : scale(matmul(Y, M), 2.0f);
    float uc[9];
    decompose(Cm, uc);
    const float inv = 1.0f / (frob2(Cm) + 1.0f);
#pragma unroll
    for (int c = 0; c < 9; ++c) yy[c][t] = uc[c] * inv;
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) *reinterpret_cast<vf*>(o + c * F) = yy[c];
}

// ================================================================================================ reverse sweeps
// Reverse sweep in the same tile layout with the same two devices (adjacency slice in LDS, balanced rows): the adjoint of the
// message sum,  gPn[i] += sum_e w[p] * gMi[col(e)],  and the layer's distance-gradient halves
// h(i <- j) = sum_{k,f} dw[p,k,f] * sum_{c in k} gMi[j,c,f] * Pn[i,c,f]  (k_message_adjoint_gd, tn_kernels.hip).  The gMi rows of
// the tile's column window sit in LDS, the Pn row of the row being walked in registers (a helper group holds the LONG row's Pn
// while it walks that row's tail, then its own); per edge a lane loads six 16-byte pieces (w, dw) and reads nine from LDS; the 8
// lanes of a row reduce their channel products and lane 0 writes the slot (channel chunk, pair, direction): one writer per slot,
// summed in fixed order by the embedding's pair kernel.
//
// The body of both reverse kernels, entered with the window (gMi rows, or gM of the tile's own rows), the slice, the row table and
// the ranks in LDS.  FOLD: the tile is closed - the window is the tile's own aligned 64 rows and always staged, the slice always in
// LDS, and gPn already holds gY, which the epilogue's read-modify-write adds to (summation order gY + acc).  Otherwise csr_lds /
// staged are the block-uniform choices of the prologue, lo the window's first row and gMi the source of an unstaged window.
// nslot / slot_p0: the tile's slot range (slot_range), read by the kernel where no store is in flight.
// 252 (FOLD) and 248 VGPRs: nothing may be added to the edge loop.
template <bool FOLD>
__device__ __forceinline__ void adjoint_tile_body(const Tile& T, int N, int F, const float* __restrict__ w,
                                                  const float* __restrict__ dw, const float* __restrict__ gMi,
                                                  const float* __restrict__ Pn, float* __restrict__ gPn, float* __restrict__ slots,
                                                  int64_t slot_stride, bool csr_lds_of_tile, bool staged_of_tile, int lo, int nslot,
                                                  int slot_p0) {
  constexpr int LPR = 8, VW = 4, U = MP_U;
  constexpr SliceSrc SRC = FOLD ? SLICE_LDS_GUARDED : SLICE_LDS_OR_GLOBAL;
  typedef f4v vf;
  const bool csr_lds = FOLD ? true : csr_lds_of_tile, staged = FOLD ? true : staged_of_tile;
  const int tid = threadIdx.x, F9 = 9 * F, F3 = 3 * F;
  const int rl = tid / LPR, i = T.r0 + rl, ql = tid & (LPR - 1), f = T.c0 + VW * ql;
  const bool live = i < T.r1;
  vf acc[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) acc[c] = (vf)(0.f);
  float* const slot_base = slots + (int64_t)T.chunk * slot_stride;
  // A store of the edge loop shares its counter with the loads: the wait for the next weights also waited for the slot store in
  // front of them to be acknowledged.  A tile that owns a contiguous slot range (slot_range) keeps its slots in LDS instead and
  // writes the range out once, coalesced, behind the walk.
  // (nslot, slot_p0: slot_range of the tile; nslot = 0: direct stores)

  // a slice read from global memory is walked by every row's own group only (no helpers)
  const TileWalk wk = walk_of_row<SRC, LPR>(T, csr_lds, csr_lds, rl, ql, T.r0);
  vf y[9];  // Pn row of the row being walked
  auto load_y = [&](int row) __attribute__((always_inline)) { load9(y, Pn + (int64_t)min(row, N - 1) * F9 + f, F); };
  bool parked = wk.lenA == 0;
  load_y(parked ? i : wk.rowA);
  int jn[U], pn[U];
#pragma unroll
  for (int u = 0; u < U; ++u) walk_record<SRC>(wk, T, csr_lds, u, jn[u], pn[u]);
  for (int t = 0; t < wk.nmax; t += U) {
    if (!parked && t == wk.lenA) {  // lenA is a multiple of U
      walk_park(acc, wk, T.lds, VW * ql);
      load_y(i);
      parked = true;
    }
    const int row_now = t < wk.lenA ? wk.rowA : i;
    int jj[U], pp[U];
    vf wv[U][3], dv[U][3];
    float msk[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      jj[u] = jn[u];
      pp[u] = pn[u];
      msk[u] = (t + u < wk.ntrip) ? 1.0f : 0.0f;
      const float* wp = w + (int64_t)pn[u] * F3 + f;
      const float* dp = dw + (int64_t)pn[u] * F3 + f;
      wv[u][0] = ldv_of<vf>(wp);
      wv[u][1] = ldv_of<vf>(wp + F);
      wv[u][2] = ldv_of<vf>(wp + 2 * F);
      dv[u][0] = ldv_of<vf>(dp);
      dv[u][1] = ldv_of<vf>(dp + F);
      dv[u][2] = ldv_of<vf>(dp + 2 * F);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) walk_record<SRC>(wk, T, csr_lds, t + U + u, jn[u], pn[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      vf s9[9];
      // closed tile: r0 <= j < r0 + 64
      load9_window_or_global(s9, staged, T.lds.win, FOLD ? ((jj[u] - T.r0) & (MP_W - 1)) : jj[u] - lo, VW * ql, gMi, jj[u], F, f);
      message_fma9(acc, wv[u], msk[u], s9);
      const vf hv = dv[u][0] * (s9[0] * y[0]) + mul_rounded(dv[u][1], s9[1] * y[1] + mul_rounded(s9[2], y[2]) + s9[3] * y[3]) +
                    dv[u][2] * (s9[4] * y[4] + mul_rounded(s9[5], y[5]) + s9[6] * y[6] + s9[7] * y[7] + s9[8] * y[8]);
      const float h = row_sum((hv[0] + hv[1]) + (hv[2] + hv[3]), LPR);
      // slot (pair, direction): direction 0 when the walked row is the pair's i (its neighbour has the smaller index); self edge: none
      if (ql == 0 && t + u < wk.ntrip && jj[u] != row_now) {
        const int sl = 2 * pp[u] + (jj[u] < row_now ? 0 : 1);
        if (nslot) T.lds.slot[sl - 2 * slot_p0] = h;
        else slot_base[sl] = h;
      }
    }
  }
  if (!parked) {  // a helper whose own row is empty
    walk_park(acc, wk, T.lds, VW * ql);
    load_y(i);
  }
  __syncthreads();  // the parked sums and the tile's slots are complete
  // The row's nine pieces of gPn are requested together: as *op = *op + acc[c], piece by piece, every load waited for the store
  // of the piece before (the compiler cannot know that they do not overlap) - nine load and store round trips in a row at the
  // end of every block.  Same sum, old + acc.  The slot write-out comes last: nothing waits for its stores.
  if (live) {
    float* o = gPn + (int64_t)i * F9 + f;
    vf old[9];
    load9(old, (const float*)o, F);
    walk_add_parked(acc, wk, T.lds, VW * ql);
#pragma unroll
    for (int c = 0; c < 9; ++c) *reinterpret_cast<vf*>(o + c * F) = old[c] + acc[c];
  }
#pragma unroll
  for (int it = 0; it < (MP_SLOTS + 64 * MP_WAVES - 1) / (64 * MP_WAVES); ++it) {  // (the range is 8-byte aligned at best: dwords)
    const int k = tid + it * 64 * MP_WAVES;
    if (k < nslot) slot_base[2 * slot_p0 + k] = T.lds.slot[k];
  }
}

// The reverse sweep on any graph: the prologue is the forward kernel's, with gMi as the window's source.
// message_adjoint_pair_ok looks at the batch as a whole (g.small_mols: the AVERAGE molecule has at most 96 atoms), so a large
// molecule in a batch of small ones does come here: a tile whose window is wider than MP_W rows gathers gMi from global memory,
// one whose slice exceeds MP_E entries reads its records from global memory and walks every row with its own group only (no
// helpers); both block-uniform, both compared with fp64 in tests/test_gpu_message.py and, through the engine, in
// tests/test_gpu_bench_scale.py.
__global__ __launch_bounds__(512) void k_message_adjoint_rows8(Graph g, int N, int F, const float* __restrict__ w,
                                                               const float* __restrict__ dw, const float* __restrict__ gMi,
                                                               const float* __restrict__ Pn, float* __restrict__ gPn,
                                                               float* __restrict__ slots, int64_t slot_stride, int nchunks) {
  constexpr int THREADS = 512;
  __shared__ __attribute__((aligned(16))) float win[MP_W * 9 * MP_FC];
  __shared__ __attribute__((aligned(16))) float s_help[(MP_TA / 2) * 9 * MP_FC];
  __shared__ int s_col[MP_E], s_pair[MP_E];
  __shared__ int s_lo[THREADS / 64], s_hi[THREADS / 64], s_rp[MP_TA], s_len[MP_TA], s_rank[MP_TA], s_byrank[MP_TA];
  __shared__ int s_prange[3 * MP_WAVES];
  __shared__ float s_slot[MP_SLOTS];
  if (g.counts[2]) return;
  const Tile T = tile_of_block(g, N, nchunks, {lds_ptr(win), lds_ptr(s_help), lds_ptr(s_col), lds_ptr(s_pair), lds_ptr(s_rp),
                                               lds_ptr(s_len), lds_ptr(s_rank), lds_ptr(s_byrank), lds_ptr(s_prange), lds_ptr(s_slot)});
  const int tid = threadIdx.x;

  const bool csr_lds = T.nE <= MP_E;  // block-uniform
  int lo = 0x7fffffff, hi = -1;
  stage_slice<THREADS, true>(g, T, csr_lds, tid, lo, hi, g.counts[0]);
  window_bounds<THREADS>(lo, hi, lds_ptr(s_lo), lds_ptr(s_hi), tid);
  const int wn = hi - lo + 1;
  const bool staged = hi >= lo && wn <= MP_W;  // block-uniform
  stage_window<THREADS, MP_FC>(gMi, F, T, lo, staged ? wn : 0, tid);

  int slot_p0;
  const int nslot = slot_range(T.lds, slot_p0);
  adjoint_tile_body<false>(T, N, F, w, dw, gMi, Pn, gPn, slots, slot_stride, csr_lds, staged, lo, nslot, slot_p0);
}

// The reverse sweep with the adjoint of the group product (k_message_bwd_node, tn_kernels.hip) folded into its prologue, for CLOSED
// tiles: every neighbour of every row of the tile lies in the tile's own aligned 64 rows (brute-force graph of a sorted batch in
// which no molecule straddles a multiple of 64 rows; the host knows it from counts[7] of the graph build).  The window then is
// the tile's own rows, and instead of staging gMi from memory the thread (row = tid / 8, piece = tid % 8) loads the nine 16-byte
// pieces of gCh, Pn and Mi of its row, runs the adjoint one channel at a time, puts gM into the window and writes gY - the
// direct part of gPn - to the row the same thread read-modify-writes in the body's epilogue: gMi never goes through memory, and
// k_message_bwd_node is not launched.  A closed tile has at most 64 x 64 = MP_E adjacency entries, so the slice always sits in
// LDS; everything behind the prologue is adjoint_tile_body<true>.
__global__ __launch_bounds__(512) void k_message_adjoint_rows8_fold(Graph g, int N, int F, const float* __restrict__ w,
                                                                    const float* __restrict__ dw, const float* __restrict__ gCh,
                                                                    const float* __restrict__ Mi, const float* __restrict__ q,
                                                                    const int64_t* __restrict__ batch, int o3,
                                                                    const float* __restrict__ Pn, float* __restrict__ gPn,
                                                                    float* __restrict__ slots, int64_t slot_stride, int nchunks) {
  constexpr int LPR = 8, VW = 4, THREADS = 512;
  static_assert(THREADS == MP_TA * (MP_FC / 4) && MP_W == MP_TA, "one thread per (row, 16-byte piece) of the tile");
  __shared__ __attribute__((aligned(16))) float win[MP_W * 9 * MP_FC];
  __shared__ __attribute__((aligned(16))) float s_help[(MP_TA / 2) * 9 * MP_FC];
  __shared__ int s_col[MP_E], s_pair[MP_E];
  __shared__ int s_rp[MP_TA], s_len[MP_TA], s_rank[MP_TA], s_byrank[MP_TA];
  __shared__ int s_prange[3 * MP_WAVES];
  __shared__ float s_slot[MP_SLOTS];
  if (g.counts[2]) return;
  const Tile T = tile_of_block(g, N, nchunks, {lds_ptr(win), lds_ptr(s_help), lds_ptr(s_col), lds_ptr(s_pair), lds_ptr(s_rp),
                                               lds_ptr(s_len), lds_ptr(s_rank), lds_ptr(s_byrank), lds_ptr(s_prange), lds_ptr(s_slot)});
  const int tid = threadIdx.x, F9 = 9 * F;

  if (T.nE > MP_E) return;  // not a closed tile (at most 64 x 64 entries): never launched on one; keeps the LDS slice in bounds
  int no_lo, no_hi;  // the window is the tile: WINDOW = false leaves them untouched
  stage_slice<THREADS, false>(g, T, true, tid, no_lo, no_hi, g.counts[0]);
  __syncthreads();
  // read here, with no store in flight: behind the prologue's gY stores the compiler waits for them in front of these LDS reads
  int slot_p0;
  const int nslot = slot_range(T.lds, slot_p0);

  const int rl = tid / LPR, i = T.r0 + rl, ql = tid & (LPR - 1), f = T.c0 + VW * ql;
  const bool live = i < T.r1;
  {
    // ---- prologue: the row's pieces of gCh, Pn and Mi are requested together; the rank of the rows is computed while they
    // are on their way.  (Requested in front of the slice, so that slice and pieces share one round trip, the kernel was slower:
    // 271.0 against 266.7 us per launch, profiles/pair_loop_stores_notes.md.)
    const int64_t base = (int64_t)min(i, N - 1) * F9 + f;
    f4v gc4[9], y4[9], m4[9];
    if (live) {
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        gc4[c] = ldg4(gCh + base + c * F);
        y4[c] = ldg4(Pn + base + c * F);
        m4[c] = ldg4(Mi + base + c * F);
      }
    }
    rank_rows(T.lds.len, T.lds.rank, T.lds.byrank, tid);
    if (live) {
      const float kap = kappa_of(q, batch, i);
#pragma unroll
      for (int t = 0; t < VW; ++t) {
        float gc[9], y9[9], m9[9], gm[9], gy[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) {
          gc[c] = gc4[c][t];
          y9[c] = y4[c][t];
          m9[c] = m4[c][t];
        }
        group_product_adjoint(gc, y9, m9, kap, o3, gm, gy);  // tn_common.h
#pragma unroll
        for (int c = 0; c < 9; ++c) {  // gc4 / m4 are dead for this channel: they carry gM / gY out
          gc4[c][t] = gm[c];
          m4[c][t] = gy[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        *reinterpret_cast<f4v*>(&win[(rl * 9 + c) * MP_FC + VW * ql]) = gc4[c];
        *reinterpret_cast<f4v*>(gPn + base + c * F) = m4[c];
      }
    }
    __syncthreads();
  }

  adjoint_tile_body<true>(T, N, F, w, dw, nullptr, Pn, gPn, slots, slot_stride, true, true, T.r0, nslot, slot_p0);
}

bool message_adjoint_pair_ok(const Graph& g, int N, int F) {
  static const bool off2 = getenv("TMDNET_NO_ADJ_ROWS8") != nullptr;  // developer switch: the row kernel k_message_adjoint_gd
  static const bool off = getenv("TMDNET_NO_MSG_ROWS8") != nullptr;   // developer switch: one-channel-per-lane sweeps
  if (off || off2 || !g.small_mols || F < MP_FC || F % MP_FC) return false;
  return (int64_t)((N + MP_TA - 1) / MP_TA) * (F / MP_FC) >= 512;
}
void launch_message_adjoint_pair(const Graph& g, int N, int F, const float* w, const float* dw, const float* gMi, const float* Pn,
                                 float* gPn, float* slots, int64_t slot_stride, hipStream_t s, const NodeAdjointFold* fold) {
  const int nchunks = F / MP_FC, tiles = (N + MP_TA - 1) / MP_TA;
  if (fold) {  // closed tiles (the caller knows): gMi is neither read nor written
    hipLaunchKernelGGL(k_message_adjoint_rows8_fold, dim3(tiles * nchunks), dim3(512), 0, s, g, N, F, w, dw, fold->gCh, fold->Mi, fold->q,
                       fold->batch, fold->o3, Pn, gPn, slots, slot_stride, nchunks);
    return;
  }
  hipLaunchKernelGGL(k_message_adjoint_rows8, dim3(tiles * nchunks), dim3(512), 0, s, g, N, F, w, dw, gMi, Pn, gPn, slots, slot_stride,
                     nchunks);
}

bool message_pair_ok(int N, int F) {
  static const bool off = getenv("TMDNET_NO_MSG_ROWS8") != nullptr;  // developer switch: one-channel-per-lane sweeps
  if (off || F < MP_FC || F % MP_FC) return false;
  return (int64_t)((N + MP_TA - 1) / MP_TA) * (F / MP_FC) >= 512;
}
void launch_message_pair(const Graph& g, int N, int F, const float* w, const float* src, const float* q, const int64_t* batch,
                         int o3, float* Mi, float* Ch, hipStream_t s, int balance_arg) {
  const int nchunks = F / MP_FC, tiles = (N + MP_TA - 1) / MP_TA;
  static const int balance_env = getenv("TMDNET_MSG_NOBALANCE") ? 0 : 1;  // developer switch: every row walked by its own group only
  const int balance = balance_arg < 0 ? balance_env : (balance_arg ? 1 : 0);
  hipLaunchKernelGGL((k_message_rows8<8, 4>), dim3(tiles * nchunks), dim3(512), 0, s, g, N, F, w, src, q, batch, o3, Mi, Ch, nchunks, balance);
}

}  // namespace tn
