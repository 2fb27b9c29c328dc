// The tile walk the kernels of kgat_att_persistent.hip share (internal): the per-relation tile prefix, a wavefront's
// share of the tiles and its cursor over relation segments, the zero fill of the never-scored tail, and the pieces
// the two fused kernels have in common.  Everything is inlined where its copy stood.  (The three-deep rings of the
// split and fold-head kernels stay two macros there: as one helper taking the step as a callable they compiled to
// other instruction sequences, 428 instructions apart in att_split_kernel<64, MODE_HEAD>.)
#pragma once
#include "kgat_att_common.h"

namespace kgat {

// Tile prefix per relation in LDS: s_tptr[r] = tiles (1 << shift items each) of the segments before r, for a
// workgroup of THREADS threads.  Returns the tile count; ends on a barrier.
template <int THREADS>
__device__ __forceinline__ int32_t att_tile_prefix(int32_t* s_tptr, const int32_t* __restrict__ seg_ptr, int n_rel,
                                                   int shift) {
  const int tid = threadIdx.x;
  for (int r = tid; r < n_rel; r += THREADS) s_tptr[r + 1] = (seg_ptr[r + 1] - seg_ptr[r] + (1 << shift) - 1) >> shift;
  __syncthreads();
  if (tid == 0) {
    int32_t run = 0;
    s_tptr[0] = 0;
    for (int r = 0; r < n_rel; ++r) {
      run += s_tptr[r + 1];
      s_tptr[r + 1] = run;
    }
  }
  __syncthreads();
  return s_tptr[n_rel];
}

// A wavefront's equal share of n items among all wavefronts of the launch: [n wv / n_waves, n (wv + 1) / n_waves),
// so the launch cannot end on a partly filled round of workgroups.
struct AttWaveShare {
  int64_t n_waves, wv;
  __device__ __forceinline__ int64_t begin(int64_t n) const { return n * wv / n_waves; }
  __device__ __forceinline__ int64_t end(int64_t n) const { return n * (wv + 1) / n_waves; }
};
template <int THREADS>
__device__ __forceinline__ AttWaveShare att_wave_share() {
  return {(int64_t)gridDim.x * (THREADS / kWave), (int64_t)blockIdx.x * (THREADS / kWave) + (int)threadIdx.x / kWave};
}

// Where a wavefront stands in its tile range: the relation segment that holds tile t, clipped to the range's end.
// All values are wave-uniform scalars.
struct AttWaveCursor {
  int r;                 // relation
  int32_t rbeg, rend;    // its items
  int32_t tfirst;        // its first tile
  int32_t seg_end;       // end of the wave's tiles in it
  int32_t n_seg;         // tiles of it owned by this wave
  int32_t item0;         // first item of the first of them
};
__device__ __forceinline__ AttWaveCursor att_wave_cursor(const int32_t* s_tptr, const int32_t* __restrict__ seg_ptr,
                                                         int n_rel, int32_t t, int32_t t_end, int shift) {
  AttWaveCursor c;
  c.r = __builtin_amdgcn_readfirstlane(segment_of(s_tptr, n_rel, t));
  c.rbeg = __builtin_amdgcn_readfirstlane(seg_ptr[c.r]);
  c.rend = __builtin_amdgcn_readfirstlane(seg_ptr[c.r + 1]);
  c.tfirst = __builtin_amdgcn_readfirstlane(s_tptr[c.r]);
  c.seg_end = __builtin_amdgcn_readfirstlane(s_tptr[c.r + 1]);
  c.seg_end = c.seg_end < t_end ? c.seg_end : t_end;
  c.n_seg = c.seg_end - t;
  c.item0 = c.rbeg + ((t - c.tfirst) << shift);
  return c;
}

// Edges whose type is outside [0, R) sit after rel_ptr[R] in the grouped order: logit 0 (DGL's zero-initialised
// column) in every output the launch has.  Each wave clears its share of that tail (the fused kernels' prologue
// below does it per workgroup).
template <bool LOGITS_EID>
__device__ __forceinline__ void att_zero_tail_wave(int64_t tail0, int64_t n_edges, const AttWaveShare& ws, int lane,
                                                   const int32_t* __restrict__ perm, const int32_t* __restrict__ pos_g,
                                                   float* __restrict__ logits, float* __restrict__ logits_csr) {
  const int64_t n_tail = n_edges - tail0;
  for (int64_t p = tail0 + ws.begin(n_tail) + lane; p < tail0 + ws.end(n_tail); p += kWave) {
    if (LOGITS_EID) logits[perm[p]] = 0.f;
    if (logits_csr) logits_csr[pos_g[p]] = 0.f;
  }
}

// ---- the fused kernels (att_fold_fused_kernel, att_fold_fused128_kernel)

// Prologue, start stamp and epilogue, as macros over names both kernels have.
// KGAT_ATT_FUSED_PROLOGUE(THREADS, PART) clears the never-scored tail (per workgroup, grid-strided, in every output the
// launch has) and DEFINES n_tiles, part, t_begin and t_end: the workgroup's contiguous tile range [t_begin, t_end),
// cost balanced (kgat_fold_tile_parts) or equal counts.  PART is the block index, or the item that gives every XCD a
// contiguous eighth of the ranges (xcd_contiguous).  It reads the kernel's OUT and tid and its parameters n_rel,
// n_edges, rel_ptr, rel_tptr, part_tptr, perm, pos_g, logits, logits_csr, logits_g.
// KGAT_ATT_FUSED_STAMP_START / KGAT_ATT_FUSED_EPILOGUE stamp the workgroup's start and end for the measurement aid
// (kgat_att_score_fused_timed_f32; 100 MHz ticks); they read clocks, tid and part.  The start stamp is its own macro
// because the kernels set up their LDS patch pointer between the range and the stamp.
// Macros, not functions: as inlined functions the zero fill and the stamps turned the part_tptr / clocks null tests
// into other branch instructions in every fused kernel, the default path's included.
#define KGAT_ATT_FUSED_PROLOGUE(THREADS, PART)                                                                         \
  for (int64_t p = (int64_t)rel_ptr[n_rel] + (int64_t)blockIdx.x * THREADS + tid; p < n_edges;                         \
       p += (int64_t)gridDim.x * THREADS) {                                                                            \
    if (OUT == 2) logits[perm[p]] = 0.f;                                                                               \
    if (OUT >= 1 && logits_csr) logits_csr[pos_g[p]] = 0.f;                                                            \
    if (logits_g) logits_g[p] = 0.f;                                                                                   \
  }                                                                                                                    \
  const int32_t n_tiles = rel_tptr[n_rel];                                                                             \
  const unsigned part = PART;                                                                                          \
  const int32_t t_begin = part_tptr ? part_tptr[part] : (int32_t)((int64_t)n_tiles * part / gridDim.x);                \
  const int32_t t_end = part_tptr ? part_tptr[part + 1] : (int32_t)((int64_t)n_tiles * (part + 1) / gridDim.x);
#define KGAT_ATT_FUSED_STAMP_START \
  if (clocks && tid == 0) clocks[2 * part] = (long long)__builtin_amdgcn_s_memrealtime();
#define KGAT_ATT_FUSED_EPILOGUE                                                           \
  if (clocks) {                                                                           \
    __syncthreads();                                                                      \
    if (tid == 0) clocks[2 * part + 1] = (long long)__builtin_amdgcn_s_memrealtime();     \
  }

// Node of lane i's head group of tile d (d.y = the tile's first group; clamped to the relation's last group).
__device__ __forceinline__ int32_t att_head_idx(const int4& d, int i, int32_t rend, const int32_t* __restrict__ g_node) {
  int32_t g = d.y + i;
  g = g < rend ? g : rend - 1;
  return g_node[g];
}

// What a lane needs for its position of a 64-position chunk of tile d starting at p0 (clamped to the tile's last
// position d.w - 1): byte offset of the source row, group slot, and where the logit goes.  The packed record is
// node | slot << 28 and N * d * 4 < 4 GiB (checked by the caller), so the node id ends below bit 32 - ROW_SHIFT and
// the shift drops exactly the slot bits.
struct AttChunkIdx { int32_t row_off, lg, oe, op; };
template <int ROW_SHIFT, int OUT>
__device__ __forceinline__ AttChunkIdx att_chunk_idx(const int4& d, int32_t p0, int lane, const int32_t* __restrict__ rec_g,
                                                     const int32_t* __restrict__ perm, const int32_t* __restrict__ pos_g,
                                                     const float* logits_csr) {
  int32_t p = p0 + lane;
  p = p < d.w ? p : d.w - 1;
  AttChunkIdx c;
  const uint32_t rec = (uint32_t)rec_g[p];
  c.row_off = (int32_t)(rec << ROW_SHIFT);
  c.lg = (int32_t)(rec >> 28);
  c.oe = OUT == 2 ? perm[p] : 0;
  c.op = (OUT >= 1 && logits_csr) ? pos_g[p] : 0;
  return c;
}

// A wave's store of a tile's V rows into its own LDS patch, between two wavefront fences: the previous tile's reads
// are done before it, and the rows are visible to every lane after it.
template <typename Store>
__device__ __forceinline__ void att_store_v_patch(Store&& store) {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  store();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Byte offset of 16-byte chunk `ch` of row `row` in a W_r piece image with ROWB-byte rows: the chunks are swizzled
// (chunk ^ (2 (row % 8) + (row / 8) % 2)) so that both products read the one image free of bank conflicts.
__device__ __forceinline__ int att_img_offset(int rowb, int row, int ch) {
  return rowb * row + 16 * (ch ^ (((row & 7) << 1) | ((row >> 3) & 1)));
}

}  // namespace kgat
