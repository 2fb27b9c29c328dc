// The finish launch of the reducers that walk the tile plan (kgat_spmm_plan.h) and are not the sum: max
// (kgat_spmm_max.hip), top-4 (kgat_spmm_kmax.hip) and R-GCN's FWD / BWD_X (kgat_rgcn.hip).  Stated once, as a template
// over LPR and a LANE type that says what is accumulated.  The three GAT walks (kgat_gat.hip) keep a copy of it.  Not
// part of the ABI.  DESIGN section 25.
//
// The decomposition all of them share.  The CSR positions [e0, e1) of a call are cut into merge_plan's tiles of te
// positions, one workgroup per tile.  LPR lanes (a lane group) cover a row and walk a run of te / NSUB consecutive
// positions with U gathers in flight, (col, row, per-edge values) handed round by shuffles; a row that ends inside the
// run is written complete, except the run's first.  A run's first and last row may continue in a neighbour run: those
// partials go through LDS (two entries per run, in run order; the entries of one row are consecutive) and the lane group
// whose entry starts a row's segment combines the segment in order.  The tile's first row (slot 0) and last row (slot 1)
// go to the workspace.  The finish launch, over the n_tiles tiles and the rows [row0, row0 + n_rows):
//   blocks below fix_blocks   one lane group (LPR lanes) per (tile, slot) item.  The tile where the row starts owns it
//                             and takes the row's partials over the tiles it spans, in tile order; a chain of kLongChain
//                             tiles and more is handed to the whole wavefront, whose lane groups stride over the tiles
//                             and fold in a fixed tree.
//   the other blocks          one lane tests one row; the wavefront's lane groups write the rows without edges in turn.
// Only blockIdx.x / gridDim.x are used here: blockIdx.y and gridDim.y belong to the lane (max's column passes).  Every
// order is fixed by the graph alone: no atomics, the same bits from every launch.
//
// The lane contract.  Lane(sl, args...) is constructed HERE from the kernel's arguments: a lane handed in by reference
// is memory while this function is optimised on its own, before it is inlined into the kernel (the top-4 finish then
// needs 65 registers for 54).
//   reset()               the accumulator becomes the identity
//   add_part(tile, slot)  takes the workspace partial of (tile, slot)
//   fold(off)             takes the accumulator of the lane `off` away (xor) in the wavefront
//   emit(row)             writes a finished row, counted from the call's first row
//   emit_no_edges(row)    writes what a row without edges gets
//
// The tile kernels - the run walk and the run-boundary combine - stay in their files: stated once over the same kind of
// lane they measured 1 - 5 % slower in all three families that were tried.  GAT's finish stays a copy because this
// template over its lane gives the forward a worse long-chain loop (both in DESIGN section 25).
#pragma once
#include "kgat_spmm_plan.h"

namespace kgat {

template <int LPR, typename Lane, typename... LaneArgs>
__device__ __forceinline__ void tile_finish(int64_t e0, int64_t e1, int32_t te, int32_t row0, int32_t n_rows,
                                            int32_t n_tiles, int32_t fix_blocks, const int32_t* indptr,
                                            const int32_t* row_of, LaneArgs... lane_args) {
  constexpr int SPW = kWave / LPR;  // lane groups per wavefront
  constexpr int WPB = spmm_threads(LPR) / kWave;
  static_assert(LPR <= kWave / 2, "a wavefront holds at least two lane groups");
  const int tid = threadIdx.x;
  const int wave = tid / kWave, lane_id = tid % kWave;
  const int q = lane_id / LPR, sl = lane_id % LPR;
  Lane lane(sl, lane_args...);
  if ((int32_t)blockIdx.x < fix_blocks) {
    const int64_t item = ((int64_t)blockIdx.x * WPB + wave) * SPW + q;
    const int32_t b = (int32_t)(item >> 1);
    const int s = (int)(item & 1);
    int32_t my_row = -1, my_bl = 0;
    if (b < n_tiles) {
      const int64_t t0 = e0 + (int64_t)b * te;
      const int64_t t1 = (t0 + te < e1) ? t0 + te : e1;
      const int32_t fr = row_of[t0], lr = row_of[t1 - 1];
      if (!(s == 1 && lr == fr)) {
        const int32_t r = s == 0 ? fr : lr;
        const int64_t rb = indptr[r], re = indptr[r + 1];
        if ((int32_t)((rb - e0) / te) == b) {  // the row starts in this tile
          my_row = r;
          my_bl = (int32_t)((re - 1 - e0) / te);
        }
      }
    }
    const bool is_long = my_row >= 0 && my_bl - b >= kLongChain;
    if (my_row >= 0 && !is_long) {
      lane.reset();
      lane.add_part(b, s);
      for (int32_t bb = b + 1; bb <= my_bl; ++bb) lane.add_part(bb, 0);
      lane.emit((size_t)(my_row - row0));
    }
    unsigned long long todo = __ballot(is_long && sl == 0);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int32_t r = __shfl(my_row, src, kWave);
      const int32_t bl = __shfl(my_bl, src, kWave);
      const int32_t bo = __shfl(b, src, kWave);
      const int so = __shfl(s, src, kWave);
      lane.reset();
      for (int32_t bb = bo + q; bb <= bl; bb += SPW) lane.add_part(bb, bb == bo ? so : 0);
#pragma unroll
      for (int off = LPR; off < kWave; off <<= 1) lane.fold(off);
      if (q == 0) lane.emit((size_t)(r - row0));
    }
  } else {
    const int64_t n_waves = (int64_t)(gridDim.x - fix_blocks) * WPB;
    const int64_t wv = (int64_t)(blockIdx.x - fix_blocks) * WPB + wave;
    for (int64_t v0 = wv * kWave; v0 < n_rows; v0 += n_waves * kWave) {
      const int64_t v = v0 + lane_id;
      bool empty = false;
      if (v < n_rows) {
        const int32_t row = row0 + (int32_t)v;
        empty = indptr[row] == indptr[row + 1];
      }
      unsigned long long m = __ballot(empty);
      int turn = 0;
      while (m) {
        const int bit = __ffsll((long long)m) - 1;
        m &= m - 1;
        if (turn == q) lane.emit_no_edges((size_t)(v0 + bit));
        turn = turn + 1 == SPW ? 0 : turn + 1;
      }
    }
  }
}

}  // namespace kgat
