// Host side of the merge-path reducers (u_mul_e -> sum, the fused Bi form, copy_src -> sum | mean, u_mul_e -> max and
// -> top-4): the geometry constants, the ONE rule that cuts a call's CSR positions into tiles (MergePlan), the argument
// checks the five entries share and their width lists.  No kernel code: kgat_spmm_impl.h (the sum / copy kernel
// templates) and kgat_tile_reduce.h (the finish launch of the max, top-4 and R-GCN reducers) include it, and so
// does kgat_gat.hip.  Not part of the ABI.
//
// A run-length retune is made HERE and nowhere else: the launchers, the workspace functions, kgat_spmm_tile_edges
// and the max and top-4 reducers all read merge_plan().
#pragma once
#include "kgat_common.h"

namespace kgat {

// (128-thread workgroups with half-size tiles, round 3: D = 64 0.0993 vs 0.0987 ms, D = 128 0.187 vs 0.179, D = 8 0.058 vs 0.066)
constexpr int kSpmmThreads = 256;

// Threads per workgroup of the kernels that are laid out in lane groups of LPR lanes.  D <= 8 (two lanes per
// row and fewer): 128 - a 256-thread workgroup holds 128 runs there, i.e. 256 run partials to combine per
// tile; halving the workgroup (not the run length, which was tried and lost) took the D = 8 launch on the
// last-fm graph from 0.066 to 0.058 ms (round 3, AB_FLAG=-DKGAT_SPMM_THREADS=128).  Round 6 re-scanned workgroup size
// x run length for the narrow rows (scripts/micro/spmm_narrow_scan.sh, profiles/r06_spmm_narrow_scan.txt): 128 threads
// also at D = 16 / 32 - 16 runs and 32 run partials per tile, as a D = 64 tile has - with the half-length runs:
// D = 32 49.4 -> 47.6 us, D = 16 47.8 -> 44.7 (full-length runs 50.9 / 46.1, quarter-length 54.2 / 51.8); D >= 64 flat.
constexpr int spmm_threads(int lpr) { return (lpr <= 8 && kSpmmThreads == 256) ? 128 : kSpmmThreads; }

// A row cut by this many tile boundaries and more is finished by a whole wavefront instead of one lane group.
constexpr int kLongChain = 8;

// C: edges per lane-group run in the merge kernels; tiles are NSUB * C <= 2048 edges (the
// LDS record stage of the second form holds one tile).  A launch over few edges - a destination
// shard of a multi-GPU run holds E/P of them - takes the short run length: a tile is walked
// serially by its lane groups, so a launch cannot be shorter than one tile's time (~25 us at
// C = 64, which is what a 458 k-edge shard's launch took: a third of the whole graph's time for an
// eighth of its edges); a quarter of the run length gives four times the tiles, each a quarter as long.
constexpr int run_len(int lpr) { return lpr >= 8 ? 64 : (lpr == 4 ? 32 : (lpr == 2 ? 16 : 8)); }
constexpr int short_run_len(int lpr) { return run_len(lpr) / 4 >= 4 ? run_len(lpr) / 4 : 4; }
constexpr int64_t kShortRunTileLimit = 4096;  // use the short runs while they give at most this many tiles
// Between the two, for rows of 64 and 128 bytes (LPR = 4, 8: a tile is 2,048 edges there): half
// the run length while that gives at most kMidRunTileLimit tiles.  A launch of a few thousand
// full-length tiles ends with its last, longest tiles running on a nearly empty chip (tile times
// spread 14 k - 52 k cycles; 1,789 tiles on 1,280 workgroup slots at D = 32 on the amazon-book
// graph), and half-length tiles halve that tail: D = 32 0.079 -> 0.066 ms, D = 16 0.066 -> 0.060
// (quarter length: 0.076; at D = 64 / 128, 16-KB tiles of 1,024 edges, half length changes nothing,
// at D = 8 it costs 6-10 %: scripts/micro/spmm_runlen_ab.py).  The two constants exist for that A/B build only.
constexpr int kSpmmMidDiv = 2;
constexpr int mid_run_len(int lpr) {
  return (lpr == 8 || lpr == 4) ? run_len(lpr) / kSpmmMidDiv : run_len(lpr);
}
constexpr int kSpmmMidLimit = 16384;
constexpr int64_t kMidRunTileLimit = kSpmmMidLimit;

// Run length of the fused form (DO > 0): the plain operator's, so that the aggregation's summation order - and
// with it every bit of the result - is that of the two-launch sequence.  (A/B builds, KGAT_FUSED_HALF_RUNS=1: half
// the run length at D = 64 - 512-edge tiles hold half the rows and leave LDS for a 56-row buffer at five
// workgroups per CU; measured slower, profiles/r04_fused_bi_ab.txt: the per-tile phases around the edge loop
// (stage, partials, combine, the dense tail) do not shrink with the tile.)
constexpr int kFusedHalfRuns = 0;
constexpr int fused_run_len(int lpr) { return (kFusedHalfRuns && lpr >= 16) ? run_len(lpr) / 2 : run_len(lpr); }
static_assert(fused_run_len(16) == run_len(16),
              "merge_plan knows one full run length: a fused form with its own needs a plan of its own");

// The widths with a lane-group geometry (LPR = D / 4 lanes per row, one 16-byte access each).
using SumWidths = WidthList<4, 8, 16, 32, 64, 128, 256>;  // the sum operator's merge and rows kernels
using TileWidths = WidthList<16, 32, 64, 128>;            // kgat_spmm_tile_edges, the copy, max, top-4 (D = 4 Q) and probe kernels

// How the CSR positions of one call are cut: every reducer's launcher, the workspace functions and
// kgat_spmm_tile_edges read this and decide nothing themselves.
struct MergePlan {
  int run_len;         // C: edges per lane-group run (short, half or full length)
  int tile_edges;      // one workgroup's tile: one run per lane group
  int64_t tiles;       // 0 for a call without edges
  size_t part_elems;   // partial buffer, one element per lane: tiles x (first row, last row) x LPR
  int32_t fix_blocks;  // finish launch: one lane group per (tile, slot) item ...
  int64_t nz_blocks;   // ... then the rows without in-edges, one lane per row, at most 2,048 workgroups
};

// Short runs while they give at most kShortRunTileLimit tiles, else half-length runs while those give at most
// kMidRunTileLimit, else full-length runs.
inline MergePlan merge_plan(int lpr, int64_t n_edges, int64_t n_rows) {
  const int threads = spmm_threads(lpr), nsub = threads / lpr;
  const auto tiles_at = [&](int c) { return n_edges > 0 ? (n_edges + (int64_t)nsub * c - 1) / ((int64_t)nsub * c) : 0; };
  MergePlan p;
  p.run_len = tiles_at(short_run_len(lpr)) <= kShortRunTileLimit ? short_run_len(lpr)
              : tiles_at(mid_run_len(lpr)) <= kMidRunTileLimit   ? mid_run_len(lpr)
                                                                 : run_len(lpr);
  p.tile_edges = nsub * p.run_len;
  p.tiles = tiles_at(p.run_len);
  p.part_elems = (size_t)p.tiles * 2 * lpr;
  p.fix_blocks = (int32_t)((p.tiles * 2 + nsub - 1) / nsub);
  p.nz_blocks = (n_rows + threads - 1) / threads;
  if (p.nz_blocks > 2048) p.nz_blocks = 2048;
  if (p.nz_blocks < 1) p.nz_blocks = 1;
  return p;
}

// The plan's run length as a template argument: f(C) with C an integral_constant, one of the three candidates of
// LPR (two of them coincide at most widths) - the set of merge kernels built.
template <int LPR, typename F>
inline int dispatch_run_len(const MergePlan& p, F&& f) {
  return dispatch_width(WidthList<short_run_len(LPR), mid_run_len(LPR), run_len(LPR)>{}, p.run_len, f);
}

// What a workspace function answers for `elem_bytes` per partial element.
inline size_t plan_workspace_bytes(size_t part_elems, size_t elem_bytes) {
  return align_up(part_elems * elem_bytes, 256) + 256;
}

inline int check_workspace(const char* what, const MergePlan& p, size_t need, const void* ws, size_t ws_bytes) {
  if (p.tiles > 0 && (ws == nullptr || ws_bytes < need)) {
    set_error("%s: workspace too small (%zu < %zu)", what, ws_bytes, need);
    return KGAT_E_WORKSPACE;
  }
  return KGAT_OK;
}

// The head every entry of the family opens with: the row range and the CSR position range of the call.
inline int check_row_ranges(const char* what, int64_t n_rows, int64_t row0, int64_t e_begin, int64_t e_end) {
  KGAT_CHECK_ARG(row0 + n_rows < INT32_MAX, "%s: row range exceeds int32", what);
  KGAT_CHECK_ARG(e_begin >= 0 && e_end >= e_begin && e_end < INT32_MAX, "%s: bad edge range", what);
  return KGAT_OK;
}
inline int check_rows(const char* what, int64_t n_rows, int64_t row0, int64_t e_begin, int64_t e_end, int D) {
  KGAT_CHECK_ARG(n_rows >= 0 && row0 >= 0 && D > 0, "%s: bad size (n_rows=%lld row0=%lld D=%d)", what,
                 (long long)n_rows, (long long)row0, D);
  return check_row_ranges(what, n_rows, row0, e_begin, e_end);
}
inline int check_rows(const char* what, int64_t n_rows, int64_t row0, int64_t e_begin, int64_t e_end) {  // two widths: the entry names them itself
  KGAT_CHECK_ARG(n_rows >= 0 && row0 >= 0, "%s: bad size (n_rows=%lld row0=%lld)", what, (long long)n_rows,
                 (long long)row0);
  return check_row_ranges(what, n_rows, row0, e_begin, e_end);
}

}  // namespace kgat
