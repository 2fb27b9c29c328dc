// u_mul_e -> sum aggregation (SpMM) for gfx950.  Row S1 / S1b of SURVEY.md 8a.
//
// Replaces g.update_all(fn.u_mul_e('h','w','m'), fn.sum('m','h_neighbor')) of reference
// models.py:63 (DGL binary_reduce(sum, mul, SRC, EDGE), (N,D) x (E,1) broadcast):
//   out[v,:] = sum_{p in row v} w_p * X[col[p],:]
//
// Design (HBM/Infinity-Cache gather bound, 0.5 FLOP/B - no MFMA):
//  * Edge-balanced ("merge-path") decomposition over the destination-sorted edge array:
//    every 256-thread workgroup owns a tile of TE consecutive CSR positions, whatever rows
//    they belong to, so a power-law in-degree distribution cannot unbalance the launch.
//  * A row of X is D floats; LPR = D/4 lanes read it with one 16-byte load each (a full
//    256-B row per 16 lanes at D = 64, coalesced).  A wavefront therefore works on 64/LPR
//    edges per load instruction; each lane group ("subgroup") walks its own run of C
//    consecutive edges with U loads in flight, accumulating in registers and flushing when
//    the destination row changes (the row id of every CSR position is a graph-static array).
//  * The (col, w, row id) triples reach the lane groups in one of two ways: the second form
//    (spmm_merge2_kernel, weights in CSR order - the path the KGAT layer uses) stages a tile's
//    triples once into LDS as 16-byte records and reads one record per edge with a
//    ds_read_b128 broadcast; the first form (spmm_merge_kernel, also serves weights given in
//    edge-id order through eid) reads them coalesced per lane group and hands them around with
//    wavefront shuffles (ds_bpermute).
//  * Rows that end inside a run are stored straight to `out`.  A run's first and last row
//    may continue in a neighbour run: those partial sums are combined through LDS in run
//    order by the workgroup; only the first/last row of the whole tile goes to a small
//    global partial buffer, which the finish kernel sums in tile order.  No float atomics:
//    the summation order is fixed, results are bitwise reproducible.
//  * The finish kernel also writes the zero rows (destinations without in-edges).
//
// Also here: copy_src -> sum | mean (kgat_copy_reduce_f32, DGL's update_all(fn.copy_src, fn.sum | fn.mean) behind
// SAGEConv and the GCN / GraphSage aggregators).  The same decomposition without a weight stream: an edge tile's
// (col, row) pairs are staged in LDS as 8-byte records (the weighted form needs 16), a lane group walks a run of
// consecutive CSR positions and adds the gathered rows, the run's first / last row go through LDS (the workgroup
// combines them in run order) and the tile's first / last row through the global partial buffer that the finish launch
// sums in tile order.  The mean divides the fp32 sum by the in-degree where a row is completed.  No float atomics:
// bitwise reproducible.  Other widths: one wavefront per row.
#include "kgat_spmm_impl.h"

namespace kgat {

// --------------------------------------------------------------------------------------------- copy_src -> sum | mean
template <bool MEAN>
__device__ __forceinline__ float4 reduce_fin(const float4& v, int32_t cnt) {
  if (!MEAN) return v;
  const float c = (float)(cnt > 1 ? cnt : 1);
  return make_float4(v.x / c, v.y / c, v.z / c, v.w / c);
}

template <int LPR, int C, bool MEAN>
__global__ __launch_bounds__(SpmmGeom<LPR>::THREADS) void copy_merge_kernel(
    int64_t e0, int64_t e1, int32_t row0, const int32_t* __restrict__ col, const int32_t* __restrict__ row_of,
    const float4* __restrict__ X, float4* __restrict__ out, float4* __restrict__ bpart) {
  constexpr int NSUB = SpmmGeom<LPR>::NSUB;
  constexpr int TE = NSUB * C;
  constexpr int G = 4;  // edges per group
  static_assert(C % G == 0, "run length must be a multiple of the group size");
  __shared__ int2 s_rec[TE];  // (source row, destination row)
  __shared__ float4 s_part[NSUB][2][LPR];
  __shared__ int32_t s_row[NSUB][2];
  __shared__ int32_t s_cnt[NSUB][2];

  const int tid = threadIdx.x;
  const int sub = tid / LPR, sl = tid % LPR;
  const unsigned tile = blockIdx.x;
  const int64_t tile0 = e0 + (int64_t)tile * TE;
  const int64_t tile1 = (tile0 + TE < e1) ? tile0 + TE : e1;
  const int n_tile = (int)(tile1 - tile0);
  for (int k = tid; k < TE; k += SpmmGeom<LPR>::THREADS) {
    int2 rec = make_int2(0, -1);
    if (k < n_tile) {
      const int64_t p = tile0 + k;
      rec = make_int2(__builtin_nontemporal_load(col + p), __builtin_nontemporal_load(row_of + p));
    }
    s_rec[k] = rec;
  }
  __syncthreads();
  const int32_t first_row = __builtin_amdgcn_readfirstlane(s_rec[0].y);
  const int32_t last_row = __builtin_amdgcn_readfirstlane(s_rec[n_tile - 1].y);

  const int2* run = s_rec + sub * C;
  const float4* const Xl = X + sl;
  int n_run = n_tile - sub * C;
  n_run = n_run < 0 ? 0 : (n_run > C ? C : n_run);
  const int ng = n_run / G;

  int32_t cur_row = n_run > 0 ? run[0].y : -1;
  int32_t cnt = 0;
  bool head_done = false;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  auto flush = [&]() {  // the open row ends here
    if (!head_done) {
      s_part[sub][0][sl] = acc;
      if (sl == 0) { s_row[sub][0] = cur_row; s_cnt[sub][0] = cnt; }
      head_done = true;
    } else {
      // opened and closed inside this run: all its edges are here
      out[(size_t)(cur_row - row0) * LPR + sl] = reduce_fin<MEAN>(acc, cnt);
    }
    acc = make_float4(0.f, 0.f, 0.f, 0.f);
    cnt = 0;
  };
  auto load_group = [&](int g, int2 (&rec)[G], float4 (&x)[G]) {
#pragma unroll
    for (int i = 0; i < G; ++i) rec[i] = run[g * G + i];
#pragma unroll
    for (int i = 0; i < G; ++i) x[i] = Xl[(size_t)rec[i].x * LPR];
  };
  auto consume = [&](const int2 (&rec)[G], const float4 (&x)[G]) {
    if (__ballot(rec[G - 1].y != cur_row) == 0ull) {  // rows are sorted: the group stays in the open row
#pragma unroll
      for (int i = 0; i < G; ++i) acc = add4(acc, x[i]);
      cnt += G;
    } else {
#pragma unroll
      for (int i = 0; i < G; ++i) {
        if (rec[i].y != cur_row) {
          flush();
          cur_row = rec[i].y;
        }
        acc = add4(acc, x[i]);
        ++cnt;
      }
    }
  };
  int2 ra[G], rb[G];
  float4 xa[G], xb[G];
  // (the next group is requested unconditionally - past the run's end its last group again - as in spmm_merge2_kernel)
  if (ng > 0) load_group(0, ra, xa);
  for (int g = 0; g < ng; g += 2) {
    load_group(g + 1 < ng ? g + 1 : ng - 1, rb, xb);
    consume(ra, xa);
    load_group(g + 2 < ng ? g + 2 : ng - 1, ra, xa);
    if (g + 1 < ng) consume(rb, xb);
  }
  for (int j = ng * G; j < n_run; ++j) {  // only the last run of the edge range is ragged
    const int2 rec = run[j];
    const float4 x = Xl[(size_t)rec.x * LPR];
    if (rec.y != cur_row) {
      flush();
      cur_row = rec.y;
    }
    acc = add4(acc, x);
    ++cnt;
  }
  if (!head_done) {
    s_part[sub][0][sl] = acc;
    if (sl == 0) {
      s_row[sub][0] = cur_row;  // -1 for an empty run
      s_cnt[sub][0] = cnt;
      s_row[sub][1] = -1;
    }
  } else {
    s_part[sub][1][sl] = acc;
    if (sl == 0) { s_row[sub][1] = cur_row; s_cnt[sub][1] = cnt; }
  }
  __syncthreads();

  // In-order combine of the run-boundary partials by lane group 0: rows inside the tile are complete, the tile's
  // first and last row go to the partial buffer (raw sums; the finish launch divides).
  if (sub == 0) {
    float4* bp = bpart + (size_t)tile * 2 * LPR;
    int32_t crow = -1, ccnt = 0;
    float4 cacc = make_float4(0.f, 0.f, 0.f, 0.f);
    auto emit = [&](int32_t rr, const float4& v, int32_t n) {
      if (rr < 0) return;
      if (rr == first_row) bp[sl] = v;
      else if (rr == last_row) bp[LPR + sl] = v;
      else out[(size_t)(rr - row0) * LPR + sl] = reduce_fin<MEAN>(v, n);
    };
    for (int s = 0; s < NSUB; ++s) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int32_t rr = s_row[s][t];
        if (rr < 0) continue;
        const float4 v = s_part[s][t][sl];
        const int32_t n = s_cnt[s][t];
        if (rr == crow) {
          cacc = add4(cacc, v);
          ccnt += n;
        } else {
          emit(crow, cacc, ccnt);
          crow = rr;
          cacc = v;
          ccnt = n;
        }
      }
    }
    emit(crow, cacc, ccnt);
  }
}

// Finish: blocks [0, fix_blocks): one lane group per (tile, first / last row) item; the tile that holds a row's first
// edge owns it and sums the row's partials in tile order, eight at a time (a hub row's chain has hundreds),
// then divides for the mean.  Blocks from fix_blocks on: rows without in-edges are written as zeros (one lane tests
// one row's offsets).
template <int LPR, int C, bool MEAN>
__global__ __launch_bounds__(SpmmGeom<LPR>::THREADS) void copy_finish_kernel(
    int64_t e0, int64_t e1, int32_t row0, int32_t n_rows, int32_t n_tiles, const int32_t* __restrict__ indptr,
    const int32_t* __restrict__ row_of, float4* __restrict__ out, const float4* __restrict__ bpart, int32_t fix_blocks) {
  constexpr int NSUB = SpmmGeom<LPR>::NSUB;
  constexpr int TE = NSUB * C;
  constexpr int WPB = SpmmGeom<LPR>::THREADS / kWave;
  const int tid = threadIdx.x;
  if ((int32_t)blockIdx.x < fix_blocks) {
    const int sub = tid / LPR, sl = tid % LPR;
    const int64_t item = (int64_t)blockIdx.x * NSUB + sub;
    const int32_t b = (int32_t)(item >> 1);
    const int s = (int)(item & 1);
    if (b >= n_tiles) return;
    const int64_t t0 = e0 + (int64_t)b * TE;
    const int64_t t1 = (t0 + TE < e1) ? t0 + TE : e1;
    const int32_t fr = row_of[t0], lr = row_of[t1 - 1];
    if (s == 1 && lr == fr) return;
    const int32_t r = s == 0 ? fr : lr;
    const int64_t rb = indptr[r], re = indptr[r + 1];
    if ((int32_t)((rb - e0) / TE) != b) return;  // another tile owns the row
    const int32_t bl = (int32_t)((re - 1 - e0) / TE);
    float4 acc = bpart[((size_t)b * 2 + s) * LPR + sl];
    int32_t bb = b + 1;
    constexpr int U = 8;
    for (; bb + U - 1 <= bl; bb += U) {
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = bpart[((size_t)(bb + u) * 2) * LPR + sl];
      // eight partials summed first, then added to the chain: a hub row's hundreds of tile partials are no single
      // sequential fp32 sum
      float4 part = v[0];
#pragma unroll
      for (int u = 1; u < U; ++u) part = add4(part, v[u]);
      acc = add4(acc, part);
    }
    for (; bb <= bl; ++bb) acc = add4(acc, bpart[((size_t)bb * 2) * LPR + sl]);
    out[(size_t)(r - row0) * LPR + sl] = reduce_fin<MEAN>(acc, (int32_t)(re - rb));
  } else {
    const int lane = tid % kWave;
    constexpr int SPW = kWave / LPR >= 1 ? kWave / LPR : 1;
    const int q = (LPR < kWave) ? lane / LPR : 0, sl = tid % LPR;
    const int64_t n_waves = (int64_t)(gridDim.x - fix_blocks) * WPB;
    const int64_t wave = (int64_t)(blockIdx.x - fix_blocks) * WPB + tid / kWave;
    for (int64_t v0 = wave * kWave; v0 < n_rows; v0 += n_waves * kWave) {
      const int64_t v = v0 + lane;
      bool empty = false;
      if (v < n_rows) {
        const int32_t row = row0 + (int32_t)v;
        empty = indptr[row] == indptr[row + 1];
      }
      unsigned long long m = __ballot(empty);
      int turn = 0;
      while (m) {
        const int bt = __ffsll((long long)m) - 1;
        m &= m - 1;
        if (turn == q) out[(size_t)(v0 + bt) * LPR + sl] = make_float4(0.f, 0.f, 0.f, 0.f);
        turn = turn + 1 == SPW ? 0 : turn + 1;
      }
    }
  }
}

// Any width: one wavefront per row, lane j covers columns j, j + 64, ...; the row's positions in CSR order, summed in
// chunks of kCopyChunk positions whose sums are then added in order (a hub row of 10^5 edges summed in one sequential
// chain lands 1e-5 of the tensor's scale away from the exact sum; in chunks, as the merge path's tiles do, 1e-7).
constexpr int kCopyChunk = 128;
template <bool MEAN>
__global__ __launch_bounds__(256) void copy_rows_generic_kernel(int32_t n_rows, int32_t row0, int D,
                                                                const int32_t* __restrict__ indptr,
                                                                const int32_t* __restrict__ col,
                                                                const float* __restrict__ X, float* __restrict__ out) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int64_t v = (int64_t)blockIdx.x * (256 / kWave) + wave;
  if (v >= n_rows) return;
  const int32_t row = row0 + (int32_t)v;
  const int32_t beg = indptr[row], end = indptr[row + 1];
  const float cntf = (float)(end - beg > 1 ? end - beg : 1);
  for (int d0 = 0; d0 < D; d0 += kWave) {
    const int d = d0 + lane;
    if (d < D) {
      float acc = 0.f;
      for (int32_t p0 = beg; p0 < end; p0 += kCopyChunk) {
        const int32_t p1 = end - p0 < kCopyChunk ? end : p0 + kCopyChunk;
        float part = 0.f;
        for (int32_t p = p0; p < p1; ++p) part += X[(size_t)col[p] * D + d];
        acc += part;
      }
      out[(size_t)v * D + d] = MEAN ? acc / cntf : acc;
    }
  }
}

// SDDMM: grad_w[e] = <X[src e], G[dst e]>.  One subgroup of 16 lanes per edge.
__global__ __launch_bounds__(256) void sddmm_dot_kernel(int64_t n_edges, int D,
                                                        const int32_t* __restrict__ src,
                                                        const int32_t* __restrict__ dst,
                                                        const float* __restrict__ X,
                                                        const float* __restrict__ G,
                                                        float* __restrict__ out) {
  constexpr int L = 16;
  const int sub = threadIdx.x / L, sl = threadIdx.x % L;
  const int64_t e = (int64_t)blockIdx.x * (256 / L) + sub;
  if (e >= n_edges) return;
  const float* x = X + (size_t)src[e] * D;
  const float* g = G + (size_t)dst[e] * D;
  float acc = 0.f;
  for (int d = sl; d < D; d += L) acc = fmaf(x[d], g[d], acc);
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, L);
  if (sl == 0) out[e] = acc;
}

// Measurement aid (bench.py's roofline.gather_ceiling): reads the rows X[col[p], :] of CSR positions [0, n_edges) and
// nothing else - no weights, no row ids, no output (a running sum keeps the loads alive; `sink` is never written for
// finite data).  LPR lanes x one float4 per row, U rows in flight per lane group: the access pattern of the
// aggregation's edge loop without the aggregation.  What this launch takes is the floor of any kernel that has to
// fetch those rows through the cache hierarchy, whatever serves them (L2, Infinity Cache, HBM).
template <int LPR, int U>
__global__ __launch_bounds__(256) void gather_probe_kernel(int64_t n_edges, const int32_t* __restrict__ col,
                                                           const float4* __restrict__ X, float4* __restrict__ sink) {
  constexpr int EPS = 64 / LPR;  // edges per wavefront step
  const int lane = threadIdx.x & 63, sl = lane % LPR, sub = lane / LPR;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  constexpr int64_t kPerWave = 512;
  const int64_t base = wave * kPerWave;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t p0 = base; p0 < base + kPerWave && p0 < n_edges; p0 += EPS * U) {
    int c[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t p = p0 + EPS * u + sub;
      c[u] = col[p < n_edges ? p : n_edges - 1];
    }
    float4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = X[(size_t)c[u] * LPR + sl];
#pragma unroll
    for (int u = 0; u < U; ++u) acc = add4(acc, v[u]);
  }
  if (acc.x == 12345.678f && acc.y == -8765.4321f) sink[wave] = acc;
}

template <int LPR, int C, bool MEAN>
static int launch_copy_c(const SpmmArgs& a, const MergePlan& p) {
  const int64_t e0 = a.e0, e1 = a.e1;
  KGAT_RETURN_IF(check_workspace("copy_reduce", p, p.part_elems * sizeof(float4), a.ws, a.ws_bytes));
  float4* bpart = static_cast<float4*>(a.ws);
  constexpr int kThreads = SpmmGeom<LPR>::THREADS;
  if (p.tiles > 0) {
    hipLaunchKernelGGL((copy_merge_kernel<LPR, C, MEAN>), dim3((unsigned)p.tiles), dim3(kThreads), 0, a.st, e0, e1,
                       (int32_t)a.row0, a.col, a.row_of, (const float4*)a.X, (float4*)a.out, bpart);
    KGAT_CHECK_LAUNCH("copy_merge");
  }
  hipLaunchKernelGGL((copy_finish_kernel<LPR, C, MEAN>), dim3((unsigned)(p.fix_blocks + p.nz_blocks)), dim3(kThreads), 0,
                     a.st, e0, e1, (int32_t)a.row0, (int32_t)a.n_rows, (int32_t)p.tiles, a.indptr, a.row_of,
                     (float4*)a.out, (const float4*)bpart, p.fix_blocks);
  KGAT_CHECK_LAUNCH("copy_finish");
  return KGAT_OK;
}

template <bool MEAN>
static int launch_copy(const SpmmArgs& a) {
  if (!has_width(TileWidths{}, a.D)) {
    const int64_t blocks = (a.n_rows + 3) / 4;
    hipLaunchKernelGGL((copy_rows_generic_kernel<MEAN>), dim3((unsigned)blocks), dim3(256), 0, a.st,
                       (int32_t)a.n_rows, (int32_t)a.row0, a.D, a.indptr, a.col, a.X, a.out);
    KGAT_CHECK_LAUNCH("copy_rows_generic");
    return KGAT_OK;
  }
  return dispatch_width(TileWidths{}, a.D, [&](auto d) {
    constexpr int LPR = decltype(d)::value / 4;
    const MergePlan p = merge_plan(LPR, a);
    return dispatch_run_len<LPR>(p, [&](auto c) { return launch_copy_c<LPR, decltype(c)::value, MEAN>(a, p); });
  });
}

}  // namespace kgat

using namespace kgat;

extern "C" {

size_t kgat_spmm_workspace_bytes(int64_t n_edges, int D) {
  if (!has_width(SumWidths{}, D) || n_edges <= 0) return 256;
  return plan_workspace_bytes(merge_plan(D / 4, n_edges, 0).part_elems, sizeof(float4));
}

int kgat_spmm_tile_edges(int64_t n_edges, int D) {
  if (n_edges < 0 || !has_width(TileWidths{}, D)) return 0;
  const int te = merge_plan(D / 4, n_edges, 0).tile_edges;
  return (te & (te - 1)) == 0 ? te : 0;  // (the consumer shifts; every shipped geometry is a power of two)
}

int kgat_spmm_umule_sum_f32(int64_t n_rows, int64_t row0, int64_t e_begin, int64_t e_end, int D,
                            const int32_t* indptr, const int32_t* col, const int32_t* row_of,
                            const int32_t* eid, const float* X, const float* w, float* out,
                            const int32_t* order, void* workspace, size_t workspace_bytes,
                            unsigned flags, int algo, float* self_out, int64_t self_stride,
                            kgat_stream_t stream) {
  KGAT_RETURN_IF(check_rows("spmm", n_rows, row0, e_begin, e_end, D));
  if (n_rows == 0) return KGAT_OK;
  KGAT_CHECK_ARG(indptr && X && out, "spmm: null pointer");
  KGAT_CHECK_ARG(e_end == e_begin || (col && w), "spmm: null col/w");
  KGAT_CHECK_ARG((flags & ~(unsigned)(KGAT_SPMM_MUL_SELF | KGAT_SPMM_DEFER_FINISH)) == 0, "spmm: unknown flags 0x%x", flags);
  KGAT_CHECK_ARG(algo >= KGAT_SPMM_ALGO_AUTO && algo <= KGAT_SPMM_ALGO_MERGE1,
                 "spmm: unknown algo %d", algo);
  const bool lanes = has_width(SumWidths{}, D);  // a lane-group geometry exists
  if (algo == KGAT_SPMM_ALGO_AUTO)
    algo = (lanes && (row_of || e_end == e_begin)) ? KGAT_SPMM_ALGO_MERGE
                                  : (lanes ? KGAT_SPMM_ALGO_ROWS : KGAT_SPMM_ALGO_GENERIC);
  if (!lanes) algo = KGAT_SPMM_ALGO_GENERIC;
  KGAT_CHECK_ARG((algo != KGAT_SPMM_ALGO_MERGE && algo != KGAT_SPMM_ALGO_MERGE1) || row_of != nullptr || e_end == e_begin,
                 "spmm: merge algorithm needs row_of");
  KGAT_CHECK_ARG(order == nullptr || algo == KGAT_SPMM_ALGO_ROWS,
                 "spmm: a row order only applies to the rows algorithm");
  if (flags & KGAT_SPMM_DEFER_FINISH) {
    KGAT_CHECK_ARG(!(flags & KGAT_SPMM_MUL_SELF) && eid == nullptr && algo == KGAT_SPMM_ALGO_MERGE &&
                       kgat_spmm_tile_edges(e_end - e_begin, D) > 0,
                   "spmm: KGAT_SPMM_DEFER_FINISH goes with the plain operator, CSR-ordered weights, the merge algorithm "
                   "and D in {16, 32, 64, 128}");
  }
  if (self_out != nullptr) {
    KGAT_CHECK_ARG((flags & KGAT_SPMM_MUL_SELF) && eid == nullptr && algo == KGAT_SPMM_ALGO_MERGE,
                   "spmm: self_out goes with KGAT_SPMM_MUL_SELF, CSR-ordered weights and the merge algorithm");
    KGAT_CHECK_ARG(self_stride >= D && self_stride % 4 == 0 && aligned16(self_out),
                   "spmm: self_out must be 16-byte aligned with a row stride that is a multiple of 4 floats >= D");
  }
  SpmmArgs a;
  a.self_out = self_out; a.self_stride = self_stride;
  a.n_rows = n_rows; a.row0 = row0; a.D = D;
  a.indptr = indptr; a.col = col; a.row_of = row_of; a.eid = eid; a.order = order;
  a.X = X; a.w = w; a.out = out; a.ws = workspace; a.ws_bytes = workspace_bytes;
  a.flags = flags; a.algo = algo;
  a.e0 = (int32_t)e_begin; a.e1 = (int32_t)e_end;
  a.st = as_stream(stream);
  const bool mul = flags & KGAT_SPMM_MUL_SELF;
  if (mul) return eid ? launch_spmm<true, true>(a) : launch_spmm<true, false>(a);
  return eid ? launch_spmm<false, true>(a) : launch_spmm<false, false>(a);
}

int kgat_copy_reduce_f32(int64_t n_rows, int64_t row0, int64_t e_begin, int64_t e_end, int D, const int32_t* indptr,
                         const int32_t* col, const int32_t* row_of, const float* X, float* out, int reduce,
                         void* workspace, size_t workspace_bytes, kgat_stream_t stream) {
  KGAT_RETURN_IF(check_rows("copy_reduce", n_rows, row0, e_begin, e_end, D));
  KGAT_CHECK_ARG(reduce == KGAT_REDUCE_SUM || reduce == KGAT_REDUCE_MEAN, "copy_reduce: unknown reduce %d", reduce);
  if (n_rows == 0) return KGAT_OK;
  KGAT_CHECK_ARG(indptr && X && out, "copy_reduce: null pointer");
  const bool merge = has_width(TileWidths{}, D);
  KGAT_CHECK_ARG(e_end == e_begin || (col && (row_of || !merge)), "copy_reduce: null col / row_of");
  KGAT_CHECK_ARG(!merge || (aligned16(X) && aligned16(out)), "copy_reduce: X and out must be 16-byte aligned");
  SpmmArgs a;
  a.n_rows = n_rows; a.row0 = row0; a.D = D;
  a.indptr = indptr; a.col = col; a.row_of = row_of; a.X = X; a.out = out;
  a.ws = workspace; a.ws_bytes = workspace_bytes;
  a.e0 = (int32_t)e_begin; a.e1 = (int32_t)e_end;
  a.st = as_stream(stream);
  return reduce == KGAT_REDUCE_MEAN ? launch_copy<true>(a) : launch_copy<false>(a);
}

int kgat_gather_probe_f32(int64_t n_edges, int D, const int32_t* col, const float* X, float* sink, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_edges >= 0, "gather_probe: bad size");
  if (n_edges == 0) return KGAT_OK;
  KGAT_CHECK_ARG(col && X && sink, "gather_probe: null pointer");
  const unsigned blocks = (unsigned)((n_edges + 2047) / 2048);
  const int rc = dispatch_width(TileWidths{}, D, [&](auto d) {  // eight rows in flight per lane group
    hipLaunchKernelGGL((gather_probe_kernel<decltype(d)::value / 4, 8>), dim3(blocks), dim3(256), 0, as_stream(stream),
                       n_edges, col, reinterpret_cast<const float4*>(X), reinterpret_cast<float4*>(sink));
    return KGAT_OK;
  });
  if (rc == KGAT_E_UNSUPPORTED) {
    set_error("gather_probe: D must be 16, 32, 64 or 128 (got %d)", D);
    return rc;
  }
  KGAT_CHECK_LAUNCH("gather_probe");
  return KGAT_OK;
}

int kgat_sddmm_dot_f32(int64_t n_edges, int D, const int32_t* src, const int32_t* dst,
                       const float* X, const float* grad_out, float* grad_w,
                       kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_edges >= 0 && D > 0, "sddmm: bad size");
  if (n_edges == 0) return KGAT_OK;
  KGAT_CHECK_ARG(src && dst && X && grad_out && grad_w, "sddmm: null pointer");
  hipLaunchKernelGGL(sddmm_dot_kernel, dim3((unsigned)((n_edges + 15) / 16)), dim3(256), 0,
                     as_stream(stream), n_edges, D, src, dst, X, grad_out, grad_w);
  KGAT_CHECK_LAUNCH("sddmm_dot");
  return KGAT_OK;
}

}  // extern "C"
