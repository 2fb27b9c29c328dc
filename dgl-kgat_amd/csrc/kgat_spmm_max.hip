// u_mul_e / copy_src -> max aggregation with argmax for gfx950 (DGL's fn.max reducer; the max-times product behind
// the attention-path explanations of the KGAT paper, section 4.5 / figure 4).  DESIGN section 16.
//
//   out[v - row0, j] = max over CSR positions p of row v of  w[p] * X[col[p], j]     (w == NULL: X[col[p], j])
//   arg[v - row0, j] = the edge that attains it: eid[p] (eid != NULL) or p
//
// An element is the pair (value, id).  (a, i) beats (b, k) iff a > b, or a == b and i < k (IEEE comparison on the fp32
// products: -0.0 ties with 0.0; the smallest id wins a tie and its bits are the result).  Ids are distinct, so this
// is a strict total order and the maximum does not depend on the order in which pairs are combined: runs, tiles and
// lane groups may combine in any grouping and every launch gives the same bits.  No atomics.
//
// Decomposition: the one kgat_tile_reduce.h describes, whose finish launch it shares; a partial is V (value, id) pairs
// per lane.
//
// V = 4: D = 4 LPR, 16-byte accesses.  V = 1: any D, sixteen lanes per row and one pass per sixteen columns
// (blockIdx.y) - the same kernels, no row is walked by one wavefront beyond a tile at any width.
#include <limits.h>

#include "kgat_tile_reduce.h"

namespace kgat {
namespace {

constexpr int kGenericLpr = 16;                                      // lanes per row of the any-width path
constexpr int kNoEdge = INT32_MAX;                                   // id of the identity (-inf, kNoEdge)

__device__ __forceinline__ void take(float& bv, int32_t& ba, float m, int32_t id) {
  const bool t = m > bv || (m == bv && id < ba);
  bv = t ? m : bv;
  ba = t ? id : ba;
}

// The V columns of one lane: loads from a row of X, stores to out / arg, the workspace partials.
template <int LPR, int V>
struct Lane {
  static constexpr int W = LPR * V;  // columns per pass
  int D, c0;                         // row length; the lane's first column
  bool ok;                           // V == 1: the last pass is ragged
  __device__ Lane(int D_, int sl) : D(D_), c0((int)blockIdx.y * W + sl * V), ok(V == 4 || c0 < D_) {}
  __device__ __forceinline__ void load(const float* __restrict__ X, int32_t row, float (&x)[V]) const {
    if constexpr (V == 4) {
      const float4 t = *reinterpret_cast<const float4*>(X + (size_t)row * D + c0);
      x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
      x[0] = ok ? X[(size_t)row * D + c0] : 0.f;
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ out, int32_t* __restrict__ arg, size_t row,
                                        const float (&bv)[V], const int32_t (&ba)[V]) const {
    const size_t o = row * D + c0;
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(out + o) = make_float4(bv[0], bv[1], bv[2], bv[3]);
      if (arg) *reinterpret_cast<int4*>(arg + o) = make_int4(ba[0], ba[1], ba[2], ba[3]);
    } else if (ok) {
      out[o] = bv[0];
      if (arg) arg[o] = ba[0];
    }
  }
};

template <int V>
__device__ __forceinline__ void reset(float (&bv)[V], int32_t (&ba)[V]) {
#pragma unroll
  for (int i = 0; i < V; ++i) { bv[i] = -__builtin_inff(); ba[i] = kNoEdge; }
}

// workspace: per (tile, pass) two slots (the tile's first row, its last row) of W values, then the same of W ids
template <int LPR, int V>
__device__ __forceinline__ size_t part_index(int64_t tile, int slot, int sl) {
  return (((size_t)tile * gridDim.y + blockIdx.y) * 2 + slot) * (LPR * V) + sl * V;
}

template <int LPR, int V>
__global__ __launch_bounds__(spmm_threads(LPR)) void spmm_max_tile_kernel(
    int64_t e0, int64_t e1, int32_t te, int32_t row0, int D, const int32_t* __restrict__ col,
    const int32_t* __restrict__ row_of, const int32_t* __restrict__ eid, const float* __restrict__ X,
    const float* __restrict__ w, float* __restrict__ out, int32_t* __restrict__ arg, float* __restrict__ bval,
    int32_t* __restrict__ barg) {
  constexpr int NSUB = spmm_threads(LPR) / LPR;
  constexpr int U = 4;  // X rows in flight per lane group
  constexpr int W = LPR * V;
  __shared__ float s_val[NSUB][2][W];
  __shared__ int32_t s_arg[NSUB][2][W];
  __shared__ int32_t s_row[NSUB][2];

  const int tid = threadIdx.x;
  const int sub = tid / LPR, sl = tid % LPR;
  const Lane<LPR, V> lane(D, sl);
  const int C = te / NSUB;  // edges per run
  const int64_t tile0 = e0 + (int64_t)blockIdx.x * te;
  const int64_t tile1 = (tile0 + te < e1) ? tile0 + te : e1;
  const int64_t p0 = tile0 + (int64_t)sub * C;
  const int64_t p1 = (p0 + C < tile1) ? p0 + C : tile1;

  int32_t cur_row = -1;
  bool head_done = false;
  float bv[V];
  int32_t ba[V];
  reset<V>(bv, ba);
  auto flush = [&]() {  // the open row ends here: the run's first row is a partial, later ones are complete
    if (!head_done) {
#pragma unroll
      for (int i = 0; i < V; ++i) { s_val[sub][0][sl * V + i] = bv[i]; s_arg[sub][0][sl * V + i] = ba[i]; }
      if (sl == 0) s_row[sub][0] = cur_row;
      head_done = true;
    } else {
      lane.store(out, arg, (size_t)(cur_row - row0), bv, ba);
    }
  };

  for (int64_t base = p0; base < p1; base += LPR) {
    const int64_t my = base + sl;
    const bool valid = my < p1;
    const int32_t c = valid ? col[my] : 0;
    const int32_t r = valid ? row_of[my] : -1;
    const float wv = (valid && w) ? w[my] : 1.f;              // copy_src: x * 1.f is x, bit for bit
    const int32_t id = (valid && eid) ? eid[my] : (int32_t)my;
    const int n = (p1 - base < LPR) ? (int)(p1 - base) : LPR;
    for (int j = 0; j < n; j += U) {
      int32_t cj[U], rj[U], ij[U];
      float wj[U], x[U][V];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        cj[i] = __shfl(c, j + i, LPR);
        rj[i] = __shfl(r, j + i, LPR);
        wj[i] = __shfl(wv, j + i, LPR);
        ij[i] = __shfl(id, j + i, LPR);
      }
#pragma unroll
      for (int i = 0; i < U; ++i) lane.load(X, cj[i], x[i]);  // positions past the run: row 0, never consumed
#pragma unroll
      for (int i = 0; i < U; ++i) {
        if (j + i < n) {
          if (rj[i] != cur_row) {
            if (cur_row >= 0) flush();
            cur_row = rj[i];
            reset<V>(bv, ba);
          }
#pragma unroll
          for (int k = 0; k < V; ++k) take(bv[k], ba[k], wj[i] * x[i][k], ij[i]);
        }
      }
    }
  }
  // the run's last open row: head slot if the run never changed row, else tail slot
  {
    const int t = head_done ? 1 : 0;
#pragma unroll
    for (int i = 0; i < V; ++i) { s_val[sub][t][sl * V + i] = bv[i]; s_arg[sub][t][sl * V + i] = ba[i]; }
    if (sl == 0) {
      s_row[sub][t] = cur_row;  // -1 for an empty run
      if (!head_done) s_row[sub][1] = -1;
    }
  }
  __syncthreads();

  // Combine of the run-boundary partials: the 2 NSUB entries are in run order and the entries of one row are
  // consecutive.  Lane group s looks at its own two; an entry that starts a row segment (the previous valid
  // entry belongs to another row) takes the rest of the segment and emits it.
  const int32_t first_row = s_row[0][0];
  const int32_t last_row = row_of[tile1 - 1];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int32_t rr = s_row[sub][t];
    if (rr < 0) continue;
    if (t == 0 && sub > 0) {  // (a tail entry always starts a segment: the run changed row)
      const int32_t pt = s_row[sub - 1][1];
      if ((pt >= 0 ? pt : s_row[sub - 1][0]) == rr) continue;
    }
#pragma unroll
    for (int i = 0; i < V; ++i) { bv[i] = s_val[sub][t][sl * V + i]; ba[i] = s_arg[sub][t][sl * V + i]; }
    for (int k = 2 * sub + t + 1; k < 2 * NSUB; ++k) {
      const int32_t r2 = s_row[k >> 1][k & 1];
      if (r2 < 0) continue;
      if (r2 != rr) break;
#pragma unroll
      for (int i = 0; i < V; ++i) take(bv[i], ba[i], s_val[k >> 1][k & 1][sl * V + i], s_arg[k >> 1][k & 1][sl * V + i]);
    }
    if (rr == first_row || rr == last_row) {
      const size_t o = part_index<LPR, V>(blockIdx.x, rr == first_row ? 0 : 1, sl);
#pragma unroll
      for (int i = 0; i < V; ++i) { bval[o + i] = bv[i]; barg[o + i] = ba[i]; }
    } else {
      lane.store(out, arg, (size_t)(rr - row0), bv, ba);
    }
  }
}

// The finish launch (kgat_tile_reduce.h): the lane takes the workspace partials with the tie rule; a row without in-edges
// gets out = 0, arg = -1.
template <int LPR, int V>
struct MaxFinishLane {
  const Lane<LPR, V> io;
  int sl;
  float* __restrict__ out;
  int32_t* __restrict__ arg;
  const float* __restrict__ bval;
  const int32_t* __restrict__ barg;
  float bv[V];
  int32_t ba[V];

  __device__ __forceinline__ MaxFinishLane(int sl_, int D, float* out_, int32_t* arg_, const float* bval_, const int32_t* barg_)
      : io(D, sl_), sl(sl_), out(out_), arg(arg_), bval(bval_), barg(barg_) {}

  __device__ __forceinline__ void reset() { kgat::reset<V>(bv, ba); }
  __device__ __forceinline__ void add_part(int64_t tile, int slot) {
    const size_t o = part_index<LPR, V>(tile, slot, sl);
#pragma unroll
    for (int i = 0; i < V; ++i) take(bv[i], ba[i], bval[o + i], barg[o + i]);
  }
  __device__ __forceinline__ void fold(int off) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const float ov = __shfl_xor(bv[i], off, kWave);
      const int32_t oa = __shfl_xor(ba[i], off, kWave);
      take(bv[i], ba[i], ov, oa);
    }
  }
  __device__ __forceinline__ void emit(size_t row) const { io.store(out, arg, row, bv, ba); }
  __device__ __forceinline__ void emit_no_edges(size_t row) {
#pragma unroll
    for (int i = 0; i < V; ++i) { bv[i] = 0.f; ba[i] = -1; }
    emit(row);
  }
};

template <int LPR, int V>
__global__ __launch_bounds__(spmm_threads(LPR)) void spmm_max_finish_kernel(
    int64_t e0, int64_t e1, int32_t te, int32_t row0, int32_t n_rows, int32_t n_tiles, int D,
    const int32_t* __restrict__ indptr, const int32_t* __restrict__ row_of, float* __restrict__ out,
    int32_t* __restrict__ arg, const float* __restrict__ bval, const int32_t* __restrict__ barg, int32_t fix_blocks) {
  tile_finish<LPR, MaxFinishLane<LPR, V>>(e0, e1, te, row0, n_rows, n_tiles, fix_blocks, indptr, row_of, D, out, arg, bval,
                                          barg);
}

struct MaxArgs {
  int64_t n_rows, row0, e0, e1;
  int D;
  const int32_t *indptr, *col, *row_of, *eid;
  const float *X, *w;
  float* __restrict__ out;
  int32_t* __restrict__ arg;
  void* ws;
  hipStream_t st;
};

struct MaxPlan {
  int lpr, v, passes;
  MergePlan m;
  size_t part_elems;  // values (and as many ids) in the workspace
};

// The sum kernel's tiles for the same edge count (the any-width path: its sixteen-lane geometry, D = 64, with one
// value per lane and a column pass per sixteen columns).
MaxPlan max_plan(int64_t n_edges, int64_t n_rows, int D) {
  MaxPlan p;
  const bool fast = has_width(TileWidths{}, D);
  p.lpr = fast ? D / 4 : kGenericLpr;
  p.v = fast ? 4 : 1;
  p.passes = fast ? 1 : (D + kGenericLpr - 1) / kGenericLpr;
  p.m = merge_plan(p.lpr, n_edges, n_rows);
  p.part_elems = p.m.part_elems * p.passes * p.v;
  return p;
}

template <int LPR, int V>
int launch_max(const MaxArgs& a, const MaxPlan& p) {
  constexpr int kThreads = spmm_threads(LPR);
  float* bval = static_cast<float*>(a.ws);
  int32_t* barg = reinterpret_cast<int32_t*>(bval + p.part_elems);
  if (p.m.tiles > 0) {
    hipLaunchKernelGGL((spmm_max_tile_kernel<LPR, V>), dim3((unsigned)p.m.tiles, (unsigned)p.passes), dim3(kThreads), 0, a.st,
                       a.e0, a.e1, (int32_t)p.m.tile_edges, (int32_t)a.row0, a.D, a.col, a.row_of, a.eid, a.X, a.w, a.out,
                       a.arg, bval, barg);
    KGAT_CHECK_LAUNCH("spmm_max_tile");
  }
  hipLaunchKernelGGL((spmm_max_finish_kernel<LPR, V>), dim3((unsigned)(p.m.fix_blocks + p.m.nz_blocks), (unsigned)p.passes),
                     dim3(kThreads), 0, a.st, a.e0, a.e1, (int32_t)p.m.tile_edges, (int32_t)a.row0, (int32_t)a.n_rows,
                     (int32_t)p.m.tiles, a.D, a.indptr, a.row_of, a.out, a.arg, (const float*)bval, (const int32_t*)barg,
                     p.m.fix_blocks);
  KGAT_CHECK_LAUNCH("spmm_max_finish");
  return KGAT_OK;
}

}  // namespace
}  // namespace kgat

using namespace kgat;

extern "C" {

size_t kgat_spmm_max_workspace_bytes(int64_t n_edges, int D) {
  if (n_edges <= 0 || D <= 0) return 256;
  return plan_workspace_bytes(max_plan(n_edges, 0, D).part_elems, sizeof(float) + sizeof(int32_t));
}

int kgat_spmm_umule_max_f32(int64_t n_rows, int64_t row0, int64_t e_begin, int64_t e_end, int D, const int32_t* indptr,
                            const int32_t* col, const int32_t* row_of, const int32_t* eid, const float* X,
                            const float* w, float* out, int32_t* arg, void* workspace, size_t workspace_bytes,
                            kgat_stream_t stream) {
  KGAT_RETURN_IF(check_rows("spmm_max", n_rows, row0, e_begin, e_end, D));
  KGAT_CHECK_ARG(D <= kGenericLpr * 65535, "spmm_max: D = %d is beyond the grid's column passes", D);
  if (n_rows == 0) return KGAT_OK;
  KGAT_CHECK_ARG(indptr && X && out, "spmm_max: null pointer");
  KGAT_CHECK_ARG(e_end == e_begin || (col && row_of), "spmm_max: null col/row_of");
  const MaxPlan p = max_plan(e_end - e_begin, n_rows, D);
  if (p.v == 4) {
    KGAT_CHECK_ARG(aligned16(X) && aligned16(out) && aligned16(arg),
                   "spmm_max: X, out and arg must be 16-byte aligned at D = %d", D);
  }
  KGAT_RETURN_IF(check_workspace("spmm_max", p.m, p.part_elems * (sizeof(float) + sizeof(int32_t)), workspace, workspace_bytes));
  MaxArgs a;
  a.n_rows = n_rows; a.row0 = row0; a.e0 = e_begin; a.e1 = e_end; a.D = D;
  a.indptr = indptr; a.col = col; a.row_of = row_of; a.eid = eid; a.X = X; a.w = w;
  a.out = out; a.arg = arg; a.ws = workspace; a.st = as_stream(stream);
  if (p.v == 1) return launch_max<kGenericLpr, 1>(a, p);  // any other width
  return dispatch_width(TileWidths{}, D, [&](auto d) { return launch_max<decltype(d)::value / 4, 4>(a, p); });
}

}  // extern "C"
