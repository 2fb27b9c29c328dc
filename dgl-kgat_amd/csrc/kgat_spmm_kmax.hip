// u_mul_e / copy_src -> top-4 aggregation with back-pointers for gfx950: the k-best max-times product behind the ranked
// attention-path explanations (explain.attention_paths(top=2..4); KGAT paper, section 4.5 / figure 4).  DESIGN section 18.
//
// X is [N x Q x 4]: Q queries with four slots each.  For destination row v and query q the candidates are
//   { (w[p] * X[col[p], q, s], id(p), s) : p a CSR position of row v, s in 0..3 }      (w == NULL: times 1.0f)
// with id(p) = eid[p] (eid != NULL) or p, and the four largest come back in order: their product bits in
// out[v - row0, q, 0..3], their ids in arg_edge, their source slots in arg_slot (one byte each, a query's four bytes
// are one 32-bit word).
//
// An element is the triple (value, id, slot).  (a, i, r) beats (b, k, s) iff a > b, or a == b and (i < k, or i == k
// and r < s): IEEE comparison on the fp32 products, -0.0 ties with 0.0.  The (id, slot) pairs of a row are distinct, so
// this is a strict total order and the four largest of a set do not depend on how the set is split or in which order
// the parts are merged: runs, tiles and lane groups merge in any grouping and every launch gives the same bits.  The
// identity is (-inf, INT32_MAX, 4); a row with an in-edge has at least four candidates, so no identity reaches `out`.
// Nothing is assumed about the order of a source's slots or about signs.  No atomics.
//
// Decomposition: the one kgat_tile_reduce.h describes, whose finish launch it shares, with LPR = Q lanes per row - one
// lane per query, whose one 16-byte load is the source's four slots and which keeps a sorted list of four triples.
// "Combine" is a merge of two 4-lists: the other list's entries are inserted one by one.
#include <limits.h>

#include "kgat_tile_reduce.h"

namespace kgat {
namespace {

constexpr int kNoEdge = INT32_MAX;  // the identity is (-inf, kNoEdge, kNoSlot)
constexpr int kNoSlot = 4;

// A lane's sorted list: entry 0 is the best.
struct Top4 {
  float v[4];
  int32_t e[4];
  int32_t s[4];
};

__device__ __forceinline__ void reset(Top4& t) {
#pragma unroll
  for (int i = 0; i < 4; ++i) { t.v[i] = -__builtin_inff(); t.e[i] = kNoEdge; t.s[i] = kNoSlot; }
}

__device__ __forceinline__ bool beats(float a, int32_t i, int32_t r, float b, int32_t k, int32_t s) {
  return a > b || (a == b && (i < k || (i == k && r < s)));
}

// Branch-free insertion: b[i] = the candidate beats entry i (monotone in i, the list is sorted); entry i becomes its
// upper neighbour where the candidate beats that one too, the candidate where it beats only entry i, else stays.
__device__ __forceinline__ void insert(Top4& t, float m, int32_t id, int32_t sl) {
  bool b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) b[i] = beats(m, id, sl, t.v[i], t.e[i], t.s[i]);
#pragma unroll
  for (int i = 3; i > 0; --i) {
    t.v[i] = b[i] ? (b[i - 1] ? t.v[i - 1] : m) : t.v[i];
    t.e[i] = b[i] ? (b[i - 1] ? t.e[i - 1] : id) : t.e[i];
    t.s[i] = b[i] ? (b[i - 1] ? t.s[i - 1] : sl) : t.s[i];
  }
  t.v[0] = b[0] ? m : t.v[0];
  t.e[0] = b[0] ? id : t.e[0];
  t.s[0] = b[0] ? sl : t.s[0];
}

__device__ __forceinline__ uint32_t pack_slots(const Top4& t) {
  return (uint32_t)t.s[0] | ((uint32_t)t.s[1] << 8) | ((uint32_t)t.s[2] << 16) | ((uint32_t)t.s[3] << 24);
}

// Merge of a stored list (four values, four ids, the packed slots) into t.
__device__ __forceinline__ void merge(Top4& t, const float4 v, const int4 e, uint32_t s) {
  insert(t, v.x, e.x, (int32_t)(s & 255u));
  insert(t, v.y, e.y, (int32_t)((s >> 8) & 255u));
  insert(t, v.z, e.z, (int32_t)((s >> 16) & 255u));
  insert(t, v.w, e.w, (int32_t)(s >> 24));
}

__device__ __forceinline__ void load_list(Top4& t, const float4 v, const int4 e, uint32_t s) {
  t.v[0] = v.x; t.v[1] = v.y; t.v[2] = v.z; t.v[3] = v.w;
  t.e[0] = e.x; t.e[1] = e.y; t.e[2] = e.z; t.e[3] = e.w;
  t.s[0] = (int32_t)(s & 255u); t.s[1] = (int32_t)((s >> 8) & 255u); t.s[2] = (int32_t)((s >> 16) & 255u);
  t.s[3] = (int32_t)(s >> 24);
}

__device__ __forceinline__ float4 vals(const Top4& t) { return make_float4(t.v[0], t.v[1], t.v[2], t.v[3]); }
__device__ __forceinline__ int4 ids(const Top4& t) { return make_int4(t.e[0], t.e[1], t.e[2], t.e[3]); }

// Query `sl` of output row `row`: the lane's 16 bytes of out and arg_edge, its word of arg_slot.
template <int LPR>
__device__ __forceinline__ void store_row(float4* __restrict__ out, int4* __restrict__ arg_edge,
                                          uint32_t* __restrict__ arg_slot, size_t row, int sl, const float4 v,
                                          const int4 e, uint32_t s) {
  const size_t o = row * LPR + sl;
  out[o] = v;
  if (arg_edge) arg_edge[o] = e;
  if (arg_slot) arg_slot[o] = s;
}

// workspace: per tile two slots (the tile's first row, its last row) of LPR lists
template <int LPR>
__device__ __forceinline__ size_t part_index(int64_t tile, int slot, int sl) {
  return ((size_t)tile * 2 + slot) * LPR + sl;
}

template <int LPR>
__global__ __launch_bounds__(spmm_threads(LPR)) void spmm_max4_tile_kernel(
    int64_t e0, int64_t e1, int32_t te, int32_t row0, const int32_t* __restrict__ col,
    const int32_t* __restrict__ row_of, const int32_t* __restrict__ eid, const float4* __restrict__ X,
    const float* __restrict__ w, float4* __restrict__ out, int4* __restrict__ arg_edge,
    uint32_t* __restrict__ arg_slot, float4* __restrict__ bval, int4* __restrict__ bid, uint32_t* __restrict__ bslot) {
  constexpr int NSUB = spmm_threads(LPR) / LPR;
  constexpr int U = 4;  // X rows in flight per lane group
  __shared__ float4 s_val[NSUB][2][LPR];
  __shared__ int4 s_id[NSUB][2][LPR];
  __shared__ uint32_t s_slot[NSUB][2][LPR];
  __shared__ int32_t s_row[NSUB][2];

  const int tid = threadIdx.x;
  const int sub = tid / LPR, sl = tid % LPR;
  const int C = te / NSUB;  // edges per run
  const int64_t tile0 = e0 + (int64_t)blockIdx.x * te;
  const int64_t tile1 = (tile0 + te < e1) ? tile0 + te : e1;
  const int64_t p0 = tile0 + (int64_t)sub * C;
  const int64_t p1 = (p0 + C < tile1) ? p0 + C : tile1;

  int32_t cur_row = -1;
  bool head_done = false;
  Top4 t;
  reset(t);
  auto flush = [&]() {  // the open row ends here: the run's first row is a partial, later ones are complete
    if (!head_done) {
      s_val[sub][0][sl] = vals(t);
      s_id[sub][0][sl] = ids(t);
      s_slot[sub][0][sl] = pack_slots(t);
      if (sl == 0) s_row[sub][0] = cur_row;
      head_done = true;
    } else {
      store_row<LPR>(out, arg_edge, arg_slot, (size_t)(cur_row - row0), sl, vals(t), ids(t), pack_slots(t));
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
      float wj[U];
      float4 x[U];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        cj[i] = __shfl(c, j + i, LPR);
        rj[i] = __shfl(r, j + i, LPR);
        wj[i] = __shfl(wv, j + i, LPR);
        ij[i] = __shfl(id, j + i, LPR);
      }
#pragma unroll
      for (int i = 0; i < U; ++i) x[i] = X[(size_t)cj[i] * LPR + sl];  // positions past the run: row 0, never consumed
#pragma unroll
      for (int i = 0; i < U; ++i) {
        if (j + i < n) {
          if (rj[i] != cur_row) {
            if (cur_row >= 0) flush();
            cur_row = rj[i];
            reset(t);
          }
          insert(t, wj[i] * x[i].x, ij[i], 0);
          insert(t, wj[i] * x[i].y, ij[i], 1);
          insert(t, wj[i] * x[i].z, ij[i], 2);
          insert(t, wj[i] * x[i].w, ij[i], 3);
        }
      }
    }
  }
  // the run's last open row: head slot if the run never changed row, else tail slot
  {
    const int k = head_done ? 1 : 0;
    s_val[sub][k][sl] = vals(t);
    s_id[sub][k][sl] = ids(t);
    s_slot[sub][k][sl] = pack_slots(t);
    if (sl == 0) {
      s_row[sub][k] = cur_row;  // -1 for an empty run
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
  for (int h = 0; h < 2; ++h) {
    const int32_t rr = s_row[sub][h];
    if (rr < 0) continue;
    if (h == 0 && sub > 0) {  // (a tail entry always starts a segment: the run changed row)
      const int32_t pt = s_row[sub - 1][1];
      if ((pt >= 0 ? pt : s_row[sub - 1][0]) == rr) continue;
    }
    load_list(t, s_val[sub][h][sl], s_id[sub][h][sl], s_slot[sub][h][sl]);
    for (int k = 2 * sub + h + 1; k < 2 * NSUB; ++k) {
      const int32_t r2 = s_row[k >> 1][k & 1];
      if (r2 < 0) continue;
      if (r2 != rr) break;
      merge(t, s_val[k >> 1][k & 1][sl], s_id[k >> 1][k & 1][sl], s_slot[k >> 1][k & 1][sl]);
    }
    if (rr == first_row || rr == last_row) {
      const size_t o = part_index<LPR>(blockIdx.x, rr == first_row ? 0 : 1, sl);
      bval[o] = vals(t);
      bid[o] = ids(t);
      bslot[o] = pack_slots(t);
    } else {
      store_row<LPR>(out, arg_edge, arg_slot, (size_t)(rr - row0), sl, vals(t), ids(t), pack_slots(t));
    }
  }
}

// The finish launch (kgat_tile_reduce.h): the lane merges the workspace's partial lists; a row without in-edges gets
// out = 0, arg_edge = -1, arg_slot = 255.
template <int LPR>
struct Max4FinishLane {
  int sl;
  float4* out;
  int4* arg_edge;
  uint32_t* arg_slot;
  const float4* bval;
  const int4* bid;
  const uint32_t* bslot;
  Top4 t;

  __device__ __forceinline__ Max4FinishLane(int sl_, float4* out_, int4* arg_edge_, uint32_t* arg_slot_, const float4* bval_,
                                            const int4* bid_, const uint32_t* bslot_)
      : sl(sl_), out(out_), arg_edge(arg_edge_), arg_slot(arg_slot_), bval(bval_), bid(bid_), bslot(bslot_) {}

  __device__ __forceinline__ void reset() { kgat::reset(t); }
  __device__ __forceinline__ void add_part(int64_t tile, int slot) {
    const size_t o = part_index<LPR>(tile, slot, sl);
    merge(t, bval[o], bid[o], bslot[o]);
  }
  __device__ __forceinline__ void fold(int off) {  // both partners hold disjoint sets and end with the same list
    float4 ov;
    int4 oe;
    ov.x = __shfl_xor(t.v[0], off, kWave); ov.y = __shfl_xor(t.v[1], off, kWave);
    ov.z = __shfl_xor(t.v[2], off, kWave); ov.w = __shfl_xor(t.v[3], off, kWave);
    oe.x = __shfl_xor(t.e[0], off, kWave); oe.y = __shfl_xor(t.e[1], off, kWave);
    oe.z = __shfl_xor(t.e[2], off, kWave); oe.w = __shfl_xor(t.e[3], off, kWave);
    const uint32_t os = (uint32_t)__shfl_xor((int)pack_slots(t), off, kWave);
    merge(t, ov, oe, os);
  }
  __device__ __forceinline__ void emit(size_t row) const {
    store_row<LPR>(out, arg_edge, arg_slot, row, sl, vals(t), ids(t), pack_slots(t));
  }
  __device__ __forceinline__ void emit_no_edges(size_t row) const {
    store_row<LPR>(out, arg_edge, arg_slot, row, sl, make_float4(0.f, 0.f, 0.f, 0.f), make_int4(-1, -1, -1, -1), 0xffffffffu);
  }
};

template <int LPR>
__global__ __launch_bounds__(spmm_threads(LPR)) void spmm_max4_finish_kernel(
    int64_t e0, int64_t e1, int32_t te, int32_t row0, int32_t n_rows, int32_t n_tiles,
    const int32_t* __restrict__ indptr, const int32_t* __restrict__ row_of, float4* __restrict__ out,
    int4* __restrict__ arg_edge, uint32_t* __restrict__ arg_slot, const float4* __restrict__ bval,
    const int4* __restrict__ bid, const uint32_t* __restrict__ bslot, int32_t fix_blocks) {
  tile_finish<LPR, Max4FinishLane<LPR>>(e0, e1, te, row0, n_rows, n_tiles, fix_blocks, indptr, row_of, out, arg_edge,
                                        arg_slot, bval, bid, bslot);
}

constexpr size_t kListBytes = sizeof(float4) + sizeof(int4) + sizeof(uint32_t);  // one lane's partial in the workspace

struct Max4Args {
  int64_t n_rows, row0, e0, e1;
  const int32_t *indptr, *col, *row_of, *eid;
  const float *X, *w;
  float* out;
  int32_t* arg_edge;
  uint8_t* arg_slot;
  void* ws;
  hipStream_t st;
};

template <int LPR>
int launch_max4(const Max4Args& a, const MergePlan& m) {
  constexpr int kThreads = spmm_threads(LPR);
  float4* bval = static_cast<float4*>(a.ws);
  int4* bid = reinterpret_cast<int4*>(bval + m.part_elems);
  uint32_t* bslot = reinterpret_cast<uint32_t*>(bid + m.part_elems);
  float4* out = reinterpret_cast<float4*>(a.out);
  int4* arg_edge = reinterpret_cast<int4*>(a.arg_edge);
  uint32_t* arg_slot = reinterpret_cast<uint32_t*>(a.arg_slot);
  if (m.tiles > 0) {
    hipLaunchKernelGGL((spmm_max4_tile_kernel<LPR>), dim3((unsigned)m.tiles), dim3(kThreads), 0, a.st, a.e0, a.e1,
                       (int32_t)m.tile_edges, (int32_t)a.row0, a.col, a.row_of, a.eid,
                       reinterpret_cast<const float4*>(a.X), a.w, out, arg_edge, arg_slot, bval, bid, bslot);
    KGAT_CHECK_LAUNCH("spmm_max4_tile");
  }
  hipLaunchKernelGGL((spmm_max4_finish_kernel<LPR>), dim3((unsigned)(m.fix_blocks + m.nz_blocks)), dim3(kThreads), 0, a.st,
                     a.e0, a.e1, (int32_t)m.tile_edges, (int32_t)a.row0, (int32_t)a.n_rows, (int32_t)m.tiles, a.indptr,
                     a.row_of, out, arg_edge, arg_slot, (const float4*)bval, (const int4*)bid, (const uint32_t*)bslot,
                     m.fix_blocks);
  KGAT_CHECK_LAUNCH("spmm_max4_finish");
  return KGAT_OK;
}

inline bool max4_width(int Q) { return Q > 0 && Q <= 32 && has_width(TileWidths{}, 4 * Q); }

}  // namespace
}  // namespace kgat

using namespace kgat;

extern "C" {

size_t kgat_spmm_max4_workspace_bytes(int64_t n_edges, int Q) {
  if (n_edges <= 0 || !max4_width(Q)) return 256;
  return plan_workspace_bytes(merge_plan(Q, n_edges, 0).part_elems, kListBytes);
}

int kgat_spmm_umule_max4_f32(int64_t n_rows, int64_t row0, int64_t e_begin, int64_t e_end, int Q, const int32_t* indptr,
                             const int32_t* col, const int32_t* row_of, const int32_t* eid, const float* X,
                             const float* w, float* out, int32_t* arg_edge, uint8_t* arg_slot, void* workspace,
                             size_t workspace_bytes, kgat_stream_t stream) {
  KGAT_RETURN_IF(check_rows("spmm_max4", n_rows, row0, e_begin, e_end, Q));
  KGAT_CHECK_ARG(max4_width(Q), "spmm_max4: Q = %d queries, the kernel covers 4, 8, 16 and 32", Q);
  if (n_rows == 0) return KGAT_OK;
  KGAT_CHECK_ARG(indptr && X && out, "spmm_max4: null pointer");
  KGAT_CHECK_ARG(e_end == e_begin || (col && row_of), "spmm_max4: null col/row_of");
  KGAT_CHECK_ARG(aligned16(X) && aligned16(out) && aligned16(arg_edge) && aligned16(workspace) &&
                     (reinterpret_cast<uintptr_t>(arg_slot) & 3u) == 0,
                 "spmm_max4: X, out, arg_edge and the workspace must be 16-byte aligned, arg_slot 4-byte aligned");
  const MergePlan m = merge_plan(Q, e_end - e_begin, n_rows);
  // (a short workspace is one of this entry's bad arguments: KGAT_E_BADARG with check_workspace's message; the bound
  // is the size function's answer, as the header states it)
  if (check_workspace("spmm_max4", m, kgat_spmm_max4_workspace_bytes(e_end - e_begin, Q), workspace, workspace_bytes) != KGAT_OK)
    return KGAT_E_BADARG;
  Max4Args a;
  a.n_rows = n_rows; a.row0 = row0; a.e0 = e_begin; a.e1 = e_end;
  a.indptr = indptr; a.col = col; a.row_of = row_of; a.eid = eid; a.X = X; a.w = w;
  a.out = out; a.arg_edge = arg_edge; a.arg_slot = arg_slot; a.ws = workspace; a.st = as_stream(stream);
  return dispatch_width(TileWidths{}, 4 * Q, [&](auto d) { return launch_max4<decltype(d)::value / 4>(a, m); });
}

}  // extern "C"
