// Multi-head graph attention (DGL 0.4.x GATConv's aggregation) for gfx950: logits, destination softmax and the weighted
// sum in one walk over the CSR, and its backward.  DESIGN section 22.
//
//   z[e,h] = el[src e, h] + er[dst e, h];  s = leaky_relu(z);  p = exp(s - m[dst e, h]);  l[v,h] = sum_{e->v} p
//   out[v,h,:] = (sum_{e->v} c[e,h] p ft[src e, h, :]) / l[v,h]          c: 0 or 1 / (1 - drop_p), by edge id and head
//
// The attention a = p / l never exists as an edge tensor.  m is exact without a rescale: leaky_relu and the fp32 add are
// monotone, so m[v,h] = leaky_relu(max_u el[u,h] + er[v,h]) - one call of the max reducer on el (copy form, D = H) and an
// elementwise pass.  No online softmax, so no rescale order to get wrong.
//
// Decomposition: the sum kernel's (kgat_spmm_plan.h).  LPR = H F / 4 lanes cover a row of H F floats, a lane holds four
// columns of ONE head (F % 4 == 0) and walks a run of consecutive CSR positions; per lane the state is (acc[4], s): the
// weighted row sum and a per-head scalar (forward: l).  Runs' first / last rows are combined through LDS in run order,
// tiles' first / last rows through the workspace and the finish launch in tile order.  No atomics: bitwise reproducible.
// The finish divides once per output element, correctly rounded; it is this file's own copy of the launch that
// kgat_tile_reduce.h states for the other reducers (below).
//
// The three walks are one kernel template:
//   FWD      rows = destinations, forward CSR:  acc = sum c p ft[u],        s = sum p          -> out, l
//   BWD_DST  rows = destinations, forward CSR:                              s = sum g_z        -> g_er
//   BWD_SRC  rows = sources, reversed CSR:      acc = sum c a g_out[v],     s = sum g_z        -> g_ft, g_el
// with a = p / l, gamma = <g_out[v,h,:], ft[u,h,:]>, g_z = a (c gamma - sg[v,h]) (z > 0 ? 1 : slope), both backward
// walks recomputing a from the saved m and l.  What the backward reads per (destination, head) - er, m, l and
// sg = <g_out, out> - is packed into one 16-byte record by a prepare launch, so the reversed walk gathers it in one
// access.  No E-sized stream in either direction.
#include "kgat_spmm_plan.h"

namespace kgat {
namespace {

enum { kFwd = 0, kBwdDst = 1, kBwdSrc = 2 };

struct GatK {
  int64_t e1;
  int32_t te, n_rows, n_tiles, fix_blocks;
  int H, F;
  const int32_t *indptr, *col, *row_of, *eid;
  const float* row_s;    // per (row, head): FWD er, BWD_SRC el
  const float* row_m;    // FWD: m
  const float4* info;    // BWD: (er, m, l, sg) per (destination, head)
  const float* col_s;    // per (col, head), gathered per edge: FWD / BWD_DST el
  const float* row_x;    // rows of H F floats on the row side: BWD_DST g_out, BWD_SRC ft
  const float* col_x;    // rows gathered per edge: FWD / BWD_DST ft, BWD_SRC g_out
  float slope, keep_scale;
  uint32_t seed, threshold;
  float* out_rows;       // FWD out, BWD_SRC g_ft
  float* out_head;       // FWD l, BWD_DST g_er, BWD_SRC g_el
  float4* part_a;        // workspace: per (tile, slot, lane) acc
  float* part_s;         // ... and s
};

__device__ __forceinline__ bool gat_keep(uint32_t seed, uint32_t index, uint32_t threshold) {
  // the counter hash of kgat_dense.hip's drop_keep over (row = edge id, d = H, col = head): ops.dropout_keep_mask
  uint32_t x = (index * 0x9E3779B1u) ^ seed;
  x ^= x >> 16; x *= 0x85EBCA6Bu;
  x ^= x >> 13; x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x >= threshold;
}

// exp of a value <= 0 by the hardware's exp2 (one ulp; the argument's rounding adds |x| 2^-24 relative, on a term of
// weight e^x): exp(0) is exactly 1 and anything below -104 exactly 0, which the exact tests rest on.  The walks are
// bound by vector instructions more than by memory (three times the gather probe's time): the library routine and the
// hash of a call without dropout together cost 3 - 6 % of the forward on the amazon-book graph.
__device__ __forceinline__ float gat_exp(float x) { return __expf(x); }

__device__ __forceinline__ void load4(const float* __restrict__ X, size_t off, float (&x)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(X + off);
  x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
}

// The lane's share of the work: its head, the row context, one edge, and what a finished row writes.
template <int LPR, int MODE>
struct GatLane {
  static constexpr int D = LPR * 4;
  static constexpr bool kAcc = MODE != kBwdDst;
  const GatK& k;
  int sl, h, fl;         // lane in the group, its head, lanes per head
  float r_s, r_m, r_l, r_sg, r_x[4];
  float acc[4], s;

  __device__ GatLane(const GatK& k_, int sl_) : k(k_), sl(sl_), h(sl_ * 4 / k_.F), fl(k_.F / 4) {}

  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = 0.f;
    s = 0.f;
  }
  __device__ __forceinline__ void open_row(int32_t row) {
    const size_t rh = (size_t)row * k.H + h;
    if constexpr (MODE == kFwd) {
      r_s = k.row_s[rh];
      r_m = k.row_m[rh];
    } else if constexpr (MODE == kBwdDst) {
      const float4 t = k.info[rh];
      r_s = t.x; r_m = t.y; r_l = t.z; r_sg = t.w;
      load4(k.row_x, (size_t)row * D + sl * 4, r_x);
    } else {
      r_s = k.row_s[rh];
      load4(k.row_x, (size_t)row * D + sl * 4, r_x);
    }
    reset();
  }
  // <a, b> over the F columns of the lane's head (the fl lanes of a head are neighbours, fl a power of two)
  __device__ __forceinline__ float head_dot(const float (&a)[4], const float (&b)[4]) const {
    float g = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    for (int off = 1; off < fl; off <<= 1) g += __shfl_xor(g, off, LPR);
    return g;
  }
  // one edge: c_s / c_i the scalar or the record gathered at (col, head), c_x the gathered row, id the edge id
  __device__ __forceinline__ void edge(float c_s, const float4& c_i, const float (&c_x)[4], int32_t id) {
    // (threshold 0 - no dropout - keeps everything at scale 1: the hash is skipped, uniformly over the launch)
    const bool keep = k.threshold == 0u || gat_keep(k.seed, (uint32_t)id * (uint32_t)k.H + (uint32_t)h, k.threshold);
    const float c = keep ? k.keep_scale : 0.f;
    if constexpr (MODE == kFwd) {
      const float z = c_s + r_s;
      const float p = gat_exp((z > 0.f ? z : z * k.slope) - r_m);
      const float cp = c * p;
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] += cp * c_x[i];
      s += p;
    } else {
      const float gamma = head_dot(r_x, c_x);
      const float er = MODE == kBwdDst ? r_s : c_i.x, el = MODE == kBwdDst ? c_s : r_s;
      const float m = MODE == kBwdDst ? r_m : c_i.y, l = MODE == kBwdDst ? r_l : c_i.z;
      const float sg = MODE == kBwdDst ? r_sg : c_i.w;
      const float z = el + er;
      const float a = __fdiv_rn(gat_exp((z > 0.f ? z : z * k.slope) - m), l);
      const float gs = a * (c * gamma - sg);
      s += z > 0.f ? gs : gs * k.slope;
      if constexpr (kAcc) {
        const float ca = c * a;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += ca * c_x[i];
      }
    }
  }
  // a finished row (a row without edges arrives as all zeros)
  __device__ __forceinline__ void emit(size_t row) const {
    if constexpr (MODE == kFwd) {
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (s > 0.f) o = make_float4(__fdiv_rn(acc[0], s), __fdiv_rn(acc[1], s), __fdiv_rn(acc[2], s), __fdiv_rn(acc[3], s));
      *reinterpret_cast<float4*>(k.out_rows + row * D + sl * 4) = o;
    } else if constexpr (MODE == kBwdSrc) {
      *reinterpret_cast<float4*>(k.out_rows + row * D + sl * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
    if (sl % fl == 0) k.out_head[row * k.H + h] = s;
  }
  __device__ __forceinline__ size_t part_index(int64_t tile, int slot) const { return ((size_t)tile * 2 + slot) * LPR + sl; }
  __device__ __forceinline__ void to_part(int64_t tile, int slot) const {
    const size_t o = part_index(tile, slot);
    if constexpr (kAcc) k.part_a[o] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    k.part_s[o] = s;
  }
  __device__ __forceinline__ void add_part(int64_t tile, int slot) {
    const size_t o = part_index(tile, slot);
    if constexpr (kAcc) {
      const float4 t = k.part_a[o];
      acc[0] += t.x; acc[1] += t.y; acc[2] += t.z; acc[3] += t.w;
    }
    s += k.part_s[o];
  }
};

template <int LPR, int MODE>
__global__ __launch_bounds__(spmm_threads(LPR)) void gat_tile_kernel(const GatK k) {
  constexpr int NSUB = spmm_threads(LPR) / LPR;
  constexpr int U = 4;  // gathered rows in flight per lane group
  constexpr int D = LPR * 4;
  constexpr bool kAcc = MODE != kBwdDst;
  __shared__ float s_acc[kAcc ? NSUB : 1][2][D];
  __shared__ float s_s[NSUB][2][LPR];
  __shared__ int32_t s_row[NSUB][2];

  const int tid = threadIdx.x;
  const int sub = tid / LPR, sl = tid % LPR;
  GatLane<LPR, MODE> lane(k, sl);
  const int C = k.te / NSUB;  // edges per run
  const int64_t tile0 = (int64_t)blockIdx.x * k.te;
  const int64_t tile1 = (tile0 + k.te < k.e1) ? tile0 + k.te : k.e1;
  const int64_t p0 = tile0 + (int64_t)sub * C;
  const int64_t p1 = (p0 + C < tile1) ? p0 + C : tile1;

  int32_t cur_row = -1;
  bool head_done = false;
  lane.reset();
  auto stage = [&](int t) {
    if constexpr (kAcc) {
#pragma unroll
      for (int i = 0; i < 4; ++i) s_acc[sub][t][sl * 4 + i] = lane.acc[i];
    }
    s_s[sub][t][sl] = lane.s;
    if (sl == 0) s_row[sub][t] = cur_row;
  };
  auto flush = [&]() {  // the open row ends here: the run's first row is a partial, later ones are complete
    if (!head_done) {
      stage(0);
      head_done = true;
    } else {
      lane.emit((size_t)cur_row);
    }
  };

  for (int64_t base = p0; base < p1; base += LPR) {
    const int64_t my = base + sl;
    const bool valid = my < p1;
    const int32_t c = valid ? k.col[my] : 0;
    const int32_t r = valid ? k.row_of[my] : -1;
    const int32_t id = (valid && k.eid) ? k.eid[my] : (int32_t)my;
    const int n = (p1 - base < LPR) ? (int)(p1 - base) : LPR;
    for (int j = 0; j < n; j += U) {
      int32_t cj[U], rj[U], ij[U];
      float cs[U], x[U][4];
      float4 ci[U];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        cj[i] = __shfl(c, j + i, LPR);
        rj[i] = __shfl(r, j + i, LPR);
        ij[i] = __shfl(id, j + i, LPR);
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {  // positions past the run: node 0, never consumed
        load4(k.col_x, (size_t)cj[i] * D + sl * 4, x[i]);
        if constexpr (MODE == kBwdSrc) {
          ci[i] = k.info[(size_t)cj[i] * k.H + lane.h];
          cs[i] = 0.f;
        } else {
          cs[i] = k.col_s[(size_t)cj[i] * k.H + lane.h];
          ci[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        if (j + i < n) {
          if (rj[i] != cur_row) {
            if (cur_row >= 0) flush();
            cur_row = rj[i];
            lane.open_row(cur_row);
          }
          lane.edge(cs[i], ci[i], x[i], ij[i]);
        }
      }
    }
  }
  // the run's last open row: head slot if the run never changed row, else tail slot
  stage(head_done ? 1 : 0);  // (row -1 for an empty run)
  if (!head_done && sl == 0) s_row[sub][1] = -1;
  __syncthreads();

  // Combine of the run-boundary partials: the 2 NSUB entries are in run order and the entries of one row are
  // consecutive.  Lane group s looks at its own two; an entry that starts a row segment (the previous valid entry
  // belongs to another row) adds the rest of the segment in order and emits it.
  const int32_t first_row = s_row[0][0];
  const int32_t last_row = k.row_of[tile1 - 1];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int32_t rr = s_row[sub][t];
    if (rr < 0) continue;
    if (t == 0 && sub > 0) {  // (a tail entry always starts a segment: the run changed row)
      const int32_t pt = s_row[sub - 1][1];
      if ((pt >= 0 ? pt : s_row[sub - 1][0]) == rr) continue;
    }
    lane.reset();
    for (int q = 2 * sub + t; q < 2 * NSUB; ++q) {
      const int32_t r2 = s_row[q >> 1][q & 1];
      if (r2 < 0) continue;
      if (r2 != rr) break;
      if constexpr (kAcc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) lane.acc[i] += s_acc[q >> 1][q & 1][sl * 4 + i];
      }
      lane.s += s_s[q >> 1][q & 1][sl];
    }
    if (rr == first_row || rr == last_row) {
      lane.to_part(blockIdx.x, rr == first_row ? 0 : 1);
    } else {
      lane.emit((size_t)rr);
    }
  }
}

// The finish launch as kgat_tile_reduce.h describes it, kept as a copy: written as tile_finish over GatLane the
// forward's long-chain loop waits for its first load before it issues the second.  A fix to
// tile_finish is made here too.  Rows without edges: zeros.
template <int LPR, int MODE>
__global__ __launch_bounds__(spmm_threads(LPR)) void gat_finish_kernel(const GatK k) {
  constexpr int SPW = kWave / LPR;  // lane groups per wavefront
  constexpr int WPB = spmm_threads(LPR) / kWave;
  static_assert(LPR <= kWave / 2, "a wavefront holds at least two lane groups");
  const int tid = threadIdx.x;
  const int wave = tid / kWave, lane_id = tid % kWave;
  const int q = lane_id / LPR, sl = lane_id % LPR;
  GatLane<LPR, MODE> lane(k, sl);
  const int32_t te = k.te;
  if ((int32_t)blockIdx.x < k.fix_blocks) {
    const int64_t item = ((int64_t)blockIdx.x * WPB + wave) * SPW + q;
    const int32_t b = (int32_t)(item >> 1);
    const int s = (int)(item & 1);
    int32_t my_row = -1, my_bl = 0;
    if (b < k.n_tiles) {
      const int64_t t0 = (int64_t)b * te;
      const int64_t t1 = (t0 + te < k.e1) ? t0 + te : k.e1;
      const int32_t fr = k.row_of[t0], lr = k.row_of[t1 - 1];
      if (!(s == 1 && lr == fr)) {
        const int32_t r = s == 0 ? fr : lr;
        const int64_t rb = k.indptr[r], re = k.indptr[r + 1];
        if ((int32_t)(rb / te) == b) {  // the row starts in this tile
          my_row = r;
          my_bl = (int32_t)((re - 1) / te);
        }
      }
    }
    const bool is_long = my_row >= 0 && my_bl - b >= kLongChain;
    if (my_row >= 0 && !is_long) {
      lane.reset();
      lane.add_part(b, s);
      for (int32_t bb = b + 1; bb <= my_bl; ++bb) lane.add_part(bb, 0);
      lane.emit((size_t)my_row);
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
      for (int off = LPR; off < kWave; off <<= 1) {
        if constexpr (MODE != kBwdDst) {
#pragma unroll
          for (int i = 0; i < 4; ++i) lane.acc[i] += __shfl_xor(lane.acc[i], off, kWave);
        }
        lane.s +=__shfl_xor(lane.s, off, kWave);
      }
      if (q == 0) lane.emit((size_t)r);
    }
  } else {
    const int64_t n_waves = (int64_t)(gridDim.x - k.fix_blocks) * WPB;
    const int64_t wv = (int64_t)(blockIdx.x - k.fix_blocks) * WPB + wave;
    lane.reset();
    for (int64_t v0 = wv * kWave; v0 < k.n_rows; v0 += n_waves * kWave) {
      const int64_t v = v0 + lane_id;
      const bool empty = v < k.n_rows && k.indptr[v] == k.indptr[v + 1];
      unsigned long long m = __ballot(empty);
      int turn = 0;
      while (m) {
        const int bit = __ffsll((long long)m) - 1;
        m &= m - 1;
        if (turn == q) lane.emit((size_t)(v0 + bit));
        turn = turn + 1 == SPW ? 0 : turn + 1;
      }
    }
  }
}

// m = leaky_relu(max_u el[u] + er), in place over the max reducer's result
__global__ __launch_bounds__(256) void gat_row_max_kernel(int64_t n, float* __restrict__ m, const float* __restrict__ er,
                                                         float slope) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const float z = m[i] + er[i];
    m[i] = z > 0.f ? z : z * slope;
  }
}

// info[v,h] = (er, m, l, <g_out[v,h,:], out[v,h,:]>): a lane per four columns, the lanes of a head fold their dots
template <int LPR>
__global__ __launch_bounds__(256) void gat_prepare_kernel(int64_t n_nodes, int H, int F, const float* __restrict__ er,
                                                         const float* __restrict__ m, const float* __restrict__ l,
                                                         const float* __restrict__ out, const float* __restrict__ g_out,
                                                         float4* __restrict__ info) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = t / LPR;
  const int sl = (int)(t % LPR), fl = F / 4;
  float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
  const bool ok = row < n_nodes;  // (256 % LPR == 0: a lane group is wholly inside or outside)
  if (ok) {
    load4(out, (size_t)row * (LPR * 4) + sl * 4, a);
    load4(g_out, (size_t)row * (LPR * 4) + sl * 4, b);
  }
  float g = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  for (int off = 1; off < fl; off <<= 1) g += __shfl_xor(g, off, LPR);
  if (ok && sl % fl == 0) {
    const size_t rh = (size_t)row * H + sl * 4 / F;
    info[rh] = make_float4(er[rh], m[rh], l[rh], g);
  }
}

struct GatPlan {
  int lpr;
  MergePlan m;
  size_t max_bytes, part_a_bytes, part_s_bytes;
};

bool gat_supported(int H, int F) { return H > 0 && F > 0 && F % 4 == 0 && H <= 128 && F <= 128 && has_width(TileWidths{}, H * F); }

GatPlan gat_plan(int64_t n_nodes, int64_t n_edges, int H, int F) {
  GatPlan p;
  p.lpr = H * F / 4;
  p.m = merge_plan(p.lpr, n_edges, n_nodes);
  p.max_bytes = kgat_spmm_max_workspace_bytes(n_edges, H);
  p.part_a_bytes = align_up(p.m.part_elems * sizeof(float4), 256);
  p.part_s_bytes = align_up(p.m.part_elems * sizeof(float), 256);
  return p;
}

size_t gat_workspace_bytes(const GatPlan& p, int64_t n_nodes, int H, bool backward) {
  const size_t parts = p.part_a_bytes + p.part_s_bytes;
  return (backward ? align_up((size_t)n_nodes * H * sizeof(float4), 256) : align_up(p.max_bytes, 256)) + parts + 256;
}

template <int LPR, int MODE>
int launch_walk(const GatK& k, const MergePlan& m, hipStream_t st) {
  constexpr int kThreads = spmm_threads(LPR);
  if (m.tiles > 0) {
    hipLaunchKernelGGL((gat_tile_kernel<LPR, MODE>), dim3((unsigned)m.tiles), dim3(kThreads), 0, st, k);
    KGAT_CHECK_LAUNCH("gat_tile");
  }
  hipLaunchKernelGGL((gat_finish_kernel<LPR, MODE>), dim3((unsigned)(m.fix_blocks + m.nz_blocks)), dim3(kThreads), 0, st, k);
  KGAT_CHECK_LAUNCH("gat_finish");
  return KGAT_OK;
}

// what both entries check alike, before any device work
int check_gat(const char* what, int64_t n_nodes, int64_t n_edges, int H, int F, float slope, float drop_p,
              const int32_t* eid) {
  KGAT_CHECK_ARG(n_nodes >= 0 && n_nodes < INT32_MAX && n_edges >= 0 && n_edges < INT32_MAX,
                 "%s: bad size (n_nodes=%lld n_edges=%lld)", what, (long long)n_nodes, (long long)n_edges);
  KGAT_CHECK_ARG(H > 0 && F > 0, "%s: bad size (H=%d F=%d)", what, H, F);
  if (!gat_supported(H, F)) {
    set_error("%s: (H, F) = (%d, %d) is not covered: H F in {16, 32, 64, 128} with F %% 4 == 0", what, H, F);
    return KGAT_E_UNSUPPORTED;
  }
  KGAT_CHECK_ARG(slope >= 0.f && slope <= 1.f, "%s: negative_slope outside [0, 1] (the row maximum rests on a monotone leaky_relu)", what);
  KGAT_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "%s: dropout probability outside [0, 1)", what);
  KGAT_CHECK_ARG((uint64_t)n_edges * (uint64_t)H < (1ull << 32), "%s: n_edges * H exceeds the hash's 32-bit index", what);
  KGAT_CHECK_ARG(drop_p == 0.f || n_edges == 0 || eid != nullptr, "%s: attention dropout is keyed by edge id: eid is required", what);
  return KGAT_OK;
}

void set_dropout(GatK& k, float drop_p, uint64_t seed) {
  const double t = (double)drop_p * 4294967296.0;
  k.threshold = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
  k.keep_scale = 1.f / (1.f - drop_p);
  k.seed = (uint32_t)(seed ^ (seed >> 32));
}

}  // namespace
}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_gat_supported(int H, int F) { return gat_supported(H, F) ? 1 : 0; }

size_t kgat_gat_workspace_bytes(int64_t n_nodes, int64_t n_edges, int H, int F, int backward) {
  if (n_nodes < 0 || n_edges < 0 || !gat_supported(H, F)) return 256;
  return gat_workspace_bytes(gat_plan(n_nodes, n_edges, H, F), n_nodes, H, backward != 0);
}

int kgat_gat_fwd_f32(int64_t n_nodes, int64_t n_edges, int H, int F, const int32_t* indptr, const int32_t* col,
                     const int32_t* row_of, const int32_t* eid, const float* ft, const float* el, const float* er,
                     float negative_slope, float drop_p, uint64_t seed, float* out, float* m, float* l, void* workspace,
                     size_t workspace_bytes, kgat_stream_t stream) {
  KGAT_RETURN_IF(check_gat("gat_fwd", n_nodes, n_edges, H, F, negative_slope, drop_p, eid));
  if (n_nodes == 0) return KGAT_OK;
  KGAT_CHECK_ARG(indptr && ft && el && er && out && m && l, "gat_fwd: null pointer");
  KGAT_CHECK_ARG(n_edges == 0 || (col && row_of), "gat_fwd: null col/row_of");
  KGAT_CHECK_ARG(aligned16(ft) && aligned16(out) && aligned16(el) && aligned16(m), "gat_fwd: ft, out, el and m must be 16-byte aligned");
  const GatPlan p = gat_plan(n_nodes, n_edges, H, F);
  const size_t need = gat_workspace_bytes(p, n_nodes, H, false);
  KGAT_CHECK_ARG(workspace == nullptr || aligned16(workspace), "gat_fwd: workspace must be 16-byte aligned");
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("gat_fwd: workspace too small (%zu < %zu)", workspace_bytes, need);
    return KGAT_E_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  Carver ws(workspace);
  void* max_ws = ws.take<char>(p.max_bytes);
  GatK k = {};
  k.part_a = ws.take<float4>(p.m.part_elems);
  k.part_s = ws.take<float>(p.m.part_elems);
  // m = leaky_relu(max_u el[u] + er): the exact max reducer on el (copy form, rows of H floats), then one elementwise pass
  KGAT_RETURN_IF(kgat_spmm_umule_max_f32(n_nodes, 0, 0, n_edges, H, indptr, col, row_of, nullptr, el, nullptr, m, nullptr,
                                         max_ws, p.max_bytes, stream));
  const int64_t nh = n_nodes * H;
  hipLaunchKernelGGL(gat_row_max_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, st, nh, m, er, negative_slope);
  KGAT_CHECK_LAUNCH("gat_row_max");
  k.e1 = n_edges; k.te = p.m.tile_edges; k.n_rows = (int32_t)n_nodes; k.n_tiles = (int32_t)p.m.tiles;
  k.fix_blocks = p.m.fix_blocks; k.H = H; k.F = F;
  k.indptr = indptr; k.col = col; k.row_of = row_of; k.eid = eid;
  k.row_s = er; k.row_m = m; k.col_s = el; k.col_x = ft;
  k.slope = negative_slope;
  set_dropout(k, drop_p, seed);
  k.out_rows = out; k.out_head = l;
  return dispatch_width(TileWidths{}, H * F, [&](auto d) { return launch_walk<decltype(d)::value / 4, kFwd>(k, p.m, st); });
}

int kgat_gat_bwd_f32(int64_t n_nodes, int64_t n_edges, int H, int F, const int32_t* indptr, const int32_t* col,
                     const int32_t* row_of, const int32_t* eid, const int32_t* rev_indptr, const int32_t* rev_col,
                     const int32_t* rev_row_of, const int32_t* rev_eid, const float* ft, const float* el, const float* er,
                     const float* m, const float* l, const float* out, const float* g_out, float negative_slope,
                     float drop_p, uint64_t seed, float* g_ft, float* g_el, float* g_er, void* workspace,
                     size_t workspace_bytes, kgat_stream_t stream) {
  KGAT_RETURN_IF(check_gat("gat_bwd", n_nodes, n_edges, H, F, negative_slope, drop_p, eid));
  KGAT_CHECK_ARG(drop_p == 0.f || n_edges == 0 || rev_eid != nullptr, "gat_bwd: attention dropout is keyed by edge id: rev_eid is required");
  if (n_nodes == 0) return KGAT_OK;
  KGAT_CHECK_ARG(indptr && rev_indptr && ft && el && er && m && l && out && g_out && g_ft && g_el && g_er, "gat_bwd: null pointer");
  KGAT_CHECK_ARG(n_edges == 0 || (col && row_of && rev_col && rev_row_of), "gat_bwd: null col/row_of");
  KGAT_CHECK_ARG(aligned16(ft) && aligned16(out) && aligned16(g_out) && aligned16(g_ft), "gat_bwd: ft, out, g_out and g_ft must be 16-byte aligned");
  const GatPlan p = gat_plan(n_nodes, n_edges, H, F);
  const size_t need = gat_workspace_bytes(p, n_nodes, H, true);
  KGAT_CHECK_ARG(workspace == nullptr || aligned16(workspace), "gat_bwd: workspace must be 16-byte aligned");
  if (workspace == nullptr || workspace_bytes < need) {
    set_error("gat_bwd: workspace too small (%zu < %zu)", workspace_bytes, need);
    return KGAT_E_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  Carver ws(workspace);
  float4* info = ws.take<float4>((size_t)n_nodes * H);
  GatK k = {};
  k.part_a = ws.take<float4>(p.m.part_elems);
  k.part_s = ws.take<float>(p.m.part_elems);
  k.e1 = n_edges; k.te = p.m.tile_edges; k.n_rows = (int32_t)n_nodes; k.n_tiles = (int32_t)p.m.tiles;
  k.fix_blocks = p.m.fix_blocks; k.H = H; k.F = F;
  k.info = info;
  k.slope = negative_slope;
  set_dropout(k, drop_p, seed);
  return dispatch_width(TileWidths{}, H * F, [&](auto d) -> int {
    constexpr int LPR = decltype(d)::value / 4;
    const int64_t threads = n_nodes * LPR;
    hipLaunchKernelGGL((gat_prepare_kernel<LPR>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, n_nodes, H, F,
                       er, m, l, out, g_out, info);
    KGAT_CHECK_LAUNCH("gat_prepare");
    GatK a = k;  // rows = destinations: g_er
    a.indptr = indptr; a.col = col; a.row_of = row_of; a.eid = eid;
    a.col_s = el; a.col_x = ft; a.row_x = g_out; a.out_head = g_er;
    KGAT_RETURN_IF((launch_walk<LPR, kBwdDst>(a, p.m, st)));
    GatK b = k;  // rows = sources (reversed CSR): g_ft, g_el; the partials are reused in stream order
    b.indptr = rev_indptr; b.col = rev_col; b.row_of = rev_row_of; b.eid = rev_eid;
    b.row_s = el; b.row_x = ft; b.col_x = g_out; b.out_rows = g_ft; b.out_head = g_el;
    return launch_walk<LPR, kBwdSrc>(b, p.m, st);
  });
}

}  // extern "C"
