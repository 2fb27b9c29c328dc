// Basis-decomposed relational graph convolution (DGL 0.4.x RelGraphConv, regularizer "basis") for gfx950: the sparse
// part, aggregate-first.  DESIGN section 24.
//
//   Z[v, b, :]  = sum_{e: u->v} (norm[e] a[etype[e], b]) x[u, :]                     (N, B, D)   forward
//   g_x[u, :]   = sum_{u->e}    sum_b (norm[e] a[etype[e], b]) g_Z[dst e, b, :]      (N, D)      backward towards x
//   g_a[r, b]   = sum_{e: etype[e] = r} norm[e] <x[src e, :], g_Z[dst e, b, :]>      (R, B)      backward towards a
//
// The dense part, h = Z.view(N, B D) @ weight.view(B D, out), is a library GEMM of the caller.  A source row is
// gathered once per edge and feeds B accumulators; nothing of size E x D or E x B exists.
//
// Decomposition: the one kgat_tile_reduce.h describes, whose finish launch FWD and BWD_X share.  LPR = D / 4 lanes cover
// a row of D floats with one 16-byte access each; the accumulator sets go through the same LDS entries one set at a
// time.  Every sum is added in run order, then tile order: no atomics, bitwise reproducible.
//
// Kernels are built for BP in {1, 2, 4, 8} accumulator sets; a call with B bases runs the next BP >= B with the
// coefficient columns B .. BP - 1 zero in LDS.  The padding costs vector FMAs (B = 3: one set in four, B = 5: three in
// eight) and their registers, no memory traffic: padded sets are neither loaded nor stored.
//
//   FWD    rows = destinations, forward CSR:   acc[b] += (norm a[t, b]) x[u]              -> Z
//   BWD_X  rows = sources, reversed CSR:       acc    += (norm a[t, b]) g_Z[v, b]  over b -> g_x
//   COEF   rows = destinations, forward CSR:   the row's B x D block of g_Z resident, x[u] gathered, B lane-group dot
//          products per edge added into a per-wavefront R x B table in LDS in edge order; the wavefronts' tables are
//          added in wavefront order into one partial per workgroup, the partials by a fixed chunked chain.
// An edge whose type is outside [0, R) contributes nothing in any of the three.
#include "kgat_tile_reduce.h"

namespace kgat {
namespace {

enum { kFwd = 0, kBwdX = 1, kCoef = 2 };

constexpr int kRgcnMaxBases = 8;
constexpr int kRgcnMaxTable = 4096;      // R * B: a wavefront's table, 16 KB; four wavefronts' fill the 64 KB of a launch
constexpr int kCoefMaxGroups = 2048;     // workgroups of the COEF walk: each takes a contiguous range of tiles
constexpr int kCoefChunk = 64;           // partial tables added per workgroup of the chain's first level
using BasisSets = WidthList<1, 2, 4, 8>;

struct RgcnK {
  int64_t e1;
  int32_t te, n_rows, n_tiles, fix_blocks;
  int B, R;
  int nb;                 // D-wide blocks per output row: FWD B, BWD_X 1
  const int32_t *indptr, *col, *row_of, *etype;
  const float* norm;      // may be null: 1
  const float* a;         // R x B
  const float4* col_x;    // rows gathered per edge: FWD / COEF x (LPR float4), BWD_X g_Z (B LPR float4)
  const float4* row_x;    // COEF: g_Z on the row side
  float4* out;            // FWD Z, BWD_X g_x
  float4* part;           // scratch: per (tile, slot, block, lane)
  float* tab_part;        // COEF: per workgroup an R x B table
  int32_t tiles_per_group;
};

// FWD and BWD_X: NACC accumulator sets per lane (FWD: BP, BWD_X: 1).
template <int LPR, int BP, int MODE>
__global__ __launch_bounds__(spmm_threads(LPR)) void rgcn_tile_kernel(const RgcnK k) {
  constexpr int THREADS = spmm_threads(LPR), NSUB = THREADS / LPR;
  constexpr int NACC = MODE == kFwd ? BP : 1;
  constexpr int U = MODE == kFwd ? 4 : (BP >= 4 ? 1 : 4 / BP);  // edges in flight per lane group
  extern __shared__ float s_a[];  // R x BP, columns B .. BP - 1 zero
  __shared__ float4 s_part[NSUB][2][LPR];
  __shared__ int32_t s_row[NSUB][2];

  const int tid = threadIdx.x;
  const int sub = tid / LPR, sl = tid % LPR;
  const int B = k.B, R = k.R, nb = k.nb;
  for (int i = tid; i < R * BP; i += THREADS) {
    const int r = i / BP, b = i % BP;
    s_a[i] = b < B ? k.a[r * B + b] : 0.f;
  }
  __syncthreads();

  const int C = k.te / NSUB;  // edges per run
  const int64_t tile0 = (int64_t)blockIdx.x * k.te;
  const int64_t tile1 = (tile0 + k.te < k.e1) ? tile0 + k.te : k.e1;
  const int64_t p0 = tile0 + (int64_t)sub * C;
  const int64_t p1 = (p0 + C < tile1) ? p0 + C : tile1;

  int32_t cur_row = -1, head_row = -1;
  bool head_done = false;
  float4 acc[NACC], head[NACC];
#pragma unroll
  for (int b = 0; b < NACC; ++b) acc[b] = head[b] = zero4();

  auto flush = [&]() {  // the open row ends here: the run's first row is a partial, later ones are complete
    if (!head_done) {
#pragma unroll
      for (int b = 0; b < NACC; ++b) head[b] = acc[b];
      head_row = cur_row;
      head_done = true;
    } else {
#pragma unroll
      for (int b = 0; b < NACC; ++b)
        if (b < nb) k.out[((size_t)cur_row * nb + b) * LPR + sl] = acc[b];
    }
#pragma unroll
    for (int b = 0; b < NACC; ++b) acc[b] = zero4();
  };

  for (int64_t base = p0; base < p1; base += LPR) {
    const int64_t my = base + sl;
    const bool valid = my < p1;
    const int32_t c = valid ? k.col[my] : 0;
    const int32_t r = valid ? k.row_of[my] : -1;
    const int32_t t = valid ? k.etype[my] : -1;
    const float nm = valid ? (k.norm ? k.norm[my] : 1.f) : 0.f;
    const int n = (p1 - base < LPR) ? (int)(p1 - base) : LPR;
    for (int j = 0; j < n; j += U) {
      int32_t cj[U], rj[U], tj[U];
      float nj[U];
      float4 x[U][MODE == kFwd ? 1 : BP];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        cj[i] = __shfl(c, j + i, LPR);
        rj[i] = __shfl(r, j + i, LPR);
        tj[i] = __shfl(t, j + i, LPR);
        nj[i] = __shfl(nm, j + i, LPR);
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {  // positions past the run: node 0, never consumed
        if constexpr (MODE == kFwd) {
          x[i][0] = k.col_x[(size_t)cj[i] * LPR + sl];
        } else {
#pragma unroll
          for (int b = 0; b < BP; ++b) x[i][b] = b < B ? k.col_x[((size_t)cj[i] * B + b) * LPR + sl] : zero4();
        }
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        if (j + i < n) {
          if (rj[i] != cur_row) {
            if (cur_row >= 0) flush();
            cur_row = rj[i];
          }
          const bool ok = (uint32_t)tj[i] < (uint32_t)R;
          const float* ar = s_a + (ok ? tj[i] : 0) * BP;
          const float scale = ok ? nj[i] : 0.f;
#pragma unroll
          for (int b = 0; b < BP; ++b) {
            const float cb = scale * ar[b];
            if constexpr (MODE == kFwd) acc[b] = fma4(cb, x[i][0], acc[b]);
            else acc[0] = fma4(cb, x[i][b], acc[0]);
          }
        }
      }
    }
  }
  // the run's last open row: head slot if the run never changed row, else tail slot
  if (!head_done) {
#pragma unroll
    for (int b = 0; b < NACC; ++b) {
      head[b] = acc[b];
      acc[b] = zero4();
    }
    head_row = cur_row;  // -1 for an empty run
    cur_row = -1;
  }
  if (sl == 0) {
    s_row[sub][0] = head_row;
    s_row[sub][1] = cur_row;
  }
  __syncthreads();

  // Combine of the run-boundary partials, one accumulator set at a time through the same 2 NSUB entries of LDS: they
  // are in run order and the entries of one row are consecutive.  Lane group s looks at its own two; an entry that
  // starts a row segment (the previous valid entry belongs to another row) adds the rest of the segment in order.
  const int32_t first_row = s_row[0][0];
  const int32_t last_row = k.row_of[tile1 - 1];
  bool starts[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int32_t rr = s_row[sub][t];
    starts[t] = rr >= 0;
    if (rr >= 0 && t == 0 && sub > 0) {  // (a tail entry always starts a segment: the run changed row)
      const int32_t pt = s_row[sub - 1][1];
      if ((pt >= 0 ? pt : s_row[sub - 1][0]) == rr) starts[t] = false;
    }
  }
#pragma unroll
  for (int b = 0; b < NACC; ++b) {
    if (b < nb) {  // (uniform over the launch)
      if (b > 0) __syncthreads();
      s_part[sub][0][sl] = head[b];
      s_part[sub][1][sl] = acc[b];
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (!starts[t]) continue;
        const int32_t rr = s_row[sub][t];
        float4 v = zero4();
        for (int q = 2 * sub + t; q < 2 * NSUB; ++q) {
          const int32_t r2 = s_row[q >> 1][q & 1];
          if (r2 < 0) continue;
          if (r2 != rr) break;
          v = add4(v, s_part[q >> 1][q & 1][sl]);
        }
        if (rr == first_row) k.part[(((size_t)blockIdx.x * 2 + 0) * nb + b) * LPR + sl] = v;
        else if (rr == last_row) k.part[(((size_t)blockIdx.x * 2 + 1) * nb + b) * LPR + sl] = v;
        else k.out[((size_t)rr * nb + b) * LPR + sl] = v;
      }
    }
  }
}

// The finish launch's lane (kgat_tile_reduce.h): NACC accumulator sets of one float4, of which the first nb exist in
// this launch; the scratch holds them per (tile, slot, block, lane).  A row without edges gets zeros.
template <int LPR, int NACC>
struct RgcnLane {
  const RgcnK& k;
  int sl, nb;
  float4 acc[NACC];

  __device__ __forceinline__ RgcnLane(int sl_, const RgcnK& k_) : k(k_), sl(sl_), nb(k_.nb) {}

  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int b = 0; b < NACC; ++b) acc[b] = zero4();
  }
  __device__ __forceinline__ void add_part(int64_t tile, int slot) {
#pragma unroll
    for (int b = 0; b < NACC; ++b)
      if (b < nb) acc[b] = add4(acc[b], k.part[(((size_t)tile * 2 + slot) * nb + b) * LPR + sl]);
  }
  __device__ __forceinline__ void emit(size_t row) const {
#pragma unroll
    for (int b = 0; b < NACC; ++b)
      if (b < nb) k.out[(row * nb + b) * LPR + sl] = acc[b];
  }
  __device__ __forceinline__ void emit_no_edges(size_t row) {
    reset();
    emit(row);
  }
  __device__ __forceinline__ void fold(int off) {
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
      float4 o;
      o.x = __shfl_xor(acc[i].x, off, kWave);
      o.y = __shfl_xor(acc[i].y, off, kWave);
      o.z = __shfl_xor(acc[i].z, off, kWave);
      o.w = __shfl_xor(acc[i].w, off, kWave);
      acc[i] = add4(acc[i], o);
    }
  }
};

template <int LPR, int NACC>
__global__ __launch_bounds__(spmm_threads(LPR)) void rgcn_finish_kernel(const RgcnK k) {
  tile_finish<LPR, RgcnLane<LPR, NACC>, const RgcnK&>(0, k.e1, k.te, 0, k.n_rows, k.n_tiles, k.fix_blocks, k.indptr,
                                                     k.row_of, k);
}

// COEF: every loop bound below is uniform over the wavefront (a run shorter than C has invalid positions instead of
// fewer steps), so the shuffles always see all 64 lanes.  Table entry (r, b) of a wavefront is only ever touched by one
// lane of it - lane b % NL - and that lane takes the wavefront's lane groups in turn: the additions are in that one
// thread's program order, lane group 0's edge first.
template <int LPR, int BP>
__global__ __launch_bounds__(spmm_threads(LPR)) void rgcn_coef_kernel(const RgcnK k) {
  constexpr int THREADS = spmm_threads(LPR), NSUB = THREADS / LPR;
  constexpr int SPW = kWave / LPR, WAVES = THREADS / kWave;
  constexpr int U = 4;
  constexpr int NL = BP < LPR ? BP : LPR;  // lanes of a wavefront that own table columns
  constexpr int ROUNDS = BP / NL;
  extern __shared__ float s_tab[];  // WAVES x R x B

  const int tid = threadIdx.x;
  const int sub = tid / LPR, sl = tid % LPR;
  const int wave = tid / kWave, lane_id = tid % kWave;
  const int B = k.B, R = k.R, RB = R * B;
  for (int i = tid; i < WAVES * RB; i += THREADS) s_tab[i] = 0.f;
  __syncthreads();
  float* const tab = s_tab + wave * RB;

  const int C = k.te / NSUB;
  const int64_t t_first = (int64_t)blockIdx.x * k.tiles_per_group;
  int64_t t_last = t_first + k.tiles_per_group;
  if (t_last > k.n_tiles) t_last = k.n_tiles;
  for (int64_t tile = t_first; tile < t_last; ++tile) {
    const int64_t tile0 = tile * k.te;
    const int64_t tile1 = (tile0 + k.te < k.e1) ? tile0 + k.te : k.e1;
    const int64_t p0 = tile0 + (int64_t)sub * C;
    const int64_t p1 = (p0 + C < tile1) ? p0 + C : tile1;
    int32_t cur_row = -1;
    float4 g[BP];
#pragma unroll
    for (int b = 0; b < BP; ++b) g[b] = zero4();
    for (int base = 0; base < C; base += LPR) {
      const int64_t my = p0 + base + sl;
      const bool valid = base + sl < C && my < p1;
      const int32_t c = valid ? k.col[my] : 0;
      const int32_t r = valid ? k.row_of[my] : -1;
      int32_t t = valid ? k.etype[my] : -1;
      if ((uint32_t)t >= (uint32_t)R) t = -1;
      const float nm = valid ? (k.norm ? k.norm[my] : 1.f) : 0.f;
      const int n = C - base < LPR ? C - base : LPR;  // a multiple of U: the run lengths are powers of two >= 8
      for (int j = 0; j < n; j += U) {
        int32_t cj[U], rj[U], tj[U];
        float nj[U];
        float4 x[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
          cj[i] = __shfl(c, j + i, LPR);
          rj[i] = __shfl(r, j + i, LPR);
          tj[i] = __shfl(t, j + i, LPR);
          nj[i] = __shfl(nm, j + i, LPR);
        }
#pragma unroll
        for (int i = 0; i < U; ++i) x[i] = k.col_x[(size_t)cj[i] * LPR + sl];  // invalid positions: node 0, unused
#pragma unroll
        for (int i = 0; i < U; ++i) {
          if (rj[i] >= 0 && rj[i] != cur_row) {  // the destination's gradient block stays in registers over its edges
            cur_row = rj[i];
#pragma unroll
            for (int b = 0; b < BP; ++b)
              if (b < B) g[b] = k.row_x[((size_t)cur_row * B + b) * LPR + sl];
          }
          float d[BP];
#pragma unroll
          for (int b = 0; b < BP; ++b) {
            float v = x[i].x * g[b].x;
            v = fmaf(x[i].y, g[b].y, v);
            v = fmaf(x[i].z, g[b].z, v);
            v = fmaf(x[i].w, g[b].w, v);
#pragma unroll
            for (int off = 1; off < LPR; off <<= 1) v += __shfl_xor(v, off, LPR);
            d[b] = nj[i] * v;
          }
          const int32_t te_ = (rj[i] >= 0) ? tj[i] : -1;
#pragma unroll
          for (int rd = 0; rd < ROUNDS; ++rd) {
            float w = d[rd * NL];
#pragma unroll
            for (int b = 1; b < NL; ++b)
              if ((sl & (NL - 1)) == b) w = d[rd * NL + b];
            const int col_b = rd * NL + (lane_id & (NL - 1));
#pragma unroll
            for (int qq = 0; qq < SPW; ++qq) {
              const int32_t tq = __shfl(te_, qq * LPR, kWave);
              const float wq = __shfl(w, qq * LPR + (lane_id & (NL - 1)), kWave);
              if (lane_id < NL && col_b < B && tq >= 0) tab[tq * B + col_b] += wq;
            }
          }
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < RB; i += THREADS) {
    float v = s_tab[i];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v += s_tab[w * RB + i];
    k.tab_part[(size_t)blockIdx.x * RB + i] = v;
  }
}

// out[j] = in[j chunk] + in[j chunk + 1] + ... (at most `chunk` tables of `rb` floats, in order); no table: zeros
__global__ __launch_bounds__(256) void rgcn_sum_tables_kernel(const float* __restrict__ in, int32_t n_in, int32_t chunk,
                                                             int32_t rb, float* __restrict__ out) {
  const int32_t t0 = (int32_t)blockIdx.x * chunk;
  const int32_t t1 = t0 + chunk < n_in ? t0 + chunk : n_in;
  for (int32_t i = threadIdx.x; i < rb; i += 256) {
    float v = 0.f;
    for (int32_t t = t0; t < t1; ++t) v += in[(size_t)t * rb + i];
    out[(size_t)blockIdx.x * rb + i] = v;
  }
}

bool rgcn_supported(int D, int B, int R) {
  return has_width(TileWidths{}, D) && B >= 1 && B <= kRgcnMaxBases && R >= 1 && (int64_t)R * B <= kRgcnMaxTable;
}

int basis_sets(int B) { return B <= 1 ? 1 : (B <= 2 ? 2 : (B <= 4 ? 4 : 8)); }

struct RgcnPlan {
  MergePlan m;
  int64_t groups, tiles_per_group, level1;  // COEF: workgroups of the walk, tiles of each, tables after the first level
  size_t bytes;
};

RgcnPlan rgcn_plan(int64_t n_nodes, int64_t n_edges, int D, int B, int R, int pass) {
  RgcnPlan p;
  p.m = merge_plan(D / 4, n_edges, n_nodes);
  p.tiles_per_group = (p.m.tiles + kCoefMaxGroups - 1) / kCoefMaxGroups;
  if (p.tiles_per_group < 1) p.tiles_per_group = 1;
  p.groups = (p.m.tiles + p.tiles_per_group - 1) / p.tiles_per_group;
  p.level1 = (p.groups + kCoefChunk - 1) / kCoefChunk;
  if (pass == kCoef) {
    p.bytes = align_up((size_t)p.groups * R * B * sizeof(float), 256) + align_up((size_t)p.level1 * R * B * sizeof(float), 256) + 256;
  } else {
    p.bytes = align_up(p.m.part_elems * (size_t)(pass == kFwd ? B : 1) * sizeof(float4), 256) + 256;
  }
  return p;
}

// what the three entries check alike, before any device work
int check_rgcn(const char* what, int64_t n_nodes, int64_t n_edges, int D, int B, int R) {
  KGAT_CHECK_ARG(n_nodes >= 0 && n_nodes < INT32_MAX && n_edges >= 0 && n_edges < INT32_MAX,
                 "%s: bad size (n_nodes=%lld n_edges=%lld)", what, (long long)n_nodes, (long long)n_edges);
  KGAT_CHECK_ARG(D > 0 && B > 0 && R > 0, "%s: bad size (D=%d B=%d R=%d)", what, D, B, R);
  if (!rgcn_supported(D, B, R)) {
    set_error("%s: (D, B, R) = (%d, %d, %d) is not covered: D in {16, 32, 64, 128}, 1 <= B <= 8, R B <= 4096", what, D, B, R);
    return KGAT_E_UNSUPPORTED;
  }
  KGAT_CHECK_ARG((int64_t)n_nodes * B * (D / 4) < ((int64_t)1 << 40), "%s: n_nodes * B * D too large", what);
  return KGAT_OK;
}

int check_scratch(const char* what, const RgcnPlan& p, const void* scratch, size_t scratch_bytes) {
  KGAT_CHECK_ARG(scratch == nullptr || aligned16(scratch), "%s: scratch must be 16-byte aligned", what);
  if (scratch == nullptr || scratch_bytes < p.bytes) {
    set_error("%s: scratch too small (%zu < %zu)", what, scratch_bytes, p.bytes);
    return KGAT_E_WORKSPACE;
  }
  return KGAT_OK;
}

RgcnK make_args(const RgcnPlan& p, int64_t n_nodes, int64_t n_edges, int B, int R, const int32_t* indptr,
                const int32_t* col, const int32_t* row_of, const int32_t* etype, const float* norm) {
  RgcnK k = {};
  k.e1 = n_edges; k.te = p.m.tile_edges; k.n_rows = (int32_t)n_nodes; k.n_tiles = (int32_t)p.m.tiles;
  k.fix_blocks = p.m.fix_blocks; k.B = B; k.R = R;
  k.indptr = indptr; k.col = col; k.row_of = row_of; k.etype = etype; k.norm = norm;
  k.tiles_per_group = (int32_t)p.tiles_per_group;
  return k;
}

template <int LPR, int BP, int MODE>
int launch_walk(const RgcnK& k, const MergePlan& m, hipStream_t st) {
  constexpr int kThreads = spmm_threads(LPR);
  constexpr int NACC = MODE == kFwd ? BP : 1;
  if (m.tiles > 0) {
    hipLaunchKernelGGL((rgcn_tile_kernel<LPR, BP, MODE>), dim3((unsigned)m.tiles), dim3(kThreads),
                       (size_t)k.R * BP * sizeof(float), st, k);
    KGAT_CHECK_LAUNCH("rgcn_tile");
  }
  hipLaunchKernelGGL((rgcn_finish_kernel<LPR, NACC>), dim3((unsigned)(m.fix_blocks + m.nz_blocks)), dim3(kThreads), 0, st, k);
  KGAT_CHECK_LAUNCH("rgcn_finish");
  return KGAT_OK;
}

template <int MODE>
int dispatch_walk(int D, int B, const RgcnK& k, const MergePlan& m, hipStream_t st) {
  return dispatch_width(TileWidths{}, D, [&](auto d) {
    return dispatch_width(BasisSets{}, basis_sets(B), [&](auto bp) {
      return launch_walk<decltype(d)::value / 4, decltype(bp)::value, MODE>(k, m, st);
    });
  });
}

}  // namespace
}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_rgcn_supported(int D, int B, int R) { return rgcn_supported(D, B, R) ? 1 : 0; }

size_t kgat_rgcn_scratch_bytes(int64_t n_nodes, int64_t n_edges, int D, int B, int R, int pass) {
  if (n_nodes < 0 || n_edges < 0 || pass < kFwd || pass > kCoef || !rgcn_supported(D, B, R)) return 256;
  return rgcn_plan(n_nodes, n_edges, D, B, R, pass).bytes;
}

int kgat_rgcn_fwd_f32(int64_t n_nodes, int64_t n_edges, int D, int B, int R, const int32_t* indptr, const int32_t* col,
                      const int32_t* row_of, const int32_t* etype_csr, const float* norm_csr, const float* x,
                      const float* a, float* Z, void* scratch, size_t scratch_bytes, kgat_stream_t stream) {
  KGAT_RETURN_IF(check_rgcn("rgcn_fwd", n_nodes, n_edges, D, B, R));
  KGAT_CHECK_ARG(indptr && x && a && Z, "rgcn_fwd: null pointer");
  KGAT_CHECK_ARG(n_edges == 0 || (col && row_of && etype_csr), "rgcn_fwd: null col/row_of/etype_csr");
  KGAT_CHECK_ARG(aligned16(x) && aligned16(Z), "rgcn_fwd: x and Z must be 16-byte aligned");
  const RgcnPlan p = rgcn_plan(n_nodes, n_edges, D, B, R, kFwd);
  KGAT_RETURN_IF(check_scratch("rgcn_fwd", p, scratch, scratch_bytes));
  if (n_nodes == 0) return KGAT_OK;
  RgcnK k = make_args(p, n_nodes, n_edges, B, R, indptr, col, row_of, etype_csr, norm_csr);
  k.nb = B; k.a = a;
  k.col_x = reinterpret_cast<const float4*>(x);
  k.out = reinterpret_cast<float4*>(Z);
  k.part = static_cast<float4*>(scratch);
  return dispatch_walk<kFwd>(D, B, k, p.m, as_stream(stream));
}

int kgat_rgcn_bwd_x_f32(int64_t n_nodes, int64_t n_edges, int D, int B, int R, const int32_t* rev_indptr,
                        const int32_t* rev_col, const int32_t* rev_row_of, const int32_t* etype_rev,
                        const float* norm_rev, const float* g_Z, const float* a, float* g_x, void* scratch,
                        size_t scratch_bytes, kgat_stream_t stream) {
  KGAT_RETURN_IF(check_rgcn("rgcn_bwd_x", n_nodes, n_edges, D, B, R));
  KGAT_CHECK_ARG(rev_indptr && g_Z && a && g_x, "rgcn_bwd_x: null pointer");
  KGAT_CHECK_ARG(n_edges == 0 || (rev_col && rev_row_of && etype_rev), "rgcn_bwd_x: null rev_col/rev_row_of/etype_rev");
  KGAT_CHECK_ARG(aligned16(g_Z) && aligned16(g_x), "rgcn_bwd_x: g_Z and g_x must be 16-byte aligned");
  const RgcnPlan p = rgcn_plan(n_nodes, n_edges, D, B, R, kBwdX);
  KGAT_RETURN_IF(check_scratch("rgcn_bwd_x", p, scratch, scratch_bytes));
  if (n_nodes == 0) return KGAT_OK;
  RgcnK k = make_args(p, n_nodes, n_edges, B, R, rev_indptr, rev_col, rev_row_of, etype_rev, norm_rev);
  k.nb = 1; k.a = a;
  k.col_x = reinterpret_cast<const float4*>(g_Z);
  k.out = reinterpret_cast<float4*>(g_x);
  k.part = static_cast<float4*>(scratch);
  return dispatch_walk<kBwdX>(D, B, k, p.m, as_stream(stream));
}

int kgat_rgcn_bwd_coef_f32(int64_t n_nodes, int64_t n_edges, int D, int B, int R, const int32_t* indptr,
                           const int32_t* col, const int32_t* row_of, const int32_t* etype_csr, const float* norm_csr,
                           const float* x, const float* g_Z, float* g_a, void* scratch, size_t scratch_bytes,
                           kgat_stream_t stream) {
  KGAT_RETURN_IF(check_rgcn("rgcn_bwd_coef", n_nodes, n_edges, D, B, R));
  KGAT_CHECK_ARG(indptr && x && g_Z && g_a, "rgcn_bwd_coef: null pointer");
  KGAT_CHECK_ARG(n_edges == 0 || (col && row_of && etype_csr), "rgcn_bwd_coef: null col/row_of/etype_csr");
  KGAT_CHECK_ARG(aligned16(x) && aligned16(g_Z), "rgcn_bwd_coef: x and g_Z must be 16-byte aligned");
  const RgcnPlan p = rgcn_plan(n_nodes, n_edges, D, B, R, kCoef);
  KGAT_RETURN_IF(check_scratch("rgcn_bwd_coef", p, scratch, scratch_bytes));
  hipStream_t st = as_stream(stream);
  const int32_t rb = R * B;
  Carver ws(scratch);
  float* tabs = ws.take<float>((size_t)p.groups * rb);
  float* level1 = ws.take<float>((size_t)p.level1 * rb);
  RgcnK k = make_args(p, n_nodes, n_edges, B, R, indptr, col, row_of, etype_csr, norm_csr);
  k.col_x = reinterpret_cast<const float4*>(x);
  k.row_x = reinterpret_cast<const float4*>(g_Z);
  k.tab_part = tabs;
  if (p.groups > 0) {
    KGAT_RETURN_IF(dispatch_width(TileWidths{}, D, [&](auto d) {
      return dispatch_width(BasisSets{}, basis_sets(B), [&](auto bp) -> int {
        constexpr int LPR = decltype(d)::value / 4;
        constexpr int kThreads = spmm_threads(LPR);
        hipLaunchKernelGGL((rgcn_coef_kernel<LPR, decltype(bp)::value>), dim3((unsigned)p.groups), dim3(kThreads),
                           (size_t)(kThreads / kWave) * rb * sizeof(float), st, k);
        KGAT_CHECK_LAUNCH("rgcn_coef");
        return KGAT_OK;
      });
    }));
  }
  // the workgroups' tables in order: chunks of kCoefChunk, then the chunks' sums (at most 32 of them)
  if (p.level1 > 1) {
    hipLaunchKernelGGL(rgcn_sum_tables_kernel, dim3((unsigned)p.level1), dim3(256), 0, st, tabs, (int32_t)p.groups,
                       kCoefChunk, rb, level1);
    KGAT_CHECK_LAUNCH("rgcn_sum_tables");
    hipLaunchKernelGGL(rgcn_sum_tables_kernel, dim3(1), dim3(256), 0, st, level1, (int32_t)p.level1, (int32_t)p.level1, rb, g_a);
  } else {
    hipLaunchKernelGGL(rgcn_sum_tables_kernel, dim3(1), dim3(256), 0, st, tabs, (int32_t)p.groups, kCoefChunk, rb, g_a);
  }
  KGAT_CHECK_LAUNCH("rgcn_sum_tables");
  return KGAT_OK;
}

}  // extern "C"
