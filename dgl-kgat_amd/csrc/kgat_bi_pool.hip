// Bi-Interaction pooling over sparse feature sets for gfx950: the operator of NFM (and, with its d outputs summed, of
// FM), the KGAT paper's "supervised learning" baselines.  A pooled set m is the multiset
//     [extra[m]] (if extra[m] >= 0)  +  ids[indptr[items[m]] : indptr[items[m] + 1]]        (n positions, extra first)
// of rows of one table V (n_nodes x d), and
//     S[m] = sum_f v_f      bi[m] = (S[m]^2 - sum_f v_f^2) / 2 = sum_{f<g} v_f * v_g      lin[m] = sum_f w_lin[f]
//     sq[m] = sum_f |v_f|^2
// In torch operators this is index_select / index_add_ under autograd: float atomics, tensors of (pairs x d).  Here:
//   forward   one wavefront per set, d / 4 lanes per row (16 bytes per lane), G = 256 / d lane groups: position p goes
//             to group p mod G, four positions of a group in flight per look; a group adds its rows in ascending
//             position from 0, the G partials are combined by the butterfly (g with g ^ G/2, then g ^ G/4, ... g ^ 1);
//             nothing of size pairs x d is written
//   sort      (backward) one workgroup each for `items` and `extra`: a stable LDS sort (kgat_lds_sort.h) gives, per
//             item / per extra id, its run of sets in ascending m; the first position of a run goes into a table over
//             the items / the nodes that a memset refilled with -1 just before (no state survives a call)
//   backward  one wavefront per row f of V: the sources of f are its own run as an extra, then the item positions of
//             its reversed list in list order; 64 sources per look are turned into their runs (table, run length), a
//             scan numbers the hits - in source order, within a run in ascending m - and hit h goes to lane group
//             h mod G; a group adds  g_bi[m] * (S[m] - v_f) + 2 g_sq[m] v_f  in ascending h from 0, the butterfly
//             above combines the groups, and the row is written once - zero where nothing hit.  A row with more than
//             256 sources (a feature most items carry) goes to a second launch: 16 wavefronts per row, look k to
//             wavefront k mod 16, each as above with its own hit count, their 16 sums added in wavefront order
// No float atomics, every order fixed: bitwise reproducible.  All arithmetic fp32 on the vector ALU.
// What bounds them: the forward one 16-byte gather per lane and feature row (the bare gather of the batch's rows); the
// backward the walk of every reversed list (4 bytes per pair, a table look-up each) plus two row reads per hit and the
// dense write of grad_V.
#include "kgat_lds_sort.h"

namespace kgat {

constexpr int kBpMaxSets = 8192;   // the sets of a call: what one workgroup sorts in LDS
constexpr int kBpPosBits = 13;     // a position among kBpMaxSets
constexpr int kBpLook = 4;         // rows a lane group requests per look
constexpr int kBpHeavy = 256;      // a row of grad_V with more sources than this is summed by 16 wavefronts
constexpr int kBpHeavyWaves = 16;
using BpWidths = WidthList<16, 32, 64, 128>;

// Everything the backward carves from the caller's scratch: the two tables (item -> first sorted position of its run,
// node -> the same for its run as an extra; refilled with -1 by one memset) | per sort, the sets in sorted order and
// the run length at a run's first position | the heavy rows' counter and list.
struct BpScratch {
  int32_t *item_tab, *extra_tab;
  int32_t *sorted_m[2], *run_len[2];
  int32_t *heavy_count, *heavy_rows;   // the rows with more than kBpHeavy sources: a counter the sort launch zeroes | the list
  int32_t heavy_cap;
  size_t tab_bytes, bytes;
};
static BpScratch bi_pool_scratch(void* base, int64_t n_sets, int64_t n_items, int64_t n_nodes, int64_t n_pairs) {
  const size_t b = (size_t)(n_sets > 0 ? n_sets : 1);
  BpScratch s;
  Carver cv(base);
  s.item_tab = cv.take<int32_t>((size_t)(n_items > 0 ? n_items : 1));
  s.extra_tab = cv.take<int32_t>((size_t)(n_nodes > 0 ? n_nodes : 1));
  s.tab_bytes = cv.off;
  for (int t = 0; t < 2; ++t) {
    s.sorted_m[t] = cv.take<int32_t>(b);
    s.run_len[t] = cv.take<int32_t>(b);
  }
  s.heavy_cap = (int32_t)((n_pairs > 0 ? n_pairs : 0) / kBpHeavy + 1);   // (such a row holds kBpHeavy pairs or more)
  s.heavy_count = cv.take<int32_t>(1);
  s.heavy_rows = cv.take<int32_t>((size_t)s.heavy_cap);
  s.bytes = cv.off;
  return s;
}

__device__ __forceinline__ int32_t bp_clamp(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the butterfly over the lane groups of a wavefront (L lanes each): strides 32, 16, ..., L
template <int L>
__device__ __forceinline__ float groups_sum(float v) {
#pragma unroll
  for (int off = kWave / 2; off >= L; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
template <int L>
__device__ __forceinline__ float4 groups_sum4(const float4& v) {
  return make_float4(groups_sum<L>(v.x), groups_sum<L>(v.y), groups_sum<L>(v.z), groups_sum<L>(v.w));
}

struct BpFwdArgs {
  int32_t n_sets, n_items, n_nodes, n_pairs;
  const float *V, *w_lin;
  const int32_t *indptr, *ids, *items, *extra;
  float *S, *bi, *lin, *sq;
};

// ---- forward: wavefront w of the grid pools set w.  A set with an item position or a feature id outside its table
// reads nothing there and gets NaN outputs (torch would fail a device-side assertion).
template <int D>
__global__ __launch_bounds__(256) void bi_pool_fwd_kernel(BpFwdArgs a) {
  constexpr int L = D / 4, G = kWave / L;
  const int lane = threadIdx.x & (kWave - 1), sl = lane % L, g = lane / L, c = 4 * sl;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= a.n_sets) return;   // (whole wavefronts leave)
  const int32_t j = a.items[m], e = a.extra ? a.extra[m] : -1;
  const int32_t he = e >= 0 ? 1 : 0;
  bool bad = (uint32_t)j >= (uint32_t)a.n_items;
  int32_t beg = 0, end = 0;
  if (!bad) {
    beg = bp_clamp(a.indptr[j], 0, a.n_pairs);
    end = bp_clamp(a.indptr[j + 1], beg, a.n_pairs);
  }
  const int32_t n = he + (end - beg);
  float4 s = zero4(), q = zero4();
  float wl = 0.f;
  for (int32_t p0 = 0; p0 < n; p0 += G * kBpLook) {
    float4 x[kBpLook];
    float w[kBpLook];
#pragma unroll
    for (int u = 0; u < kBpLook; ++u) {
      const int32_t p = p0 + u * G + g;
      x[u] = zero4();
      w[u] = 0.f;
      if (p < n) {
        const int32_t id = p < he ? e : a.ids[beg + (p - he)];
        if ((uint32_t)id < (uint32_t)a.n_nodes) {
          x[u] = *reinterpret_cast<const float4*>(a.V + (size_t)id * D + c);
          if (a.w_lin) w[u] = a.w_lin[id];
        } else {
          bad = true;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kBpLook; ++u) {   // (a position past the end adds +0: no bit changes)
      s = add4(s, x[u]);
      q = make_float4(fmaf(x[u].x, x[u].x, q.x), fmaf(x[u].y, x[u].y, q.y), fmaf(x[u].z, x[u].z, q.z), fmaf(x[u].w, x[u].w, q.w));
      wl += w[u];
    }
  }
  s = groups_sum4<L>(s);
  q = groups_sum4<L>(q);
  wl = groups_sum<L>(wl);
  float sq = (q.x + q.y) + (q.z + q.w);
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) sq += __shfl_xor(sq, off, kWave);
  float4 bi = make_float4(0.5f * fmaf(s.x, s.x, -q.x), 0.5f * fmaf(s.y, s.y, -q.y), 0.5f * fmaf(s.z, s.z, -q.z),
                          0.5f * fmaf(s.w, s.w, -q.w));
  if (__ballot(bad) != 0ull) {
    const float nan = __builtin_nanf("");
    s = bi = make_float4(nan, nan, nan, nan);
    wl = sq = nan;
  }
  if (g == 0) {
    *reinterpret_cast<float4*>(a.S + (size_t)m * D + c) = s;
    *reinterpret_cast<float4*>(a.bi + (size_t)m * D + c) = bi;
  }
  if (lane == 0) {
    if (a.lin) a.lin[m] = wl;
    if (a.sq) a.sq[m] = sq;
  }
}

struct BpSortArgs {
  int32_t n_sets;
  const int32_t* keys[2];   // items, extra (NULL: no extras)
  int32_t n_keys[2];        // n_items, n_nodes
  int key_bits[2];
  int32_t *tab[2], *sorted_m[2], *run_len[2];
  int32_t* heavy_count;
};

// ---- the sorts of the backward: workgroup 0 `items`, workgroup 1 `extra`.  A key outside its table (extra = -1 among
// them) sorts behind every real key and enters no table.
__global__ __launch_bounds__(kLdsSortThreads) void bi_pool_sort_kernel(BpSortArgs a) {
  __shared__ LdsSort<uint64_t, kBpMaxSets, 8, kBpPosBits> s_sort;
  const int job = blockIdx.x, tid = threadIdx.x;
  if (job == 0 && tid == 0) a.heavy_count[0] = 0;
  const int32_t* __restrict__ keys = a.keys[job];
  if (!keys) return;
  const int32_t n = a.n_sets;
  const uint32_t n_keys = (uint32_t)a.n_keys[job];
  for (int32_t i = tid; i < n; i += kLdsSortThreads) {
    const uint32_t k = (uint32_t)keys[i];
    s_sort.buf[0][i] = ((uint64_t)(k < n_keys ? k : n_keys) << kBpPosBits) | (uint64_t)i;
  }
  const uint64_t* s = s_sort.sort(n, a.key_bits[job]);
  for (int32_t q = tid; q < n; q += kLdsSortThreads) {
    const uint64_t key = s[q] >> kBpPosBits;
    a.sorted_m[job][q] = (int32_t)(s[q] & (uint64_t)(kBpMaxSets - 1));
    int32_t len = 0;
    if (key < n_keys && (q == 0 || (s[q - 1] >> kBpPosBits) != key)) {
      int32_t lo = q + 1, hi = n;   // the run's end: the first position behind q with another key
      while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if ((s[mid] >> kBpPosBits) == key) lo = mid + 1; else hi = mid;
      }
      len = lo - q;
      a.tab[job][key] = q;
    }
    a.run_len[job][q] = len;
  }
}

struct BpBwdArgs {
  int32_t n_sets, n_items, n_nodes, n_pairs;
  const float* V;
  const int32_t *rev_indptr, *rev_items;
  const float *g_bi, *g_lin, *g_sq, *S;
  const int32_t *item_tab, *extra_tab;
  const int32_t *sorted_m[2], *run_len[2];   // items, extra
  int32_t *heavy_count, *heavy_rows;         // the rows left to the 16-wavefront kernel
  int32_t heavy_cap;
  float *grad_V, *grad_w;
};

// The sources of row f: source 0 is f as an extra, source s >= 1 entry s - 1 of its reversed list.
struct BpRow {
  int32_t beg, n_src;
};
__device__ __forceinline__ BpRow bp_row(const BpBwdArgs& a, int64_t f) {
  const int32_t beg = bp_clamp(a.rev_indptr[f], 0, a.n_pairs);
  const int32_t end = bp_clamp(a.rev_indptr[f + 1], beg, a.n_pairs);
  return BpRow{beg, 1 + (end - beg)};
}

// One wavefront's share of row f: the looks (64 sources each) first_look, first_look + look_stride, ...  Per look the
// sources become their runs (table, run length), a scan numbers the hits - in source order, within a run in ascending
// m - and continues the wavefront's count; hit h goes to lane group h mod G, which adds its terms in ascending h.
// Leaves the G group partials in acc / accw (groups_sum combines them).
template <int D>
__device__ __forceinline__ void bp_walk(const BpBwdArgs& a, int64_t f, const BpRow row, int first_look, int look_stride,
                                        const float4 v, float4& acc, float& accw) {
  constexpr int L = D / 4, G = kWave / L;
  const int lane = threadIdx.x & (kWave - 1), sl = lane % L, g = lane / L, c = 4 * sl;
  const int32_t beg = row.beg, n_src = row.n_src;
  int base = 0;   // this wavefront's hits so far, mod G
  for (int32_t s0 = first_look * kWave; s0 < n_src; s0 += look_stride * kWave) {
    const int32_t src = s0 + lane;
    int32_t first = -1, which = 0;
    if (src == 0) {
      first = a.extra_tab[f];
      which = 1;
    } else if (src < n_src) {
      const int32_t j = a.rev_items[beg + (src - 1)];
      if ((uint32_t)j < (uint32_t)a.n_items) first = a.item_tab[j];
    }
    int32_t cnt = 0;
    if (first >= 0 && first < a.n_sets) cnt = bp_clamp(a.run_len[which][first], 0, a.n_sets - first);
    if (__ballot(cnt > 0) == 0ull) continue;   // (wave-uniform)
    int32_t inc = cnt;   // the hits of sources 0 .. lane of this look
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int32_t up = __shfl_up(inc, o, kWave);
      if (lane >= o) inc += up;
    }
    const int32_t total = __shfl(inc, kWave - 1, kWave);
    const int32_t exc = inc - cnt;
    for (int32_t wb = 0; wb < total; wb += kWave) {
      // lane t of the window holds hit wb + t: the set at its place in the run of the source that owns it (the first
      // lane whose inclusive count exceeds the hit's number)
      const int32_t h = wb + lane;
      int lo = 0;
#pragma unroll
      for (int step = kWave / 2; step > 0; step >>= 1) {
        const int32_t probe = __shfl(inc, lo + step - 1, kWave);
        if (probe <= h) lo += step;
      }
      const int owner = lo & (kWave - 1);
      const int32_t o_first = __shfl(first, owner, kWave), o_exc = __shfl(exc, owner, kWave);
      const int32_t o_which = __shfl(which, owner, kWave);
      int32_t m = 0;
      if (h < total) m = bp_clamp(a.sorted_m[o_which][bp_clamp(o_first + (h - o_exc), 0, a.n_sets - 1)], 0, a.n_sets - 1);
      const int32_t valid = total - wb < kWave ? total - wb : kWave;
      const int rot = (g - base + G) % G;   // group g takes the hits whose number is g mod G
      for (int r0 = 0; r0 * G < valid; r0 += kBpLook) {
        float4 gb[kBpLook], ss[kBpLook];
        float gs[kBpLook], gl[kBpLook];
        bool on[kBpLook];
#pragma unroll
        for (int u = 0; u < kBpLook; ++u) {
          const int t = (r0 + u) * G + rot;
          const int32_t mt = __shfl(m, t & (kWave - 1), kWave);
          on[u] = t < valid;
          gb[u] = ss[u] = zero4();
          gs[u] = gl[u] = 0.f;
          if (on[u]) {
            if (a.g_bi) {
              gb[u] = *reinterpret_cast<const float4*>(a.g_bi + (size_t)mt * D + c);
              ss[u] = *reinterpret_cast<const float4*>(a.S + (size_t)mt * D + c);
            }
            if (a.g_sq) gs[u] = a.g_sq[mt];
            if (a.g_lin) gl[u] = a.g_lin[mt];
          }
        }
#pragma unroll
        for (int u = 0; u < kBpLook; ++u) {
          if (on[u]) {
            const float k2 = 2.f * gs[u];
            acc.x += fmaf(gb[u].x, ss[u].x - v.x, k2 * v.x);
            acc.y += fmaf(gb[u].y, ss[u].y - v.y, k2 * v.y);
            acc.z += fmaf(gb[u].z, ss[u].z - v.z, k2 * v.z);
            acc.w += fmaf(gb[u].w, ss[u].w - v.w, k2 * v.w);
            accw += gl[u];
          }
        }
      }
      base = (base + valid) % G;
    }
  }
}

// ---- backward, rows of at most kBpHeavy sources: wavefront w of the grid forms row w of grad_V and grad_w[w]; a row
// with more sources is appended to the heavy list (an integer counter: the list's order does not reach any sum).
template <int D>
__global__ __launch_bounds__(256) void bi_pool_bwd_kernel(BpBwdArgs a) {
  constexpr int L = D / 4, G = kWave / L;
  const int lane = threadIdx.x & (kWave - 1), sl = lane % L, g = lane / L, c = 4 * sl;
  const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= a.n_nodes) return;   // (whole wavefronts leave)
  const BpRow row = bp_row(a, f);
  if (row.n_src > kBpHeavy) {
    if (lane == 0) {
      const int32_t slot = atomicAdd(a.heavy_count, 1);
      if (slot < a.heavy_cap) a.heavy_rows[slot] = (int32_t)f;
    }
    return;
  }
  const float4 v = *reinterpret_cast<const float4*>(a.V + (size_t)f * D + c);
  float4 acc = zero4();
  float accw = 0.f;
  bp_walk<D>(a, f, row, 0, 1, v, acc, accw);
  acc = groups_sum4<L>(acc);
  accw = groups_sum<L>(accw);
  if (g == 0) *reinterpret_cast<float4*>(a.grad_V + (size_t)f * D + c) = acc;
  if (lane == 0 && a.grad_w) a.grad_w[f] = accw;
}

// ---- backward, the heavy rows: a workgroup of 16 wavefronts per row, look k to wavefront k mod 16; the 16 wavefront
// sums are added in wavefront order from 0.
template <int D>
__global__ __launch_bounds__(kBpHeavyWaves * kWave) void bi_pool_bwd_heavy_kernel(BpBwdArgs a) {
  constexpr int L = D / 4, G = kWave / L;
  __shared__ float4 s_acc[kBpHeavyWaves][L];
  __shared__ float s_w[kBpHeavyWaves];
  const int lane = threadIdx.x & (kWave - 1), sl = lane % L, g = lane / L, c = 4 * sl, w = threadIdx.x >> 6;
  const int32_t count = bp_clamp(a.heavy_count[0], 0, a.heavy_cap);
  for (int32_t i = blockIdx.x; i < count; i += gridDim.x) {
    const int64_t f = a.heavy_rows[i];
    if ((uint64_t)f >= (uint64_t)a.n_nodes) continue;   // (block-uniform)
    const float4 v = *reinterpret_cast<const float4*>(a.V + (size_t)f * D + c);
    float4 acc = zero4();
    float accw = 0.f;
    bp_walk<D>(a, f, bp_row(a, f), w, kBpHeavyWaves, v, acc, accw);
    acc = groups_sum4<L>(acc);
    accw = groups_sum<L>(accw);
    if (g == 0) s_acc[w][sl] = acc;
    if (lane == 0) s_w[w] = accw;
    __syncthreads();
    if (w == 0 && g == 0) {
      float4 t = s_acc[0][sl];
      for (int q = 1; q < kBpHeavyWaves; ++q) t = add4(t, s_acc[q][sl]);
      *reinterpret_cast<float4*>(a.grad_V + (size_t)f * D + c) = t;
    }
    if (threadIdx.x == 0 && a.grad_w) {
      float t = s_w[0];
      for (int q = 1; q < kBpHeavyWaves; ++q) t += s_w[q];
      a.grad_w[f] = t;
    }
    __syncthreads();
  }
}

// the checks both entries share
static int bi_pool_check(const char* who, int64_t n_sets, int d, int64_t n_nodes, int64_t n_items, int64_t n_pairs) {
  KGAT_CHECK_ARG(n_sets >= 0 && n_nodes > 0 && n_nodes < INT32_MAX && n_items > 0 && n_items < INT32_MAX && n_pairs >= 0 &&
                 n_pairs < INT32_MAX, "%s: needs n_sets >= 0, 1 <= n_nodes, n_items < 2^31, 0 <= n_pairs < 2^31 (n_sets=%lld "
                 "n_nodes=%lld n_items=%lld n_pairs=%lld)", who, (long long)n_sets, (long long)n_nodes, (long long)n_items,
                 (long long)n_pairs);
  if (!kgat_bi_pool_supported(d, n_sets)) {
    set_error("%s: needs d in {16, 32, 64, 128} and 1 <= n_sets <= %d (d=%d n_sets=%lld)", who, kBpMaxSets, d, (long long)n_sets);
    return KGAT_E_UNSUPPORTED;
  }
  return KGAT_OK;
}

}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_bi_pool_supported(int d, int64_t n_sets) { return has_width(BpWidths{}, d) && n_sets >= 1 && n_sets <= kBpMaxSets; }

size_t kgat_bi_pool_scratch_bytes(int64_t n_sets, int64_t n_items, int64_t n_nodes, int64_t n_pairs) {
  return bi_pool_scratch(nullptr, n_sets, n_items, n_nodes, n_pairs).bytes;
}

int kgat_bi_pool_fwd_f32(int64_t n_sets, int d, int64_t n_nodes, int64_t n_items, int64_t n_pairs, const float* V,
                         const float* w_lin, const int32_t* indptr, const int32_t* ids, const int32_t* items,
                         const int32_t* extra, float* S, float* bi, float* lin, float* sq, kgat_stream_t stream) {
  KGAT_RETURN_IF(bi_pool_check("bi_pool_fwd", n_sets, d, n_nodes, n_items, n_pairs));
  KGAT_CHECK_ARG(V && indptr && ids && items && S && bi, "bi_pool_fwd: null pointer");
  KGAT_CHECK_ARG(aligned16(V) && aligned16(S) && aligned16(bi), "bi_pool_fwd: V, S and bi must be 16-byte aligned");
  BpFwdArgs a;
  a.n_sets = (int32_t)n_sets; a.n_items = (int32_t)n_items; a.n_nodes = (int32_t)n_nodes; a.n_pairs = (int32_t)n_pairs;
  a.V = V; a.w_lin = w_lin; a.indptr = indptr; a.ids = ids; a.items = items; a.extra = extra;
  a.S = S; a.bi = bi; a.lin = lin; a.sq = sq;
  const unsigned blocks = (unsigned)((n_sets + 3) / 4);
  hipStream_t st = as_stream(stream);
  return dispatch_width(BpWidths{}, d, [&](auto w) -> int {
    hipLaunchKernelGGL(bi_pool_fwd_kernel<decltype(w)::value>, dim3(blocks), dim3(256), 0, st, a);
    KGAT_CHECK_LAUNCH("bi_pool_fwd");
    return (int)KGAT_OK;
  });
}

int kgat_bi_pool_bwd_f32(int64_t n_sets, int d, int64_t n_nodes, int64_t n_items, int64_t n_pairs, const float* V,
                         const int32_t* rev_indptr, const int32_t* rev_items, const int32_t* items, const int32_t* extra,
                         const float* g_bi, const float* g_lin, const float* g_sq, const float* S, float* grad_V,
                         float* grad_w, void* scratch, size_t scratch_bytes, kgat_stream_t stream) {
  KGAT_RETURN_IF(bi_pool_check("bi_pool_bwd", n_sets, d, n_nodes, n_items, n_pairs));
  KGAT_CHECK_ARG(V && rev_indptr && rev_items && items && S && grad_V && scratch, "bi_pool_bwd: null pointer");
  KGAT_CHECK_ARG(aligned16(V) && aligned16(S) && aligned16(grad_V) && aligned16(g_bi) && aligned16(scratch),
                 "bi_pool_bwd: V, S, g_bi, grad_V and the scratch must be 16-byte aligned");
  const BpScratch w = bi_pool_scratch(scratch, n_sets, n_items, n_nodes, n_pairs);
  if (scratch_bytes < w.bytes) {
    set_error("bi_pool_bwd: scratch too small (%zu < %zu)", scratch_bytes, w.bytes);
    return KGAT_E_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(w.item_tab, 0xFF, w.tab_bytes, st) != hipSuccess) {
    set_error("bi_pool_bwd: memset failed");
    return KGAT_E_HIP;
  }
  BpSortArgs sa;
  sa.n_sets = (int32_t)n_sets;
  sa.keys[0] = items; sa.keys[1] = extra;
  sa.n_keys[0] = (int32_t)n_items; sa.n_keys[1] = (int32_t)n_nodes;
  sa.key_bits[0] = bits_for(n_items); sa.key_bits[1] = bits_for(n_nodes);
  sa.tab[0] = w.item_tab; sa.tab[1] = w.extra_tab;
  for (int t = 0; t < 2; ++t) { sa.sorted_m[t] = w.sorted_m[t]; sa.run_len[t] = w.run_len[t]; }
  sa.heavy_count = w.heavy_count;
  hipLaunchKernelGGL(bi_pool_sort_kernel, dim3(2), dim3(kLdsSortThreads), 0, st, sa);
  KGAT_CHECK_LAUNCH("bi_pool_bwd (sort)");
  BpBwdArgs a;
  a.n_sets = (int32_t)n_sets; a.n_items = (int32_t)n_items; a.n_nodes = (int32_t)n_nodes; a.n_pairs = (int32_t)n_pairs;
  a.V = V; a.rev_indptr = rev_indptr; a.rev_items = rev_items;
  a.g_bi = g_bi; a.g_lin = g_lin; a.g_sq = g_sq; a.S = S;
  a.item_tab = w.item_tab; a.extra_tab = w.extra_tab;
  for (int t = 0; t < 2; ++t) { a.sorted_m[t] = w.sorted_m[t]; a.run_len[t] = w.run_len[t]; }
  a.heavy_count = w.heavy_count; a.heavy_rows = w.heavy_rows; a.heavy_cap = w.heavy_cap;
  a.grad_V = grad_V; a.grad_w = grad_w;
  const unsigned blocks = (unsigned)((n_nodes + 3) / 4);
  // (the heavy rows' count stays on the device: a fixed grid strides over the list)
  const unsigned heavy_blocks = (unsigned)(w.heavy_cap < 1024 ? w.heavy_cap : 1024);
  return dispatch_width(BpWidths{}, d, [&](auto wd) -> int {
    hipLaunchKernelGGL(bi_pool_bwd_kernel<decltype(wd)::value>, dim3(blocks), dim3(256), 0, st, a);
    KGAT_CHECK_LAUNCH("bi_pool_bwd");
    hipLaunchKernelGGL(bi_pool_bwd_heavy_kernel<decltype(wd)::value>, dim3(heavy_blocks), dim3(kBpHeavyWaves * kWave), 0, st, a);
    KGAT_CHECK_LAUNCH("bi_pool_bwd (heavy rows)");
    return (int)KGAT_OK;
  });
}

}  // extern "C"
