// TransR link prediction for gfx950: the filtered rank of a triple's true tail (or head) among the entities under the
// score of reference models.py:120-126,
//     |u_h + u_r - u_t|^2,   u_x = a_x / max(|a_x|, 1e-12),  a_x = e_x W_r,   u_r = rel_r / max(|rel_r|, 1e-12)
// (the normalisation of the training kernel, kgat_transr.hip lines 4-6).  With q = u_h + u_r (tail side) or
// q = u_t - u_r (head side) and p_i the projected candidate, the distance is |q|^2 + |p_i|^2 - 2 q.p_i: per query
// the order of the candidates is that of  s_i = n2_i - 2 q.p_i,  n2_i = |p_i|^2.
//
// Two kernels, no (entities x k) temporary per query batch and no (queries x entities) score matrix:
//  1. transr_project_kernel: out = normalise(ent[rows] W_r) [+ sign * normalise(rel_r)], n2 = |normalise(..)|^2, on
//     v_mfma_f32_16x16x4_f32 in the operand-swapped form of kgat_sage.hip (a lane ends up with four consecutive
//     columns of one row): one wavefront per 16-row tile, W_r staged once per workgroup in LDS in fragment order
//     (d x k floats: 64 KB at 128 x 128).  ROW-MAJOR output (n_rows x k) - what the sweep below and the top-K sweep
//     of kgat_eval_topk.hip (kg_complete) both read.
//  2. transr_rank_kernel: a wavefront keeps 32 queries as MFMA B fragments in registers (two groups of 16, k / 2
//     values per lane) and streams 16-candidate tiles of a contiguous segment of the candidate range as A fragments
//     (one 16-byte load per lane per four MFMAs, used by both query groups).  The product leaves the QUERY on the
//     lane (four lanes per query, four candidates each), so a lane compares its scores with its query's s_t and counts
//     lt = #{s_i < s_t}, eq = #{s_i == s_t} in two integer registers.  The filter - a sorted id list per query - is
//     walked along with the tiles: a lane keeps the next filter id of its query in a register, and only a tile that
//     holds one builds the 16-bit mask.  s_t comes from the same tile routine (the rows t of the wavefront's 16
//     queries as one tile, the diagonal of the product), so it carries the bits the sweep gives that row, and a
//     candidate whose row is bit-identical to the true answer's counts in eq wherever it lies.  Segments of the same
//     queries run in different workgroups and add their counts with integer atomics into zeroed outputs: integer sums
//     do not depend on order - exact and bitwise reproducible.  No float atomics.
#include "kgat_common.h"

namespace kgat {

typedef float floatx4_r __attribute__((ext_vector_type(4)));

using RankWidths = WidthList<16, 32, 64, 128>;

// ------------------------------------------------------------------------------------------------ projection
// Fragment order of W_r (D x K row-major, the contraction runs over its rows) for the operand-swapped product:
// s_w[(s * KT + c) * 64 + q * 16 + i] = W[16 (s >> 2) + 4q + (s & 3)][16c + i], KT = K / 16, s < D / 4.
template <int D, int K>
__device__ __forceinline__ void stage_project_weight(const float* __restrict__ W, float* s_w) {
  constexpr int KT = K / 16;
  for (int idx = threadIdx.x * 4; idx < D * K; idx += 256 * 4) {
    const float4 v = *reinterpret_cast<const float4*>(W + idx);
    const int k = idx / K, n0 = idx % K;
    const int s = (k >> 4) * 4 + (k & 3), q = (k >> 2) & 3;
    const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = n0 + t;
      s_w[(s * KT + (n >> 4)) * kWave + q * 16 + (n & 15)] = vv[t];
    }
  }
}

template <int D, int K>
__global__ __launch_bounds__(256) void transr_project_kernel(int32_t n_rows, int64_t n_ent, const float* __restrict__ ent,
                                                             const int32_t* __restrict__ ids, int64_t row0,
                                                             const float* __restrict__ W, const float* __restrict__ rel,
                                                             float sign, float* __restrict__ out,
                                                             float* __restrict__ n2) {
  constexpr int KS = D / 4, KT = K / 16;
  __shared__ float s_w[D * K];
  stage_project_weight<D, K>(W, s_w);
  __syncthreads();
  const int lane = threadIdx.x % kWave;
  const int i = lane & 15, q = lane >> 4;
  // sign * rel / max(|rel|, 1e-12) at the lane's output columns 16c + 4q + j (the four q groups hold all K columns)
  float ur[KT][4];
  {
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < KT; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ur[c][j] = rel ? rel[16 * c + 4 * q + j] : 0.f;
        ss = fmaf(ur[c][j], ur[c][j], ss);
      }
    ss += __shfl_xor(ss, 16, kWave);
    ss += __shfl_xor(ss, 32, kWave);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int c = 0; c < KT; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) ur[c][j] = sign * (ur[c][j] / nrm);
  }
  const int64_t n_waves = (int64_t)gridDim.x * (256 / kWave);
  const int64_t wv = (int64_t)blockIdx.x * (256 / kWave) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int32_t n_tiles = (n_rows + 15) >> 4;
  const int32_t t_begin = (int32_t)((int64_t)n_tiles * wv / n_waves);
  const int32_t t_end = (int32_t)((int64_t)n_tiles * (wv + 1) / n_waves);
  for (int32_t t = t_begin; t < t_end; ++t) {
    const int32_t row = (t << 4) + i;
    const int32_t r = row < n_rows ? row : n_rows - 1;
    int64_t e = ids ? (int64_t)ids[r] : row0 + r;
    e = e < 0 ? 0 : (e >= n_ent ? n_ent - 1 : e);     // (the caller checks the ids; a bad one reads a wrong row, never outside)
    float a[KS];
    const float4* pa = reinterpret_cast<const float4*>(ent + (size_t)e * D) + q;
#pragma unroll
    for (int m = 0; m < D / 16; ++m) {
      const float4 v = pa[4 * m];
      a[4 * m + 0] = v.x; a[4 * m + 1] = v.y; a[4 * m + 2] = v.z; a[4 * m + 3] = v.w;
    }
    floatx4_r acc[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) acc[c] = (floatx4_r){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int c = 0; c < KT; ++c)
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w[(s * KT + c) * kWave + lane], a[s], acc[c], 0, 0, 0);
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < KT; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) ss = fmaf(acc[c][j], acc[c][j], ss);
    ss += __shfl_xor(ss, 16, kWave);
    ss += __shfl_xor(ss, 32, kWave);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
    float s2 = 0.f;
#pragma unroll
    for (int c = 0; c < KT; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float u = acc[c][j] / nrm;
        s2 = fmaf(u, u, s2);
        acc[c][j] = u + ur[c][j];
      }
    s2 += __shfl_xor(s2, 16, kWave);
    s2 += __shfl_xor(s2, 32, kWave);
    if (row < n_rows) {
#pragma unroll
      for (int c = 0; c < KT; ++c)
        *reinterpret_cast<float4*>(out + (size_t)row * K + 16 * c + 4 * q) =
            make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
      if (n2 && q == 0) n2[row] = s2;
    }
  }
}

// ------------------------------------------------------------------------------------------------ rank sweep
constexpr int kRankWaves = 4;            // wavefronts per workgroup
constexpr int kRankQ = 32;               // queries per wavefront: two B fragments
constexpr int kRankMinTiles = 8;         // candidate tiles per segment at least
constexpr int kRankMaxSeg = 4096;

// One 16 x 16 tile of q.p for the two query groups: A = the lane's candidate row (KS4 float4 of it), B = the queries.
// The ONLY place a score's dot product is formed - the sweep and s_t both call it, so equal rows give equal bits.
template <int K>
__device__ __forceinline__ void rank_tile(const float4 (&a)[K / 16], const float (&b0)[K / 4], const float (&b1)[K / 4],
                                          floatx4_r& d0, floatx4_r& d1) {
  d0 = (floatx4_r){0.f, 0.f, 0.f, 0.f};
  d1 = (floatx4_r){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < K / 16; ++m) {
    const float av[4] = {a[m].x, a[m].y, a[m].z, a[m].w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], b0[4 * m + u], d0, 0, 0, 0);
      d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], b1[4 * m + u], d1, 0, 0, 0);
    }
  }
}

__device__ __forceinline__ float rank_score(float n2, float dot) { return fmaf(-2.f, dot, n2); }

template <int K>
__device__ __forceinline__ void rank_load_rows(const float* __restrict__ M, int64_t row, int q, float4 (&a)[K / 16]) {
  const float4* p = reinterpret_cast<const float4*>(M + (size_t)row * K) + q;
#pragma unroll
  for (int m = 0; m < K / 16; ++m) a[m] = p[4 * m];
}

// an entity id as a position in the candidate range, formed in 64 bits (any int32 id, c0 >= 0: no overflow); every id
// below the range becomes -1
__device__ __forceinline__ int32_t rank_position(int32_t id, int32_t c0) {
  const int64_t v = (int64_t)id - c0;
  return v < 0 ? -1 : (int32_t)v;
}

// first position in the ascending list f[lo, hi) whose id is >= v
__device__ __forceinline__ int32_t rank_lower_bound(const int32_t* __restrict__ f, int32_t lo, int32_t hi, int32_t v) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (f[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <int K>
__global__ __launch_bounds__(kRankWaves * 64) void transr_rank_kernel(
    int32_t n_q, int32_t n_c, int32_t c0, int32_t tiles_per_seg, const float* __restrict__ Q,
    const int32_t* __restrict__ t_ids, const float* __restrict__ P, const float* __restrict__ n2,
    const int32_t* __restrict__ f_ptr, const int32_t* __restrict__ f_ids, int32_t n_f, int32_t* __restrict__ lt_out,
    int32_t* __restrict__ eq_out) {
  constexpr int KS = K / 4;
  const int lane = threadIdx.x % kWave;
  const int i = lane & 15, qd = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int32_t q_base = ((int32_t)blockIdx.x * kRankWaves + w) * kRankQ;
  if (q_base >= n_q) return;
  const int32_t n_tiles = (n_c + 15) >> 4;
  const int32_t tile_lo = (int32_t)blockIdx.y * tiles_per_seg;
  const int32_t tile_hi = tile_lo + tiles_per_seg < n_tiles ? tile_lo + tiles_per_seg : n_tiles;
  if (tile_lo >= tile_hi) return;

  // the lane's two queries (groups 0 and 1): B fragments, true answers, filter cursors
  float b[2][KS];
  int32_t qi[2], tc[2], fp[2], fe[2], fn[2];
  bool live[2];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const int32_t qq = q_base + 16 * g + i;
    live[g] = qq < n_q;
    qi[g] = live[g] ? qq : n_q - 1;
    float4 r[K / 16];
    rank_load_rows<K>(Q, qi[g], qd, r);
#pragma unroll
    for (int m = 0; m < K / 16; ++m) { b[g][4 * m + 0] = r[m].x; b[g][4 * m + 1] = r[m].y; b[g][4 * m + 2] = r[m].z; b[g][4 * m + 3] = r[m].w; }
    const int32_t t = rank_position(t_ids[qi[g]], c0);   // the true answer as a candidate position
    tc[g] = t < 0 ? 0 : (t >= n_c ? n_c - 1 : t);       // (checked by the caller; clamped: never outside)
    int32_t lo = f_ptr[qi[g]], hi = f_ptr[qi[g] + 1];
    lo = lo < 0 ? 0 : (lo > n_f ? n_f : lo);
    hi = hi < lo ? lo : (hi > n_f ? n_f : hi);
    fp[g] = rank_lower_bound(f_ids, lo, hi, c0 + tile_lo * 16);
    fe[g] = hi;
    fn[g] = fp[g] < fe[g] ? rank_position(f_ids[fp[g]], c0) : INT32_MAX;   // next filtered candidate position
  }

  // s_t: the rows t of the 16 queries of a group as one tile; the diagonal of the product, handed to the query's lanes
  float st[2];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    float4 a[K / 16];
    rank_load_rows<K>(P, tc[g], qd, a);
    floatx4_r d0, d1;
    rank_tile<K>(a, b[0], b[1], d0, d1);
    const floatx4_r d = g == 0 ? d0 : d1;
    // candidate m = 4 qd + j of the tile against query i sits in lane (i, qd), element j: the diagonal m = i
    const int j = i & 3;
    const float mine = j == 0 ? d[0] : (j == 1 ? d[1] : (j == 2 ? d[2] : d[3]));
    const float dot = __shfl(mine, (i >> 2) * 16 + i, kWave);
    st[g] = rank_score(n2[tc[g]], dot);
  }

  int32_t lt[2] = {0, 0}, eq[2] = {0, 0};
  float4 a_cur[K / 16], a_nxt[K / 16];
  {
    const int32_t r = tile_lo * 16 + i;
    rank_load_rows<K>(P, r < n_c ? r : n_c - 1, qd, a_cur);
  }
  for (int32_t tile = tile_lo; tile < tile_hi; ++tile) {
    const int32_t base = tile * 16;
    if (tile + 1 < tile_hi) {                                   // the next tile's rows are requested before this one's MFMAs
      const int32_t r = base + 16 + i;
      rank_load_rows<K>(P, r < n_c ? r : n_c - 1, qd, a_nxt);
    }
    float nn[4];
    if (base + 16 <= n_c) {
      const float4 v = *reinterpret_cast<const float4*>(n2 + base + 4 * qd);
      nn[0] = v.x; nn[1] = v.y; nn[2] = v.z; nn[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const int32_t c = base + 4 * qd + j; nn[j] = n2[c < n_c ? c : n_c - 1]; }
    }
    floatx4_r d[2];
    rank_tile<K>(a_cur, b[0], b[1], d[0], d[1]);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      // candidates of this tile the query leaves out: the filter's ids in [base, base + 16), the true answer
      unsigned mask = 0u;
      while (fn[g] < base + 16) {
        if (fn[g] >= base) mask |= 1u << (fn[g] - base);
        ++fp[g];
        fn[g] = fp[g] < fe[g] ? rank_position(f_ids[fp[g]], c0) : INT32_MAX;
      }
      if (tc[g] >= base && tc[g] < base + 16) mask |= 1u << (tc[g] - base);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = 4 * qd + j;
        const bool on = base + m < n_c && !(mask >> m & 1u);
        const float s = rank_score(nn[j], d[g][j]);
        lt[g] += on && s < st[g] ? 1 : 0;
        eq[g] += on && s == st[g] ? 1 : 0;
      }
    }
    if (tile + 1 < tile_hi) {
#pragma unroll
      for (int m = 0; m < K / 16; ++m) a_cur[m] = a_nxt[m];
    }
  }
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    lt[g] += __shfl_xor(lt[g], 16, kWave);
    lt[g] += __shfl_xor(lt[g], 32, kWave);
    eq[g] += __shfl_xor(eq[g], 16, kWave);
    eq[g] += __shfl_xor(eq[g], 32, kWave);
    if (qd == 0 && live[g]) {
      if (lt[g]) atomicAdd(lt_out + qi[g], lt[g]);
      if (eq[g]) atomicAdd(eq_out + qi[g], eq[g]);
    }
  }
}

}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_transr_project_supported(int d, int k) { return has_width(RankWidths{}, d) && has_width(RankWidths{}, k) ? 1 : 0; }

int kgat_transr_project_f32(int64_t n_rows, int64_t n_ent, int d, int k, const float* ent, const int32_t* ids,
                            int64_t row0, const float* W_r, const float* rel_row, float sign, float* out, float* n2,
                            kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_rows >= 0 && n_rows < INT32_MAX && n_ent >= 1 && d > 0 && k > 0, "transr_project: bad size");
  KGAT_CHECK_ARG(sign == 1.f || sign == -1.f, "transr_project: sign must be +1 or -1");
  KGAT_CHECK_ARG(ids != nullptr || (row0 >= 0 && row0 + n_rows <= n_ent),
                 "transr_project: rows [%lld, %lld) outside the %lld entities", (long long)row0,
                 (long long)(row0 + n_rows), (long long)n_ent);
  if (!kgat_transr_project_supported(d, k)) {
    set_error("transr_project: unsupported widths %d -> %d (d, k in {16, 32, 64, 128})", d, k);
    return KGAT_E_UNSUPPORTED;
  }
  if (n_rows == 0) return KGAT_OK;
  KGAT_CHECK_ARG(ent && W_r && out, "transr_project: null pointer");
  KGAT_CHECK_ARG(aligned16(ent) && aligned16(W_r) && aligned16(out), "transr_project: ent, W_r and out must be 16-byte aligned");
  const int64_t tiles = (n_rows + 15) / 16;
  int64_t blocks = (tiles + 3) / 4;
  // a workgroup stages the whole weight: enough tiles per workgroup to pay for it, at most two workgroups per CU
  const int64_t most = (int64_t)device_cu_count() * 2;
  if (blocks > most) blocks = most;
  const int rc = dispatch_widths(MfmaWidths{}, d, k, [&](auto dd, auto kk) -> int {
    hipLaunchKernelGGL((transr_project_kernel<decltype(dd)::value, decltype(kk)::value>), dim3((unsigned)blocks),
                       dim3(256), 0, as_stream(stream), (int32_t)n_rows, n_ent, ent, ids, row0, W_r, rel_row, sign, out, n2);
    KGAT_CHECK_LAUNCH("transr_project");
    return KGAT_OK;
  });
  if (rc == KGAT_E_UNSUPPORTED) set_error("transr_project: unsupported widths %d -> %d", d, k);
  return rc;
}

int kgat_transr_rank_supported(int k) { return has_width(RankWidths{}, k) ? 1 : 0; }

int kgat_transr_rank_f32(int64_t n_q, int64_t n_c, int64_t c0, int k, const float* q, const int32_t* t, const float* p,
                         const float* n2, const int32_t* filter_ptr, const int32_t* filter_ids, int64_t n_filter,
                         int32_t* lt, int32_t* eq, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_q >= 1 && n_c >= 1 && c0 >= 0 && n_filter >= 0, "transr_rank: n_q, n_c >= 1, c0, n_filter >= 0");
  KGAT_CHECK_ARG(n_q < INT32_MAX - 256 && c0 + n_c < INT32_MAX - 32 && n_filter < INT32_MAX,
                 "transr_rank: sizes beyond 32-bit ids");
  if (!kgat_transr_rank_supported(k)) {
    set_error("transr_rank: unsupported width %d (k in {16, 32, 64, 128})", k);
    return KGAT_E_UNSUPPORTED;
  }
  KGAT_CHECK_ARG(q && t && p && n2 && filter_ptr && lt && eq && (n_filter == 0 || filter_ids), "transr_rank: null pointer");
  KGAT_CHECK_ARG(aligned16(q) && aligned16(p) && aligned16(n2), "transr_rank: q, p and n2 must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(lt, 0, (size_t)n_q * 4, st) != hipSuccess || hipMemsetAsync(eq, 0, (size_t)n_q * 4, st) != hipSuccess) {
    set_error("transr_rank: cannot clear the counts");
    return KGAT_E_HIP;
  }
  // (query blocks) x (candidate segments): about two workgroups per CU, a segment no shorter than kRankMinTiles tiles
  const int64_t n_tiles = (n_c + 15) / 16;
  const int64_t qblocks = (n_q + kRankWaves * kRankQ - 1) / (kRankWaves * kRankQ);
  int64_t n_seg = ((int64_t)device_cu_count() * 2 + qblocks - 1) / qblocks;
  const int64_t max_seg = n_tiles / kRankMinTiles > 0 ? n_tiles / kRankMinTiles : 1;
  if (n_seg > max_seg) n_seg = max_seg;
  if (n_seg > kRankMaxSeg) n_seg = kRankMaxSeg;
  if (n_seg < 1) n_seg = 1;
  const int64_t per = (n_tiles + n_seg - 1) / n_seg;
  n_seg = (n_tiles + per - 1) / per;
  return dispatch_width(RankWidths{}, k, [&](auto kk) -> int {
    hipLaunchKernelGGL((transr_rank_kernel<decltype(kk)::value>), dim3((unsigned)qblocks, (unsigned)n_seg),
                       dim3(kRankWaves * 64), 0, st, (int32_t)n_q, (int32_t)n_c, (int32_t)c0, (int32_t)per, q, t, p, n2,
                       filter_ptr, filter_ids, (int32_t)n_filter, lt, eq);
    KGAT_CHECK_LAUNCH("transr_rank");
    return KGAT_OK;
  });
}

}  // extern "C"
