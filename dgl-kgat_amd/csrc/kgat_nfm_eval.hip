// All-pairs evaluation of a one-hidden-layer NFM (fm_models.NFM, layers = (hidden,)) for gfx950: per user the K best
// unseen items and their scores, nothing of size users x items written.  DESIGN.md 30.
//
// From bi({u} + F(i)) = v_u * P_i + T_i (fm_models.pool_items) the first layer of pair (u, i) is
//     pre[j] = sum_c (W1[j,c] v_u[c]) P_i[c] + C_i[j],     C = T W1^T + b1  (item-only, the caller's addmm)
// so a user is a (hidden x d) matrix a = fl(W1 * v_u) and a tile of 32 items a small GEMM against the k-major item
// fragments that kgat_eval_items_kmajor_f32 writes (emb = P, F = d).
//
//  1. nfm_c_layout_kernel: C (n_items x hidden, row-major) as the accumulator's start, [tile][block of 32 hidden units]
//     [lane][16] - a lane's sixteen values are four 16-byte loads.
//  2. nfm_eval_sweep_kernel: ONE USER per wavefront, four per workgroup, a contiguous segment of item tiles.  A = the
//     user's matrix in registers (d / 2 per block of 32 hidden units), B = the item fragment: one 16-byte load feeds
//     4 x hidden / 32 v_mfma_f32_32x32x2_f32.  A lane then holds ONE item column and sixteen hidden units of every
//     block: relu and the contraction with h are in-lane FMAs plus one exchange between the half-waves.  The 32 keys of
//     a tile lie across the lanes: those at or above the user's K-th best so far are appended to the user's candidate
//     buffer in LDS (ballot + prefix count), a full buffer is pruned by selection (training items dropped by binary
//     search, the K-th best key bisected, ties by position) - the scheme of kgat_eval_sweep_body.h for one user.
//  3. nfm_eval_merge_kernel: one wavefront per user merges the segments' lists through the same buffer and prune,
//     ranks the K survivors and writes positions and scores (+ the per-user constant).
//
// The order is (key descending, IEEE compare, position ascending), total: the lists do not depend on the segments, on
// the users sharing a launch or on K beyond their length.  No float atomics; bitwise reproducible.
// The candidate buffer, its append and prune and the merge kernel are kgat_topk_wave.h (shared with kgat_ripple_eval.hip).
#include "kgat_topk_wave.h"

namespace kgat {

typedef float floatx4n __attribute__((ext_vector_type(4)));

// hidden unit of register r of a lane's accumulator of block hb (the MFMA's 32 x 32 output: row (r & 3) + 8 (r >> 2) +
// 4 half, column lane & 31)
__host__ __device__ constexpr int nfm_unit(int hb, int r, int half) { return 32 * hb + (r & 3) + 8 * (r >> 2) + 4 * half; }

__global__ __launch_bounds__(256) void nfm_c_layout_kernel(int64_t n_items, int hidden, int64_t total,
                                                           const float* __restrict__ C, float* __restrict__ Clay) {
  const int HB = hidden / 32;
  for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < total; x += (int64_t)gridDim.x * 256) {
    const int r = (int)(x & 15), lane = (int)(x >> 4 & 63);
    const int64_t th = x >> 10;
    const int hb = (int)(th % HB);
    const int64_t it = th / HB * kEvalTile + (lane & 31);
    Clay[x] = it < n_items ? C[(size_t)it * hidden + nfm_unit(hb, r, lane >> 5)] : 0.f;
  }
}

// D: the embedding width, HB: blocks of 32 hidden units.  Registers: the user's matrix HB x D / 2, the accumulators and
// the next tile's C 16 HB each, two buffers of item fragments.
template <int D, int HB>
__global__ __launch_bounds__(kNfmNW * 64) void nfm_eval_sweep_kernel(
    int64_t n_users, const int32_t* __restrict__ user_ids, int64_t n_items, int64_t n_tiles, int FP2,
    const float* __restrict__ V, int64_t v_stride, const float* __restrict__ W1, const float* __restrict__ itemT,
    const float* __restrict__ Clay, const float* __restrict__ h, const float* __restrict__ item_lin,
    const int32_t* __restrict__ train_ptr, const int32_t* __restrict__ train_items, int K,
    float* __restrict__ part_s, int32_t* __restrict__ part_i) {
  constexpr int S = D / 2;                 // k pairs of a row
  constexpr int CH = S < 16 ? S : 16;      // k pairs of a chunk: the loads in flight behind a chunk's MFMAs
  constexpr int NC = S / CH, Q = CH / 4;
  __shared__ float cand_s[kNfmNW * kNfmCap];
  __shared__ int32_t cand_i[kNfmNW * kNfmCap];
  __shared__ __attribute__((aligned(16))) float h_s[HB * 32];   // [block][half][16]: a lane's h values in register order
  if (threadIdx.x < HB * 32) {
    const int x = threadIdx.x;
    h_s[x] = h[nfm_unit(x >> 5, x & 15, x >> 4 & 1)];
  }
  __syncthreads();                                              // (the only workgroup barrier: before any wavefront leaves)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ul = lane & 31, half = lane >> 5;
  const int64_t u = (int64_t)blockIdx.x * kNfmNW + w;           // position in user_ids
  if (u >= n_users) return;
  const int seg = blockIdx.y, n_seg = gridDim.y;
  const int64_t t_lo = n_tiles * seg / n_seg, t_hi = n_tiles * (seg + 1) / n_seg;   // (n_seg <= n_tiles: never empty)
  float* cs = cand_s + w * kNfmCap;
  int32_t* ci = cand_i + w * kNfmCap;
  const int32_t tr_lo = train_ptr[u], tr_hi = train_ptr[u + 1];

  // a[hb][s] = fl(W1[j, c] * v_u[c]) for the lane's A-operand element: j = 32 hb + (lane & 31), c = 2 s + half
  const float* row = V + (size_t)user_ids[u] * v_stride;
  float a[HB][S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const float v = row[2 * s + half];
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) a[hb][s] = W1[(size_t)(32 * hb + ul) * D + 2 * s + half] * v;
  }

  const floatx4n* frag = reinterpret_cast<const floatx4n*>(itemT) + lane;     // + ((tile FP2 / 4) + quad) 64
  const floatx4n* cl = reinterpret_cast<const floatx4n*>(Clay) + lane * 4;    // + (tile HB + hb) 256 + q
  const floatx4n* hv = reinterpret_cast<const floatx4n*>(h_s) + half * 4;     // + hb 8 + q
  const int FQ = FP2 / 4;

  floatx4n cur[Q], nxt[Q];
  floatx16 cn[HB];
  float ln;
#pragma unroll
  for (int q = 0; q < Q; ++q) cur[q] = frag[((size_t)t_lo * FQ + q) * 64];
#pragma unroll
  for (int hb = 0; hb < HB; ++hb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const floatx4n c4 = cl[((size_t)t_lo * HB + hb) * 256 + q];
#pragma unroll
      for (int c = 0; c < 4; ++c) cn[hb][4 * q + c] = c4[c];
    }
  {
    const int64_t it = t_lo * kEvalTile + ul;
    ln = it < n_items ? item_lin[it] : 0.f;
  }

  int cnt = 0, kept = 0;
  float tau = kNegInf;   // the user's K-th best key so far: -inf while fewer than K are held
  for (int64_t t = t_lo; t < t_hi; ++t) {
    floatx16 acc[HB];
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) acc[hb] = cn[hb];
    const float lin_t = ln;
    const int64_t tn = t + 1 < t_hi ? t + 1 : t_hi - 1;   // (past the end the last tile is read again, unused)
#pragma unroll
    for (int hb = 0; hb < HB; ++hb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const floatx4n c4 = cl[((size_t)tn * HB + hb) * 256 + q];
#pragma unroll
        for (int c = 0; c < 4; ++c) cn[hb][4 * q + c] = c4[c];
      }
    {
      const int64_t it = tn * kEvalTile + ul;
      ln = it < n_items ? item_lin[it] : 0.f;
    }
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
      // the next chunk's fragments go out ahead of this chunk's MFMAs
      const size_t nq = ch + 1 < NC ? ((size_t)t * FQ + (ch + 1) * Q) : (size_t)tn * FQ;
#pragma unroll
      for (int q = 0; q < Q; ++q) nxt[q] = frag[(nq + q) * 64];
      __builtin_amdgcn_sched_barrier(0);
      // the chain of a hidden unit runs in ascending c: k pair s = CH ch + 4 q + c, columns 2 s then 2 s + 1
#pragma unroll
      for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int hb = 0; hb < HB; ++hb)
            acc[hb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[hb][ch * CH + 4 * q + c], cur[q][c], acc[hb], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < Q; ++q) cur[q] = nxt[q];
    }
    // s_i = sum_j h_j relu(pre_j): a lane sums its 16 HB units in ascending (block, register) order from 0, one fma
    // each; the two half-waves' sums are added (lower half + upper half: the same bits on both lanes)
    float part = 0.f;
#pragma unroll
    for (int hb = 0; hb < HB; ++hb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const floatx4n h4 = hv[hb * 8 + q];
#pragma unroll
        for (int c = 0; c < 4; ++c) part = fmaf(h4[c], fmaxf(acc[hb][4 * q + c], 0.f), part);
      }
    const float other = __shfl_xor(part, 32, 64);
    const float sum = half ? other + part : part + other;
    const float key = sum + lin_t;
    const int64_t it = t * kEvalTile + ul;
    // (the padded end of the last tile and the upper half-wave's copies are never candidates)
    const bool pass = half == 0 && it < n_items && key >= tau;
    nfm_append(cs, ci, lane, K, pass, key, (int32_t)it, train_items, tr_lo, tr_hi, cnt, kept, tau);
  }
  // the segment's list: at most K entries, in no order, padded with (-inf, pad)
  nfm_prune(cs, ci, lane, K, train_items, tr_lo, tr_hi, cnt, kept, tau);
  for (int x = lane; x < K; x += 64) {
    const size_t o = ((size_t)u * n_seg + seg) * K + x;
    part_s[o] = x < cnt ? cs[x] : kNegInf;
    part_i[o] = x < cnt ? ci[x] : kIdxPad;
  }
}

using NfmWidths = WidthList<16, 32, 64, 128>;

// item segments of a launch: about two rounds of resident wavefronts, at least eight tiles each
static int nfm_segments(int64_t n_users, int64_t n_tiles) {
  const int64_t want = (int64_t)device_cu_count() * 16;   // 4 SIMDs x 2 wavefronts x 2 rounds
  int64_t seg = (want + n_users - 1) / (n_users > 0 ? n_users : 1);
  const int64_t most = n_tiles / 8 > 0 ? n_tiles / 8 : 1;
  if (seg > most) seg = most;
  if (seg > kNfmMaxSeg) seg = kNfmMaxSeg;
  return seg < 1 ? 1 : (int)seg;
}

struct NfmScratch { float* Clay; float* part_s; int32_t* part_i; size_t bytes; };
static NfmScratch nfm_carve(void* scratch, int64_t n_users, int64_t n_items, int hidden, int K) {
  const int64_t n_tiles = (n_items + kEvalTile - 1) / kEvalTile;
  const size_t lists = (size_t)n_users * nfm_segments(n_users, n_tiles) * K;
  Carver cv(scratch);
  NfmScratch s;
  s.Clay = cv.take<float>((size_t)n_tiles * hidden * 32);
  s.part_s = cv.take<float>(lists);
  s.part_i = cv.take<int32_t>(lists);
  s.bytes = cv.off;
  return s;
}

template <int D, int HB, typename... Args>
static void nfm_launch_sweep(dim3 grid, hipStream_t st, Args... args) {
  hipLaunchKernelGGL((nfm_eval_sweep_kernel<D, HB>), grid, dim3(kNfmNW * 64), 0, st, args...);
}

}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_nfm_eval_supported(int d, int hidden, int K) {
  return has_width(NfmWidths{}, d) && (hidden == 32 || hidden == 64) && K >= 1 && K <= kNfmMaxK;
}

size_t kgat_nfm_eval_scratch_bytes(int64_t n_users, int64_t n_items, int d, int hidden, int K) {
  if (n_users <= 0 || n_items <= 0 || !kgat_nfm_eval_supported(d, hidden, K)) return 256;
  return nfm_carve(nullptr, n_users, n_items, hidden, K).bytes;
}

int kgat_nfm_eval_topk_f32(int64_t n_users, const int32_t* user_ids, int64_t n_items, int d, int hidden, const float* V,
                           int64_t v_stride, const float* W1, const float* itemT, const float* C, const float* h,
                           const float* item_lin, const float* user_const, const int32_t* train_ptr,
                           const int32_t* train_items, int K, void* scratch, size_t scratch_bytes, int32_t* topk_items,
                           float* topk_scores, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_users >= 0 && n_items >= 1 && n_items < ((int64_t)1 << 31) - kEvalTile && v_stride >= 1,
                 "nfm_eval_topk: bad sizes (n_users = %lld, n_items = %lld, v_stride = %lld)", (long long)n_users,
                 (long long)n_items, (long long)v_stride);
  if (!kgat_nfm_eval_supported(d, hidden, K)) {
    set_error("nfm_eval_topk: d = %d (16, 32, 64, 128), hidden = %d (32, 64) or K = %d (1..%d) not supported", d, hidden,
              K, kNfmMaxK);
    return KGAT_E_UNSUPPORTED;
  }
  KGAT_CHECK_ARG(v_stride >= d, "nfm_eval_topk: v_stride %lld below d = %d", (long long)v_stride, d);
  KGAT_CHECK_ARG(user_ids && V && W1 && itemT && C && h && item_lin && train_ptr && scratch && topk_items,
                 "nfm_eval_topk: null pointer");
  KGAT_CHECK_ARG(aligned16(itemT) && aligned16(scratch), "nfm_eval_topk: itemT and scratch must be 16-byte aligned");
  if (scratch_bytes < kgat_nfm_eval_scratch_bytes(n_users, n_items, d, hidden, K)) {
    set_error("nfm_eval_topk: scratch too small (%zu bytes, %zu needed)", scratch_bytes,
              kgat_nfm_eval_scratch_bytes(n_users, n_items, d, hidden, K));
    return KGAT_E_WORKSPACE;
  }
  if (n_users == 0) return KGAT_OK;
  const int64_t n_tiles = (n_items + kEvalTile - 1) / kEvalTile;
  const int n_seg = nfm_segments(n_users, n_tiles);
  const NfmScratch ws = nfm_carve(scratch, n_users, n_items, hidden, K);
  hipStream_t st = as_stream(stream);
  const int64_t total = n_tiles * hidden * 32;
  int64_t lay_grid = (total + 255) / 256;
  if (lay_grid > 65536) lay_grid = 65536;
  hipLaunchKernelGGL(nfm_c_layout_kernel, dim3((unsigned)lay_grid), dim3(256), 0, st, n_items, hidden, total, C, ws.Clay);
  KGAT_CHECK_LAUNCH("nfm_eval_topk: C layout");
  const unsigned gx = (unsigned)((n_users + kNfmNW - 1) / kNfmNW);
  const dim3 grid(gx, (unsigned)n_seg);
  const int FP2 = eval_fp2(d);
  const int rc = dispatch_width(NfmWidths{}, d, [&](auto D) {
    if (hidden == 32)
      nfm_launch_sweep<D(), 1>(grid, st, n_users, user_ids, n_items, n_tiles, FP2, V, v_stride, W1, itemT,
                               (const float*)ws.Clay, h, item_lin, train_ptr, train_items, K, ws.part_s, ws.part_i);
    else
      nfm_launch_sweep<D(), 2>(grid, st, n_users, user_ids, n_items, n_tiles, FP2, V, v_stride, W1, itemT,
                               (const float*)ws.Clay, h, item_lin, train_ptr, train_items, K, ws.part_s, ws.part_i);
    return KGAT_OK;
  });
  if (rc != KGAT_OK) return rc;
  KGAT_CHECK_LAUNCH("nfm_eval_sweep");
  hipLaunchKernelGGL(nfm_eval_merge_kernel, dim3(gx), dim3(kNfmNW * 64), 0, st, n_users, n_seg, K,
                     (const float*)ws.part_s, (const int32_t*)ws.part_i, user_const, topk_items, topk_scores);
  KGAT_CHECK_LAUNCH("nfm_eval_merge");
  return KGAT_OK;
}

}  // extern "C"
