// Ranked item lists for K up to 128 and the metrics of the KGAT paper's table at several cut-offs, beside the
// K <= 32 recall / ndcg path of kgat_eval.hip (reference metric.py:36-68; the paper reports recall, ndcg, precision
// and hit ratio at K = 20 ... 100).  DESIGN.md 13.
//
//  1. eval_topk_wide_kernel: the sweep of kgat_eval.hip (it includes the same kgat_eval_sweep_body.h - MFMA walk, register
//     and LDS forms, two-ended append, shared threshold, segment plan) over a candidate buffer of 128 entries per user
//     (32 < K <= 64) or 156 (K <= 128): the pruning wavefront holds 2 / up to 3 entries per lane.  A wavefront's buffer
//     is 32 KB / 39 KB of the CU's 160 KB, so a CU holds four wavefronts, one per SIMD (workgroups of two in the
//     register forms); 156 entries are the most that four fit (256 entries - two wavefronts per CU - measured 16.8 ms
//     against 11.9 at K = 100 and 17.5 against 16.1 at K = 128 on the amazon-book shape).
//     K <= 32 launches the sweep of kgat_eval.hip itself.
//  2. eval_topk_merge_kernel: one wavefront per user merges the segments' lists - 2 K <= 64 E entries, E per lane,
//     a bitonic network over lanes (shuffles) and registers - with the masked training items (`mask`, metric.py:50) or
//     without them (`drop`: training items are never listed), and writes positions and scores.
//  3. eval_metrics_at_ks_kernel: hits of a ranked list in the user's test list, then recall / ndcg / precision / hit
//     ratio at up to 8 cut-offs, in fp64, the discounts summed in ascending rank order.
//
// The order is the one of kgat_eval.hip - (score descending, position ascending), total - so the lists are bitwise
// reproducible and their first K' entries are the list at K'.
#include "kgat_eval_common.h"

namespace kgat {

// (the LDS leaves room for one wavefront per SIMD at most in every form: the allocator may use the whole register file)
template <int NW, int KG, int CAP_>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(1, 1))) void eval_topk_wide_kernel(
    int64_t n_users, const int32_t* __restrict__ user_ids, int64_t n_items, int FP2, int F, EvalBounds bounds,
    const float* __restrict__ emb, int64_t emb_stride,
    const float* __restrict__ itemT, const int32_t* __restrict__ train_ptr, const int32_t* __restrict__ train_items,
    int K, float* __restrict__ part_s, int32_t* __restrict__ part_i, unsigned* __restrict__ tau_shared) {
  constexpr int CAP = CAP_;
#include "kgat_eval_sweep_body.h"
}

// Descending bitonic sort of 64 E (score, position) entries, entry x = 64 e + lane in register e of the lane: a
// partner at distance j < 64 is another lane (a shuffle), at j >= 64 another register of the same lane.
template <int E>
__device__ __forceinline__ void wave_sort_desc_wide(float (&s)[E], int (&i)[E], int lane) {
#pragma unroll
  for (int k = 2; k <= 64 * E; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j >= 64) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int eo = e | (j >> 6);
          if ((e & (j >> 6)) != 0 || eo >= E) continue;       // (e is the lower entry of its pair)
          const bool desc = ((64 * e) & k) == 0;
          const bool first = ranks_before(s[e], i[e], s[eo], i[eo]);
          const bool swap = desc != first;
          const float ts = s[e];
          const int ti = i[e];
          s[e] = swap ? s[eo] : ts;
          i[e] = swap ? i[eo] : ti;
          s[eo] = swap ? ts : s[eo];
          i[eo] = swap ? ti : i[eo];
        }
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const float so = __shfl_xor(s[e], j, 64);
          const int io = __shfl_xor(i[e], j, 64);
          const bool lower = (lane & j) == 0;
          const bool desc = ((64 * e + lane) & k) == 0;
          const bool mine_first = ranks_before(s[e], i[e], so, io);
          const bool keep = (lower == desc) ? mine_first : !mine_first;
          s[e] = keep ? s[e] : so;
          i[e] = keep ? i[e] : io;
        }
      }
    }
  }
}

// One wavefront per user; K <= 32 E.  The K best so far sit at entries [0, K), a segment's list goes to [32 E, 32 E + K).
template <int E>
__global__ __launch_bounds__(256) void eval_topk_merge_kernel(
    int64_t n_users, int n_seg, int K, const float* __restrict__ part_s, const int32_t* __restrict__ part_i,
    const int32_t* __restrict__ train_ptr, const int32_t* __restrict__ train_items, int drop_train,
    int32_t* __restrict__ topk_items, float* __restrict__ topk_scores) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;
  float s[E];
  int i[E];
#pragma unroll
  for (int e = 0; e < E; ++e) { s[e] = kNegInf; i[e] = kIdxPad; }
  if (!drop_train) {
    // the masked training items (metric.py:50): score 0.0; only the K lowest positions can rank
    const int32_t tr_lo = train_ptr[u], tr_hi = train_ptr[u + 1];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int x = 64 * e + lane;
      if (x < K && tr_lo + x < tr_hi) { s[e] = 0.f; i[e] = train_items[tr_lo + x]; }
    }
  }
  for (int g = 0; g < n_seg; ++g) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int x = 64 * e + lane - 32 * E;
      if (x >= 0 && x < K) {
        const size_t o = ((size_t)u * n_seg + g) * K + x;
        s[e] = part_s[o];
        i[e] = part_i[o];
      }
    }
    wave_sort_desc_wide<E>(s, i, lane);
  }
  if (n_seg == 0) wave_sort_desc_wide<E>(s, i, lane);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int x = 64 * e + lane;
    if (x < K) {
      const bool pad = i[e] == kIdxPad;
      topk_items[(size_t)u * K + x] = pad ? -1 : i[e];
      if (topk_scores) topk_scores[(size_t)u * K + x] = pad ? kNegInf : s[e];
    }
  }
}

constexpr int kEvalMaxKs = 8;
struct EvalKs { int32_t k[kEvalMaxKs]; };

// One wavefront per user: a lane marks the hits of ranks lane and lane + 64, then lane j sums cut-off j.
__global__ __launch_bounds__(256) void eval_metrics_at_ks_kernel(
    int64_t n_users, int K, const int32_t* __restrict__ topk_items, const int32_t* __restrict__ test_ptr,
    const int32_t* __restrict__ test_items, int n_ks, EvalKs ks, const double* __restrict__ disc,
    double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;
  const int32_t te_lo = test_ptr[u], te_hi = test_ptr[u + 1];
  unsigned long long hits[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int x = 64 * e + lane;
    const int32_t it = x < K ? topk_items[(size_t)u * K + x] : -1;   // (padding, -1, never hits)
    hits[e] = __ballot(it >= 0 && in_sorted(test_items, te_lo, te_hi, it));
  }
  if (lane < n_ks) {
    const int kj = ks.k[lane];
    int nh = 0;
    double dcg = 0.0, ideal = 0.0;
    for (int k = 0; k < kj; ++k)   // ascending ranks, as eval_merge_kernel sums them
      if ((k < 64 ? hits[0] : hits[1]) >> (k & 63) & 1ull) { dcg += disc[k]; ++nh; }
    for (int k = 0; k < nh; ++k) ideal += disc[k];
    const int n_pos = te_hi - te_lo;
    double* o = out + ((size_t)u * n_ks + lane) * 4;
    o[0] = n_pos > 0 ? (double)nh / (double)n_pos : 0.0;
    o[1] = ideal > 0.0 ? dcg / ideal : 0.0;
    o[2] = (double)nh / (double)kj;
    o[3] = nh > 0 ? 1.0 : 0.0;
  }
}

// The sweep at 32 < K <= 128 over a plan made with eval_cap(K).
static int eval_sweep_wide_launch(int64_t n_users, const int32_t* user_ids, int64_t n_items, int F, const float* emb,
                                  int64_t emb_stride, const float* itemT, const int32_t* train_ptr,
                                  const int32_t* train_items, int K, const EvalPlanH& pl, const EvalListsWs& ws,
                                  hipStream_t st) {
  const int cap = eval_cap(K), kg = eval_reg_kg(F);
  const auto kernel =
      cap == kEvalCapWide
          ? eval_with_form<2>(kg, pl.nw, [](auto NW, auto KG) { return &eval_topk_wide_kernel<NW(), KG(), kEvalCapWide>; })
          : eval_with_form<2>(kg, pl.nw, [](auto NW, auto KG) { return &eval_topk_wide_kernel<NW(), KG(), kEvalCapWidest>; });
  KGAT_RETURN_IF(eval_lists_sweep("eval_topk", kernel, cap, n_users, user_ids, n_items, F, emb, emb_stride, itemT,
                                  train_ptr, train_items, K, pl, ws, st));
  KGAT_CHECK_LAUNCH("eval_topk_wide");
  return KGAT_OK;
}

}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_eval_topk_supported(int F, int K) {
  return F >= 1 && K >= 1 && K <= kEvalTopkMaxK && eval_waves_per_block(F, eval_cap(K)) > 0;
}

size_t kgat_eval_topk_workspace_bytes(int64_t n_users, int64_t n_items, int F, int K) {
  if (n_users <= 0 || n_items <= 0 || !kgat_eval_topk_supported(F, K)) return 256;
  return eval_lists_workspace_bytes(n_users, eval_plan(n_users, n_items, F, eval_cap(K)), K);
}

int kgat_eval_topk_f32(int64_t n_users, const int32_t* user_ids, int64_t n_items, int F, const float* emb,
                       int64_t emb_stride, const float* itemT, const int32_t* train_ptr, const int32_t* train_items,
                       int K, int drop_train, void* workspace, size_t workspace_bytes, int32_t* topk_items,
                       float* topk_scores, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_users >= 0 && n_items >= 0 && F >= 1 && emb_stride >= F, "eval_topk: bad sizes");
  if (!kgat_eval_topk_supported(F, K)) {
    set_error("eval_topk: K = %d (1..%d) or F = %d not supported", K, kEvalTopkMaxK, F);
    return KGAT_E_UNSUPPORTED;
  }
  if (n_users == 0) return KGAT_OK;
  if (drop_train)
    KGAT_CHECK_ARG(n_items >= 1, "eval_topk: no items to rank");
  else
    KGAT_CHECK_ARG(n_items >= K, "eval_topk: fewer items (%lld) than K (%d): the reference indexes rank K - 1",
                   (long long)n_items, K);
  KGAT_CHECK_ARG(user_ids && emb && itemT && train_ptr && topk_items && workspace, "eval_topk: null pointer");
  if (workspace_bytes < kgat_eval_topk_workspace_bytes(n_users, n_items, F, K)) {
    set_error("eval_topk: workspace too small");
    return KGAT_E_WORKSPACE;
  }
  const EvalPlanH pl = eval_plan(n_users, n_items, F, eval_cap(K));
  const EvalListsWs ws = eval_lists_carve(workspace, n_users, pl, K);
  hipStream_t st = as_stream(stream);
  const int rc = K <= kEvalMaxK
                     ? eval_sweep_launch("eval_topk", n_users, user_ids, n_items, F, emb, emb_stride, itemT, train_ptr,
                                         train_items, K, pl, ws.part_s, ws.part_i, ws.tau_shared, st)
                     : eval_sweep_wide_launch(n_users, user_ids, n_items, F, emb, emb_stride, itemT, train_ptr,
                                              train_items, K, pl, ws, st);
  if (rc != KGAT_OK) return rc;
  const dim3 grid((unsigned)((n_users + 3) / 4));
#define KGAT_EVAL_MERGE(E)                                                                                          \
  hipLaunchKernelGGL(eval_topk_merge_kernel<E>, grid, dim3(256), 0, st, n_users, pl.n_lists, K, ws.part_s, ws.part_i, \
                     train_ptr, train_items, drop_train, topk_items, topk_scores)
  if (K <= 32) KGAT_EVAL_MERGE(1);
  else if (K <= 64) KGAT_EVAL_MERGE(2);
  else KGAT_EVAL_MERGE(4);
#undef KGAT_EVAL_MERGE
  KGAT_CHECK_LAUNCH("eval_topk_merge");
  return KGAT_OK;
}

int kgat_eval_metrics_at_ks(int64_t n_users, int K, const int32_t* topk_items, const int32_t* test_ptr,
                            const int32_t* test_items, int n_ks, const int32_t* ks, const double* disc, double* out,
                            kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_users >= 0 && K >= 1 && K <= kEvalTopkMaxK, "eval_metrics_at_ks: bad sizes (K = %d, 1..%d)", K,
                 kEvalTopkMaxK);
  KGAT_CHECK_ARG(n_ks >= 1 && n_ks <= kEvalMaxKs && ks, "eval_metrics_at_ks: 1..%d cut-offs", kEvalMaxKs);
  EvalKs kv = {};
  for (int j = 0; j < n_ks; ++j) {
    KGAT_CHECK_ARG(ks[j] >= 1 && ks[j] <= K && (j == 0 || ks[j] > ks[j - 1]),
                   "eval_metrics_at_ks: the cut-offs must ascend within 1..K (cut-off %d is %d, K = %d)", j, ks[j], K);
    kv.k[j] = ks[j];
  }
  if (n_users == 0) return KGAT_OK;
  KGAT_CHECK_ARG(topk_items && test_ptr && disc && out, "eval_metrics_at_ks: null pointer");
  hipLaunchKernelGGL(eval_metrics_at_ks_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, as_stream(stream),
                     n_users, K, topk_items, test_ptr, test_items, n_ks, kv, disc, out);
  KGAT_CHECK_LAUNCH("eval_metrics_at_ks");
  return KGAT_OK;
}

}  // extern "C"
