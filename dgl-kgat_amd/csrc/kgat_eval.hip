// Evaluation of the reference's metric.py:36-68 (calc_recall_ndcg) for gfx950: per test user the scores
// against every item (metric.py:48), the training items' scores set to 0.0 (:50), the K best of a
// descending sort (:51-59, ties: lower item position first, as a stable sort gives), then recall@K
// (:5-7) and ndcg@K against the user's OWN sorted hit list (:23-34).  SURVEY.md 8f #4.
//
// Three launches, no (users x items) score matrix in memory:
//  1. eval_items_kmajor_kernel: the item rows as MFMA A fragments, [32-item tile][group of 8 k pairs][half][lane][4] -
//     one coalesced 16-byte load per lane per FOUR v_mfma_f32_32x32x2_f32 later.
//  2. eval_topk_kernel: a wavefront owns 32 users (the B operand: their rows, in registers at the reference's readout
//     width, in LDS otherwise) and a contiguous segment of item tiles; scores come out of the fp32 MFMA (an exact
//     k-ordered fmaf chain, 157 TF peak: 620 GFLOP on the amazon-book shape) with the USER on the lane, so a lane
//     compares its 16 scores of a tile with its user's current K-th best and only the rare survivors (about
//     K ln(n / K) per user over the whole sweep) are appended to the user's candidate buffer in LDS.  A full buffer is
//     pruned by the whole wavefront: entries that are training items are dropped (binary search in the user's sorted
//     list), every entry's place is counted on (score descending, position ascending), the K best stay and renew the
//     threshold.  One grid; the segments of a user block share their K-th best as they go.
//  3. eval_merge_kernel: one wavefront per user merges the segments' partial lists with the masked
//     training items - min(K, |train_u|) entries (0.0, lowest positions), which is all of them that can
//     rank - marks the hits (binary search in the sorted test list) and writes recall and ndcg in fp64.
//
// The order is total - (score descending, position ascending) - so the result does not depend on how
// items were cut into tiles and segments: bitwise reproducible, equal to a stable descending sort.
//
// Launch 2's body is kgat_eval_sweep_body.h around the tile walk of kgat_eval_walk.h; the plan and the launch are
// kgat_eval_common.h's.  kgat_eval_topk.hip (ranked lists with scores for K up to 128, metrics at several cut-offs)
// includes the same body over a larger candidate buffer, kgat_eval_rank.hip (exact ranks) the same walk.
#include "kgat_eval_common.h"

namespace kgat {

__global__ __launch_bounds__(256) void eval_items_kmajor_kernel(int64_t n_items, int F, int FP2, int64_t n_tiles,
                                                                const float* __restrict__ emb, int64_t emb_stride,
                                                                const int32_t* __restrict__ item_ids,
                                                                float* __restrict__ itemT) {
  // one thread per element of itemT: coalesced stores, gathered 4-byte loads (a 17 MB one-off per call).
  // Layout (round 6): [tile][group of 8 k pairs][half of the group][lane][4 k pairs] - a lane's A operands of FOUR
  // consecutive MFMAs are one 16-byte load, a wavefront's one contiguous KB (it was [tile][k pair][lane]: one 4-byte
  // load per MFMA, and on this chip a vector-memory instruction costs the fp32 MFMA stream about as much issue time as
  // an MFMA does - NOTEBOOK 3.2)
  const int64_t total = n_tiles * FP2 * 64;
  for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < total; x += (int64_t)gridDim.x * 256) {
    const int u4 = (int)(x & 3);
    const int lane = (int)(x >> 2 & 63);
    const int64_t tq = x >> 8;                       // (tile, group, half) = tile * (FP2 / 4) + quad of k pairs
    const int s = (int)(tq % (FP2 / 4)) * 4 + u4;
    const int64_t tile = tq / (FP2 / 4);
    const int64_t it = tile * kEvalTile + (lane & 31);
    const int k = 2 * s + (lane >> 5);
    float v = 0.f;
    if (it < n_items && k < F) v = emb[(size_t)item_ids[it] * emb_stride + k];
    itemT[x] = v;
  }
}

// (two wavefronts per SIMD at most - the LDS allows no more in either form - so the allocator may use 256 registers:
// left to its default budget it kept 150 and spilled the users' rows to scratch)
template <int NW, int KG>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2), amdgpu_num_vgpr(248))) void eval_topk_kernel(
    int64_t n_users, const int32_t* __restrict__ user_ids, int64_t n_items, int FP2, int F, EvalBounds bounds,
    const float* __restrict__ emb, int64_t emb_stride,
    const float* __restrict__ itemT, const int32_t* __restrict__ train_ptr, const int32_t* __restrict__ train_items,
    int K, float* __restrict__ part_s, int32_t* __restrict__ part_i, unsigned* __restrict__ tau_shared) {
  constexpr int CAP = kEvalCap;
#include "kgat_eval_sweep_body.h"
}

__global__ __launch_bounds__(256) void eval_merge_kernel(
    int64_t n_users, int n_seg, int K, const float* __restrict__ part_s, const int32_t* __restrict__ part_i,
    const int32_t* __restrict__ train_ptr, const int32_t* __restrict__ train_items,
    const int32_t* __restrict__ test_ptr, const int32_t* __restrict__ test_items, const double* __restrict__ disc,
    double* __restrict__ recall, double* __restrict__ ndcg, int32_t* __restrict__ topk) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;
  float s = kNegInf;
  int i = kIdxPad;
  // the masked training items (metric.py:50): score 0.0; only the K lowest positions can rank
  const int32_t tr_lo = train_ptr[u], tr_hi = train_ptr[u + 1];
  if (lane < K && tr_lo + lane < tr_hi) { s = 0.f; i = train_items[tr_lo + lane]; }
  for (int g = 0; g < n_seg; ++g) {
    if (lane >= 32 && lane - 32 < K) {
      const size_t o = ((size_t)u * n_seg + g) * K + (lane - 32);
      s = part_s[o];
      i = part_i[o];
    }
    wave_sort_desc(s, i, lane);  // the K best so far in lanes [0, K), K <= 32
  }
  if (n_seg == 0) wave_sort_desc(s, i, lane);
  const int32_t te_lo = test_ptr[u], te_hi = test_ptr[u + 1];
  const bool hit = lane < K && i != kIdxPad && in_sorted(test_items, te_lo, te_hi, i);
  const unsigned long long hits = __ballot(hit);
  if (topk && lane < K) topk[(size_t)u * K + lane] = i == kIdxPad ? -1 : i;
  if (lane == 0) {
    const int nh = __popcll(hits);
    const int n_pos = te_hi - te_lo;
    double dcg = 0.0, ideal = 0.0;
    for (int k = 0; k < K; ++k)
      if (hits >> k & 1ull) dcg += disc[k];
    for (int k = 0; k < nh; ++k) ideal += disc[k];
    recall[u] = n_pos > 0 ? (double)nh / (double)n_pos : 0.0;
    ndcg[u] = ideal > 0.0 ? dcg / ideal : 0.0;
  }
}

// The sweep at K <= 32 (declared in kgat_eval_common.h: kgat_eval_topk_f32 launches it too).
int eval_sweep_launch(const char* who, int64_t n_users, const int32_t* user_ids, int64_t n_items, int F, const float* emb,
                      int64_t emb_stride, const float* itemT, const int32_t* train_ptr, const int32_t* train_items, int K,
                      const EvalPlanH& pl, float* part_s, int32_t* part_i, unsigned* tau_shared, hipStream_t st) {
  const auto kernel = eval_with_form<4>(eval_reg_kg(F), pl.nw, [](auto NW, auto KG) { return &eval_topk_kernel<NW(), KG()>; });
  KGAT_RETURN_IF(eval_lists_sweep(who, kernel, kEvalCap, n_users, user_ids, n_items, F, emb, emb_stride, itemT, train_ptr,
                                  train_items, K, pl, EvalListsWs{part_s, part_i, tau_shared}, st));
  KGAT_CHECK_LAUNCH("eval_topk");
  return KGAT_OK;
}

}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_eval_supported(int F, int K) {
  return F >= 1 && K >= 1 && K <= kEvalMaxK && eval_waves_per_block(F) > 0;
}

int64_t kgat_eval_items_elems(int64_t n_items, int F) {
  if (n_items < 0 || F < 1) return 0;
  const int64_t n_tiles = (n_items + kEvalTile - 1) / kEvalTile;
  return n_tiles * eval_fp2(F) * 64;
}

int kgat_eval_items_kmajor_f32(int64_t n_items, int F, const float* emb, int64_t emb_stride, const int32_t* item_ids,
                               float* itemT, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_items >= 0 && F >= 1 && emb_stride >= F, "eval_items_kmajor: bad sizes");
  if (n_items == 0) return KGAT_OK;
  KGAT_CHECK_ARG(emb && item_ids && itemT, "eval_items_kmajor: null pointer");
  const int FP2 = eval_fp2(F);
  const int64_t n_tiles = (n_items + kEvalTile - 1) / kEvalTile;
  const int64_t total = n_tiles * FP2 * 64;
  int64_t grid = (total + 255) / 256;
  if (grid > 65536) grid = 65536;
  hipLaunchKernelGGL(eval_items_kmajor_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), n_items, F, FP2,
                     n_tiles, emb, emb_stride, item_ids, itemT);
  KGAT_CHECK_LAUNCH("eval_items_kmajor");
  return KGAT_OK;
}

size_t kgat_eval_workspace_bytes(int64_t n_users, int64_t n_items, int F, int K) {
  if (n_users <= 0 || n_items <= 0 || !kgat_eval_supported(F, K)) return 256;
  return eval_lists_workspace_bytes(n_users, eval_plan(n_users, n_items, F), K);
}

int kgat_eval_recall_ndcg_f32(int64_t n_users, const int32_t* user_ids, int64_t n_items, int F, const float* emb,
                              int64_t emb_stride, const float* itemT, const int32_t* train_ptr,
                              const int32_t* train_items, const int32_t* test_ptr, const int32_t* test_items, int K,
                              const double* disc, void* workspace, size_t workspace_bytes, double* recall_out,
                              double* ndcg_out, int32_t* topk_out, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_users >= 0 && n_items >= 0 && F >= 1 && emb_stride >= F, "eval_recall_ndcg: bad sizes");
  if (!kgat_eval_supported(F, K)) {
    set_error("eval_recall_ndcg: K = %d (1..%d) or F = %d not supported", K, kEvalMaxK, F);
    return KGAT_E_UNSUPPORTED;
  }
  if (n_users == 0) return KGAT_OK;
  KGAT_CHECK_ARG(n_items >= K, "eval_recall_ndcg: fewer items (%lld) than K (%d): the reference indexes rank K - 1",
                 (long long)n_items, K);
  KGAT_CHECK_ARG(user_ids && emb && itemT && train_ptr && test_ptr && disc && recall_out && ndcg_out && workspace,
                 "eval_recall_ndcg: null pointer");
  if (workspace_bytes < kgat_eval_workspace_bytes(n_users, n_items, F, K)) {
    set_error("eval_recall_ndcg: workspace too small");
    return KGAT_E_WORKSPACE;
  }
  const EvalPlanH pl = eval_plan(n_users, n_items, F);
  const EvalListsWs ws = eval_lists_carve(workspace, n_users, pl, K);
  hipStream_t st = as_stream(stream);
  const int rc = eval_sweep_launch("eval_recall_ndcg", n_users, user_ids, n_items, F, emb, emb_stride, itemT, train_ptr,
                                   train_items, K, pl, ws.part_s, ws.part_i, ws.tau_shared, st);
  if (rc != KGAT_OK) return rc;
  hipLaunchKernelGGL(eval_merge_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, st, n_users, pl.n_lists, K,
                     ws.part_s, ws.part_i, train_ptr, train_items, test_ptr, test_items, disc, recall_out, ndcg_out,
                     topk_out);
  KGAT_CHECK_LAUNCH("eval_merge");
  return KGAT_OK;
}

}  // extern "C"
