// One wavefront's K best of a stream of (key, item position) entries, K <= 128: the candidate buffer in LDS, the
// ballot-append, the bisection prune and the merge of partial lists.  Shared by the all-pairs sweeps that put ONE user's
// keys of a tile across the lanes (kgat_nfm_eval.hip, kgat_ripple_eval.hip).  Not part of the ABI.
//
// The order is (key descending, IEEE compare, position ascending), total: the lists do not depend on how the entries
// were cut into partial lists or on K beyond their length.  No float atomics; bitwise reproducible.
#pragma once
#include "kgat_eval_common.h"

namespace kgat {

constexpr int kNfmCap = 256;      // candidate entries of a user: four per lane of the pruning wavefront
constexpr int kNfmNW = 4;         // wavefronts per workgroup
constexpr int kNfmMaxSeg = 64;
constexpr int kNfmMaxK = 128;
static_assert(kNfmCap >= kNfmMaxK + kEvalTile, "a pruned buffer takes a whole tile");

// Keep the K best of the cnt entries of a user's buffer (all lanes of the wavefront; cnt, kept, tau wave-uniform).
// Entries [kept, cnt) are new: those that are training items (position in the ascending train_items[lo, hi)) are
// dropped first.  The K-th best key is selected by bisection over the bits of the scores' order-preserving form,
// entries that tie with it are taken in position order; the survivors are compacted to [0, keep) in lane order, not
// sorted.  tau becomes the K-th best key once K entries are held.
__device__ __forceinline__ void nfm_prune(float* __restrict__ cs, int32_t* __restrict__ ci, int lane, int K,
                                          const int32_t* __restrict__ train_items, int32_t lo, int32_t hi, int& cnt,
                                          int& kept, float& tau) {
  constexpr int EPL = kNfmCap / 64;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();                          // the appended entries are in LDS
  float s[EPL];
  int i[EPL];
  unsigned key[EPL];
  int n_valid = 0;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int x = lane + 64 * e;
    const bool have = x < cnt;
    s[e] = kNegInf;
    i[e] = kIdxPad;
    if (have) { s[e] = cs[x]; i[e] = ci[x]; }
    if (x >= kept && have && in_sorted(train_items, lo, hi, i[e])) { s[e] = kNegInf; i[e] = kIdxPad; }
    const bool valid = i[e] != kIdxPad;
    // (s + 0 maps -0 to +0, equal for the compare; 0 - below the key of every float - for an entry that is not there)
    key[e] = valid ? ordered_bits(s[e] + 0.f) : 0u;
    n_valid += (int)__popcll(__ballot(valid));
  }
  const int keep = n_valid < K ? n_valid : K;
  unsigned T = 0u;   // the keep-th largest key: the largest T with at least `keep` keys >= T
  if (keep > 0) {
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned c = T | (1u << bit);
      int n = 0;
#pragma unroll
      for (int e = 0; e < EPL; ++e) n += (int)__popcll(__ballot(key[e] >= c));
      if (n >= keep) T = c;
    }
  }
  bool sel[EPL];
  int n_above = 0, n_tied = 0;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {   // (T > 0: an entry that is not there is neither above nor tied)
    const bool above = keep > 0 && key[e] > T, tied = keep > 0 && key[e] == T;
    n_above += (int)__popcll(__ballot(above));
    n_tied += (int)__popcll(__ballot(tied));
    sel[e] = above || tied;
  }
  const int need_tied = keep - n_above;                // >= 1 when keep > 0
  if (n_tied > need_tied) {
    // the need_tied lowest positions among the tied entries (positions are distinct): the largest I with fewer than
    // need_tied tied positions below it
    int I = 0;
    for (int bit = 30; bit >= 0; --bit) {
      const int c = I | (1 << bit);
      int n = 0;
#pragma unroll
      for (int e = 0; e < EPL; ++e) n += (int)__popcll(__ballot(key[e] == T && i[e] < c));
      if (n < need_tied) I = c;
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) sel[e] = key[e] > T || (key[e] == T && i[e] <= I);
  }
  int pos[EPL], n_before = 0;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const unsigned long long m = __ballot(sel[e]);
    pos[e] = n_before + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    n_before += (int)__popcll(m);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();                          // every lane has read its entries
#pragma unroll
  for (int e = 0; e < EPL; ++e)
    if (sel[e]) { cs[pos[e]] = s[e]; ci[pos[e]] = i[e]; }
  cnt = keep;
  kept = keep;
  if (keep == K) {
    const float ts = from_ordered_bits(T);
    if (ts > tau) tau = ts;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Append the lanes' entries with `pass` to the buffer, pruning first where they would not fit (a pruned buffer holds
// at most K <= 128 entries: the 64 a wavefront can append at a time always fit).
__device__ __forceinline__ void nfm_append(float* __restrict__ cs, int32_t* __restrict__ ci, int lane, int K, bool pass,
                                           float sc, int32_t it, const int32_t* __restrict__ train_items, int32_t lo,
                                           int32_t hi, int& cnt, int& kept, float& tau) {
  const unsigned long long m = __ballot(pass);
  if (m == 0ull) return;                                   // wave-uniform
  const int n = (int)__popcll(m);
  if (cnt + n > kNfmCap) nfm_prune(cs, ci, lane, K, train_items, lo, hi, cnt, kept, tau);
  const int p = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
  if (pass) { cs[p] = sc; ci[p] = it; }
  cnt += n;
}

// One wavefront per user: the segments' lists through the buffer and its prune (no training items left among them),
// then every survivor's place is counted on the total order and the list written in rank order.
// (static: every translation unit that includes this header launches its own copy)
static __global__ __launch_bounds__(kNfmNW * 64) void nfm_eval_merge_kernel(
    int64_t n_users, int n_seg, int K, const float* __restrict__ part_s, const int32_t* __restrict__ part_i,
    const float* __restrict__ user_const, int32_t* __restrict__ topk_items, float* __restrict__ topk_scores) {
  __shared__ float cand_s[kNfmNW * kNfmCap];
  __shared__ int32_t cand_i[kNfmNW * kNfmCap];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t u = (int64_t)blockIdx.x * kNfmNW + w;
  if (u >= n_users) return;
  float* cs = cand_s + w * kNfmCap;
  int32_t* ci = cand_i + w * kNfmCap;
  int cnt = 0, kept = 0;
  float tau = kNegInf;
  for (int g = 0; g < n_seg; ++g)
    for (int x0 = 0; x0 < K; x0 += 64) {
      const int x = x0 + lane;
      float s = kNegInf;
      int32_t i = kIdxPad;
      if (x < K) {
        const size_t o = ((size_t)u * n_seg + g) * K + x;
        s = part_s[o];
        i = part_i[o];
      }
      nfm_append(cs, ci, lane, K, i != kIdxPad && s >= tau, s, i, nullptr, 0, 0, cnt, kept, tau);
    }
  nfm_prune(cs, ci, lane, K, nullptr, 0, 0, cnt, kept, tau);
  const float uc = user_const ? user_const[u] : 0.f;
  for (int x = lane; x < K; x += 64) {
    if (x < cnt) {
      const float s = cs[x];
      const int32_t i = ci[x];
      int rank = 0;
      for (int y = 0; y < cnt; ++y) rank += ranks_before(cs[y], ci[y], s, i) ? 1 : 0;
      topk_items[(size_t)u * K + rank] = i;
      // the per-user constant enters here, once per listed item
      if (topk_scores) topk_scores[(size_t)u * K + rank] = user_const ? s + uc : s;
    } else {
      topk_items[(size_t)u * K + x] = -1;
      if (topk_scores) topk_scores[(size_t)u * K + x] = kNegInf;
    }
  }
}

}  // namespace kgat
