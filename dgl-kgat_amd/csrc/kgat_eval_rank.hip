// The exact rank of every held-out item, at any depth, beside the top-K lists of kgat_eval.hip / kgat_eval_topk.hip
// (reference metric.py:36-68; the KGAT release's `auc` field).  DESIGN.md 21.
//
// For user u and a test entry at item position t, with s'(u,i) = 0.0f for a masked training item (metric.py:50) and
// score(u,i) otherwise, `above` = #{ candidates i != t that rank before t } under the order of kgat_eval_common.h
// (ranks_before: score descending, position ascending).  No candidate buffer, so no K:
//
//  1. eval_rank_slots: the users' test lists are cut into groups of kRankGroup thresholds; a group is a SLOT, the
//     column of a wavefront's MFMA.  A user with 300 test entries occupies 19 slots, one without entries none: every
//     lane of the sweep compares against at most kRankGroup thresholds whatever the lists' lengths are.
//     (slot counts -> exclusive scan -> slot_user; the grid is sized by the host's bound on the number of slots.)
//  2. eval_rank_pairs_kernel: score(u,i) of every (user, test item) and (user, training item) pair with the sweep's
//     bits: 32 pairs are the 32 rows and the 32 columns of one v_mfma_f32_32x32x2_f32 chain - the items' fragments read
//     from itemT, the users' rows from emb, the same k order and zero padding as the sweep - and the DIAGONAL of the
//     product is kept.  An output element of the MFMA depends on its own row and column alone, so the diagonal element
//     carries the bits the sweep gives that pair.  (31 of 32 products are thrown away: about 1 % of the sweep's MFMAs
//     for the test pairs, 4 % for the training pairs at the amazon-book shape.)
//  3. eval_rank_sweep_kernel: the tile walk of the top-K sweeps (kgat_eval_walk.h, included here as there: 32 columns
//     per wavefront, item tiles of 32, the register forms KG 6 / 11 / 16 / 22 and the LDS form) with counting in the
//     place of the candidate handling: a score becomes a 64-bit key (order-preserving score bits, then the position
//     descending), a threshold likewise, and `key > threshold` is ranks_before.  The sweep counts over ALL items with
//     their raw scores; item segments add into the zeroed output with integer atomics.
//  4. eval_rank_fix_kernel: one wavefront per user takes the training items out again (their raw scores from launch 2)
//     and, in mask mode, puts them back at 0.0f; in drop mode a test entry that is a training item gets -1.
//
// kgat_eval_rank_metrics: per user the distinct ranked entries are ordered by counting (place = #{smaller}), then
// every sum runs in ascending rank order in fp64 (the loads 64 at a time, the adds one after the other).  Integer counts and fixed summation orders: bitwise reproducible.
#include "kgat_eval_common.h"

namespace kgat {

constexpr int kRankGroup = 16;         // thresholds per slot
constexpr int kRankMaxKs = 64;         // cut-offs of kgat_eval_rank_metrics: one lane each

// (score, position) as an unsigned key: a ranks before b  <=>  key(a) > key(b).  s + 0 maps -0 to +0 (equal under the
// IEEE compare).  A NaN compares false with everything: as a score its key is below every threshold's, as a threshold
// above every score's.
__device__ __forceinline__ unsigned long long rank_key(float s, int pos) {
  return ((unsigned long long)ordered_bits(s + 0.f) << 32) | (unsigned)(kIdxPad - pos);
}
constexpr unsigned long long kRankNever = ~0ull;

// LDS per wavefront: the slots' thresholds [kRankGroup][32] keys, then (LDS form only) the users' rows [FP2][64]
__host__ __device__ constexpr size_t rank_lds_per_wave(int FP2, bool rows_in_registers) {
  return (size_t)kRankGroup * 32 * 8 + (rows_in_registers ? (size_t)0 : (size_t)FP2 * 64 * 4);
}

// ------------------------------------------------------------------------------------------------ slots
__global__ __launch_bounds__(256) void eval_rank_slot_count_kernel(int64_t n_users, const int32_t* __restrict__ test_ptr,
                                                                   int32_t* __restrict__ slot_base) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u > n_users) return;
  slot_base[u] = u < n_users ? (test_ptr[u + 1] - test_ptr[u] + kRankGroup - 1) / kRankGroup : 0;   // ([n_users]: the total)
}

__global__ __launch_bounds__(256) void eval_rank_slot_fill_kernel(int64_t n_users, const int32_t* __restrict__ slot_base,
                                                                  int64_t max_slots, int32_t* __restrict__ slot_user) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= n_users) return;
  for (int64_t s = slot_base[u]; s < slot_base[u + 1] && s < max_slots; ++s) slot_user[s] = (int32_t)u;
}

// ------------------------------------------------------------------------------------------------ pairs
// pair x < n_test: test entry x; beyond it training entry x - n_test.  One wavefront per 32 pairs.
__global__ __launch_bounds__(256) void eval_rank_pairs_kernel(
    int64_t n_users, const int32_t* __restrict__ user_ids, int64_t n_items, int FP2, int F, const float* __restrict__ emb,
    int64_t emb_stride, const float* __restrict__ itemT, const int32_t* __restrict__ train_ptr,
    const int32_t* __restrict__ train_items, const int32_t* __restrict__ test_ptr, const int32_t* __restrict__ test_items,
    int64_t n_test, int64_t n_train, int drop_train, int vec_rows, float* __restrict__ thr_s,
    float* __restrict__ train_s) {
  typedef float floatx4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63, p = lane & 31, half = lane >> 5;
  const int64_t x0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
  const int64_t n_pairs = n_test + n_train;
  if (x0 >= n_pairs) return;
  const bool ok = x0 + p < n_pairs;
  const int64_t x = ok ? x0 + p : n_pairs - 1;
  const bool is_test = x < n_test;
  const int32_t e = (int32_t)(is_test ? x : x - n_test);
  const int u = segment_of(is_test ? test_ptr : train_ptr, (int)n_users, e);
  const int32_t it = is_test ? test_items[e] : train_items[e];
  const float* row = emb + (size_t)user_ids[u] * emb_stride;
  // the item's fragment: itemT[tile][quad of k pairs][half][lane][4] (eval_items_kmajor_kernel)
  const floatx4* ap = reinterpret_cast<const floatx4*>(itemT) + ((size_t)(it >> 5) * (FP2 / 4)) * 64 + (half << 5 | (it & 31));
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  // four k pairs per step: the item's are one 16-byte load; the user's elements k = 8 sq + 2 c + half are picked from
  // the row's 32 bytes (two 16-byte loads) where the rows are 16-byte aligned (vec_rows) and the eight lie inside F
  auto load = [&](int sq, floatx4& a, float (&b)[4]) {
    a = ap[(size_t)sq * 64];
    if (vec_rows && 8 * sq + 8 <= F) {
      const floatx4 v0 = *reinterpret_cast<const floatx4*>(row + 8 * sq), v1 = *reinterpret_cast<const floatx4*>(row + 8 * sq + 4);
      b[0] = half ? v0[1] : v0[0];
      b[1] = half ? v0[3] : v0[2];
      b[2] = half ? v1[1] : v1[0];
      b[3] = half ? v1[3] : v1[2];
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int k = 2 * (4 * sq + c) + half;
        b[c] = k < F ? row[k] : 0.f;
      }
    }
  };
  floatx4 a0;
  float b0[4];
  load(0, a0, b0);
  const int n_sq = FP2 / 4;
  for (int sq = 0; sq < n_sq; ++sq) {   // (the next step's loads ahead of this step's MFMAs)
    floatx4 a1 = a0;
    float b1[4] = {0.f, 0.f, 0.f, 0.f};
    if (sq + 1 < n_sq) load(sq + 1, a1, b1);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[c], b0[c], acc, 0, 0, 0);
    a0 = a1;
#pragma unroll
    for (int c = 0; c < 4; ++c) b0[c] = b1[c];
  }
  // acc[r] of lane (p, half): row (r & 3) + 8 (r >> 2) + 4 half, column p.  The diagonal element of pair p sits in
  // the lane of half (p >> 2) & 1 at r = (p & 3) + 4 (p >> 3).
  if (!ok || half != ((p >> 2) & 1)) return;
  const int rd = (p & 3) | (p >> 3) << 2;
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) s = r == rd ? acc[r] : s;
  if (is_test) {
    // s'(u,t): a masked training item's 0.0f (metric.py:50) in mask mode
    if (!drop_train && in_sorted(train_items, train_ptr[u], train_ptr[u + 1], it)) s = 0.f;
    thr_s[e] = s;
  } else {
    train_s[e] = s;
  }
}

// A lane's 16 scores of a tile (acc[r]: item position ib + (r & 3) + 8 (r >> 2)) against the first GM thresholds of its
// slot (thr_ul[32 g]; the entries behind the slot's own are kRankNever).  Four scores at a time become keys; a threshold
// is read once per four (one ds_read_b64) and compared with them: a 64-bit compare and an add per (score, threshold).
// GM is a compile-time bound - straight-line code; the caller picks it from the most thresholds of the wavefront's slots.
template <int GM>
__device__ __forceinline__ void rank_count_tile(const floatx16& acc, int ib, const unsigned long long* thr_ul,
                                                int (&cnt)[kRankGroup]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned long long key[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int r = 4 * q + rr;
      const float sc = acc[r];
      const unsigned hi = sc == sc ? ordered_bits(sc + 0.f) : 0u;   // (a NaN never ranks before anything)
      key[rr] = ((unsigned long long)hi << 32) | (unsigned)(kIdxPad - (ib + (r & 3) + 8 * (r >> 2)));
    }
#pragma unroll
    for (int g = 0; g < GM; ++g) {
      const unsigned long long th = thr_ul[g * 32];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) cnt[g] += key[rr] > th ? 1 : 0;
    }
    // (one four at a time: left to itself the scheduler hoists every threshold read of the tile and spills)
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ------------------------------------------------------------------------------------------------ the counting sweep
// (WPE wavefronts per SIMD: two where the users' rows leave the registers for the counters and the keys - KG 6 and 11;
// KG 16 and 22 spilled at 256 registers)
template <int NW, int KG, int WPE>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void eval_rank_sweep_kernel(
    int64_t n_users, const int32_t* __restrict__ slot_base, const int32_t* __restrict__ slot_user,
    const int32_t* __restrict__ user_ids, int64_t n_items, int FP2, int F, EvalBounds bounds,
    const float* __restrict__ emb, int64_t emb_stride, const float* __restrict__ itemT,
    const int32_t* __restrict__ test_ptr, const int32_t* __restrict__ test_items, const float* __restrict__ thr_s,
    int32_t* __restrict__ above) {
  extern __shared__ __attribute__((aligned(16))) char s_raw[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ul = lane & 31, half = lane >> 5;
  constexpr int G = kRankGroup;
  char* base = s_raw + (size_t)w * rank_lds_per_wave(FP2, KG > 0);
  unsigned long long* thr = reinterpret_cast<unsigned long long*>(base);   // [G][32]
  float* ub = reinterpret_cast<float*>(base + G * 32 * 8);

  const int64_t n_slots = slot_base[n_users];
  const int64_t u0 = ((int64_t)blockIdx.x * NW + w) * 32;      // the wavefront's 32 slots
  const int seg = blockIdx.y;
  if (u0 >= n_slots) return;                                   // (no workgroup barrier anywhere below)
  const bool u_ok = u0 + ul < n_slots;
  const int64_t sl = u_ok ? u0 + ul : n_slots - 1;
  const int32_t up = slot_user[sl];                            // the slot's user (position in user_ids)
  // the slot's thresholds: entries [e_lo, e_lo + n_thr) of the test CSR
  const int32_t e_lo = test_ptr[up] + (int32_t)(sl - slot_base[up]) * G;
  const int n_thr = u_ok ? (test_ptr[up + 1] - e_lo < G ? test_ptr[up + 1] - e_lo : G) : 0;
  int gmax = n_thr;
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) {
    const int o = __shfl_xor(gmax, off, 64);
    gmax = o > gmax ? o : gmax;
  }
  gmax = __builtin_amdgcn_readfirstlane(gmax);                 // the most thresholds of a slot of this wavefront
  if (half == 0) {
    for (int g = 0; g < G; ++g) {
      unsigned long long key = kRankNever;
      if (g < n_thr) {
        const float s = thr_s[e_lo + g];
        if (s == s) key = rank_key(s, test_items[e_lo + g]);
      }
      thr[g * 32 + ul] = key;
    }
  }
  const float* row = emb + (size_t)user_ids[up] * emb_stride;
#define KGAT_EVAL_WALK_PART 1
#include "kgat_eval_walk.h"   // REG, NT, U; breg[] / ub[] from `row`
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();

  const int64_t t_lo = bounds.b[seg], t_hi = bounds.b[seg + 1];
  int cnt[G];   // entries that rank before threshold g among this lane's scores
#pragma unroll
  for (int g = 0; g < G; ++g) cnt[g] = 0;

#define KGAT_EVAL_WALK_PART 2
#include "kgat_eval_walk.h"   // acc[NT] (acc[t][r]: slot ul), nan_padded_tail
  auto check = [&](int64_t t0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t0 + t >= t_hi) break;  // wave-uniform
      const int ib = (int)((t0 + t) * kEvalTile) + 4 * half;
      nan_padded_tail(t, t0 + t, ib);   // (never counted)
      if (gmax <= 4) rank_count_tile<4>(acc[t], ib, thr + ul, cnt);          // (wave-uniform)
      else if (gmax <= 8) rank_count_tile<8>(acc[t], ib, thr + ul, cnt);
      else if (gmax <= 12) rank_count_tile<12>(acc[t], ib, thr + ul, cnt);
      else rank_count_tile<kRankGroup>(acc[t], ib, thr + ul, cnt);
    }
  };
#define KGAT_EVAL_WALK_PART 3
#include "kgat_eval_walk.h"   // the walk over tiles [t_lo, t_hi): check(t0) after a tile group's last MFMA
  // the two halves of a slot hold different items of every tile: their sum is the segment's count
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int c = cnt[g] + __shfl_xor(cnt[g], 32, 64);
    if (half == 0 && g < n_thr && c != 0) atomicAdd(above + e_lo + g, c);
  }
}

// ------------------------------------------------------------------------------------------------ training items
// One wavefront per user.  The sweep counted every item with its raw score; a training item is no candidate (drop) or a
// candidate at 0.0f (mask).
__global__ __launch_bounds__(256) void eval_rank_fix_kernel(
    int64_t n_users, const int32_t* __restrict__ train_ptr, const int32_t* __restrict__ train_items,
    const float* __restrict__ train_s, const int32_t* __restrict__ test_ptr, const int32_t* __restrict__ test_items,
    const float* __restrict__ thr_s, int drop_train, int32_t* __restrict__ above) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;
  const int32_t tr_lo = train_ptr[u], tr_hi = train_ptr[u + 1];
  const int32_t te_lo = test_ptr[u], te_hi = test_ptr[u + 1];
  if (tr_lo == tr_hi) return;
  for (int32_t e = te_lo; e < te_hi; ++e) {
    const int32_t t = test_items[e];
    const float st = thr_s[e];
    if (drop_train && in_sorted(train_items, tr_lo, tr_hi, t)) {   // (wave-uniform) never ranked
      if (lane == 0) above[e] = -1;
      continue;
    }
    int d = 0;
    for (int32_t j = tr_lo + lane; j < tr_hi; j += 64) {
      const int32_t i = train_items[j];
      d -= ranks_before(train_s[j], i, st, t) ? 1 : 0;
      if (!drop_train) d += ranks_before(0.f, i, st, t) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
    if (lane == 0 && d != 0) above[e] += d;
  }
}

// ------------------------------------------------------------------------------------------------ metrics
struct RankKs { int32_t k[kRankMaxKs]; };

__device__ __forceinline__ double readlane_f64(double v, int l) {   // l wave-uniform
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// One wavefront per user, three passes over the user's entries 64 at a time:
//  1. the distinct ranked entries (test positions ascend: a duplicate follows its twin; -1 is not ranked) are compacted
//     into comp[] in list order;
//  2. each is placed in ascending rank order by counting - ranks of distinct items differ, so place = #{smaller} -
//     into srt[] (T^2 / 64 compares per lane, the entries read 64 per load: no bound on T);
//  3. the sums.  The loads (disc[a], the quotients of ap) are made 64 at a time in parallel, the ADDS run in ascending
//     rank order: the lanes walk the 64 values through v_readlane, lane j adding those below its cut-off ks[j].
__global__ __launch_bounds__(256) void eval_rank_metrics_kernel(
    int64_t n_users, const int32_t* __restrict__ above, const int32_t* __restrict__ test_ptr,
    const int32_t* __restrict__ test_items, const int32_t* __restrict__ n_candidates, int n_ks, RankKs ks,
    const double* __restrict__ disc, int32_t* comp_all, int32_t* srt_all, double* __restrict__ out_at_k,
    double* __restrict__ out_scalar) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n_users) return;
  const int32_t lo = test_ptr[u], hi = test_ptr[u + 1];
  int32_t* comp = comp_all + lo;
  int32_t* srt = srt_all + lo;
  int T = 0;
  for (int32_t e0 = lo; e0 < hi; e0 += 64) {
    const int32_t e = e0 + lane;
    int32_t a = -1;
    if (e < hi && (e == lo || test_items[e] != test_items[e - 1])) a = above[e];
    const unsigned long long m = __ballot(a >= 0);
    if (a >= 0) comp[T + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = a;
    T += (int)__popcll(m);
  }
  // (the other lanes' stores, through global memory.  Workgroup scope: writer and reader are one wavefront, on one
  //  CU's L1; at agent scope the release writes the whole L2 back - measured 0.85 ms per fence over 70,679 users)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  for (int i0 = 0; i0 < T; i0 += 64) {
    const int i = i0 + lane;
    const int32_t a = i < T ? comp[i] : 0;
    int place = 0;
    for (int f0 = 0; f0 < T; f0 += 64) {   // (64 entries per load, walked through v_readlane: a load per compare is a
      //                                       round trip to memory per compare, milliseconds on a list of hundreds)
      const int32_t c = f0 + lane < T ? comp[f0 + lane] : 0;
      const int n = T - f0 < 64 ? T - f0 : 64;
      for (int l = 0; l < n; ++l) place += __builtin_amdgcn_readlane(c, l) < a ? 1 : 0;
    }
    if (i < T) srt[place] = a;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  // srt[0] < ... < srt[T - 1]: the 0-based ranks
  const int k_max = ks.k[n_ks - 1];
  const int kj = lane < n_ks ? ks.k[lane] : 0;   // (a lane without a cut-off: nothing is below it)
  int nh = 0;
  double dcg = 0.0, ideal = 0.0, ap = 0.0;
  long long gap = 0, ranks = 0;
  for (int c0 = 0; c0 < T; c0 += 64) {
    const int i = c0 + lane;
    const bool ok = i < T;
    const int32_t x = ok ? srt[i] : kIdxPad;
    const double d = x < k_max ? disc[x] : 0.0;
    const double term = ok ? (double)(i + 1) / (double)(x + 1) : 0.0;
    gap += ok ? x - i : 0;
    ranks += ok ? x + 1 : 0;
    const int n = T - c0 < 64 ? T - c0 : 64;
    for (int l = 0; l < n; ++l) {   // ascending rank order
      const int32_t xl = __builtin_amdgcn_readlane(x, l);
      const double dl = readlane_f64(d, l);
      if (xl < kj) { dcg += dl; ++nh; }
      ap += readlane_f64(term, l);
    }
  }
  int nh_max = nh;   // the ideal DCG: disc[0 .. nh) in ascending order, per cut-off
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(nh_max, off, 64);
    nh_max = o > nh_max ? o : nh_max;
    gap += __shfl_xor(gap, off, 64);
    ranks += __shfl_xor(ranks, off, 64);
  }
  nh_max = __builtin_amdgcn_readfirstlane(nh_max);
  for (int c0 = 0; c0 < nh_max; c0 += 64) {
    const int i = c0 + lane;
    const double d = i < nh_max ? disc[i] : 0.0;   // (nh_max <= k_max)
    const int n = nh_max - c0 < 64 ? nh_max - c0 : 64;
    for (int l = 0; l < n; ++l) {
      const double dl = readlane_f64(d, l);
      if (c0 + l < nh) ideal += dl;
    }
  }
  if (lane < n_ks) {
    const int n_pos = hi - lo;
    double* o = out_at_k + ((size_t)u * n_ks + lane) * 4;
    o[0] = n_pos > 0 ? (double)nh / (double)n_pos : 0.0;
    o[1] = ideal > 0.0 ? dcg / ideal : 0.0;
    o[2] = (double)nh / (double)kj;
    o[3] = nh > 0 ? 1.0 : 0.0;
  }
  if (lane == 0) {
    const long long C = n_candidates[u];
    double* o = out_scalar + (size_t)u * 4;
    o[0] = T > 0 ? 1.0 / (double)(srt[0] + 1) : 0.0;
    o[1] = T > 0 ? ap / (double)T : 0.0;
    o[2] = (T > 0 && C > T) ? 1.0 - (double)gap / ((double)T * (double)(C - T)) : 0.0;
    o[3] = T > 0 ? (double)ranks / (double)T : 0.0;
  }
}

// the host's bound on the number of slots: sum of ceil(T_u / G) <= n_users + n_test / G, and <= n_test
static int64_t rank_max_slots(int64_t n_users, int64_t n_test) {
  const int64_t a = n_users + n_test / kRankGroup;
  return a < n_test ? a : n_test;
}

static EvalPlanH rank_plan(int64_t max_slots, int64_t n_items, int F) { return eval_plan(max_slots, n_items, F); }

}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_eval_rank_supported(int F) { return F >= 1 && eval_waves_per_block(F) > 0; }

size_t kgat_eval_rank_workspace_bytes(int64_t n_users, int64_t n_items, int F, int64_t n_train, int64_t n_test) {
  if (n_users <= 0 || n_items <= 0 || n_train < 0 || n_test <= 0 || !kgat_eval_rank_supported(F)) return 256;
  return align_up((size_t)(n_users + 1) * 4, 256) + align_up(scan_workspace_elems(n_users + 1) * 4, 256) +
         align_up((size_t)rank_max_slots(n_users, n_test) * 4, 256) + align_up((size_t)n_test * 4, 256) +
         align_up((size_t)n_train * 4, 256) + 256;
}

int kgat_eval_rank_f32(int64_t n_users, const int32_t* user_ids, int64_t n_items, int F, const float* emb,
                       int64_t emb_stride, const float* itemT, const int32_t* train_ptr, const int32_t* train_items,
                       int64_t n_train, const int32_t* test_ptr, const int32_t* test_items, int64_t n_test,
                       int drop_train, void* workspace, size_t workspace_bytes, int32_t* above, float* target_score,
                       kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_users >= 0 && n_items >= 0 && F >= 1 && emb_stride >= F && n_train >= 0 && n_test >= 0,
                 "eval_rank: bad sizes");
  KGAT_CHECK_ARG(n_users < INT32_MAX && n_items < INT32_MAX && n_train < INT32_MAX && n_test < INT32_MAX &&
                     n_train + n_test < INT32_MAX, "eval_rank: more than 2^31 users, items or pairs");
  if (!kgat_eval_rank_supported(F)) {
    set_error("eval_rank: F = %d not supported", F);
    return KGAT_E_UNSUPPORTED;
  }
  if (n_users == 0 || n_test == 0) return KGAT_OK;
  KGAT_CHECK_ARG(n_items >= 1, "eval_rank: no items to rank");
  KGAT_CHECK_ARG(user_ids && emb && itemT && train_ptr && test_ptr && test_items && above && workspace,
                 "eval_rank: null pointer");
  KGAT_CHECK_ARG(n_train == 0 || train_items, "eval_rank: null pointer");
  if (workspace_bytes < kgat_eval_rank_workspace_bytes(n_users, n_items, F, n_train, n_test)) {
    set_error("eval_rank: workspace too small");
    return KGAT_E_WORKSPACE;
  }
  const int64_t max_slots = rank_max_slots(n_users, n_test);
  const EvalPlanH pl = rank_plan(max_slots, n_items, F);
  const int FP2 = eval_fp2(F), kg = eval_reg_kg(F);
  KGAT_RETURN_IF(eval_check_segments("eval_rank", pl, FP2));
  Carver cv(workspace);
  int32_t* slot_base = cv.take<int32_t>((size_t)n_users + 1);
  int32_t* scan_ws = cv.take<int32_t>(scan_workspace_elems(n_users + 1));
  int32_t* slot_user = cv.take<int32_t>((size_t)max_slots);
  float* thr_ws = cv.take<float>((size_t)n_test);
  float* train_s = cv.take<float>((size_t)n_train);
  float* thr_s = target_score ? target_score : thr_ws;
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(above, 0, (size_t)n_test * 4, st) != hipSuccess) {
    set_error("eval_rank: cannot clear the counters");
    return KGAT_E_HIP;
  }
  const unsigned ub = (unsigned)((n_users + 1 + 255) / 256);
  hipLaunchKernelGGL(eval_rank_slot_count_kernel, dim3(ub), dim3(256), 0, st, n_users, test_ptr, slot_base);
  KGAT_CHECK_LAUNCH("eval_rank_slot_count");
  const int rc = exclusive_scan_i32(slot_base, n_users + 1, scan_ws, st);
  if (rc != KGAT_OK) return rc;
  hipLaunchKernelGGL(eval_rank_slot_fill_kernel, dim3(ub), dim3(256), 0, st, n_users, (const int32_t*)slot_base,
                     max_slots, slot_user);
  KGAT_CHECK_LAUNCH("eval_rank_slot_fill");
  const int64_t n_pairs = n_test + n_train;
  hipLaunchKernelGGL(eval_rank_pairs_kernel, dim3((unsigned)((n_pairs + 127) / 128)), dim3(256), 0, st, n_users, user_ids,
                     n_items, FP2, F, emb, emb_stride, itemT, train_ptr, train_items, test_ptr, test_items, n_test, n_train,
                     drop_train, ((emb_stride & 3) == 0 && aligned16(emb)) ? 1 : 0, thr_s, train_s);
  KGAT_CHECK_LAUNCH("eval_rank_pairs");
  // (WPE: two wavefronts per SIMD where the registers allow - see eval_rank_sweep_kernel)
  const auto kernel = eval_with_form<4>(kg, pl.nw, [](auto NW, auto KG) {
    return &eval_rank_sweep_kernel<NW(), KG(), (KG() == 16 || KG() == 22) ? 1 : 2>;
  });
  KGAT_RETURN_IF(eval_launch_sweep("eval_rank", kernel, max_slots, pl, rank_lds_per_wave(FP2, kg > 0), st, n_users,
                                   (const int32_t*)slot_base, (const int32_t*)slot_user, user_ids, n_items, FP2, F,
                                   pl.bounds, emb, emb_stride, itemT, test_ptr, test_items, (const float*)thr_s, above));
  KGAT_CHECK_LAUNCH("eval_rank_sweep");
  if (n_train > 0) {
    hipLaunchKernelGGL(eval_rank_fix_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, st, n_users, train_ptr,
                       train_items, (const float*)train_s, test_ptr, test_items, (const float*)thr_s, drop_train, above);
    KGAT_CHECK_LAUNCH("eval_rank_fix");
  }
  return KGAT_OK;
}

size_t kgat_eval_rank_metrics_workspace_bytes(int64_t n_test) {
  return 2 * align_up((size_t)(n_test > 0 ? n_test : 0) * 4, 256) + 256;   // comp[], srt[]
}

int kgat_eval_rank_metrics(int64_t n_users, int64_t n_items, const int32_t* above, const int32_t* test_ptr,
                           const int32_t* test_items, int64_t n_test, const int32_t* n_candidates, int n_ks,
                           const int32_t* ks, const double* disc, void* workspace, size_t workspace_bytes,
                           double* out_at_k, double* out_scalar, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_users >= 0 && n_items >= 0 && n_test >= 0 && n_test < INT32_MAX, "eval_rank_metrics: bad sizes");
  KGAT_CHECK_ARG(n_ks >= 1 && n_ks <= kRankMaxKs && ks, "eval_rank_metrics: 1..%d cut-offs", kRankMaxKs);
  RankKs kv = {};
  for (int j = 0; j < n_ks; ++j) {
    KGAT_CHECK_ARG(ks[j] >= 1 && ks[j] <= n_items && (j == 0 || ks[j] > ks[j - 1]),
                   "eval_rank_metrics: the cut-offs must ascend within 1..n_items (cut-off %d is %d, n_items = %lld)", j,
                   ks[j], (long long)n_items);
    kv.k[j] = ks[j];
  }
  if (n_users == 0) return KGAT_OK;
  KGAT_CHECK_ARG(test_ptr && n_candidates && disc && out_at_k && out_scalar && workspace,
                 "eval_rank_metrics: null pointer");
  KGAT_CHECK_ARG(n_test == 0 || (above && test_items), "eval_rank_metrics: null pointer");
  if (workspace_bytes < kgat_eval_rank_metrics_workspace_bytes(n_test)) {
    set_error("eval_rank_metrics: workspace too small");
    return KGAT_E_WORKSPACE;
  }
  Carver cv(workspace);
  int32_t* comp = cv.take<int32_t>((size_t)n_test);
  int32_t* srt = cv.take<int32_t>((size_t)n_test);
  hipLaunchKernelGGL(eval_rank_metrics_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, as_stream(stream),
                     n_users, above, test_ptr, test_items, n_candidates, n_ks, kv, disc, comp, srt, out_at_k, out_scalar);
  KGAT_CHECK_LAUNCH("eval_rank_metrics");
  return KGAT_OK;
}

}  // extern "C"
