  // The body of the sweep kernels (included inside eval_topk_kernel of kgat_eval.hip and eval_topk_wide_kernel of
  // kgat_eval_topk.hip, which declare the arguments and `constexpr int CAP`: the candidate entries per user, with
  // CAP - K >= 24): the candidate buffer, its prune, the shared threshold and the list write-out around the tile walk
  // of kgat_eval_walk.h.  Shared as text, not through a template parameter: the K <= 32 instantiations keep the
  // registers and the code they had.
  constexpr int EPL = CAP <= 64 ? 1 : (CAP <= 128 ? 2 : 4);   // entries per lane of the pruning wavefront (64 EPL >= CAP)
  static_assert(CAP <= 256, "at most four entries per lane");
  extern __shared__ __attribute__((aligned(16))) char s_raw[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ul = lane & 31, half = lane >> 5;
  char* base = s_raw + (size_t)w * EvalLds::per_wave_bytes(FP2, KG > 0, CAP);
  float* cand_s = reinterpret_cast<float*>(base);
  int32_t* cand_i = reinterpret_cast<int32_t*>(base + 32 * CAP * 4);
  int32_t* kept = reinterpret_cast<int32_t*>(base + 32 * CAP * 8);  // entries known not to be training items
  float* ub = reinterpret_cast<float*>(base + 32 * CAP * 8 + 256);

  const int64_t u0 = ((int64_t)blockIdx.x * NW + w) * 32;      // the wavefront's 32 users (positions in user_ids)
  const int seg = blockIdx.y;
  if (u0 >= n_users) return;                                   // (no workgroup barrier anywhere below)
  const int64_t up = u0 + ul;
  const bool u_ok = up < n_users;
  const int64_t up_c = u_ok ? up : n_users - 1;
  const float* row = emb + (size_t)user_ids[up_c] * emb_stride;
#define KGAT_EVAL_WALK_PART 1
#include "kgat_eval_walk.h"   // REG, NT, U; breg[] / ub[] from `row`
  if (lane < 32) kept[lane] = 0;
  const int32_t tr_lo = train_ptr[up_c], tr_hi = train_ptr[up_c + 1];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();

  // The segment's tiles (bounds, from the host's plan).  Workgroups are dispatched x-fastest: one segment row (all user
  // blocks) after the other, so the segments of a user block mostly run one after the other and a later one starts
  // from the K-th best the earlier ones have published (tau_shared below; any published value is a valid bound).
  // (Rounds 5-6 seeded the thresholds with a sample sweep over the first 512 items - first a launch of its own, 0.9 ms of
  // candidate handling with almost no MFMAs, then segment 0 of this grid; with the shared threshold it measures the same
  // with and without, 500 ... 300,000 users: profiles/r06_eval_scan.txt - and it is gone.)
  const int n_lists = gridDim.y;
  const int64_t t_lo = bounds.b[seg], t_hi = bounds.b[seg + 1];
  // the user's K-th best score so far: -inf while fewer than K are held (+inf on a lane without a user: nothing passes)
  float tau_s = u_ok ? kNegInf : __builtin_inff();
  // A user's buffer of CAP entries is filled from BOTH ends: the lane of half 0 appends upwards from position 0,
  // the lane of half 1 downwards from CAP - 1 - no coordination between the two per append (round 6: it was one
  // counter per user, a ballot per register and 64-bit shifts to order the two lanes behind each other: about twenty
  // vector instructions per register of a tile, all of them taken from the other wavefront's MFMAs).  wp = the lane's
  // next free entry (index into cand_s / cand_i).
  int wp = ul * CAP + (half ? CAP - 1 : 0);
  const int dir = half ? -1 : 1;
  // Round 6: the segments of a user's item range run side by side (one wavefront each), every one warming up its own
  // K-th best: they now SHARE it.  tau_shared[user] holds the best K-th score any segment has published (atomicMax on
  // order-preserving bits; zero-filled = below every float): K entries of some segment rank at or before it, so
  // nothing that scores below it can be among the user's K best - a valid bound whenever it is read, however stale.
  // A wavefront takes it over when it beats its own (ties on the score stay candidates: position "pad"), reads it
  // once per tile group - requested at the end of a check, used by the next - and publishes after every prune.  The
  // result is the exact top K either way; fewer candidates are appended and pruned on the way.
  float sh_next = kNegInf;
  if (tau_shared != nullptr)
    sh_next = from_ordered_bits(__hip_atomic_load(tau_shared + up_c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  auto adopt_shared = [&]() {
    if (sh_next > tau_s) tau_s = sh_next;   // (ties on the score stay candidates: the filter is >=)
  };

  // Keep the K best entries of user `v` (wave-uniform), dropping training items among the new ones.  The K-th best
  // key is SELECTED, not ranked: a bisection over the 32 bits of the scores' order-preserving form - per bit one vector
  // compare against a scalar and a scalar population count - instead of one broadcast + compare + add per entry and
  // lane (round 6: the rank count was three quarters of a prune's vector instructions, and on this chip every vector
  // instruction of this wavefront is taken from the other wavefront's fp32 MFMAs; scalar instructions are not).  Entries
  // that tie with the K-th score are taken in position order (a second bisection over the positions, only when the tie
  // straddles the cut).  The survivors are compacted to the low end of the buffer in lane order - not sorted: the order
  // is total, so the SET is what matters; the merge launch sorts.
  auto prune = [&](int v) {
    if constexpr (EPL == 1) {
      // (one entry per lane, as it was written for it: the K <= 32 kernels keep their code)
      const int base = v * CAP, kp = kept[v];
      // entries [0, p_lo) and (p_hi, CAP) of the buffer are in use (p_lo <= p_hi + 1)
      const int p_lo = __builtin_amdgcn_readlane(wp, v) - base, p_hi = __builtin_amdgcn_readlane(wp, v + 32) - base;
      const bool have = lane < p_lo || lane > p_hi;
      float s = kNegInf;
      int i = kIdxPad;
      if (have) { s = cand_s[base + lane]; i = cand_i[base + lane]; }
      const int32_t lo = __builtin_amdgcn_readlane(tr_lo, v), hi = __builtin_amdgcn_readlane(tr_hi, v);
      if (lane >= kp && have && in_sorted(train_items, lo, hi, i)) { s = kNegInf; i = kIdxPad; }
      const bool valid = i != kIdxPad;
      // the score as an unsigned key of the same order (s + 0 maps -0 to +0, equal for the reference's compare); 0 - below
      // the key of every float - for a lane without an entry
      const unsigned key = valid ? ordered_bits(s + 0.f) : 0u;
      const int n_valid = __popcll(__ballot(valid));
      const int keep = n_valid < K ? n_valid : K;
      unsigned T = 0u;   // the keep-th largest key: the largest T with at least `keep` keys >= T
      if (keep > 0) {
        for (int bit = 31; bit >= 0; --bit) {
          const unsigned c = T | (1u << bit);
          if ((int)__popcll(__ballot(key >= c)) >= keep) T = c;
        }
      }
      const bool above = keep > 0 && key > T, tied = keep > 0 && key == T;   // (T > 0: an empty lane is neither)
      const int need_tied = keep - (int)__popcll(__ballot(above));                // >= 1 when keep > 0
      bool sel = above || tied;
      if ((int)__popcll(__ballot(tied)) > need_tied) {
        // the need_tied lowest positions among the tied entries: I = the need_tied-th smallest of them (positions are
        // distinct), found as the largest I with fewer than need_tied tied positions below it
        int I = 0;
        for (int bit = 30; bit >= 0; --bit) {
          const int c = I | (1 << bit);
          if ((int)__popcll(__ballot(tied && i < c)) < need_tied) I = c;
        }
        sel = above || (tied && i <= I);
      }
      const unsigned long long sel_mask = __ballot(sel);
      const int pos = __builtin_amdgcn_mbcnt_hi((unsigned)(sel_mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)sel_mask, 0u));
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();                        // every lane has read its entry
      if (sel) { cand_s[base + pos] = s; cand_i[base + pos] = i; }
      const float ts = from_ordered_bits(T);                  // the K-th best score when keep == K
      if (ul == v) {  // both lanes of the user
        // (never below what is already known: a shared bound may be ahead of this segment's own K-th best)
        if (keep == K && ts > tau_s) tau_s = ts;
        wp = base + (half ? CAP - 1 : keep);
      }
      if (lane == 0) {
        kept[v] = keep;
        if (keep == K && tau_shared != nullptr) atomicMax(tau_shared + (u0 + v), T);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    } else {
      // (the same selection over EPL entries per lane: the bisections count on summed ballots, the compaction takes a
      //  prefix over the lane's entries)
      const int base = v * CAP, kp = kept[v];
      // entries [0, p_lo) and (p_hi, CAP) of the buffer are in use (p_lo <= p_hi + 1); a lane holds entries lane + 64 e
      const int p_lo = __builtin_amdgcn_readlane(wp, v) - base, p_hi = __builtin_amdgcn_readlane(wp, v + 32) - base;
      const int32_t lo = __builtin_amdgcn_readlane(tr_lo, v), hi = __builtin_amdgcn_readlane(tr_hi, v);
      float s[EPL];
      int i[EPL];
      unsigned key[EPL];
      int n_valid = 0;
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const int x = lane + 64 * e;
        const bool have = x < CAP && (x < p_lo || x > p_hi);
        s[e] = kNegInf;
        i[e] = kIdxPad;
        if (have) { s[e] = cand_s[base + x]; i[e] = cand_i[base + x]; }
        if (x >= kp && have && in_sorted(train_items, lo, hi, i[e])) { s[e] = kNegInf; i[e] = kIdxPad; }
        const bool valid = i[e] != kIdxPad;
        // the score as an unsigned key of the same order (s + 0 maps -0 to +0, equal for the reference's compare); 0 -
        // below the key of every float - for an entry that is not there
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
        // the need_tied lowest positions among the tied entries: I = the need_tied-th smallest of them (positions are
        // distinct), found as the largest I with fewer than need_tied tied positions below it
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
      // the survivors' places: a prefix over the lane's entries, then over the lanes
      int pos[EPL], n_before = 0;
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const unsigned long long sel_mask = __ballot(sel[e]);
        pos[e] = n_before + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(sel_mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)sel_mask, 0u));
        n_before += (int)__popcll(sel_mask);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();                        // every lane has read its entries
#pragma unroll
      for (int e = 0; e < EPL; ++e)
        if (sel[e]) { cand_s[base + pos[e]] = s[e]; cand_i[base + pos[e]] = i[e]; }
      const float ts = from_ordered_bits(T);                  // the K-th best score when keep == K
      if (ul == v) {  // both lanes of the user
        // (never below what is already known: a shared bound may be ahead of this segment's own K-th best)
        if (keep == K && ts > tau_s) tau_s = ts;
        wp = base + (half ? CAP - 1 : keep);
      }
      if (lane == 0) {
        kept[v] = keep;
        if (keep == K && tau_shared != nullptr) atomicMax(tau_shared + (u0 + v), T);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  };

#define KGAT_EVAL_WALK_PART 2
#include "kgat_eval_walk.h"   // acc[NT] (acc[t][r]: user ul), nan_padded_tail
  auto check = [&](int64_t t0) {
    adopt_shared();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t0 + t >= t_hi) break;  // wave-uniform
      const int ib = (int)((t0 + t) * kEvalTile) + 4 * half;
      nan_padded_tail(t, t0 + t, ib);   // (never a candidate)
      // the maximum of every four registers, then of all sixteen: a tile without a candidate costs the ten maxima and one
      // compare, a tile with one walks only the quads that hold it
      float mq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        mq[q] = fmaxf(fmaxf(acc[t][4 * q], acc[t][4 * q + 1]), fmaxf(acc[t][4 * q + 2], acc[t][4 * q + 3]));
      const float m = fmaxf(fmaxf(mq[0], mq[1]), fmaxf(mq[2], mq[3]));
      if (__ballot(m >= tau_s) != 0ull) {
        // every score at or above the user's K-th best so far is appended (a tie on the score with a later position is
        // sorted out by the prune: the order there is total); after every four registers - at most four entries from
        // either end - a buffer with fewer than eight free entries is pruned
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (__ballot(mq[q] >= tau_s) == 0ull) continue;   // wave-uniform
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int r = 4 * q + rr;
            const float sc = acc[t][r];
            if (sc >= tau_s) {
              cand_s[wp] = sc;
              cand_i[wp] = ib + (r & 3) + 8 * (r >> 2);
              wp += dir;
            }
          }
          // both lanes of a user see both write positions: v_permlane32_swap hands every lane the lower half's value
          // and the upper half's
          const auto both = __builtin_amdgcn_permlane32_swap((unsigned)wp, (unsigned)wp, false, false);
          unsigned long long need = __ballot((int)both[1] - (int)both[0] + 1 < 8);
          if (need) {
            need &= 0xffffffffull;   // (one bit per user)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            do {
              const int v = __builtin_ctzll(need);
              need &= need - 1;
              prune(v);
            } while (need);
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
    if (tau_shared != nullptr)   // for the next tile group's check (an L2 round trip behind that group's MFMAs)
      sh_next = from_ordered_bits(__hip_atomic_load(tau_shared + up_c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));   // (past the L1)
  };
#define KGAT_EVAL_WALK_PART 3
#include "kgat_eval_walk.h"   // the walk over tiles [t_lo, t_hi): check(t0) after a tile group's last MFMA
  // the segment's list of every user: K entries, padded with (-inf, pad)
  for (int v = 0; v < 32; ++v) {
    if (u0 + v >= n_users) break;
    prune(v);
    const int n = __builtin_amdgcn_readlane(wp, v) - v * CAP;   // (the kept entries, at the low end)
    if constexpr (EPL == 1) {
      if (lane < K) {
        const size_t o = ((size_t)(u0 + v) * n_lists + seg) * K + lane;
        part_s[o] = lane < n ? cand_s[v * CAP + lane] : kNegInf;
        part_i[o] = lane < n ? cand_i[v * CAP + lane] : kIdxPad;
      }
    } else {
      for (int x = lane; x < K; x += 64) {
        const size_t o = ((size_t)(u0 + v) * n_lists + seg) * K + x;
        part_s[o] = x < n ? cand_s[v * CAP + x] : kNegInf;
        part_i[o] = x < n ? cand_i[v * CAP + x] : kIdxPad;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
