// One-workgroup stable sort in LDS, shared by the TransR step's sorts (kgat_transr.hip) and the BPR gradient's slice
// sort (kgat_bpr.hip).
#pragma once
#include "kgat_common.h"

namespace kgat {

constexpr int kLdsSortWaves = 16;
constexpr int kLdsSortThreads = kLdsSortWaves * kWave;   // the block size of every kernel that sorts with LdsSort

// Stable LSD radix sort of n <= CAP values packed as key << POS_BITS | position in the input (PT: uint32_t or uint64_t),
// DIGIT_BITS per pass, both buffers and the counters in LDS: each of the 16 wavefronts owns a contiguous slice of the
// current order and its own column of the 2^DIGIT_BITS x 16 counter table, counts its digits (LDS atomics - counts do
// not depend on order), a block scan turns the table into offsets in (digit, wavefront) order, and the wavefront walks
// its slice 64 keys at a time ranking equal digits by lane with ballots - so equal keys keep their order.
// Use: a kernel of kLdsSortThreads threads declares one `__shared__ LdsSort<...>`, every thread fills buf[0][0 .. n)
// (no barrier needed: sort() begins with one), all threads call sort(), and read the result after it.
template <typename PT, int CAP, int DIGIT_BITS, int POS_BITS>
struct LdsSort {
  static constexpr int kDigits = 1 << DIGIT_BITS;
  alignas(16) PT buf[2][CAP];
  alignas(16) int32_t cnt[kDigits * kLdsSortWaves];   // (16 bytes: the scan reads a thread's counters as one piece)
  int32_t wsum[kLdsSortWaves];   // the scan's wavefront totals; the caller's to reuse after sort()

  // the buffer that sort() did not return: free once the caller has read what it needs from the sorted one
  __device__ __forceinline__ PT* other(const PT* sorted) { return buf[sorted == buf[0] ? 1 : 0]; }

  // ceil(key_bits / DIGIT_BITS) passes, at least one; returns the sorted buffer (all threads may read it on return)
  __device__ __forceinline__ const PT* sort(int32_t n, int key_bits) {
    constexpr int CPT = kDigits * kLdsSortWaves / kLdsSortThreads;   // counters per thread in the scan
    const int tid = threadIdx.x, lane = tid % kWave, w = tid / kWave;
    const int32_t slice = ((n + kLdsSortThreads - 1) / kLdsSortThreads) * kWave;  // per wavefront, a multiple of 64
    const int32_t lo = w * slice, hi = lo + slice < n ? lo + slice : n;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    int cur = 0;
    const int passes = (key_bits + DIGIT_BITS - 1) / DIGIT_BITS > 0 ? (key_bits + DIGIT_BITS - 1) / DIGIT_BITS : 1;
    for (int pass = 0; pass < passes; ++pass) {
      const int shift = POS_BITS + DIGIT_BITS * pass;
      for (int i = tid; i < kDigits * kLdsSortWaves; i += kLdsSortThreads) cnt[i] = 0;
      __syncthreads();
      for (int32_t i = lo + lane; i < hi; i += kWave)
        atomicAdd(&cnt[(uint32_t)((buf[cur][i] >> shift) & (PT)(kDigits - 1)) * kLdsSortWaves + w], 1);
      __syncthreads();
      {  // exclusive scan of the counters in (digit, wavefront) order, CPT per thread
        int32_t c[CPT];
        int32_t mine = 0;
#pragma unroll
        for (int q = 0; q < CPT; ++q) { c[q] = cnt[CPT * tid + q]; mine += c[q]; }
        int32_t inc = mine;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
          const int32_t up = __shfl_up(inc, d, kWave);
          if (lane >= d) inc += up;
        }
        if (lane == kWave - 1) wsum[w] = inc;
        __syncthreads();
        int32_t base = inc - mine;
        for (int q = 0; q < w; ++q) base += wsum[q];
#pragma unroll
        for (int q = 0; q < CPT; ++q) {
          cnt[CPT * tid + q] = base;
          base += c[q];
        }
      }
      __syncthreads();
      for (int32_t i0 = lo; i0 < hi; i0 += kWave) {
        const int32_t i = i0 + lane;
        const bool valid = i < hi;
        const PT v = valid ? buf[cur][i] : (PT)0;
        const uint32_t dgt = (uint32_t)((v >> shift) & (PT)(kDigits - 1));
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < DIGIT_BITS; ++bit) {
          const bool on = (dgt >> bit) & 1u;
          const uint64_t bal = __ballot(on);
          peers &= on ? bal : ~bal;
        }
        const int rank = __popcll(peers & lt_mask);
        const int32_t basep = valid ? cnt[dgt * kLdsSortWaves + w] : 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();  // every lane has its base before a leader moves it
        if (valid) {
          buf[cur ^ 1][basep + rank] = v;
          if (rank == 0) cnt[dgt * kLdsSortWaves + w] = basep + __popcll(peers);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      __syncthreads();
      cur ^= 1;
    }
    return buf[cur];
  }
};

}  // namespace kgat
