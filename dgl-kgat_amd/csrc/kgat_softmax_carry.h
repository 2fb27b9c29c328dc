// The edge softmax's carry record and the arithmetic over the chains of cut rows, shared by the two places that
// finish a cut row: softmax_cut_rows_kernel (kgat_softmax.hip) and the fused bin pass of the planned permutation
// (kgat_permute.hip).  Both must form (M, S) of a row by exactly the same sequence of operations - the helpers below
// are that sequence - so that the two paths give the same bits.
#pragma once
#include "kgat_common.h"

namespace kgat {

// positions per lane: 16 (1,024 per wavefront), or 8 for launches over fewer than kSmSmallEdges
// positions, where the sweep is a latency chain rather than a stream and twice the wavefronts with half
// the chain each finish sooner.
constexpr int kSmMaxEPL = 16;
constexpr int64_t kSmSmallEdges = 8 << 20;
template <int EPL> struct SmGeom {
  static constexpr int EPW = kWave * EPL;   // positions per wavefront
};
constexpr float kSmNegBig = -3.0e38f;     // stands in for -inf (keeps the combine NaN-free)

struct __attribute__((aligned(16))) SmCarry {
  int32_t row;    // -1: no entry
  int32_t count;  // positions of this wavefront that belong to the row
  float m, s;     // partial max, partial sum of exp(x - m)
  int32_t head;   // wavefront in which the row starts (its `b` entry heads the chain)
  int32_t last;   // wavefront in which the row ends
  int32_t pad0, pad1;
};

// exp(x) for x <= 0 on the hardware exp2: the product x*log2(e) is split into its rounded value
// and the rounding remainder (fma), the remainder enters as a first-order factor - about 1.5 ulp,
// against ~|x| ulp for exp2(x * log2e) alone.  Results below the normal range flush to zero.
__device__ __forceinline__ float sm_exp(float x) {
  x = fmaxf(x, -128.0f);  // exp2(-184) is already 0; keeps the split finite for the -3e38 stand-in
  const float t = x * 1.44269504088896341f;
  const float lo = fmaf(x, 1.44269504088896341f, -t) + x * 1.92596299112661746e-8f;
  return __builtin_amdgcn_exp2f(t) * fmaf(lo, 0.693147180559945309f, 1.0f);
}

// (m, s) <- (m, s) (+) (m2, s2): the smaller maximum's sum is rescaled by exp(-|m - m2|).  Branch-free
// (one exp, selects).  Used where partial results of different wavefronts meet (the chains of cut rows).
__device__ __forceinline__ void sm_combine(float& m, float& s, float m2, float s2) {
  const bool keep = m >= m2;
  const float e = sm_exp(keep ? m2 - m : m - m2);
  const float big = keep ? s : s2, small = keep ? s2 : s;
  s = fmaf(small, e, big);
  m = keep ? m : m2;
}

// The ordered tree over the 64 lanes' entries (pm, ps) of one block of a chain - (kSmNegBig, 0) in a lane past the
// chain's end - for kB independent blocks side by side (their shuffles and combines interleave; every block sees the
// operations of a tree on its own).  Every lane returns with the blocks' totals.
template <int kB>
__device__ __forceinline__ void sm_chain_trees(float (&pm)[kB], float (&ps)[kB], int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    float m2[kB], s2[kB];
#pragma unroll
    for (int b = 0; b < kB; ++b) { m2[b] = __shfl_down(pm[b], d, kWave); s2[b] = __shfl_down(ps[b], d, kWave); }
    if ((lane & (2 * d - 1)) == 0) {
#pragma unroll
      for (int b = 0; b < kB; ++b) sm_combine(pm[b], ps[b], m2[b], s2[b]);
    }
  }
#pragma unroll
  for (int b = 0; b < kB; ++b) { pm[b] = __shfl(pm[b], 0, kWave); ps[b] = __shfl(ps[b], 0, kWave); }
}

// (M, S) of a cut row from the carries of its chain: the head wavefront's `b` entry, then the `a`
// entries of the followers head+1 .. last in blocks of 64 (ordered tree inside a block).  Every
// wavefront of the chain runs exactly this sequence, so all of them normalise with the same bits.
__device__ __forceinline__ void sm_chain_total(const SmCarry* __restrict__ carry, int32_t head, int32_t last,
                                               int lane, float& M, float& S) {
  const SmCarry h = carry[2 * (int64_t)head + 1];
  float m = h.m, s = h.s;
  for (int64_t j0 = (int64_t)head + 1; j0 <= last; j0 += kWave) {
    const int64_t j = j0 + lane;
    float pm[1] = {kSmNegBig}, ps[1] = {0.f};
    if (j <= last) {
      const SmCarry f = carry[2 * j];
      pm[0] = f.m; ps[0] = f.s;
    }
    sm_chain_trees<1>(pm, ps, lane);
    sm_combine(m, s, pm[0], ps[0]);
  }
  M = m; S = s;
}

// The followers' entries of one block, first follower j0, as the tree takes them.  The load is unconditional, a lane
// past the end clamped to the last entry (`last` >= 0) and its value replaced afterwards: a load under a lane mask is
// waited for where the mask ends, and the loads of several blocks are meant to be in flight together.
__device__ __forceinline__ void sm_chain_load(const SmCarry* __restrict__ carry, int64_t j0, int32_t last, int lane,
                                              float& pm, float& ps) {
  const int64_t j = j0 + lane;
  const SmCarry* f = carry + 2 * (j <= last ? j : (int64_t)last);
  const float fm = f->m, fs = f->s;
  pm = j <= last ? fm : kSmNegBig;
  ps = j <= last ? fs : 0.f;
}

// The sequence of sm_chain_total from follower j0 on, (m, s) holding the total so far, with the loads of kAhead blocks
// in flight together and their trees side by side: a block's addresses follow from (j0, last) alone.
template <int kAhead>
__device__ __forceinline__ void sm_chain_rest(const SmCarry* __restrict__ carry, int64_t j0, int32_t last, int lane,
                                              float& m, float& s) {
  for (; j0 <= last; j0 += kAhead * kWave) {
    float pm[kAhead], ps[kAhead];
#pragma unroll
    for (int b = 0; b < kAhead; ++b) sm_chain_load(carry, j0 + b * kWave, last, lane, pm[b], ps[b]);
    sm_chain_trees<kAhead>(pm, ps, lane);
#pragma unroll
    for (int b = 0; b < kAhead; ++b)
      if (j0 + b * kWave <= last) sm_combine(m, s, pm[b], ps[b]);
  }
}

// The permutation's two passes with the cut-row rescale folded into the bin pass (kgat_permute.hip): `w` holds the
// sweep's CSR-ordered values over [0, n) - the cut rows' provisional - and `carry` the sweep's entries for ranges of
// `epw` positions.  Leaves `w` finished in place and out[i] = w[src_of[i]].  permute_softmax_fits: whether the
// bin pass's chunks and wavefront rounds are whole multiples / whole fractions of such ranges.
bool permute_softmax_fits(int epw);
int permute_softmax_launch(int epw, int64_t n, const uint16_t* slot_a, const int32_t* dst_a, const uint16_t* slot_b,
                           const SmCarry* carry, float* w, float* out, float* tmp, hipStream_t st);

}  // namespace kgat
