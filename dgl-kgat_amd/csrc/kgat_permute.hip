// A graph-static permutation of 4-byte per-edge values, out[i] = in[src_of[i]], as two streaming passes with no
// random global access (the gather of kgat_graph.hip reads one 64-byte sector per 4-byte item when src_of is random:
// 234 MB of sector traffic for 14.7 MB of attention weights on the amazon-book CKG).  The permutation is cut once per
// graph (ops.permute_plan) into two local ones that each fit a workgroup's LDS:
//   bin pass,   one workgroup per chunk of kPermTile consecutive SOURCE positions: values + 16-bit slots stream in,
//               every value is written to its LDS slot (slots ordered by destination block, then source position),
//               the LDS image is read linearly and stored to tmp[dst_a[...]] - inside a (chunk, block) run consecutive
//               lanes store to consecutive addresses;
//   place pass, one workgroup per block of kPermTile consecutive DESTINATIONS: the block's segment of tmp + 16-bit
//               slots stream in, LDS scatter, the image leaves as 16-byte non-temporal stores (the edge-id-ordered
//               tensor is not read on the path: the policy of the gather it replaces).
// No atomics, nothing between workgroups, no dependence on their placement.  Values move as 32-bit words (NaN
// payloads and -0.0 survive).  Slots are masked to the tile and tmp indices checked against n, so a damaged plan gives
// wrong values, never an access out of bounds.
// permute_bin_softmax_kernel is the bin pass specialised for the edge softmax's CSR-ordered output: it also finishes the
// rows the softmax's sweep left provisional (kgat_edge_softmax_permuted_f32, kgat_softmax.hip).
#include "kgat_common.h"
#include "kgat_softmax_carry.h"

#ifndef KGAT_PERMUTE_TILE
#define KGAT_PERMUTE_TILE 16384
#endif

namespace {

using namespace kgat;

constexpr int kPermTile = KGAT_PERMUTE_TILE;  // source chunk = destination block = one 64 KB LDS image
constexpr int kPermThreads = 1024;
constexpr int kPermMinRun = 16;               // mean (chunk, block) run kPermTile^2 / n of at least one 64-byte sector
static_assert(kPermTile % (kPermThreads * 8) == 0 && kPermTile <= 65536, "tile: whole 8-item rounds, 16-bit slots");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// val[0, cnt) -> lds[slot[i]]: eight consecutive items per thread and round (two 16-byte value loads, one 16-byte
// load of eight slots), every load of the tile issued before the first LDS write.  `val` and `slot` 16-byte aligned.
__device__ __forceinline__ void scatter_to_lds(const uint32_t* __restrict__ val, const uint16_t* __restrict__ slot, int cnt,
                                               uint32_t* lds) {
  constexpr int kRounds = kPermTile / (kPermThreads * 8);
  u32x4 lo[kRounds], hi[kRounds], s[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int i = (r * kPermThreads + (int)threadIdx.x) * 8;
    if (i + 8 <= cnt) {
      lo[r] = *reinterpret_cast<const u32x4*>(val + i);
      hi[r] = *reinterpret_cast<const u32x4*>(val + i + 4);
      s[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(slot + i));
    }
  }
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int i = (r * kPermThreads + (int)threadIdx.x) * 8;
    if (i + 8 <= cnt) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lds[(s[r][k >> 1] >> (16 * (k & 1))) & (kPermTile - 1)] = lo[r][k];
        lds[(s[r][2 + (k >> 1)] >> (16 * (k & 1))) & (kPermTile - 1)] = hi[r][k];
      }
    } else {
      for (int k = i; k < cnt; ++k) lds[slot[k] & (kPermTile - 1)] = val[k];
    }
  }
}

__global__ __launch_bounds__(kPermThreads) void permute_bin_kernel(int64_t n, const uint16_t* __restrict__ slot_a,
                                                                   const int32_t* __restrict__ dst_a,
                                                                   const uint32_t* __restrict__ in,
                                                                   uint32_t* __restrict__ tmp) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kPermTile];
  constexpr int kPer = kPermTile / kPermThreads;
  const int64_t base = (int64_t)blockIdx.x * kPermTile;
  const int cnt = (int)(n - base < kPermTile ? n - base : kPermTile);
  uint32_t dst[kPer];  // where this thread's LDS slots go: loaded ahead of the barrier
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = j * kPermThreads + (int)threadIdx.x;
    dst[j] = i < cnt ? (uint32_t)__builtin_nontemporal_load(dst_a + base + i) : 0xffffffffu;
  }
  scatter_to_lds(in + base, slot_a + base, cnt, lds);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (dst[j] < (uint64_t)n) tmp[dst[j]] = lds[j * kPermThreads + (int)threadIdx.x];
}

__global__ __launch_bounds__(kPermThreads) void permute_place_kernel(int64_t n, const uint16_t* __restrict__ slot_b,
                                                                     const uint32_t* __restrict__ tmp,
                                                                     uint32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kPermTile];
  constexpr int kRounds = kPermTile / (kPermThreads * 4);
  const int64_t base = (int64_t)blockIdx.x * kPermTile;
  const int cnt = (int)(n - base < kPermTile ? n - base : kPermTile);
  scatter_to_lds(tmp + base, slot_b + base, cnt, lds);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int i = (r * kPermThreads + (int)threadIdx.x) * 4;
    if (i + 4 <= cnt) {
      __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(lds + i), reinterpret_cast<u32x4*>(out + base + i));
    } else {
      for (int k = i; k < cnt; ++k) out[base + k] = lds[k];
    }
  }
}

// One cut row of a wavefront round, as the bin pass sees it: the range's `a` entry (the row cut by the range's start:
// positions [0, count) of the range) or its `b` entry (the row cut by its end: the last `count` positions).  A round's
// 8 x 64 positions lie inside ONE range of the softmax's sweep (EPW a multiple of 512, chunk boundaries range
// boundaries), so everything here is wave-uniform.  (M, S) of the whole row is formed by the sequence of
// softmax_cut_rows_kernel: a chain of two ranges by the shortcut with its operand order - the neighbour's entry was
// requested together with the range's own, so it costs no further round trip - any other by the walk of
// sm_chain_total.  Chain indices are held inside [0, n_ranges): the entries are the sweep's, and a damaged one gives
// wrong values, never a stray read.
struct PermCut {
  int32_t row;         // -1: no such cut row
  int32_t count;
  int32_t head, last;  // the chain to walk (walk = true)
  bool walk;
  float m;             // the range's partial maximum of the row
  float M, S;
};

__device__ __forceinline__ PermCut perm_cut_a(const SmCarry& ca, const SmCarry& pv, int64_t g, int32_t top) {
  PermCut c;
  c.row = ca.row; c.count = ca.count; c.m = ca.m; c.walk = false;
  c.head = ca.head < 0 ? 0 : (ca.head < top ? ca.head : top);
  c.last = ca.last < 0 ? 0 : (ca.last < top ? ca.last : top);
  c.M = pv.m; c.S = pv.s;
  if (ca.row >= 0) {
    if (ca.head == g - 1 && ca.last == g) sm_combine(c.M, c.S, ca.m, ca.s);  // (same operands, same order as the walk)
    else c.walk = true;
  }
  return c;
}

__device__ __forceinline__ PermCut perm_cut_b(const SmCarry& cb, const SmCarry& nx, int64_t g, int32_t top) {
  PermCut c;  // (the head entry of its chain: the row starts in this range)
  c.row = cb.row; c.count = cb.count; c.m = cb.m; c.walk = false;
  c.head = cb.head < 0 ? 0 : (cb.head < top ? cb.head : top);
  c.last = cb.last < 0 ? 0 : (cb.last < top ? cb.last : top);
  c.M = cb.m; c.S = cb.s;
  if (cb.row >= 0) {
    if (cb.last == g + 1) sm_combine(c.M, c.S, nx.m, nx.s);
    else c.walk = true;
  }
  return c;
}

// The walks of a workgroup's cut rows, each row walked ONCE per workgroup: a hub fills every range of a chunk, and
// sixteen wavefronts walking the same chain - some 200 VALU instructions per block of 64 followers, four wavefronts to
// a SIMD - is what the bin pass then waits for.  The wavefront round whose range is the row's first inside the chunk
// walks (the row's head range - its `b` cut - or, for a row that began in an earlier chunk, the chunk's first range)
// and leaves (M, S) in LDS; the rounds of the row's later ranges - `a` cuts - read it after a barrier.  The same
// sequence, run once instead of many times: the same bits.  A walk requests the head's entry and four blocks of
// followers at once (addresses follow from (head, last); the head's entry is a vector load with its index pinned in a
// VGPR, a scalar load being waited for, on its own counter, before the followers are requested) and runs their trees
// side by side; a chain of more than 257 ranges carries on in sm_chain_rest.  ONE copy of the walk's code: a loop over
// the cuts, the cut picked by selects.  slot = 2 * (range inside the chunk) + (1 for the `b` cut).
template <int kCuts>
__device__ __forceinline__ void perm_walk_chains(const SmCarry* __restrict__ carry, PermCut (&c)[kCuts],
                                                 const int (&own)[kCuts], const int (&src)[kCuts], float* walk_m,
                                                 float* walk_s, int lane) {
#pragma unroll 1
  for (int e = 0; e < kCuts; ++e) {
    int32_t head = 0, last = 0;
    int slot = -1;
#pragma unroll
    for (int k = 0; k < kCuts; ++k)
      if (k == e) { head = c[k].head; last = c[k].last; slot = c[k].walk ? own[k] : -1; }
    if (slot < 0) continue;
    int32_t hv = head;
    asm volatile("" : "+v"(hv));
    const SmCarry* hp = carry + (2 * (int64_t)hv + 1);
    float M = hp->m, S = hp->s;
    float pm[4], ps[4];
    const int64_t j0 = (int64_t)head + 1;
#pragma unroll
    for (int b = 0; b < 4; ++b) sm_chain_load(carry, j0 + b * kWave, last, lane, pm[b], ps[b]);
    sm_chain_trees<4>(pm, ps, lane);
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (j0 + b * kWave <= last) sm_combine(M, S, pm[b], ps[b]);
    sm_chain_rest<4>(carry, j0 + 4 * kWave, last, lane, M, S);
    if (lane == 0) { walk_m[slot] = M; walk_s[slot] = S; }
#pragma unroll
    for (int k = 0; k < kCuts; ++k)
      if (k == e) { c[k].M = M; c[k].S = S; }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kCuts; ++k)
    if (c[k].walk && own[k] < 0) { c[k].M = walk_m[src[k]]; c[k].S = walk_s[src[k]]; }
}

__device__ __forceinline__ uint32_t perm_scaled(uint32_t bits, float f) { return __float_as_uint(__uint_as_float(bits) * f); }

// The bin pass over the edge softmax's CSR-ordered output, with the softmax's second launch folded in: the values of
// the rows that the sweep's ranges cut arrive provisional (exp(x - m) of the range's partial maximum) and are
// multiplied by exp(m - M) / S of their whole row while this pass holds them in registers - the same x * f as
// softmax_cut_rows_kernel, the other positions untouched - then written back to `w` in place (only the 16-byte pieces
// that hold a corrected position; the workgroup loads and stores only its own chunk of `w`) and binned as in
// permute_bin_kernel.  The carries are requested beside the value / slot / dst_a loads and the factors computed
// while those are in flight; a wavefront needs the factors of its own rounds only, so they stay in its registers
// (only the total of a chain that had to be walked travels through LDS: perm_walk_chains).
template <int EPW>
__global__ __launch_bounds__(kPermThreads) void permute_bin_softmax_kernel(int64_t n, const uint16_t* __restrict__ slot_a,
                                                                           const int32_t* __restrict__ dst_a,
                                                                           const SmCarry* __restrict__ carry, uint32_t* w,
                                                                           uint32_t* __restrict__ tmp) {
  static_assert(EPW % (kWave * 8) == 0, "a wavefront round (8 x 64 positions) lies inside one range");
  __shared__ __attribute__((aligned(16))) uint32_t lds[kPermTile];
  constexpr int kPer = kPermTile / kPermThreads;
  constexpr int kRounds = kPermTile / (kPermThreads * 8);
  const int64_t base = (int64_t)blockIdx.x * kPermTile;
  const int cnt = (int)(n - base < kPermTile ? n - base : kPermTile);
  const int lane = (int)threadIdx.x % kWave;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int64_t n_ranges = (n + EPW - 1) / EPW;
  constexpr int kRanges = kPermTile / EPW;
  static_assert((kRanges & (kRanges - 1)) == 0, "ranges per chunk: a power of two (slot masks)");
  __shared__ float walk_m[2 * kRanges], walk_s[2 * kRanges];
  uint32_t dst[kPer];  // where this thread's LDS slots go: loaded ahead of the barrier
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int i = j * kPermThreads + (int)threadIdx.x;
    dst[j] = i < cnt ? (uint32_t)__builtin_nontemporal_load(dst_a + base + i) : 0xffffffffu;
  }
  uint32_t* val = w + base;
  const uint16_t* slot = slot_a + base;
  u32x4 lo[kRounds], hi[kRounds], s[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int i = (r * kPermThreads + (int)threadIdx.x) * 8;
    if (i + 8 <= cnt) {
      lo[r] = *reinterpret_cast<const u32x4*>(val + i);
      hi[r] = *reinterpret_cast<const u32x4*>(val + i + 4);
      s[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(slot + i));
    }
  }
  // ---- the carries of the ranges this wavefront's rounds lie in, and their neighbours': scalar loads, which travel
  // beside the vector loads above.  (Placed first, the compiler made the value loads wait for them: their buffer's
  // kernel argument arrived under the same counter.)
  SmCarry ca[kRounds], cb[kRounds], pv[kRounds], nx[kRounds];
  int64_t g[kRounds];
  bool live[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t gr = (base + (int64_t)(r * kPermThreads + wave * kWave) * 8) / EPW;
    live[r] = gr < n_ranges;
    g[r] = live[r] ? gr : n_ranges - 1;  // (a round past the end: loads nothing it uses, walks nothing)
    ca[r] = carry[2 * g[r]];
    cb[r] = carry[2 * g[r] + 1];
    pv[r] = carry[2 * (g[r] > 0 ? g[r] - 1 : 0) + 1];
    nx[r] = carry[2 * (g[r] + 1 < n_ranges ? g[r] + 1 : g[r])];
  }
  // ---- factors (wave-uniform), while the values are on their way: entry 2r the `a`, 2r + 1 the `b` cut of round r
  const int32_t top = (int32_t)(n_ranges - 1);
  const int64_t g_first = base / EPW;  // the chunk's first range
  PermCut cut[2 * kRounds];
  int own[2 * kRounds], src[2 * kRounds];  // the LDS slot this round's walk fills (-1: not its walk) / reads
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    cut[2 * r] = perm_cut_a(ca[r], pv[r], g[r], top);
    cut[2 * r + 1] = perm_cut_b(cb[r], nx[r], g[r], top);
    if (!live[r]) cut[2 * r].walk = cut[2 * r + 1].walk = false;
    const int gl = (int)(g[r] - g_first) & (kRanges - 1);
    const int64_t hl = cut[2 * r].head - g_first;  // where the `a` cut's row starts, in ranges of this chunk
    own[2 * r] = gl == 0 ? 0 : -1;
    src[2 * r] = hl < 0 ? 0 : (2 * (int)hl + 1) & (2 * kRanges - 1);
    own[2 * r + 1] = src[2 * r + 1] = 2 * gl + 1;
  }
  perm_walk_chains(carry, cut, own, src, walk_m, walk_s, lane);
  // ---- rescale the cut rows' values, write the corrected pieces back, scatter into the LDS image
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int i = (r * kPermThreads + (int)threadIdx.x) * 8;
    const int q0 = (int)((base + i) % EPW);  // position inside the range
    // positions q < na of the range take fa, positions q >= b0 take fb, the others nothing
    const PermCut &a = cut[2 * r], &b = cut[2 * r + 1];
    const int len = (int)(n - g[r] * EPW < EPW ? n - g[r] * EPW : EPW);
    const int na = a.row >= 0 ? a.count : 0, b0 = b.row >= 0 ? len - b.count : EPW;
    const float fa = a.row >= 0 ? sm_exp(a.m - a.M) / a.S : 1.0f, fb = b.row >= 0 ? sm_exp(b.m - b.M) / b.S : 1.0f;
    if (i + 8 <= cnt) {
      if (q0 < na || q0 + 7 >= b0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          lo[r][k] = q0 + k < na ? perm_scaled(lo[r][k], fa) : (q0 + k >= b0 ? perm_scaled(lo[r][k], fb) : lo[r][k]);
          hi[r][k] = q0 + 4 + k < na ? perm_scaled(hi[r][k], fa) : (q0 + 4 + k >= b0 ? perm_scaled(hi[r][k], fb) : hi[r][k]);
        }
        if (q0 < na || q0 + 3 >= b0) *reinterpret_cast<u32x4*>(val + i) = lo[r];
        if (q0 + 4 < na || q0 + 7 >= b0) *reinterpret_cast<u32x4*>(val + i + 4) = hi[r];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lds[(s[r][k >> 1] >> (16 * (k & 1))) & (kPermTile - 1)] = lo[r][k];
        lds[(s[r][2 + (k >> 1)] >> (16 * (k & 1))) & (kPermTile - 1)] = hi[r][k];
      }
    } else {
      for (int k = i; k < cnt; ++k) {
        const int q = q0 + (k - i);
        uint32_t v = val[k];
        if (q < na || q >= b0) {
          v = perm_scaled(v, q < na ? fa : fb);
          val[k] = v;
        }
        lds[slot[k] & (kPermTile - 1)] = v;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPer; ++j)
    if (dst[j] < (uint64_t)n) tmp[dst[j]] = lds[j * kPermThreads + (int)threadIdx.x];
}

}  // namespace

namespace kgat {

bool permute_softmax_fits(int epw) { return epw > 0 && kPermTile % epw == 0 && epw % (kWave * 8) == 0; }

int permute_softmax_launch(int epw, int64_t n, const uint16_t* slot_a, const int32_t* dst_a, const uint16_t* slot_b,
                           const SmCarry* carry, float* w, float* out, float* tmp, hipStream_t st) {
  const dim3 grid((unsigned)((n + kPermTile - 1) / kPermTile)), block(kPermThreads);
  uint32_t* wv = reinterpret_cast<uint32_t*>(w);
  uint32_t* tv = reinterpret_cast<uint32_t*>(tmp);
  if (epw == SmGeom<8>::EPW && permute_softmax_fits(epw))
    hipLaunchKernelGGL(permute_bin_softmax_kernel<SmGeom<8>::EPW>, grid, block, 0, st, n, slot_a, dst_a, carry, wv, tv);
  else if (epw == SmGeom<16>::EPW && permute_softmax_fits(epw))
    hipLaunchKernelGGL(permute_bin_softmax_kernel<SmGeom<16>::EPW>, grid, block, 0, st, n, slot_a, dst_a, carry, wv, tv);
  else {
    set_error("permute_softmax: ranges of %d positions do not tile chunks of %d", epw, kPermTile);
    return KGAT_E_UNSUPPORTED;
  }
  KGAT_CHECK_LAUNCH("permute_bin_softmax");
  hipLaunchKernelGGL(permute_place_kernel, grid, block, 0, st, n, slot_b, (const uint32_t*)tv, reinterpret_cast<uint32_t*>(out));
  KGAT_CHECK_LAUNCH("permute_place");
  return KGAT_OK;
}

}  // namespace kgat

extern "C" {

int kgat_permute_tile(void) { return kPermTile; }

int kgat_permute_supported(int64_t n) {
  return n >= 0 && n * kPermMinRun <= (int64_t)kPermTile * kPermTile ? 1 : 0;
}

int kgat_permute_f32(int64_t n, const uint16_t* slot_a, const int32_t* dst_a, const uint16_t* slot_b, const float* in,
                     float* out, float* tmp, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n >= 0, "permute: negative size");
  if (n == 0) return KGAT_OK;
  if (!kgat_permute_supported(n)) {
    set_error("permute: %lld items give runs shorter than %d (limit %lld): use kgat_gather_f32", (long long)n, kPermMinRun,
              (long long)kPermTile * kPermTile / kPermMinRun);
    return KGAT_E_UNSUPPORTED;
  }
  KGAT_CHECK_ARG(slot_a && dst_a && slot_b && in && out && tmp, "permute: null pointer");
  KGAT_CHECK_ARG(aligned16(slot_a) && aligned16(slot_b) && aligned16(in) && aligned16(out) && aligned16(tmp),
                 "permute: slot_a, slot_b, in, out and tmp must be 16-byte aligned");
  KGAT_CHECK_ARG(in != out && in != tmp && out != tmp, "permute: in, out and tmp must be three buffers");
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)((n + kPermTile - 1) / kPermTile)), block(kPermThreads);
  hipLaunchKernelGGL(permute_bin_kernel, grid, block, 0, st, n, slot_a, dst_a, reinterpret_cast<const uint32_t*>(in),
                     reinterpret_cast<uint32_t*>(tmp));
  KGAT_CHECK_LAUNCH("permute_bin");
  hipLaunchKernelGGL(permute_place_kernel, grid, block, 0, st, n, slot_b, reinterpret_cast<const uint32_t*>(tmp),
                     reinterpret_cast<uint32_t*>(out));
  KGAT_CHECK_LAUNCH("permute_place");
  return KGAT_OK;
}

}  // extern "C"
