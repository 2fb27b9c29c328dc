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
#include "kgat_common.h"

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

}  // namespace

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
