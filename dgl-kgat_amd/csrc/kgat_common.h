// Internal helpers shared by the gfx950 kernels of libkgat_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/kgat_hip.h"

namespace kgat {

constexpr int kWave = 64;  // gfx950 wavefront

void set_error(const char* fmt, ...);

inline hipStream_t as_stream(kgat_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }  // float4 / int4 accesses

// bits of a radix sort's keys: enough for every key in [0, max_key], at least 1, at most 31
inline int bits_for(int64_t max_key) {
  int b = 1;
  while (b < 31 && ((int64_t)1 << b) <= max_key) ++b;
  return b;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// float4 arithmetic, element by element
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 fma4(float a, const float4& x, const float4& c) {
  return make_float4(fmaf(a, x.x, c.x), fmaf(a, x.y, c.y), fmaf(a, x.z, c.z), fmaf(a, x.w, c.w));
}
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 mul4(const float4& a, const float4& b) {
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}

// The blocks behind a launch's real work (block `first_block` on, `threads` each) clear zero[0 .. n_zero), n_zero a
// multiple of 4: a zero fill rides beside launches that are chains of round trips on a few workgroups.
__device__ __forceinline__ void zero_fill_behind(float* __restrict__ zero, int64_t n_zero, unsigned first_block,
                                                 int threads) {
  const int64_t n4 = n_zero / 4, stride = (int64_t)(gridDim.x - first_block) * threads;
  float4* z = reinterpret_cast<float4*>(zero);
  for (int64_t i = (int64_t)(blockIdx.x - first_block) * threads + threadIdx.x; i < n4; i += stride)
    z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// Carves 256-byte aligned regions out of a caller-provided workspace.
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* p) : base(static_cast<char*>(p)) {}
  template <typename T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(base + off);
    off = align_up(off + count * sizeof(T), 256);
    return p;
  }
};

// Compute units of the current device; the attribute query is made once per device ordinal.
inline int device_cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cached[dev] == 0) {
    int v = 0;
    cached[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
  }
  return cached[dev];
}

// Workgroups per compute unit of a persistent launch of `Kernel` with `threads` threads: what the kernel's registers
// and LDS admit, at most 8.  The occupancy query is made once per kernel instantiation.
template <auto Kernel>
inline int resident_blocks_per_cu(int threads) {
  static int cached = 0;
  if (cached == 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, Kernel, threads, 0) != hipSuccess || nb < 1) nb = 1;
    cached = nb > 8 ? 8 : nb;
  }
  return cached;
}

// The segment that holds item t: the largest r in [0, n) with prefix[r] <= t (prefix non-decreasing, prefix[0] <= t).
// Among empty segments, which share their prefix value with the next one, that is the last.
template <typename T>
__device__ __forceinline__ int segment_of(const int32_t* prefix, int n, T t) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

// Workgroups are dealt round-robin over the 8 XCDs (observed placement, a speed matter only: blocks b and
// b + 8 share an L2; MI355X_MICROARCH.md, Workgroup dispatch).  The work item of block b out of n such
// that the blocks of one XCD take a CONTIGUOUS eighth of the items (bijective for any n).  Used by the fused
// attention kernel at d <= 64 (KGAT_ATT_XCD_REMAP); slower on the aggregation's tiles and on the d = 128 attention
// (notes at KGAT_SPMM_XCD_REMAP, KGAT_ATT128_XCD_REMAP: A/B builds).
__device__ __forceinline__ unsigned xcd_contiguous(unsigned b, unsigned n) {
  const unsigned q = n / 8, r = n % 8, x = b % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

// Host-side width dispatch: the (d_in, d_out) a caller passes -> the kernel instantiation compiled for that pair.
// dispatch_widths(table, a, b, f) calls the generic lambda f(A, B) with the two widths as
// std::integral_constant<int, ...> (A() and B() are constant expressions: template arguments of the launch) and
// returns what it returns, or KGAT_E_UNSUPPORTED for a pair the table does not hold.  f is instantiated once per
// pair of the table and for no other, so the table IS the set of kernels built.
template <int... D> struct WidthSquare {};              // every pair of D x D
template <int A, int B> struct WidthPair {};
template <typename... P> struct WidthPairs {};          // the listed pairs
using MfmaWidths = WidthSquare<16, 32, 64, 128>;        // the MFMA dense kernels: whole 16-column tiles up to 128

template <typename F, int A, int B>
inline bool try_widths(WidthPair<A, B>, int a, int b, F& f, int& rc) {
  if (a != A || b != B) return false;
  rc = f(std::integral_constant<int, A>{}, std::integral_constant<int, B>{});
  return true;
}
template <typename F, int... A, int... B>
inline int dispatch_widths(WidthPairs<WidthPair<A, B>...>, int a, int b, F&& f) {
  int rc = KGAT_E_UNSUPPORTED;
  (void)(try_widths(WidthPair<A, B>{}, a, b, f, rc) || ...);
  return rc;
}
template <typename F, int... D>
inline int dispatch_widths(WidthSquare<D...>, int a, int b, F&& f) {
  int rc = KGAT_E_UNSUPPORTED;
  auto row = [&](auto wa) { return (try_widths(WidthPair<decltype(wa)::value, D>{}, a, b, f, rc) || ...); };
  (void)((a == D && row(std::integral_constant<int, D>{})) || ...);
  return rc;
}
// One width: a list is the diagonal of a pair table, so the same machinery serves it.  dispatch_width(list, d, f) calls
// f(D) under the contract above; has_width(list, d) / has_widths(table, a, b) are the membership tests a `_supported`
// predicate states.
template <int... D> using WidthList = WidthPairs<WidthPair<D, D>...>;
template <typename F, typename... P>
inline int dispatch_width(WidthPairs<P...> list, int d, F&& f) {
  return dispatch_widths(list, d, d, [&](auto w, auto) { return f(w); });
}
template <int... D>
constexpr bool has_width(WidthPairs<WidthPair<D, D>...>, int d) { return ((d == D) || ...); }
template <int... A, int... B>
constexpr bool has_widths(WidthPairs<WidthPair<A, B>...>, int a, int b) { return ((a == A && b == B) || ...); }

// Device-side primitives implemented in kgat_graph.hip, reused by other translation units.
size_t scan_workspace_elems(int64_t n);
// In-place exclusive scan of int32 data[n]; ws has scan_workspace_elems(n) int32.
int exclusive_scan_i32(int32_t* data, int64_t n, int32_t* ws, hipStream_t st);

size_t radix_sort_workspace_bytes(int64_t n);
// Stable LSD radix sort of (key, index) pairs on the low `key_bits` bits of keys_in[n].
// vals_out[n] receives the source index of each sorted position; *sorted_keys (optional)
// receives a pointer (inside ws) to the sorted keys.
int radix_sort_index(const int32_t* keys_in, int64_t n, int key_bits, int32_t* vals_out,
                     const int32_t** sorted_keys, void* ws, size_t ws_bytes, hipStream_t st);

}  // namespace kgat

#define KGAT_CHECK_ARG(cond, ...)   \
  do {                              \
    if (!(cond)) {                  \
      kgat::set_error(__VA_ARGS__); \
      return KGAT_E_BADARG;         \
    }                               \
  } while (0)

// A check function's result: an error is returned, a positive value ("nothing to do") ends the entry with KGAT_OK.
#define KGAT_RETURN_IF(rc_expr)                            \
  do {                                                     \
    const int rc__ = (rc_expr);                            \
    if (rc__ != KGAT_OK) return rc__ > 0 ? KGAT_OK : rc__; \
  } while (0)

#define KGAT_CHECK_LAUNCH(what)                                                    \
  do {                                                                             \
    hipError_t e__ = hipGetLastError();                                            \
    if (e__ != hipSuccess) {                                                       \
      kgat::set_error("%s: launch failed: %s", what, hipGetErrorString(e__));      \
      return KGAT_E_HIP;                                                           \
    }                                                                              \
  } while (0)
