// Edge weights of the propagation layer that do not come from the attention: the Laplacian weights of the "w/o Att"
// ablation (kgat_edge_norm_f32) and node dropout's dropped copy of a weight stream (kgat_edge_dropout_f32).
// Both are streaming, elementwise over the E positions of a CSR: 16-byte loads and stores where the arrays'
// alignment allows, non-temporal loads for the streams read once (the CSR's record arrays, `key`, `w_in` - as the
// aggregation reads its record streams), a scalar tail.  The outputs are read again by the next aggregation: plain
// stores.  Nothing is allocated or synchronised here.
#include <math.h>

#include "kgat_common.h"

using namespace kgat;

namespace {

typedef int i4v __attribute__((ext_vector_type(4)));
typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int64_t kMaxBlocks = 2048;  // 256 CUs x 8 blocks; the rest of a larger E is grid-strided

inline unsigned grid_for(int64_t n_vec, int64_t n_tail) {
  const int64_t items = n_vec > n_tail ? n_vec : n_tail;
  int64_t blocks = (items + kBlock - 1) / kBlock;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

// ------------------------------------------------------------------------------------------------- Laplacian weights
// The weight of the edge u -> v from the two degree arrays.  A node id outside [0, n_nodes) (no CSR of
// kgat_csr_from_coo holds one) gives NaN and reads nothing.
template <int MODE>
__device__ __forceinline__ float edge_norm_weight(uint32_t n_nodes, const int32_t* __restrict__ indptr,
                                                  const int32_t* __restrict__ out_indptr, int32_t v, int32_t u) {
  if ((uint32_t)v >= n_nodes) return __builtin_nanf("");
  const float indeg = (float)(indptr[v + 1] - indptr[v]);
  if (MODE == KGAT_NORM_SI) return 1.f / indeg;
  if ((uint32_t)u >= n_nodes) return __builtin_nanf("");
  const float outdeg = (float)(out_indptr[u + 1] - out_indptr[u]);
  return 1.f / sqrtf(outdeg * indeg);
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void edge_norm_kernel(uint32_t n_nodes, int64_t n, int64_t n_vec,
                                                           const int32_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ row_of,
                                                           const int32_t* __restrict__ col,
                                                           const int32_t* __restrict__ eid,
                                                           const int32_t* __restrict__ out_indptr,
                                                           float* __restrict__ w_csr, float* __restrict__ w_eid) {
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t g = tid; g < n_vec; g += stride) {
    const i4v v = __builtin_nontemporal_load(reinterpret_cast<const i4v*>(row_of) + g);
    i4v u = {0, 0, 0, 0};
    if (MODE == KGAT_NORM_BI) u = __builtin_nontemporal_load(reinterpret_cast<const i4v*>(col) + g);
    f4v w;
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = edge_norm_weight<MODE>(n_nodes, indptr, out_indptr, v[k], u[k]);
    reinterpret_cast<f4v*>(w_csr)[g] = w;
    if (w_eid) {
      const i4v e = __builtin_nontemporal_load(reinterpret_cast<const i4v*>(eid) + g);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((uint64_t)(uint32_t)e[k] < (uint64_t)n) w_eid[e[k]] = w[k];
    }
  }
  for (int64_t p = 4 * n_vec + tid; p < n; p += stride) {
    const int32_t u = MODE == KGAT_NORM_BI ? __builtin_nontemporal_load(col + p) : 0;
    const float w = edge_norm_weight<MODE>(n_nodes, indptr, out_indptr, __builtin_nontemporal_load(row_of + p), u);
    w_csr[p] = w;
    if (w_eid) {
      const int32_t e = __builtin_nontemporal_load(eid + p);
      if ((uint64_t)(uint32_t)e < (uint64_t)n) w_eid[e] = w;
    }
  }
}

// ------------------------------------------------------------------------------------------------- node dropout
__device__ __forceinline__ bool edge_keep(uint32_t seed, uint32_t index, uint32_t threshold) {
  // the counter hash of kgat_dense.hip's drop_keep over (row = edge id, d = 1, col = 0): ops.dropout_keep_mask
  uint32_t x = (index * 0x9E3779B1u) ^ seed;
  x ^= x >> 16; x *= 0x85EBCA6Bu;
  x ^= x >> 13; x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x >= threshold;
}

// W_VEC: w_in is 16-byte aligned as well (key and w_out always are where n_vec > 0)
template <bool W_VEC>
__global__ __launch_bounds__(kBlock) void edge_dropout_kernel(int64_t n, int64_t n_vec, const float* __restrict__ w_in,
                                                              const int32_t* __restrict__ key, uint32_t threshold,
                                                              float keep_scale, uint32_t seed,
                                                              float* __restrict__ w_out) {
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t g = tid; g < n_vec; g += stride) {
    const int64_t p0 = 4 * g;
    i4v e;
    if (key) {
      e = __builtin_nontemporal_load(reinterpret_cast<const i4v*>(key) + g);
    } else {
      e = i4v{(int)p0, (int)p0 + 1, (int)p0 + 2, (int)p0 + 3};
    }
    f4v w;
    if (W_VEC) {
      w = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(w_in) + g);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = __builtin_nontemporal_load(w_in + p0 + k);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = edge_keep(seed, (uint32_t)e[k], threshold) ? w[k] * keep_scale : 0.f;
    reinterpret_cast<f4v*>(w_out)[g] = w;
  }
  for (int64_t p = 4 * n_vec + tid; p < n; p += stride) {
    const uint32_t e = key ? (uint32_t)__builtin_nontemporal_load(key + p) : (uint32_t)p;
    const float w = __builtin_nontemporal_load(w_in + p);
    w_out[p] = edge_keep(seed, e, threshold) ? w * keep_scale : 0.f;
  }
}

}  // namespace

extern "C" {

int kgat_edge_norm_f32(int64_t n_nodes, int64_t n_edges, const int32_t* indptr, const int32_t* row_of,
                       const int32_t* col, const int32_t* eid, const int32_t* out_indptr, int mode, float* w_csr,
                       float* w_eid, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_nodes >= 0 && n_nodes < INT32_MAX && n_edges >= 0 && n_edges < INT32_MAX,
                 "edge_norm: bad size (n_nodes=%lld n_edges=%lld)", (long long)n_nodes, (long long)n_edges);
  KGAT_CHECK_ARG(mode == KGAT_NORM_SI || mode == KGAT_NORM_BI, "edge_norm: unknown mode %d", mode);
  if (n_edges == 0) return KGAT_OK;
  KGAT_CHECK_ARG(indptr && row_of && w_csr, "edge_norm: null pointer");
  KGAT_CHECK_ARG(mode == KGAT_NORM_SI || (col && out_indptr), "edge_norm: KGAT_NORM_BI needs col and out_indptr");
  KGAT_CHECK_ARG(w_eid == nullptr || eid != nullptr, "edge_norm: w_eid asked for without eid");
  const bool vec = aligned16(row_of) && aligned16(w_csr) && (mode == KGAT_NORM_SI || aligned16(col)) &&
                   (w_eid == nullptr || aligned16(eid));
  const int64_t n_vec = vec ? n_edges / 4 : 0;
  const unsigned grid = grid_for(n_vec, n_edges - 4 * n_vec);
  if (mode == KGAT_NORM_SI) {
    hipLaunchKernelGGL(edge_norm_kernel<KGAT_NORM_SI>, dim3(grid), dim3(kBlock), 0, as_stream(stream), (uint32_t)n_nodes,
                       n_edges, n_vec, indptr, row_of, col, eid, out_indptr, w_csr, w_eid);
  } else {
    hipLaunchKernelGGL(edge_norm_kernel<KGAT_NORM_BI>, dim3(grid), dim3(kBlock), 0, as_stream(stream), (uint32_t)n_nodes,
                       n_edges, n_vec, indptr, row_of, col, eid, out_indptr, w_csr, w_eid);
  }
  KGAT_CHECK_LAUNCH("edge_norm");
  return KGAT_OK;
}

int kgat_edge_dropout_f32(int64_t n_edges, const float* w_in, const int32_t* key, float drop_p, uint64_t seed,
                          float* w_out, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_edges >= 0 && n_edges < INT32_MAX, "edge_dropout: bad size (n_edges=%lld)", (long long)n_edges);
  KGAT_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "edge_dropout: dropout probability outside [0, 1)");
  if (n_edges == 0) return KGAT_OK;
  KGAT_CHECK_ARG(w_in && w_out, "edge_dropout: null pointer");
  const double t = (double)drop_p * 4294967296.0;
  const uint32_t threshold = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
  const float keep_scale = 1.f / (1.f - drop_p);
  const uint32_t seed32 = (uint32_t)(seed ^ (seed >> 32));
  const bool vec = aligned16(w_out) && (key == nullptr || aligned16(key));
  const int64_t n_vec = vec ? n_edges / 4 : 0;
  const unsigned grid = grid_for(n_vec, n_edges - 4 * n_vec);
  if (aligned16(w_in)) {
    hipLaunchKernelGGL(edge_dropout_kernel<true>, dim3(grid), dim3(kBlock), 0, as_stream(stream), n_edges, n_vec, w_in,
                       key, threshold, keep_scale, seed32, w_out);
  } else {
    hipLaunchKernelGGL(edge_dropout_kernel<false>, dim3(grid), dim3(kBlock), 0, as_stream(stream), n_edges, n_vec, w_in,
                       key, threshold, keep_scale, seed32, w_out);
  }
  KGAT_CHECK_LAUNCH("edge_dropout");
  return KGAT_OK;
}

}  // extern "C"
