// GraphSAGE (mean aggregator) layer for gfx950: the kernels behind dgl.nn.pytorch.conv.SAGEConv(aggregator_type="mean")
// of reference models.py:98-100,107-109 (gnn_model = "graphsage").  DGL 0.4.x SAGEConv.forward, homogeneous graph:
//   hd = feat_drop(h);  h_neigh[v] = mean_{u->v} hd[u] (0 without in-edges);  rst = fc_self(hd) + fc_neigh(h_neigh)
//   followed by the activation.  The dense operators:
//  * the aggregation itself is kgat_copy_reduce_f32 (update_all(fn.copy_src, fn.sum | fn.mean)), which lives with the
//    other merge-path reducers in kgat_spmm.hip.  The backward of copy_src -> mean w.r.t. the source feature is the same
//    operator (sum) on the reversed CSR over rows pre-scaled by 1 / max(deg, 1) of their destination
//    (sage_bwd_input_kernel writes them so).
//  * sage_dense: Z = act(H W_self^T + HN W_neigh^T + b_self + b_neigh) on v_mfma_f32_16x16x4_f32 (exact fp32): one
//    wavefront per 16-row tile, both weights staged once per workgroup in MFMA fragment order in LDS; optional
//    L2-normalised copy into a slice of the readout and the ego block (a copy of H) as kgat_aggregator_f32.
//  * dropout_rows: out = (x [+ x2]) * keep / (1 - p) with the counter hash of the bi-interaction's dropout.
//  * sage_bwd_input / sage_bwd_weight: grad_pre W_self, (grad_pre W_neigh) / max(deg, 1) and per-workgroup partials
//    of grad_pre^T H, grad_pre^T HN and the column sums of grad_pre.
#include "kgat_common.h"

namespace kgat {

typedef float floatx4_g __attribute__((ext_vector_type(4)));

// --------------------------------------------------------------------------------------------- dense forward
// Waves per SIMD the dense kernels ask the compiler for: two up to 2,048 weight elements; beyond, the weight fragments
// the compiler keeps in registers across the tile loop need more than half the register file (1 wave, no spills; at
// two waves 64 x 64 and wider spill to scratch).
constexpr int sage_waves(int di, int dout) { return di * dout <= 2048 ? 2 : 1; }

// Fragment order of a weight in LDS for the operand-swapped product (kgat_dense.hip): W (DO x DI) row-major,
// s_w[(s * KT + c) * 64 + q * 16 + i] = W[16c + i][16 (s >> 2) + 4q + (s & 3)], KT = DO / 16, s < DI / 4.
template <int DI, int DO>
__device__ __forceinline__ void stage_fwd_weight(const float* __restrict__ W, float* s_w) {
  constexpr int KT = DO / 16;
  for (int idx = threadIdx.x * 4; idx < DO * DI; idx += 256 * 4) {
    const float4 v = *reinterpret_cast<const float4*>(W + idx);
    const int j = idx / DI, k0 = idx % DI;
    const int c = j >> 4, i = j & 15;
    const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = k0 + t;
      const int s = (k >> 4) * 4 + (k & 3), q = (k >> 2) & 3;
      s_w[(s * KT + c) * kWave + q * 16 + i] = vv[t];
    }
  }
}

template <int DI, int DO, bool RELU>
__global__ __launch_bounds__(256, sage_waves(DI, DO)) void sage_dense_kernel(int32_t n_rows, const float* __restrict__ H,
                                                         const float* __restrict__ HN, const float* __restrict__ Ws,
                                                         const float* __restrict__ Wn, const float* __restrict__ bs,
                                                         const float* __restrict__ bn, float* __restrict__ h_out,
                                                         float* __restrict__ norm_out, int64_t norm_stride,
                                                         float* __restrict__ self_out, int64_t self_stride) {
  constexpr int KS = DI / 4, KT = DO / 16;
  __shared__ float s_ws[KS * KT * kWave];
  __shared__ float s_wn[KS * KT * kWave];
  stage_fwd_weight<DI, DO>(Ws, s_ws);
  stage_fwd_weight<DI, DO>(Wn, s_wn);
  __syncthreads();
  const int lane = threadIdx.x % kWave;
  const int i = lane & 15, q = lane >> 4;
  // bias of the lane's output columns 16c + 4q + j
  float bias[KT][4];
#pragma unroll
  for (int c = 0; c < KT; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = 16 * c + 4 * q + j;
      bias[c][j] = (bs ? bs[n] : 0.f) + (bn ? bn[n] : 0.f);
    }
  const int64_t n_waves = (int64_t)gridDim.x * (256 / kWave);
  const int64_t wv = (int64_t)blockIdx.x * (256 / kWave) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int32_t n_tiles = (n_rows + 15) >> 4;
  const int32_t t_begin = (int32_t)((int64_t)n_tiles * wv / n_waves);
  const int32_t t_end = (int32_t)((int64_t)n_tiles * (wv + 1) / n_waves);
  if (t_begin >= t_end) return;

  auto load = [&](int32_t t, float (&a)[KS], float (&b)[KS]) {
    int32_t r = (t << 4) + i;
    r = r < n_rows ? r : n_rows - 1;
    const float4* pa = reinterpret_cast<const float4*>(H + (size_t)r * DI) + q;
    const float4* pb = reinterpret_cast<const float4*>(HN + (size_t)r * DI) + q;
#pragma unroll
    for (int m = 0; m < DI / 16; ++m) {
      const float4 v = pa[4 * m];
      a[4 * m + 0] = v.x; a[4 * m + 1] = v.y; a[4 * m + 2] = v.z; a[4 * m + 3] = v.w;
    }
#pragma unroll
    for (int m = 0; m < DI / 16; ++m) {
      const float4 v = pb[4 * m];
      b[4 * m + 0] = v.x; b[4 * m + 1] = v.y; b[4 * m + 2] = v.z; b[4 * m + 3] = v.w;
    }
  };
  auto tile = [&](int32_t t, const float (&a)[KS], const float (&b)[KS]) {
    const int32_t row = (t << 4) + i;
    if (self_out != nullptr && row < n_rows) {
      float4* pe = reinterpret_cast<float4*>(self_out + (size_t)row * self_stride) + q;
#pragma unroll
      for (int m = 0; m < DI / 16; ++m) pe[4 * m] = make_float4(a[4 * m + 0], a[4 * m + 1], a[4 * m + 2], a[4 * m + 3]);
    }
    floatx4_g acc[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) acc[c] = (floatx4_g){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int c = 0; c < KT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_ws[(s * KT + c) * kWave + lane], a[s], acc[c], 0, 0, 0);
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int c = 0; c < KT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_wn[(s * KT + c) * kWave + lane], b[s], acc[c], 0, 0, 0);
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < KT; ++c) {
      float part = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float z = acc[c][j] + bias[c][j];
        if (RELU) z = z > 0.f ? z : 0.f;
        acc[c][j] = z;
        part = j == 0 ? z * z : fmaf(z, z, part);
      }
      part += __shfl_xor(part, 16, kWave);
      part += __shfl_xor(part, 32, kWave);
      ss = c == 0 ? part : ss + part;
    }
    const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    if (row < n_rows) {
#pragma unroll
      for (int c = 0; c < KT; ++c) {
        const float z0 = acc[c][0], z1 = acc[c][1], z2 = acc[c][2], z3 = acc[c][3];
        if (h_out) *reinterpret_cast<float4*>(h_out + (size_t)row * DO + 16 * c + 4 * q) = make_float4(z0, z1, z2, z3);
        if (norm_out)
          *reinterpret_cast<float4*>(norm_out + (size_t)row * norm_stride + 16 * c + 4 * q) =
              make_float4(z0 * inv, z1 * inv, z2 * inv, z3 * inv);
      }
    }
  };
  // two stages: the next tile's rows are requested before the current one is computed
  float a0[KS], b0[KS], a1[KS], b1[KS];
  load(t_begin, a0, b0);
  for (int32_t t = t_begin; t < t_end; t += 2) {
    if (t + 1 < t_end) load(t + 1, a1, b1);
    tile(t, a0, b0);
    if (t + 1 < t_end) {
      if (t + 2 < t_end) load(t + 2, a0, b0);
      tile(t + 1, a1, b1);
    }
  }
}

// --------------------------------------------------------------------------------------------- dropout of rows
__device__ __forceinline__ bool sage_keep(uint32_t seed, uint32_t index, uint32_t threshold) {
  // the counter hash of kgat_dense.hip's drop_keep (ops.dropout_keep_mask restates it)
  uint32_t x = (index * 0x9E3779B1u) ^ seed;
  x ^= x >> 16; x *= 0x85EBCA6Bu;
  x ^= x >> 13; x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x >= threshold;
}

__global__ __launch_bounds__(256) void dropout_rows_kernel(int64_t n, const float* __restrict__ x,
                                                           const float* __restrict__ x2, uint32_t threshold,
                                                           float keep_scale, uint32_t seed, float* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    float v = x[e];
    if (x2) v += x2[e];
    out[e] = sage_keep(seed, (uint32_t)e, threshold) ? v * keep_scale : 0.f;
  }
}

// --------------------------------------------------------------------------------------------- dense backward
// grad_self = G W_self, grad_agg = (G W_neigh) / max(deg, 1): the contraction runs over DO (the columns of G).
// Fragment order: s_w[(s * KT + c) * 64 + q * 16 + i] = W[16 (s >> 2) + 4q + (s & 3)][16c + i], KT = DI / 16, s < DO / 4.
template <int DI, int DO>
__device__ __forceinline__ void stage_bwd_weight(const float* __restrict__ W, float* s_w) {
  constexpr int KT = DI / 16;
  for (int idx = threadIdx.x * 4; idx < DO * DI; idx += 256 * 4) {
    const float4 v = *reinterpret_cast<const float4*>(W + idx);
    const int k = idx / DI, n0 = idx % DI;
    const int s = (k >> 4) * 4 + (k & 3), q = (k >> 2) & 3;
    const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = n0 + t;
      s_w[(s * KT + (n >> 4)) * kWave + q * 16 + (n & 15)] = vv[t];
    }
  }
}

template <int DI, int DO>
__global__ __launch_bounds__(256, sage_waves(DI, DO)) void sage_bwd_input_kernel(int32_t n_rows, const float* __restrict__ G,
                                                             const float* __restrict__ Ws, const float* __restrict__ Wn,
                                                             const int32_t* __restrict__ indptr,
                                                             float* __restrict__ g_self, float* __restrict__ g_agg) {
  constexpr int KS = DO / 4, KT = DI / 16;
  __shared__ float s_ws[KS * KT * kWave];
  __shared__ float s_wn[KS * KT * kWave];
  stage_bwd_weight<DI, DO>(Ws, s_ws);
  stage_bwd_weight<DI, DO>(Wn, s_wn);
  __syncthreads();
  const int lane = threadIdx.x % kWave;
  const int i = lane & 15, q = lane >> 4;
  const int64_t n_waves = (int64_t)gridDim.x * (256 / kWave);
  const int64_t wv = (int64_t)blockIdx.x * (256 / kWave) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int32_t n_tiles = (n_rows + 15) >> 4;
  const int32_t t_begin = (int32_t)((int64_t)n_tiles * wv / n_waves);
  const int32_t t_end = (int32_t)((int64_t)n_tiles * (wv + 1) / n_waves);
  for (int32_t t = t_begin; t < t_end; ++t) {
    int32_t r = (t << 4) + i;
    const bool valid = r < n_rows;
    r = valid ? r : n_rows - 1;
    float a[KS];
    const float4* pg = reinterpret_cast<const float4*>(G + (size_t)r * DO) + q;
#pragma unroll
    for (int m = 0; m < DO / 16; ++m) {
      const float4 v = pg[4 * m];
      a[4 * m + 0] = v.x; a[4 * m + 1] = v.y; a[4 * m + 2] = v.z; a[4 * m + 3] = v.w;
    }
    const int32_t deg = indptr[r + 1] - indptr[r];
    const float dinv = (float)(deg > 1 ? deg : 1);
    floatx4_g as[KT], an[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) as[c] = an[c] = (floatx4_g){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int c = 0; c < KT; ++c) {
        as[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_ws[(s * KT + c) * kWave + lane], a[s], as[c], 0, 0, 0);
        an[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_wn[(s * KT + c) * kWave + lane], a[s], an[c], 0, 0, 0);
      }
    if (valid) {
#pragma unroll
      for (int c = 0; c < KT; ++c) {
        *reinterpret_cast<float4*>(g_self + (size_t)r * DI + 16 * c + 4 * q) = make_float4(as[c][0], as[c][1], as[c][2], as[c][3]);
        *reinterpret_cast<float4*>(g_agg + (size_t)r * DI + 16 * c + 4 * q) =
            make_float4(an[c][0] / dinv, an[c][1] / dinv, an[c][2] / dinv, an[c][3] / dinv);
      }
    }
  }
}

// Weight gradients as per-workgroup partials (the layout of kgat_dense.hip's bi_bwd_weight_kernel): workgroup b walks
// the 64-row slabs b, b + n_partials, ... with the rows of G, H and HN staged in LDS; the contraction index of the
// MFMA is the row.  part_self[b] = sum G^T H, part_neigh[b] = sum G^T HN (DO x DI), part_bias[b] = column sums of G
// (summed row by row in slab order).
template <int DO, int DI>
__global__ __launch_bounds__(256) void sage_bwd_weight_kernel(int32_t n_rows, const float* __restrict__ G,
                                                              const float* __restrict__ H, const float* __restrict__ HN,
                                                              float* __restrict__ part_self, float* __restrict__ part_neigh,
                                                              float* __restrict__ part_bias) {
  constexpr int SLAB = 64;
  constexpr int LG = DO == 16 ? 16 : DO + 16, LP = DI == 16 ? 16 : DI + 16;
  constexpr int TM = DO / 16, TN = DI / 16, TT = TM * TN;
  constexpr int TPW = (TT + 3) / 4;
  __shared__ float s_g[SLAB * LG];
  __shared__ float s_h[SLAB * LP];
  __shared__ float s_n[SLAB * LP];
  const int tid = threadIdx.x, lane = tid % kWave, w = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int i = lane & 15, q = lane >> 4;
  const int32_t n_slabs = (n_rows + SLAB - 1) / SLAB;
  floatx4_g acc_s[TPW], acc_n[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) acc_s[t] = acc_n[t] = (floatx4_g){0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  for (int32_t slab = blockIdx.x; slab < n_slabs; slab += gridDim.x) {
    const int32_t r0 = slab * SLAB;
    __syncthreads();  // the previous slab has been read
    for (int e = tid * 4; e < SLAB * DO; e += 256 * 4) {
      const int32_t r = r0 + e / DO;
      *reinterpret_cast<float4*>(&s_g[(e / DO) * LG + e % DO]) =
          r < n_rows ? *reinterpret_cast<const float4*>(G + (size_t)r * DO + e % DO) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int e = tid * 4; e < SLAB * DI; e += 256 * 4) {
      const int32_t r = r0 + e / DI;
      const bool in = r < n_rows;
      *reinterpret_cast<float4*>(&s_h[(e / DI) * LP + e % DI]) =
          in ? *reinterpret_cast<const float4*>(H + (size_t)r * DI + e % DI) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(&s_n[(e / DI) * LP + e % DI]) =
          in ? *reinterpret_cast<const float4*>(HN + (size_t)r * DI + e % DI) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    if (tid < DO) {
      for (int r = 0; r < SLAB; ++r) bsum += s_g[r * LG + tid];
    }
    if (w < TT) {
#pragma unroll 4
      for (int k0 = 0; k0 < SLAB; k0 += 4) {
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          const int tl = w + 4 * t;
          if (tl < TT) {
            const int cm = tl / TN, cn = tl % TN;
            const float a = s_g[(k0 + q) * LG + 16 * cm + i];
            acc_s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, s_h[(k0 + q) * LP + 16 * cn + i], acc_s[t], 0, 0, 0);
            acc_n[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, s_n[(k0 + q) * LP + 16 * cn + i], acc_n[t], 0, 0, 0);
          }
        }
      }
    }
  }
  float* ps = part_self + (size_t)blockIdx.x * DO * DI;
  float* pn = part_neigh + (size_t)blockIdx.x * DO * DI;
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int tl = w + 4 * t;
    if (tl < TT) {
      const int cm = tl / TN, cn = tl % TN;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ps[(size_t)(16 * cm + 4 * q + j) * DI + 16 * cn + i] = acc_s[t][j];
        pn[(size_t)(16 * cm + 4 * q + j) * DI + 16 * cn + i] = acc_n[t][j];
      }
    }
  }
  if (tid < DO) part_bias[(size_t)blockIdx.x * DO + tid] = bsum;
}

static bool sage_width(int d) { return d == 16 || d == 32 || d == 64 || d == 128; }

}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_sage_dense_supported(int d_in, int d_out) { return sage_width(d_in) && sage_width(d_out) ? 1 : 0; }

int kgat_sage_dense_f32(int64_t n_rows, int d_in, int d_out, const float* H, const float* HN, const float* W_self,
                        const float* W_neigh, const float* b_self, const float* b_neigh, int act, float* h_out,
                        float* norm_out, int64_t norm_stride, float* self_out, int64_t self_stride,
                        kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_rows >= 0 && n_rows < INT32_MAX && d_in > 0 && d_out > 0, "sage_dense: bad size");
  KGAT_CHECK_ARG(act == KGAT_ACT_NONE || act == KGAT_ACT_RELU, "sage_dense: unknown activation %d", act);
  KGAT_CHECK_ARG(norm_out == nullptr || (norm_stride >= d_out && norm_stride % 4 == 0 && aligned16(norm_out)),
                 "sage_dense: norm_out must be 16-byte aligned with a row stride that is a multiple of 4 floats >= d_out");
  KGAT_CHECK_ARG(self_out == nullptr || (self_stride >= d_in && self_stride % 4 == 0 && aligned16(self_out)),
                 "sage_dense: self_out must be 16-byte aligned with a row stride that is a multiple of 4 floats >= d_in");
  if (!kgat_sage_dense_supported(d_in, d_out)) {
    set_error("sage_dense: unsupported widths %d -> %d (d_in, d_out in {16, 32, 64, 128})", d_in, d_out);
    return KGAT_E_UNSUPPORTED;
  }
  if (n_rows == 0) return KGAT_OK;
  KGAT_CHECK_ARG(H && HN && W_self && W_neigh, "sage_dense: null pointer");
  KGAT_CHECK_ARG(aligned16(H) && aligned16(HN) && aligned16(W_self) && aligned16(W_neigh) &&
                     (h_out == nullptr || aligned16(h_out)),
                 "sage_dense: H, HN, W_self, W_neigh and h_out must be 16-byte aligned");
  const int64_t tiles = (n_rows + 15) / 16;
  int64_t blocks = (tiles + 3) / 4;
  if (blocks > 512) blocks = 512;
  const int rc = dispatch_widths(MfmaWidths{}, d_in, d_out, [&](auto di, auto dout) -> int {
    constexpr int DI = decltype(di)::value, DO = decltype(dout)::value;
    if (act == KGAT_ACT_RELU)
      hipLaunchKernelGGL((sage_dense_kernel<DI, DO, true>), dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                         (int32_t)n_rows, H, HN, W_self, W_neigh, b_self, b_neigh, h_out, norm_out, norm_stride,
                         self_out, self_stride);
    else
      hipLaunchKernelGGL((sage_dense_kernel<DI, DO, false>), dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                         (int32_t)n_rows, H, HN, W_self, W_neigh, b_self, b_neigh, h_out, norm_out, norm_stride,
                         self_out, self_stride);
    KGAT_CHECK_LAUNCH("sage_dense");
    return KGAT_OK;
  });
  if (rc == KGAT_E_UNSUPPORTED) set_error("sage_dense: unsupported widths %d -> %d", d_in, d_out);
  return rc;
}

int kgat_dropout_rows_f32(int64_t n_rows, int d, const float* x, const float* x2, float drop_p, uint64_t seed,
                          float* out, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_rows >= 0 && d > 0 && (uint64_t)n_rows * (uint64_t)d < (1ull << 32), "dropout_rows: bad size");
  KGAT_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "dropout_rows: dropout probability outside [0, 1)");
  if (n_rows == 0) return KGAT_OK;
  KGAT_CHECK_ARG(x && out, "dropout_rows: null pointer");
  const double t = (double)drop_p * 4294967296.0;
  const uint32_t threshold = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
  const float keep_scale = 1.f / (1.f - drop_p);
  const uint32_t seed32 = (uint32_t)(seed ^ (seed >> 32));
  const int64_t n = n_rows * d;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(dropout_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), n, x, x2, threshold,
                     keep_scale, seed32, out);
  KGAT_CHECK_LAUNCH("dropout_rows");
  return KGAT_OK;
}

int kgat_sage_bwd_input_f32(int64_t n_rows, int d_in, int d_out, const float* grad_pre, const float* W_self,
                            const float* W_neigh, const int32_t* indptr, float* grad_self, float* grad_agg,
                            kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_rows >= 0 && n_rows < INT32_MAX && d_in > 0 && d_out > 0, "sage_bwd_input: bad size");
  if (!kgat_sage_dense_supported(d_in, d_out)) {
    set_error("sage_bwd_input: unsupported widths %d -> %d", d_in, d_out);
    return KGAT_E_UNSUPPORTED;
  }
  if (n_rows == 0) return KGAT_OK;
  KGAT_CHECK_ARG(grad_pre && W_self && W_neigh && indptr && grad_self && grad_agg, "sage_bwd_input: null pointer");
  KGAT_CHECK_ARG(aligned16(grad_pre) && aligned16(W_self) && aligned16(W_neigh) && aligned16(grad_self) &&
                     aligned16(grad_agg),
                 "sage_bwd_input: buffers must be 16-byte aligned");
  const int64_t tiles = (n_rows + 15) / 16;
  int64_t blocks = (tiles + 3) / 4;
  if (blocks > 512) blocks = 512;
  const int rc = dispatch_widths(MfmaWidths{}, d_in, d_out, [&](auto di, auto dout) -> int {
    hipLaunchKernelGGL((sage_bwd_input_kernel<decltype(di)::value, decltype(dout)::value>), dim3((unsigned)blocks),
                       dim3(256), 0, as_stream(stream), (int32_t)n_rows, grad_pre, W_self, W_neigh, indptr, grad_self,
                       grad_agg);
    KGAT_CHECK_LAUNCH("sage_bwd_input");
    return KGAT_OK;
  });
  if (rc == KGAT_E_UNSUPPORTED) set_error("sage_bwd_input: unsupported widths %d -> %d", d_in, d_out);
  return rc;
}

int kgat_sage_bwd_weight_f32(int64_t n_rows, int d_in, int d_out, const float* grad_pre, const float* H,
                             const float* HN, float* part_self, float* part_neigh, float* part_bias, int64_t n_partials,
                             kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_rows >= 0 && n_rows < INT32_MAX && d_in > 0 && d_out > 0, "sage_bwd_weight: bad size");
  KGAT_CHECK_ARG(n_partials == kgat_bi_interaction_bwd_weight_partials(n_rows),
                 "sage_bwd_weight: n_partials must be kgat_bi_interaction_bwd_weight_partials(n_rows)");
  if (!kgat_sage_dense_supported(d_in, d_out)) {
    set_error("sage_bwd_weight: unsupported widths %d -> %d", d_in, d_out);
    return KGAT_E_UNSUPPORTED;
  }
  KGAT_CHECK_ARG(part_self && part_neigh && part_bias && (n_rows == 0 || (grad_pre && H && HN)),
                 "sage_bwd_weight: null pointer");
  KGAT_CHECK_ARG(n_rows == 0 || (aligned16(grad_pre) && aligned16(H) && aligned16(HN)),
                 "sage_bwd_weight: buffers must be 16-byte aligned");
  const int rc = dispatch_widths(MfmaWidths{}, d_out, d_in, [&](auto dout, auto di) -> int {
    hipLaunchKernelGGL((sage_bwd_weight_kernel<decltype(dout)::value, decltype(di)::value>), dim3((unsigned)n_partials),
                       dim3(256), 0, as_stream(stream), (int32_t)n_rows, grad_pre, H, HN, part_self, part_neigh,
                       part_bias);
    KGAT_CHECK_LAUNCH("sage_bwd_weight");
    return KGAT_OK;
  });
  if (rc == KGAT_E_UNSUPPORTED) set_error("sage_bwd_weight: unsupported widths %d -> %d", d_in, d_out);
  return rc;
}

}  // extern "C"
