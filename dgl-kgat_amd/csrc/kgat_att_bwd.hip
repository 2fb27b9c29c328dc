// Backward of the attention logits (reference models.py:135-154 under autograd) for gfx950.
//
//   p = ent[h] W_r + rel[r]    T = tanh(p)    V = W_r T    logit_e = ent[t] . V        (the folded forward's T and V)
//
// With gamma_e the gradient arriving at the logit, the backward factorises over the (head, relation) groups G of
// kgat_head_groups:
//   A_G = sum_{e in G} gamma_e ent[t(e)]      B_G = A_G W_r      dP_G = B_G * (1 - T_G^2)      H_G = dP_G W_r^T
//   grad ent[t(e)] += gamma_e V_G   (per edge)        grad ent[h] += H_G   (per group)
//   grad rel[r] += dP_G                               grad W_r += A_G^T (x) T_G + ent[h]^T (x) dP_G
//
// Four steps on one stream, no float atomics, every sum in a fixed order (bitwise reproducible):
//  1. A_tab[G] = sum over the group's grouped positions of gamma_p ent[src_g[p]]: the aggregation kernel
//     (kgat_spmm_umule_sum_f32) with indptr = first position of each group, col = src_g, row id = gid.
//  2. att_bwd_dense_kernel (this file, v_mfma_f32_16x16x4_f32): tiles of at most 16 consecutive groups of one
//     relation.  A workgroup owns a contiguous tile range, keeps W_r in LDS while the relation lasts, recomputes T
//     from ent[h] (nothing is saved by the forward), writes the tile's V and H rows to a table and accumulates its
//     grad W_r / grad rel contribution in registers; it flushes to partial slot (workgroup + relation) when the
//     relation changes - at most n_workgroups + R slots, each written once.
//  3. att_bwd_reduce_kernel: grad W_r / grad rel = the slots of the relation's workgroups, summed in workgroup order;
//     relations without a group are written as zeros.
//  4. grad_ent[n] = sum_{out-edges p of n} gamma_p V[gid[p]] + sum_{groups G headed by n} H_G: the aggregation kernel
//     again, over a graph-static CSR whose columns index the [V ; H] table (2 n_groups rows) and whose weight stream
//     is [gamma ; 1.0] read through an index (its `eid` argument): the caller's gradient buffer has one float of room
//     after the scored positions and the call writes the 1.0 there, so no pass over E copies gamma.  Rows without an
//     entry are written as zeros.
#include "kgat_att_common.h"
#include "kgat_common.h"

namespace kgat {

typedef float floatx4_b __attribute__((ext_vector_type(4)));

constexpr int kBwdGpt = 16;  // groups per tile (the M of the MFMA)

// one thread: tile prefix per relation (16 groups per tile, relations kept apart) and the constant weight 1.0 that
// follows gamma in the weight stream of step 4
__global__ void att_bwd_prep_kernel(int n_rel, const int32_t* __restrict__ gptr, int32_t* __restrict__ bptr,
                                    float* __restrict__ one) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int32_t run = 0;
  bptr[0] = 0;
  for (int r = 0; r < n_rel; ++r) {
    run += (gptr[r + 1] - gptr[r] + kBwdGpt - 1) / kBwdGpt;
    bptr[r + 1] = run;
  }
  *one = 1.0f;
}

__device__ __forceinline__ int32_t bwd_tiles_per_wg(int32_t n_tiles, int32_t n_wg) { return (n_tiles + n_wg - 1) / n_wg; }

// Lane maps of v_mfma_f32_16x16x4_f32 (i = lane & 15, q = lane >> 4): A operand A[m = i][k = q], B operand
// B[k = q][n = i], result register j = C[m = 4 q + j][n = i].  The products that sum over the relation-space index
// take four consecutive k per lane group (k = k0 + 4 q + s in step s): both operands then come as one 16-byte LDS read.
template <int D>
__global__ __launch_bounds__(256) void att_bwd_dense_kernel(int n_rel, const int32_t* __restrict__ gptr,
                                                            const int32_t* __restrict__ bptr,
                                                            const int32_t* __restrict__ g_node,
                                                            const float* __restrict__ ent, const float* __restrict__ W_R,
                                                            const float* __restrict__ rel, const float* __restrict__ A_tab,
                                                            float* __restrict__ VH, int64_t n_groups,
                                                            float* __restrict__ partW, float* __restrict__ partR) {
  constexpr int LD = D + 4;  // row stride in LDS: rows stay 16-byte aligned, columns spread over the banks
  constexpr int NB = D / 16, TT = NB * NB, TPW = (TT + 3) / 4;
  __shared__ __attribute__((aligned(16))) float s_w[D * LD];
  __shared__ __attribute__((aligned(16))) float s_e[kBwdGpt * LD];
  __shared__ __attribute__((aligned(16))) float s_a[kBwdGpt * LD];
  __shared__ __attribute__((aligned(16))) float s_t[kBwdGpt * LD];
  __shared__ __attribute__((aligned(16))) float s_p[kBwdGpt * LD];
  __shared__ float s_rel[D];
  const int tid = threadIdx.x, lane = tid % kWave, w = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int i = lane & 15, q = lane >> 4;
  const int32_t n_tiles = bptr[n_rel];
  const int32_t tpw = bwd_tiles_per_wg(n_tiles, (int32_t)gridDim.x);
  const int32_t t0 = (int32_t)blockIdx.x * tpw;
  const int32_t t1 = t0 + tpw < n_tiles ? t0 + tpw : n_tiles;
  if (t0 >= t1) return;
  int r = segment_of(bptr, n_rel, t0);  // the relation of tile t0
  int r_held = -1;
  floatx4_b acc[TPW];
  float rsum = 0.f;
  for (int32_t t = t0; t < t1; ++t) {
    while (bptr[r + 1] <= t) ++r;  // (skips relations without a tile)
    __syncthreads();               // the previous tile has been read
    if (r != r_held) {
      if (r_held >= 0) {
        float* pw = partW + (size_t)(blockIdx.x + r_held) * D * D;
#pragma unroll
        for (int c = 0; c < TPW; ++c) {
          const int tl = w + 4 * c;
          if (tl < TT) {
            const int cm = tl / NB, cn = tl % NB;
#pragma unroll
            for (int j = 0; j < 4; ++j) pw[(size_t)(16 * cm + 4 * q + j) * D + 16 * cn + i] = acc[c][j];
          }
        }
        if (tid < D) partR[(size_t)(blockIdx.x + r_held) * D + tid] = rsum;
      }
#pragma unroll
      for (int c = 0; c < TPW; ++c) acc[c] = (floatx4_b){0.f, 0.f, 0.f, 0.f};
      rsum = 0.f;
      r_held = r;
      const float* Wr = W_R + (size_t)r * D * D;
      for (int e = tid * 4; e < D * D; e += 256 * 4)
        *reinterpret_cast<float4*>(&s_w[(e / D) * LD + e % D]) = *reinterpret_cast<const float4*>(Wr + e);
      if (tid < D) s_rel[tid] = rel[(size_t)r * D + tid];
    }
    const int32_t g0 = gptr[r] + (t - bptr[r]) * kBwdGpt;
    const int32_t ng = gptr[r + 1] - g0 < kBwdGpt ? gptr[r + 1] - g0 : kBwdGpt;
    for (int e = tid * 4; e < kBwdGpt * D; e += 256 * 4) {
      const int row = e / D, c = e % D;
      float4 ve = make_float4(0.f, 0.f, 0.f, 0.f), va = ve;
      if (row < ng) {
        ve = *reinterpret_cast<const float4*>(ent + (size_t)g_node[g0 + row] * D + c);
        va = *reinterpret_cast<const float4*>(A_tab + (size_t)(g0 + row) * D + c);
      }
      *reinterpret_cast<float4*>(&s_e[row * LD + c]) = ve;
      *reinterpret_cast<float4*>(&s_a[row * LD + c]) = va;
    }
    __syncthreads();
    // P = ent[h] W_r, B = A W_r (sum over the entity-space index); T = tanh(P + rel), dP = B (1 - T^2)
    for (int nb = w; nb < NB; nb += 4) {
      floatx4_b ap = {0.f, 0.f, 0.f, 0.f}, ab = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int k0 = 0; k0 < D; k0 += 4) {
        const float b = s_w[(k0 + q) * LD + 16 * nb + i];
        ap = __builtin_amdgcn_mfma_f32_16x16x4f32(s_e[i * LD + k0 + q], b, ap, 0, 0, 0);
        ab = __builtin_amdgcn_mfma_f32_16x16x4f32(s_a[i * LD + k0 + q], b, ab, 0, 0, 0);
      }
      const float rv = s_rel[16 * nb + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float tv = tanhf(ap[j] + rv);
        s_t[(4 * q + j) * LD + 16 * nb + i] = tv;
        s_p[(4 * q + j) * LD + 16 * nb + i] = ab[j] * (1.f - tv * tv);
      }
    }
    __syncthreads();
    // V = T W_r^T, H = dP W_r^T (sum over the relation-space index): rows of the [V ; H] table
    for (int nb = w; nb < NB; nb += 4) {
      floatx4_b av = {0.f, 0.f, 0.f, 0.f}, ah = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
      for (int k0 = 0; k0 < D; k0 += 16) {
        const float4 wb = *reinterpret_cast<const float4*>(&s_w[(16 * nb + i) * LD + k0 + 4 * q]);
        const float4 tv = *reinterpret_cast<const float4*>(&s_t[i * LD + k0 + 4 * q]);
        const float4 pv = *reinterpret_cast<const float4*>(&s_p[i * LD + k0 + 4 * q]);
        av = __builtin_amdgcn_mfma_f32_16x16x4f32(tv.x, wb.x, av, 0, 0, 0);
        ah = __builtin_amdgcn_mfma_f32_16x16x4f32(pv.x, wb.x, ah, 0, 0, 0);
        av = __builtin_amdgcn_mfma_f32_16x16x4f32(tv.y, wb.y, av, 0, 0, 0);
        ah = __builtin_amdgcn_mfma_f32_16x16x4f32(pv.y, wb.y, ah, 0, 0, 0);
        av = __builtin_amdgcn_mfma_f32_16x16x4f32(tv.z, wb.z, av, 0, 0, 0);
        ah = __builtin_amdgcn_mfma_f32_16x16x4f32(pv.z, wb.z, ah, 0, 0, 0);
        av = __builtin_amdgcn_mfma_f32_16x16x4f32(tv.w, wb.w, av, 0, 0, 0);
        ah = __builtin_amdgcn_mfma_f32_16x16x4f32(pv.w, wb.w, ah, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 4 * q + j;
        if (row < ng) {
          VH[(size_t)(g0 + row) * D + 16 * nb + i] = av[j];
          VH[(size_t)(n_groups + g0 + row) * D + 16 * nb + i] = ah[j];
        }
      }
    }
    // grad W_r += A^T T + ent[h]^T dP (sum over the tile's groups; rows past the last group are zeros in A and dP),
    // grad rel += column sums of dP
    if (tid < D) {
      for (int g = 0; g < kBwdGpt; ++g) rsum += s_p[g * LD + tid];
    }
#pragma unroll
    for (int k0 = 0; k0 < kBwdGpt; k0 += 4) {
#pragma unroll
      for (int c = 0; c < TPW; ++c) {
        const int tl = w + 4 * c;
        if (tl < TT) {
          const int cm = tl / NB, cn = tl % NB;
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_a[(k0 + q) * LD + 16 * cm + i], s_t[(k0 + q) * LD + 16 * cn + i],
                                                        acc[c], 0, 0, 0);
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_e[(k0 + q) * LD + 16 * cm + i], s_p[(k0 + q) * LD + 16 * cn + i],
                                                        acc[c], 0, 0, 0);
        }
      }
    }
  }
  float* pw = partW + (size_t)(blockIdx.x + r_held) * D * D;
#pragma unroll
  for (int c = 0; c < TPW; ++c) {
    const int tl = w + 4 * c;
    if (tl < TT) {
      const int cm = tl / NB, cn = tl % NB;
#pragma unroll
      for (int j = 0; j < 4; ++j) pw[(size_t)(16 * cm + 4 * q + j) * D + 16 * cn + i] = acc[c][j];
    }
  }
  if (tid < D) partR[(size_t)(blockIdx.x + r_held) * D + tid] = rsum;
}

// grad W_r (dd floats per relation) and grad rel (k floats): the partial slots of the workgroups whose tile range
// meets the relation's, in workgroup order.  blockIdx.y = relation.
__global__ __launch_bounds__(256) void att_bwd_reduce_kernel(int n_rel, int dd, int k, int32_t n_wg,
                                                             const int32_t* __restrict__ bptr,
                                                             const float* __restrict__ partW,
                                                             const float* __restrict__ partR, float* __restrict__ grad_W,
                                                             float* __restrict__ grad_rel) {
  const int r = blockIdx.y;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= dd + k) return;
  const int32_t b0 = bptr[r], b1 = bptr[r + 1];
  float s = 0.f;
  if (b1 > b0) {
    const int32_t tpw = bwd_tiles_per_wg(bptr[n_rel], n_wg);
    const int32_t w0 = b0 / tpw, w1 = (b1 - 1) / tpw;
    if (e < dd) {
      for (int32_t wg = w0; wg <= w1; ++wg) s += partW[(size_t)(wg + r) * dd + e];
    } else {
      for (int32_t wg = w0; wg <= w1; ++wg) s += partR[(size_t)(wg + r) * k + (e - dd)];
    }
  }
  if (e < dd) grad_W[(size_t)r * dd + e] = s;
  else grad_rel[(size_t)r * k + (e - dd)] = s;
}

// workgroups of the dense kernel: a function of the sizes and of the device's compute-unit count (the partial slots and
// the summation order follow it, so results are bitwise reproducible on one device model, not across models).  Per
// compute unit: what the kernel's registers and LDS let be resident at once (d = 64: 138 VGPRs -> 3 waves per SIMD;
// d = 128: 256 VGPRs and 102 KB of LDS -> 1; d <= 32: 5-6 waves per SIMD) - a choice by occupancy, not a tuned one.
static int bwd_workgroups(int64_t n_groups, int d, int n_rel) {
  const int64_t tiles_max = n_groups / kBwdGpt + n_rel;
  int64_t n = (tiles_max + 3) / 4;  // a few tiles per workgroup on small graphs: W_r is staged once per range
  const int64_t cap = (int64_t)device_cu_count() * (d == 128 ? 1 : (d == 64 ? 3 : 5));
  if (n > cap) n = cap;
  return (int)(n < 1 ? 1 : n);
}

struct BwdCarve {
  float *A_tab, *VH, *partW, *partR;
  int32_t* bptr;
  void* spmm_ws;
  size_t spmm_bytes, total;
};

static BwdCarve bwd_carve(void* base, int64_t n_scored, int64_t n_groups, int d, int k, int n_rel) {
  Carver cv(base);
  BwdCarve c;
  const size_t ng = (size_t)(n_groups > 0 ? n_groups : 0);
  const size_t slots = (size_t)bwd_workgroups(n_groups, d, n_rel) + (size_t)n_rel;
  c.A_tab = cv.take<float>(ng * d + 4);
  c.VH = cv.take<float>(2 * ng * d + 4);
  c.bptr = cv.take<int32_t>((size_t)n_rel + 2);
  c.partW = cv.take<float>(slots * d * k);
  c.partR = cv.take<float>(slots * k);
  const size_t s1 = kgat_spmm_workspace_bytes(n_scored, d), s2 = kgat_spmm_workspace_bytes(n_scored + n_groups, d);
  c.spmm_bytes = s1 > s2 ? s1 : s2;
  c.spmm_ws = cv.take<char>(c.spmm_bytes);
  c.total = cv.off + 256;  // what kgat_att_score_bwd_workspace_bytes answers is what the entry asks for
  return c;
}

}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_att_score_bwd_supported(int64_t n_nodes, int d, int k, int n_rel) {
  return n_nodes >= 0 && att_shape_ok(n_nodes, d, k, n_rel, AttWidths128{});
}

size_t kgat_att_score_bwd_workspace_bytes(int64_t n_nodes, int64_t n_scored, int64_t n_groups, int d, int k, int n_rel) {
  if (!kgat_att_score_bwd_supported(n_nodes, d, k, n_rel) || n_scored < 0 || n_groups < 0) return 256;
  return bwd_carve(nullptr, n_scored, n_groups, d, k, n_rel).total;
}

int kgat_att_score_bwd_f32(int64_t n_nodes, int64_t n_scored, int64_t n_groups, int d, int k, int n_rel,
                           const int32_t* src_g, const int32_t* gid, const int32_t* gstart, const int32_t* gptr,
                           const int32_t* g_node, const int32_t* node_ptr, const int32_t* node_col,
                           const int32_t* node_row, const int32_t* node_wsrc, const float* ent, const float* W_R,
                           const float* rel, float* grad_logits_g, float* grad_ent, float* grad_W_R,
                           float* grad_rel, void* workspace, size_t workspace_bytes, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_nodes >= 0 && n_scored >= 0 && n_groups >= 0 && n_groups <= n_scored &&
                     n_scored + n_groups < INT32_MAX - 1,
                 "att_score_bwd: bad size");
  if (!kgat_att_score_bwd_supported(n_nodes, d, k, n_rel)) {
    set_error("att_score_bwd: needs d == k in {16,32,64,128}, 0 < R <= %d, N*d*4 < 4 GiB (N=%lld d=%d k=%d R=%d)",
              kAttMaxRelLds, (long long)n_nodes, d, k, n_rel);
    return KGAT_E_UNSUPPORTED;
  }
  KGAT_CHECK_ARG((n_scored == 0) == (n_groups == 0), "att_score_bwd: scored positions and groups go together");
  KGAT_CHECK_ARG(gptr && W_R && rel && grad_W_R && grad_rel && workspace, "att_score_bwd: null pointer");
  KGAT_CHECK_ARG(n_nodes == 0 || (ent && grad_ent && node_ptr), "att_score_bwd: null pointer");
  KGAT_CHECK_ARG(grad_logits_g != nullptr, "att_score_bwd: null pointer (grad_logits_g holds n_scored + 1 floats)");
  KGAT_CHECK_ARG(n_scored == 0 || (src_g && gid && gstart && g_node && node_col && node_row && node_wsrc),
                 "att_score_bwd: null pointer");
  KGAT_CHECK_ARG((reinterpret_cast<uintptr_t>(ent) & 15u) == 0 && (reinterpret_cast<uintptr_t>(W_R) & 15u) == 0 &&
                     (reinterpret_cast<uintptr_t>(grad_ent) & 15u) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0,
                 "att_score_bwd: ent, W_R, grad_ent and the workspace must be 16-byte aligned");
  const BwdCarve c = bwd_carve(workspace, n_scored, n_groups, d, k, n_rel);
  if (workspace_bytes < c.total) {
    set_error("att_score_bwd: workspace too small (%zu < %zu)", workspace_bytes, c.total);
    return KGAT_E_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(att_bwd_prep_kernel, dim3(1), dim3(64), 0, st, n_rel, gptr, c.bptr, grad_logits_g + n_scored);
  KGAT_CHECK_LAUNCH("att_bwd_prep");
  int rc;
  if (n_scored > 0) {
    // 1. A_tab: rows = groups, positions = the scored grouped positions
    rc = kgat_spmm_umule_sum_f32(n_groups, 0, 0, n_scored, d, gstart, src_g, gid, nullptr, ent, grad_logits_g, c.A_tab, nullptr,
                                 c.spmm_ws, c.spmm_bytes, 0, KGAT_SPMM_ALGO_AUTO, nullptr, 0, stream);
    if (rc != KGAT_OK) return rc;
    // 2. the dense part per tile
    const int n_wg = bwd_workgroups(n_groups, d, n_rel);
#define KGAT_BWD_LAUNCH(D_)                                                                                           \
  hipLaunchKernelGGL((att_bwd_dense_kernel<D_>), dim3((unsigned)n_wg), dim3(256), 0, st, n_rel, gptr,                 \
                     (const int32_t*)c.bptr, g_node, ent, W_R, rel, (const float*)c.A_tab, c.VH, n_groups, c.partW, \
                     c.partR)
    switch (d) {
      case 16: KGAT_BWD_LAUNCH(16); break;
      case 32: KGAT_BWD_LAUNCH(32); break;
      case 64: KGAT_BWD_LAUNCH(64); break;
      default: KGAT_BWD_LAUNCH(128); break;
    }
#undef KGAT_BWD_LAUNCH
    KGAT_CHECK_LAUNCH("att_bwd_dense");
  }
  // 3. grad W_R, grad rel (zeros for relations without a group)
  {
    const int n_wg = bwd_workgroups(n_groups, d, n_rel);
    const int elems = d * k + k;
    hipLaunchKernelGGL(att_bwd_reduce_kernel, dim3((unsigned)((elems + 255) / 256), (unsigned)n_rel), dim3(256), 0, st,
                       n_rel, d * k, k, (int32_t)n_wg, (const int32_t*)c.bptr, (const float*)c.partW,
                       (const float*)c.partR, grad_W_R, grad_rel);
    KGAT_CHECK_LAUNCH("att_bwd_reduce");
  }
  // 4. grad_ent: tail role per out-edge + head role per group, one fixed-order row sum
  rc = kgat_spmm_umule_sum_f32(n_nodes, 0, 0, n_scored + n_groups, d, node_ptr, node_col, node_row, node_wsrc, c.VH,
                               grad_logits_g, grad_ent, nullptr, c.spmm_ws, c.spmm_bytes, 0, KGAT_SPMM_ALGO_AUTO, nullptr, 0,
                               stream);
  return rc;
}

}  // extern "C"
