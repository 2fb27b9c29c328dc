// The pieces the fused train-and-step iterations share (kgat_transr.hip, kgat_transe.hip, kgat_bpr.hip) and, where it
// is the same thing, the one-launch optimiser (kgat_optim.hip).  The design: the per-sample kernel writes gradient rows
// at SORTED positions, so the contributions of one table row are consecutive; workgroups riding in that launch tag the
// batch's rows in `row_slot`; the Adam launch streams p, m, v of every element - torch's dense Adam moves every row -
// and forms a row's gradient on the way: 0 unless the row's word carries this call's tag, else the ordered sum of the
// row's run.  Every sum has a fixed order: no float atomics, bitwise reproducible.  Not part of the ABI.
#pragma once
#include <math.h>

#include "kgat_adam_common.h"

namespace kgat {

constexpr int kAdamChunk = 4096;  // elements per workgroup of an Adam launch: 256 threads x 4 float4

__device__ __forceinline__ int32_t clamp_i32(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- the Adam launch

// Elements [i, i + 4) of one tensor, 16-byte aligned: gradient gg, one 16-byte access per stream.
__device__ __forceinline__ void adam_four(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, int64_t i,
                                          float4 gg, float w1, float beta2, float w2, float ss, float bs, float eps) {
  float4 pp = *reinterpret_cast<const float4*>(p + i);
  float4 mm = *reinterpret_cast<const float4*>(m + i);
  float4 vv = *reinterpret_cast<const float4*>(v + i);
  adam_one(pp.x, gg.x, mm.x, vv.x, w1, beta2, w2, ss, bs, eps);
  adam_one(pp.y, gg.y, mm.y, vv.y, w1, beta2, w2, ss, bs, eps);
  adam_one(pp.z, gg.z, mm.z, vv.z, w1, beta2, w2, ss, bs, eps);
  adam_one(pp.w, gg.w, mm.w, vv.w, w1, beta2, w2, ss, bs, eps);
  *reinterpret_cast<float4*>(p + i) = pp;
  *reinterpret_cast<float4*>(m + i) = mm;
  *reinterpret_cast<float4*>(v + i) = vv;
}

// The tensors of one Adam launch: workgroup b works on tensor t, first_block[t] <= b < first_block[t + 1], and there
// on elements [(b - first_block[t]) kAdamChunk, + kAdamChunk).
template <int N>
struct AdamTensors {
  float *p[N], *m[N], *v[N];
  int64_t n[N];
  int first_block[N + 1];
  float step_size[N];   // lr / (1 - beta1^t)
  float bc2_sqrt[N];    // sqrt(1 - beta2^t)
  int count;
};

// One workgroup's kAdamChunk elements of tensor t (whose size is a multiple of 4): lane l takes the 16 bytes at
// 1024 k + 4 l, k = 0..3, of each stream; grad_at(i) is the float4 gradient of elements [i, i + 4).
template <int N, typename GradAt>
__device__ __forceinline__ void adam_chunk_walk(const AdamTensors<N>& a, int t, float w1, float beta2, float w2, float eps,
                                                GradAt grad_at) {
  const int64_t base = (int64_t)((int)blockIdx.x - a.first_block[t]) * kAdamChunk;
  float* __restrict__ p = a.p[t];
  float* __restrict__ m = a.m[t];
  float* __restrict__ v = a.v[t];
  const int64_t n = a.n[t];
  const float ss = a.step_size[t], bs = a.bc2_sqrt[t];
#pragma unroll
  for (int k = 0; k < kAdamChunk / 1024; ++k) {
    const int64_t i = base + (int64_t)k * 1024 + threadIdx.x * 4;
    if (i >= n) break;
    adam_four(p, m, v, i, grad_at(i), w1, beta2, w2, ss, bs, eps);
  }
}

// Host side: the hyper-parameter check, then tensor after tensor into `a` - state and (vector_only: the fused
// iterations have no scalar arm) alignment checks, the first_block table, the step-dependent scalars formed in double
// as torch.optim.adam forms them (python floats), then fp32 in the kernels.  Empty tensors are left out; kept[c] (if
// given) is the caller's index of the record's tensor c.  The launch's workgroup count is a.first_block[a.count].
template <int N>
int adam_fill(const char* who, AdamTensors<N>& a, int n_tensors, const int64_t* sizes, float* const* params,
              float* const* exp_avg, float* const* exp_avg_sq, const int64_t* steps, double lr, double beta1, double beta2,
              double eps, bool vector_only, int* kept = nullptr) {
  KGAT_CHECK_ARG(n_tensors >= 0 && n_tensors <= N, "%s: %d tensors (at most %d per call)", who, n_tensors, N);
  KGAT_CHECK_ARG(lr >= 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps >= 0, "%s: bad hyperparameter", who);
  a.count = 0;
  int blocks = 0;
  for (int t = 0; t < n_tensors; ++t) {
    KGAT_CHECK_ARG(sizes[t] >= 0 && steps[t] >= 1, "%s: tensor %d: bad size, or a step count after this step below 1", who, t);
    if (sizes[t] == 0) continue;
    KGAT_CHECK_ARG(params[t] && exp_avg[t] && exp_avg_sq[t], "%s: tensor %d: null pointer", who, t);
    KGAT_CHECK_ARG(!vector_only || (sizes[t] % 4 == 0 && aligned16(params[t]) && aligned16(exp_avg[t]) && aligned16(exp_avg_sq[t])),
                   "%s: tensor %d: parameters and moments must be 16-byte aligned", who, t);
    const int c = a.count++;
    if (kept) kept[c] = t;
    a.p[c] = params[t]; a.m[c] = exp_avg[t]; a.v[c] = exp_avg_sq[t];
    a.n[c] = sizes[t];
    a.first_block[c] = blocks;
    const int64_t nb = (sizes[t] + kAdamChunk - 1) / kAdamChunk;
    KGAT_CHECK_ARG(nb + blocks < (int64_t)1 << 31, "%s: too many elements", who);
    blocks += (int)nb;
    a.step_size[c] = (float)(lr / (1.0 - pow(beta1, (double)steps[t])));
    a.bc2_sqrt[c] = (float)sqrt(1.0 - pow(beta2, (double)steps[t]));
  }
  a.first_block[a.count] = blocks;
  return KGAT_OK;
}

// ---- the row tag: one 64-bit word per table row, call tag << kBits | (sorted position of the head of the row's run
// + 1).  A stale word carries an older tag, so nothing is ever cleared.  kBits: enough for the batch's sorted positions
// (14 for the KG block's 3 B <= 8,192, 17 for MF's 65,536).
template <int kBits>
int row_tag_check(const char* who, uint64_t tag) {
  KGAT_CHECK_ARG(tag >= 1 && tag < (1ull << (64 - kBits)), "%s: tag must be in [1, 2^%d)", who, 64 - kBits);
  return KGAT_OK;
}

// One thread per sorted position q of the batch's `total` ids: the head of a run of a real row writes the row's word.
template <int kBits>
__device__ __forceinline__ void row_tag_write(unsigned long long* __restrict__ row_slot, unsigned long long tag, int64_t q,
                                              int64_t total, const int32_t* __restrict__ run_len,
                                              const int32_t* __restrict__ sorted_ids, int64_t n_nodes) {
  if (q >= total || run_len[q] <= 0) return;
  const int32_t id = sorted_ids[q];
  if ((uint64_t)(uint32_t)id < (uint64_t)n_nodes) row_slot[id] = (tag << kBits) | (unsigned long long)(q + 1);
}

// The sorted position where this call's run of `row` starts, or -1: no gradient.
template <int kBits>
__device__ __forceinline__ int32_t row_tag_position(const unsigned long long* __restrict__ row_slot, int64_t row,
                                                    unsigned long long tag, int32_t total) {
  const unsigned long long slot = row_slot[row];
  const int32_t q = (int32_t)(slot & ((1ull << kBits) - 1ull)) - 1;
  return (slot >> kBits) == tag && q >= 0 && q < total ? q : -1;
}

// the length of the run that starts at sorted position q, inside the batch whatever the array holds
__device__ __forceinline__ int32_t run_length(const int32_t* __restrict__ run_len, int32_t q, int32_t total) {
  return clamp_i32(run_len[q], 1, total - q);
}

// ---- THE order of every run sum and chunk sum: rows [q, q + len) of `rows` (row stride `stride` floats), columns
// [c, c + 4), added one after the other onto acc.  kLook rows are requested per look - their loads are in flight
// together - because a load per addition makes the sum a chain of L2 round trips at the tail of the launch: batches are
// drawn from the triples, so a hub entity heads dozens of samples of a batch, and the most frequent relation has ten
// partial chunks.  The additions stay in row order, so the look count does not enter the bits.
template <int kLook>
__device__ __forceinline__ float4 ordered_row_sum(const float* __restrict__ rows, size_t stride, int64_t q, int32_t len,
                                                  int c, float4 acc = zero4()) {
  const float* src = rows + (size_t)q * stride + c;
  for (int32_t t0 = 0; t0 < len; t0 += kLook) {
    float4 x[kLook];
#pragma unroll
    for (int t = 0; t < kLook; ++t) x[t] = *reinterpret_cast<const float4*>(src + (size_t)(t0 + t < len ? t0 + t : len - 1) * stride);
#pragma unroll
    for (int t = 0; t < kLook; ++t)
      if (t0 + t < len) acc = add4(acc, x[t]);
  }
  return acc;
}

// the gradient of the table row whose run starts at sorted position q of the gradient rows DX (d floats each)
template <int kLook>
__device__ __forceinline__ float4 run_sum(const float* __restrict__ DX, const int32_t* __restrict__ run_len, int32_t q,
                                          int32_t total, int d, int c) {
  return ordered_row_sum<kLook>(DX, (size_t)d, q, run_length(run_len, q, total), c);
}

// the gradient of relation r: its chunk rows (the presort's chunk table) in chunk order
template <int kLook>
__device__ __forceinline__ float4 chunk_sum(const float* __restrict__ part, size_t stride,
                                            const int32_t* __restrict__ chunk_ptr, int n_part, int64_t r, int c) {
  const int32_t first = clamp_i32(chunk_ptr[r], 0, n_part);
  return ordered_row_sum<kLook>(part, stride, first, clamp_i32(chunk_ptr[r + 1], first, n_part) - first, c);
}

// ---- loss[0] = the mean of losses[0..batch) by one workgroup of 256 threads: each thread's strided sum, then a tree
// over the 256 - a fixed order
__device__ __forceinline__ void loss_mean_256(const float* __restrict__ losses, int32_t batch, float* __restrict__ loss) {
  __shared__ float s_l[256];
  float v = 0.f;
  for (int32_t s = threadIdx.x; s < batch; s += 256) v += losses[s];
  s_l[threadIdx.x] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_l[threadIdx.x] += s_l[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = s_l[0] / (float)batch;
}

}  // namespace kgat
