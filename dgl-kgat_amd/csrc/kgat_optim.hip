// Adam for the training loop of reference kgat.py:85 (optim.Adam(model.parameters(), lr)) as ONE launch over
// every parameter tensor that has a gradient: the reference's optimiser is torch's dense Adam, so every row of
// the 159k x 64 embedding table moves in every step (the moments decay even where the gradient is zero) - a
// streaming pass over p, g, m, v (28 bytes per element), which torch takes as ten multi-tensor launches (0.13 ms
// of the 0.31 ms KG step) and this takes as one.
//
// Per element, in fp32, the operations of torch.optim.Adam (amsgrad = False, weight_decay = 0, maximize = False),
// in torch's order:
//   m  <- m + (1 - beta1) (g - m)                    (Tensor.lerp_)
//   v  <- v beta2 + (1 - beta2) g g                  (mul_, addcmul_)
//   p  <- p - (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// with the step-dependent scalars formed in double on the host exactly as torch forms them.
//
// Global-norm gradient clipping (reference kgat.py:32 `--grad_norm`, kgat.py:162 clip_grad_norm_ between backward and
// step) rides on the same decomposition: one launch reads every gradient once and leaves one fp32 sum of squares per
// 4,096-element chunk, one workgroup adds the chunk sums in double and writes the fp32 norm and clip coefficient to
// device memory, and the Adam launch multiplies each gradient element by that coefficient in the register it already
// holds.  The order of additions is fixed (no float atomics), the coefficient never visits the host.
#include "kgat_step_common.h"

#include <math.h>

namespace kgat {

constexpr int kAdamMaxTensors = 16;

struct AdamArgs {
  AdamTensors<kAdamMaxTensors> t;   // (kgat_step_common.h)
  float* g[kAdamMaxTensors];
};

// kClip: every gradient element is first multiplied by the device scalar *coef (a product with its own rounding, as
// torch's in-place clip leaves it in memory); the stored gradient is not rewritten.  kClip = false is the plain step.
template <bool kClip>
__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a, float w1, float beta2, float w2, float eps,
                                                   int zero_grads, const float* __restrict__ coef) {
#pragma clang fp contract(off)
  float c = 1.0f;
  if constexpr (kClip) c = *coef;
  int t = 0;
  while (t + 1 < a.t.count && (int)blockIdx.x >= a.t.first_block[t + 1]) ++t;
  const int64_t base = (int64_t)(blockIdx.x - a.t.first_block[t]) * kAdamChunk;
  float* __restrict__ p = a.t.p[t];
  float* __restrict__ g = a.g[t];
  float* __restrict__ m = a.t.m[t];
  float* __restrict__ v = a.t.v[t];
  const int64_t n = a.t.n[t];
  const float ss = a.t.step_size[t], bs = a.t.bc2_sqrt[t];
  const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                     reinterpret_cast<uintptr_t>(v)) & 15) == 0;
#pragma unroll
  for (int k = 0; k < kAdamChunk / 1024; ++k) {
    const int64_t i = base + (int64_t)k * 1024 + threadIdx.x * 4;
    if (i >= n) break;
    if (vec && i + 4 <= n) {
      float4 gg = *reinterpret_cast<const float4*>(g + i);
      if constexpr (kClip) { gg.x = gg.x * c; gg.y = gg.y * c; gg.z = gg.z * c; gg.w = gg.w * c; }
      adam_four(p, m, v, i, gg, w1, beta2, w2, ss, bs, eps);
      if (zero_grads) *reinterpret_cast<float4*>(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int64_t j = i; j < i + 4 && j < n; ++j) {
        float pp = p[j], mm = m[j], vv = v[j], gj = g[j];
        if constexpr (kClip) gj = gj * c;
        adam_one(pp, gj, mm, vv, w1, beta2, w2, ss, bs, eps);
        p[j] = pp; m[j] = mm; v[j] = vv;
        if (zero_grads) g[j] = 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------- global gradient norm (kgat.py:32,162)
struct GradArgs {
  float* g[kAdamMaxTensors];
  int64_t n[kAdamMaxTensors];
  int first_block[kAdamMaxTensors + 1];
  int count;
};

// The longest chain of fp32 additions a square passes through: 16 serial adds in its lane (4 float4 of the chunk), 6
// levels of the wavefront's tree, 2 levels over the workgroup's 4 wavefronts.  The chunk sums are added in double.
constexpr int kGradNormChain = kAdamChunk / 256 + 6 + 2;
static_assert(kGradNormChain <= 64, "ops.GRAD_NORM_CHAIN is documented as at most 64");

// One fp32 sum of squares per 4,096-element chunk (adam_kernel's decomposition: block -> tensor through first_block).
// Lane l of the workgroup owns elements base + 1024 k + 4 l .. + 3 (k = 0..3) and adds their squares in that order,
// whichever way they were loaded (16-byte loads when the pointer is 16-byte aligned), elements past the end as +0;
// then the fixed tree.  No atomics: partials[blockIdx.x] is this workgroup's alone.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(GradArgs a, float* __restrict__ partials) {
#pragma clang fp contract(off)
  int t = 0;
  while (t + 1 < a.count && (int)blockIdx.x >= a.first_block[t + 1]) ++t;
  const int64_t base = (int64_t)(blockIdx.x - a.first_block[t]) * kAdamChunk;
  const float* __restrict__ g = a.g[t];
  const int64_t n = a.n[t];
  const bool vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
  float4 x[kAdamChunk / 1024];
#pragma unroll
  for (int k = 0; k < kAdamChunk / 1024; ++k) {
    const int64_t i = base + (int64_t)k * 1024 + threadIdx.x * 4;
    if (vec && i + 4 <= n) {
      x[k] = *reinterpret_cast<const float4*>(g + i);
    } else {
      x[k].x = i < n ? g[i] : 0.f;
      x[k].y = i + 1 < n ? g[i + 1] : 0.f;
      x[k].z = i + 2 < n ? g[i + 2] : 0.f;
      x[k].w = i + 3 < n ? g[i + 3] : 0.f;
    }
  }
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < kAdamChunk / 1024; ++k) {
    acc = acc + x[k].x * x[k].x;
    acc = acc + x[k].y * x[k].y;
    acc = acc + x[k].z * x[k].z;
    acc = acc + x[k].w * x[k].w;
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) acc = acc + __shfl_down(acc, off, kWave);
  __shared__ float wave_sum[256 / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) wave_sum[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// One workgroup: thread t adds partials t, t + 256, ... in double in index order, then the same fixed tree in double.
//   norm = (float)sqrt(sumsq);  coef = fminf(max_norm / (norm + 1e-6f), 1.0f)   (torch's clip_grad_norm_, fp32)
// except that a NaN quotient stays NaN, as under torch.clamp(max=1.0) - fminf alone would return 1.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const float* __restrict__ partials, int64_t n,
                                                               float max_norm, float* __restrict__ norm_out,
                                                               float* __restrict__ coef_out) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc = acc + (double)partials[i];
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) acc = acc + __shfl_down(acc, off, kWave);
  __shared__ double wave_sum[256 / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) wave_sum[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sumsq = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
    const float norm = (float)sqrt(sumsq);
    *norm_out = norm;
    const float denom = norm + 1e-6f;
    const float q = max_norm / denom;
    *coef_out = q >= 1.0f ? 1.0f : q;
  }
}

// g <- g * coef in place over up to kAdamMaxTensors tensors (the stand-alone clip_grad_norm_).  coef == 1 changes no
// bit of a gradient, so that case writes nothing.
__global__ __launch_bounds__(256) void scale_grads_kernel(GradArgs a, const float* __restrict__ coef) {
  const float c = *coef;
  if (c == 1.0f) return;
  int t = 0;
  while (t + 1 < a.count && (int)blockIdx.x >= a.first_block[t + 1]) ++t;
  const int64_t base = (int64_t)(blockIdx.x - a.first_block[t]) * kAdamChunk;
  float* __restrict__ g = a.g[t];
  const int64_t n = a.n[t];
  const bool vec = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
#pragma unroll
  for (int k = 0; k < kAdamChunk / 1024; ++k) {
    const int64_t i = base + (int64_t)k * 1024 + threadIdx.x * 4;
    if (i >= n) break;
    if (vec && i + 4 <= n) {
      float4 gg = *reinterpret_cast<const float4*>(g + i);
      gg.x *= c; gg.y *= c; gg.z *= c; gg.w *= c;
      *reinterpret_cast<float4*>(g + i) = gg;
    } else {
      for (int64_t j = i; j < i + 4 && j < n; ++j) g[j] = g[j] * c;
    }
  }
}

}  // namespace kgat

using namespace kgat;

namespace {

int adam_step(const char* what, int n_tensors, const int64_t* sizes_host, float* const* params_host,
              float* const* grads_host, float* const* exp_avg_host, float* const* exp_avg_sq_host,
              const int64_t* steps_host, double lr, double beta1, double beta2, double eps, int zero_grads, bool clip,
              const float* grad_coef, kgat_stream_t stream) {
  KGAT_CHECK_ARG(!clip || grad_coef, "%s: null grad_coef", what);
  if (n_tensors == 0) return KGAT_OK;
  KGAT_CHECK_ARG(sizes_host && params_host && grads_host && exp_avg_host && exp_avg_sq_host && steps_host,
                 "%s: null pointer", what);
  AdamArgs a;
  int kept[kAdamMaxTensors];
  KGAT_RETURN_IF(adam_fill(what, a.t, n_tensors, sizes_host, params_host, exp_avg_host, exp_avg_sq_host, steps_host, lr, beta1,
                           beta2, eps, false, kept));
  for (int c = 0; c < a.t.count; ++c) {
    KGAT_CHECK_ARG(grads_host[kept[c]], "%s: tensor %d: null pointer", what, kept[c]);
    a.g[c] = grads_host[kept[c]];
  }
  if (a.t.count == 0) return KGAT_OK;
  const int blocks = a.t.first_block[a.t.count];
  if (clip)
    hipLaunchKernelGGL(adam_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a,
                       (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, zero_grads, grad_coef);
  else
    hipLaunchKernelGGL(adam_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a,
                       (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, zero_grads,
                       (const float*)nullptr);
  KGAT_CHECK_LAUNCH(what);
  return KGAT_OK;
}

// The non-empty tensors of a gradient list as launch arguments; the number of chunks (= workgroups) in *blocks.
int grad_args(const char* what, int n_tensors, const int64_t* sizes_host, float* const* grads_host, GradArgs* a,
              int64_t* blocks) {
  KGAT_CHECK_ARG(n_tensors >= 0 && n_tensors <= kAdamMaxTensors, "%s: %d tensors (at most %d per call)", what,
                 n_tensors, kAdamMaxTensors);
  KGAT_CHECK_ARG(n_tensors == 0 || (sizes_host && grads_host), "%s: null pointer", what);
  a->count = 0;
  int64_t nb = 0;
  for (int t = 0; t < n_tensors; ++t) {
    KGAT_CHECK_ARG(sizes_host[t] >= 0, "%s: tensor %d: negative size", what, t);
    if (sizes_host[t] == 0) continue;
    KGAT_CHECK_ARG(grads_host[t], "%s: tensor %d: null pointer", what, t);
    const int c = a->count++;
    a->g[c] = grads_host[t];
    a->n[c] = sizes_host[t];
    a->first_block[c] = (int)nb;
    nb += (sizes_host[t] + kAdamChunk - 1) / kAdamChunk;
    KGAT_CHECK_ARG(nb < (int64_t)1 << 31, "%s: too many elements", what);
  }
  a->first_block[a->count] = (int)nb;
  *blocks = nb;
  return KGAT_OK;
}

}  // namespace

extern "C" {

int kgat_adam_max_tensors(void) { return kAdamMaxTensors; }

int kgat_adam_step_f32(int n_tensors, const int64_t* sizes_host, float* const* params_host, float* const* grads_host,
                       float* const* exp_avg_host, float* const* exp_avg_sq_host, const int64_t* steps_host, double lr,
                       double beta1, double beta2, double eps, int zero_grads, kgat_stream_t stream) {
  return adam_step("adam_step", n_tensors, sizes_host, params_host, grads_host, exp_avg_host, exp_avg_sq_host,
                   steps_host, lr, beta1, beta2, eps, zero_grads, false, nullptr, stream);
}

int kgat_adam_step_clipped_f32(int n_tensors, const int64_t* sizes_host, float* const* params_host,
                               float* const* grads_host, float* const* exp_avg_host, float* const* exp_avg_sq_host,
                               const int64_t* steps_host, double lr, double beta1, double beta2, double eps,
                               int zero_grads, const float* grad_coef, kgat_stream_t stream) {
  return adam_step("adam_step_clipped", n_tensors, sizes_host, params_host, grads_host, exp_avg_host, exp_avg_sq_host,
                   steps_host, lr, beta1, beta2, eps, zero_grads, true, grad_coef, stream);
}

int kgat_grad_norm_chain(void) { return kGradNormChain; }

int64_t kgat_grad_sumsq_partials(int n_tensors, const int64_t* sizes_host) {
  if (n_tensors < 0 || n_tensors > kAdamMaxTensors || (n_tensors > 0 && !sizes_host)) {
    set_error("grad_sumsq_partials: bad tensor count or null pointer");
    return -1;
  }
  int64_t nb = 0;
  for (int t = 0; t < n_tensors; ++t) {
    if (sizes_host[t] < 0) {
      set_error("grad_sumsq_partials: tensor %d: negative size", t);
      return -1;
    }
    nb += (sizes_host[t] + kAdamChunk - 1) / kAdamChunk;
  }
  return nb;
}

int kgat_grad_sumsq_f32(int n_tensors, const int64_t* sizes_host, float* const* grads_host, float* partials,
                        int64_t partials_cap, kgat_stream_t stream) {
  GradArgs a;
  int64_t blocks = 0;
  const int rc = grad_args("grad_sumsq", n_tensors, sizes_host, grads_host, &a, &blocks);
  if (rc != KGAT_OK) return rc;
  KGAT_CHECK_ARG(partials_cap >= blocks, "grad_sumsq: %lld partials do not fit the buffer of %lld", (long long)blocks,
                 (long long)partials_cap);
  if (blocks == 0) return KGAT_OK;
  KGAT_CHECK_ARG(partials, "grad_sumsq: null partials");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a, partials);
  KGAT_CHECK_LAUNCH("grad_sumsq");
  return KGAT_OK;
}

int kgat_grad_norm_finish_f32(int64_t n_partials, const float* partials, double max_norm, float* norm, float* coef,
                              kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_partials >= 0 && (n_partials == 0 || partials), "grad_norm_finish: negative count or null partials");
  KGAT_CHECK_ARG(norm && coef, "grad_norm_finish: null output");
  KGAT_CHECK_ARG(isfinite(max_norm) && max_norm > 0, "grad_norm_finish: max_norm must be finite and > 0");
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, as_stream(stream), partials, n_partials,
                     (float)max_norm, norm, coef);
  KGAT_CHECK_LAUNCH("grad_norm_finish");
  return KGAT_OK;
}

int kgat_scale_grads_f32(int n_tensors, const int64_t* sizes_host, float* const* grads_host, const float* coef,
                         kgat_stream_t stream) {
  GradArgs a;
  int64_t blocks = 0;
  const int rc = grad_args("scale_grads", n_tensors, sizes_host, grads_host, &a, &blocks);
  if (rc != KGAT_OK) return rc;
  KGAT_CHECK_ARG(coef, "scale_grads: null coef");
  if (blocks == 0) return KGAT_OK;
  hipLaunchKernelGGL(scale_grads_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a, coef);
  KGAT_CHECK_LAUNCH("scale_grads");
  return KGAT_OK;
}

}  // extern "C"
