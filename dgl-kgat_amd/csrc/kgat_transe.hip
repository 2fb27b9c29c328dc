// TransE KG-embedding step for gfx950: the objective of reference models.py:114-133 (`transR`, with `_L2_loss_mean`
// :9-11) with the projection removed - the KG-embedding half of the KGAT paper's CFKG baseline:
//     u_x = ent[x] / max(|ent[x]|, 1e-12)  (x = head, positive tail, negative tail),  u_r = rel[r] / max(|rel[r]|, 1e-12)
//     pos = |u_h + u_r - u_p|^2,           neg = |u_h + u_r - u_n|^2
//     loss = mean softplus(pos - neg) + lambda * sum_{v in h,r,p,n} mean(|u_v|^2 / 2)
// i.e. transR with every W_R[r] = I, without the d x k products, the W_R gradient partials and the W_R Adam pass.
// In torch operators this is ~60 small launches forward and backward; here it is gather-bound, small-launch work:
//   presort   kgat_transr_presort_f32's block serves as it is (samples by relation + the chunk table; the 3 B entity
//             ids with their inverse permutation and run lengths): kgat_kg_sorted.h
//   sample    d / 4 lanes per sample (16 bytes per lane and row, the four rows of a sample in flight together, 4-16
//             samples per wavefront): normalisation, both distances, softplus, the four gradient rows pushed through
//             the normalisation's Jacobian; the relation's row is written at the sample's relation-sorted position,
//             the three entity rows at the SORTED positions of their ids, so the contributions of one entity, and of
//             one relation, are consecutive rows
//   partials  a relation's rows summed per chunk of <= 64 sorted samples (the presort's chunk table), in sorted
//             order; the last workgroup reduces the loss
//   gradient  (the two halves / the one call) grad_ent[id] = the sum of the id's run of rows in sorted order, rows
//             outside the batch zero; grad_rel[r] = the sum of r's chunk rows in chunk order
//   Adam      (the fused iteration) dense torch.optim.Adam over ent and rel in place; a row's gradient is formed on the
//             way, by the same additions, and is 0 for a row the batch does not touch (row_slot tags)
// No float atomics; every sum has a fixed order: runs of equal ids in sorted order, the samples of a relation in sorted
// order (per chunk, then the chunks in order).  Bitwise reproducible, and the fused iteration has the bits of the two
// halves followed by a dense Adam step.  All arithmetic fp32 on the vector ALU.
#include <math.h>

#include "kgat_kg_sorted.h"
#include "kgat_step_common.h"

namespace kgat {

constexpr int kTeMaxDim = 256;   // d / 4 lanes per sample: at most one wavefront

// Everything a call carves from the caller's scratch: per-sample losses (B) | the relation rows GR (B x d, relation-
// sorted) | the entity rows DX (3 B x d, at the sorted positions of their ids) | the chunk rows (n_part x d) | for the
// entries that sort themselves, one presort block.  One size for every entry.
struct TeScratch {
  float *losses, *GR, *DX, *part;
  unsigned char* sorted;
  int n_part;
  size_t bytes;
};
static TeScratch transe_scratch(void* base, int64_t batch, int d, int n_rel) {
  const size_t b = (size_t)(batch > 0 ? batch : 1), dd = (size_t)(d > 4 ? d : 4);
  TeScratch s;
  Carver cv(base);
  s.n_part = (int)transr_max_chunks(batch, n_rel);
  s.losses = cv.take<float>(b);
  s.GR = cv.take<float>(b * dd);
  s.DX = cv.take<float>(3 * b * dd);
  s.part = cv.take<float>((size_t)s.n_part * dd);
  s.sorted = cv.take<unsigned char>(transr_sorted_layout(batch, n_rel > 0 ? n_rel : 0).bytes);
  s.bytes = cv.off;
  return s;
}

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, G);
  return v;
}
__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}

struct TeSampleArgs {
  int32_t batch, n_rel;
  int64_t n_nodes;
  int d;
  const int32_t *h, *r, *pt, *nt;
  const float *ent, *rel;
  float lambda;
  KgSorted so;
  float *losses, *GR, *DX;
  // the fused iteration: workgroups behind the samples' tag the batch's entity rows (NULL: none)
  unsigned long long* row_slot;
  unsigned long long tag;
  int sample_blocks;
};

// ---- per-sample kernel.  G lanes per relation-sorted sample s (G: the power of two >= d / 4 among 16, 32, 64); lane
// sl owns floats [4 sl, 4 sl + 4) of each of the sample's four rows.  What bounds it: four dependent-free 16-byte
// gathers per lane, then eleven G-lane reductions (four cross-lane steps each at G = 16) and thirty-two divisions -
// the latency of one gather round trip plus a few hundred VALU cycles, on B G / 64 wavefronts.
// A sample with an id outside its table reads nothing, makes the loss NaN (torch would fail a device-side assertion)
// and leaves zero rows.
template <int G>
__global__ __launch_bounds__(256) void transe_sample_kernel(TeSampleArgs a) {
  const int32_t B = a.batch;
  if ((int)blockIdx.x >= a.sample_blocks) {
    row_tag_write<kTrSlotBits>(a.row_slot, a.tag, ((int)blockIdx.x - a.sample_blocks) * 256 + (int)threadIdx.x, 3 * B,
                               a.so.run_len, a.so.sorted_ids, a.n_nodes);
    return;
  }
  constexpr int SPB = 256 / G;   // samples per workgroup
  const int sl = threadIdx.x % G;
  const int32_t s = (int32_t)blockIdx.x * SPB + (int32_t)(threadIdx.x / G);
  if (s >= B) return;   // (whole lane groups leave; the reductions below stay inside a group)
  const int d = a.d;
  const int32_t b = clamp_i32(a.so.order[s], 0, B - 1);
  const int32_t ids[3] = {a.h[b], a.pt[b], a.nt[b]};
  const int32_t rr = a.r[b];
  const bool ok = (uint64_t)(uint32_t)ids[0] < (uint64_t)a.n_nodes && (uint64_t)(uint32_t)ids[1] < (uint64_t)a.n_nodes &&
                  (uint64_t)(uint32_t)ids[2] < (uint64_t)a.n_nodes && (uint32_t)rr < (uint32_t)a.n_rel;
  const int c = 4 * sl;
  const bool live = c < d;
  // the rows of DX: the sorted positions of entries 3 b + v of the id list
  int32_t dxr[3];
#pragma unroll
  for (int v = 0; v < 3; ++v) dxr[v] = clamp_i32(a.so.inv_pos[3 * b + v], 0, 3 * B - 1);
  float4 x[4];   // head, positive tail, negative tail, relation
#pragma unroll
  for (int v = 0; v < 4; ++v) x[v] = zero4();
  if (ok && live) {
#pragma unroll
    for (int v = 0; v < 3; ++v) x[v] = *reinterpret_cast<const float4*>(a.ent + (size_t)ids[v] * d + c);
    x[3] = *reinterpret_cast<const float4*>(a.rel + (size_t)rr * d + c);
  }
  // F.normalize(p=2, dim=1, eps=1e-12): x / clamp_min(|x|, eps); below the clamp the norm gets no gradient
  float nrm[4];
  bool clamped[4];
  float4 u[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float nr = sqrtf(group_sum<G>(dot4(x[v], x[v])));
    clamped[v] = nr < 1e-12f;
    nrm[v] = fmaxf(nr, 1e-12f);
    u[v] = make_float4(x[v].x / nrm[v], x[v].y / nrm[v], x[v].z / nrm[v], x[v].w / nrm[v]);
  }
  const float4 hr = add4(u[0], u[3]);
  const float4 dp = make_float4(hr.x - u[1].x, hr.y - u[1].y, hr.z - u[1].z, hr.w - u[1].w);
  const float4 dn = make_float4(hr.x - u[2].x, hr.y - u[2].y, hr.z - u[2].z, hr.w - u[2].w);
  const float pos = group_sum<G>(dot4(dp, dp));
  const float neg = group_sum<G>(dot4(dn, dn));
  const float reg = group_sum<G>(dot4(u[0], u[0]) + dot4(u[1], u[1]) + dot4(u[2], u[2]) + dot4(u[3], u[3]));
  const float z = pos - neg;   // -logsigmoid(neg - pos) = softplus(z)
  if (sl == 0)
    a.losses[s] = ok ? fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))) + a.lambda * 0.5f * reg : __builtin_nanf("");
  const float sg = 1.f / (1.f + expf(-z));   // d softplus / dz
  const float c2 = 2.f * sg / (float)B, lb = a.lambda / (float)B;
  // gradients with respect to the normalised vectors ...
  float4 g[4];
  {
    const float4 dd = make_float4(c2 * (dp.x - dn.x), c2 * (dp.y - dn.y), c2 * (dp.z - dn.z), c2 * (dp.w - dn.w));
    g[0] = fma4(lb, u[0], dd);
    g[3] = fma4(lb, u[3], dd);
    g[1] = fma4(lb, u[1], make_float4(-c2 * dp.x, -c2 * dp.y, -c2 * dp.z, -c2 * dp.w));
    g[2] = fma4(lb, u[2], make_float4(c2 * dn.x, c2 * dn.y, c2 * dn.z, c2 * dn.w));
  }
  // ... then through the normalisation: (g - u <u, g>) / |x|, or g / eps for a row below the clamp
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    float dot = group_sum<G>(dot4(u[v], g[v]));
    if (clamped[v]) dot = 0.f;
    g[v] = make_float4((g[v].x - u[v].x * dot) / nrm[v], (g[v].y - u[v].y * dot) / nrm[v], (g[v].z - u[v].z * dot) / nrm[v],
                       (g[v].w - u[v].w * dot) / nrm[v]);
    if (!ok) g[v] = zero4();
  }
  if (live) {
#pragma unroll
    for (int v = 0; v < 3; ++v) *reinterpret_cast<float4*>(a.DX + (size_t)dxr[v] * d + c) = g[v];
    *reinterpret_cast<float4*>(a.GR + (size_t)s * d + c) = g[3];
  }
}

constexpr int kTeLook = 8;   // rows requested per look of every run sum and chunk sum of this file (ordered_row_sum)

// ---- second launch: wavefront w of the grid sums chunk w of the presort's chunk table (<= 64 relation-sorted rows of
// GR); the last workgroup reduces the loss - the sums of 256 threads, then a tree over them: a fixed order
__global__ __launch_bounds__(256) void transe_partial_kernel(int part_blocks, int n_part, int32_t batch, int d, int n_rel,
                                                             KgSorted so, const float* __restrict__ GR,
                                                             float* __restrict__ part, const float* __restrict__ losses,
                                                             float* __restrict__ loss) {
  if ((int)blockIdx.x >= part_blocks) {
    loss_mean_256(losses, batch, loss);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int32_t ck = (int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6);
  if (ck >= clamp_i32(so.chunk_ptr[n_rel], 0, n_part)) return;
  const int2 e = so.chunks[ck];
  const int32_t rel = clamp_i32(e.x, 0, n_rel - 1);
  const int32_t beg = clamp_i32(e.y, 0, batch), seg_end = clamp_i32(so.seg[rel + 1], beg, batch);
  const int32_t end = beg + kTrChunk < seg_end ? beg + kTrChunk : seg_end;
  const int c = 4 * lane;
  if (c < d) *reinterpret_cast<float4*>(part + (size_t)ck * d + c) = ordered_row_sum<kTeLook>(GR, (size_t)d, beg, end - beg, c);
}

// ---- the dense gradients (the backward half; grad_ent zeroed by the memset in front): thread t < n_rel d / 4 one
// 16-byte piece of grad_rel, the threads behind them one piece of the run that starts at a sorted position
__global__ __launch_bounds__(256) void transe_grad_kernel(int32_t batch, int64_t n_nodes, int d, int n_rel, int n_part,
                                                          KgSorted so, const float* __restrict__ DX,
                                                          const float* __restrict__ part,
                                                          const float* __restrict__ grad_scale,
                                                          float* __restrict__ grad_ent, float* __restrict__ grad_rel) {
  const int d4 = d / 4;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n_rel_t = (int64_t)n_rel * d4;
  float4 v;
  float* dst;
  if (t < n_rel_t) {
    const int64_t r = t / d4;
    const int c = 4 * (int)(t - r * d4);
    v = chunk_sum<kTeLook>(part, (size_t)d, so.chunk_ptr, n_part, r, c);
    dst = grad_rel + (size_t)r * d + c;
  } else {
    const int64_t e = t - n_rel_t;
    const int32_t q = (int32_t)(e / d4);
    if (e >= (int64_t)3 * batch * d4 || so.run_len[q] <= 0) return;
    const int32_t id = so.sorted_ids[q];
    if ((uint64_t)(uint32_t)id >= (uint64_t)n_nodes) return;
    const int c = 4 * (int)(e - (int64_t)q * d4);
    v = run_sum<kTeLook>(DX, so.run_len, q, 3 * batch, d, c);
    dst = grad_ent + (size_t)id * d + c;
  }
  if (grad_scale) {   // the gradient arriving at the loss (device scalar)
    const float sc = grad_scale[0];
    v = make_float4(v.x * sc, v.y * sc, v.z * sc, v.w * sc);
  }
  *reinterpret_cast<float4*>(dst) = v;
}

// ---- third launch of the fused iteration: Adam over the entity table (gradient through row_slot) and the relation
// table (gradient = the ordered sum of the relation's chunk rows): adam_chunk_walk.
struct TeAdamArgs {
  AdamTensors<2> t;   // entity table, relation table
  int d, n_part;
  int32_t total;   // 3 B
  const unsigned long long* row_slot;
  unsigned long long tag;
  const float *DX, *part;
  const int32_t *run_len, *chunk_ptr;
};

__global__ __launch_bounds__(256) void transe_adam_kernel(TeAdamArgs a, float w1, float beta2, float w2, float eps) {
  if ((int)blockIdx.x < a.t.first_block[1]) {
    adam_chunk_walk(a.t, 0, w1, beta2, w2, eps, [&](int64_t i) {
      const int64_t row = i / a.d;
      const int32_t q = row_tag_position<kTrSlotBits>(a.row_slot, row, a.tag, a.total);
      return q < 0 ? zero4() : run_sum<kTeLook>(a.DX, a.run_len, q, a.total, a.d, (int)(i - row * a.d));
    });
  } else {
    adam_chunk_walk(a.t, 1, w1, beta2, w2, eps, [&](int64_t i) {
      const int64_t row = i / a.d;
      return chunk_sum<kTeLook>(a.part, (size_t)a.d, a.chunk_ptr, a.n_part, row, (int)(i - row * a.d));
    });
  }
}

// The first two launches of every form: the per-sample kernel (+ the row tags of the fused iteration), then the chunk
// sums + the loss.
static int transe_launch_forward(const char* who, int64_t n_nodes, int n_rel, int d, int64_t batch, const int32_t* h,
                                 const int32_t* r, const int32_t* pos_t, const int32_t* neg_t, const float* ent,
                                 const float* rel, float reg_lambda, float* loss, const KgSorted& so, const TeScratch& w,
                                 unsigned long long* row_slot, unsigned long long tag, hipStream_t st) {
  const int32_t B = (int32_t)batch;
  const int G = d <= 64 ? 16 : (d <= 128 ? 32 : 64);
  TeSampleArgs a;
  a.batch = B; a.n_rel = n_rel; a.n_nodes = n_nodes; a.d = d;
  a.h = h; a.r = r; a.pt = pos_t; a.nt = neg_t; a.ent = ent; a.rel = rel; a.lambda = reg_lambda; a.so = so;
  a.losses = w.losses; a.GR = w.GR; a.DX = w.DX;
  a.row_slot = row_slot; a.tag = tag;
  a.sample_blocks = (int)((batch * G + 255) / 256);
  const unsigned blocks = (unsigned)a.sample_blocks + (row_slot ? (unsigned)((3 * batch + 255) / 256) : 0u);
  if (G == 16) hipLaunchKernelGGL(transe_sample_kernel<16>, dim3(blocks), dim3(256), 0, st, a);
  else if (G == 32) hipLaunchKernelGGL(transe_sample_kernel<32>, dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(transe_sample_kernel<64>, dim3(blocks), dim3(256), 0, st, a);
  if (hipGetLastError() != hipSuccess) {
    set_error("%s: launch of the per-sample kernel failed", who);
    return KGAT_E_HIP;
  }
  const int part_blocks = (w.n_part + 3) / 4;
  hipLaunchKernelGGL(transe_partial_kernel, dim3((unsigned)part_blocks + 1u), dim3(256), 0, st, part_blocks, w.n_part, B, d,
                     n_rel, so, (const float*)w.GR, w.part, (const float*)w.losses, loss);
  if (hipGetLastError() != hipSuccess) {
    set_error("%s: launch of the chunk sums failed", who);
    return KGAT_E_HIP;
  }
  return KGAT_OK;
}

static int transe_launch_backward(const char* who, int64_t n_nodes, int n_rel, int d, int64_t batch, const KgSorted& so,
                                  const TeScratch& w, const float* grad_scale, float* grad_ent, float* grad_rel,
                                  hipStream_t st) {
  if (hipMemsetAsync(grad_ent, 0, (size_t)n_nodes * d * sizeof(float), st) != hipSuccess) {
    set_error("%s: memset failed", who);
    return KGAT_E_HIP;
  }
  const int64_t threads = ((int64_t)n_rel + 3 * batch) * (d / 4);
  hipLaunchKernelGGL(transe_grad_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, (int32_t)batch, n_nodes, d,
                     n_rel, w.n_part, so, (const float*)w.DX, (const float*)w.part, grad_scale, grad_ent, grad_rel);
  if (hipGetLastError() != hipSuccess) {
    set_error("%s: launch of the gradient sums failed", who);
    return KGAT_E_HIP;
  }
  return KGAT_OK;
}

// the checks the three autograd entries share; 0, or the code to return
static int transe_check(const char* who, int64_t n_nodes, int n_rel, int d, int64_t batch, const int32_t* h,
                        const int32_t* r, const int32_t* pos_t, const int32_t* neg_t, const void* scratch,
                        size_t scratch_bytes) {
  if (!kgat_transe_supported(n_nodes, d, n_rel, batch)) {
    set_error("%s: needs d a multiple of 4 and <= %d, 1 <= batch <= %d, 1 <= n_rel <= %d, 1 <= n_nodes < 2^31 (d=%d batch=%lld "
              "n_rel=%d n_nodes=%lld)", who, kTeMaxDim, kTrSmallSort / 3, kTrMaxRel, d, (long long)batch, n_rel, (long long)n_nodes);
    return KGAT_E_UNSUPPORTED;
  }
  if (!(h && r && pos_t && neg_t && scratch)) {
    set_error("%s: null pointer", who);
    return KGAT_E_BADARG;
  }
  if (!aligned16(scratch)) {
    set_error("%s: the scratch must be 16-byte aligned", who);
    return KGAT_E_BADARG;
  }
  if (scratch_bytes < transe_scratch(nullptr, batch, d, n_rel).bytes) {
    set_error("%s: scratch too small", who);
    return KGAT_E_WORKSPACE;
  }
  return KGAT_OK;
}

}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_transe_supported(int64_t n_nodes, int d, int n_rel, int64_t batch) {
  return d >= 4 && d % 4 == 0 && d <= kTeMaxDim && n_rel > 0 && n_rel <= kTrMaxRel && batch > 0 && 3 * batch <= kTrSmallSort &&
         n_nodes > 0 && n_nodes < INT32_MAX;
}

size_t kgat_transe_scratch_bytes(int64_t batch, int d, int n_rel) { return transe_scratch(nullptr, batch, d, n_rel).bytes; }

size_t kgat_transe_sorted_bytes(int64_t batch, int n_rel) { return transr_sorted_layout(batch, n_rel > 0 ? n_rel : 0).bytes; }

int kgat_transe_presort_f32(int64_t n_nodes, int n_rel, int64_t n_batches, int64_t batch, const int32_t* h,
                            const int32_t* r, const int32_t* pos_t, const int32_t* neg_t, void* sorted,
                            size_t sorted_bytes, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_batches >= 0 && n_batches < (1 << 30), "transe_presort: bad batch count");
  if (!kgat_transe_supported(n_nodes, 4, n_rel, batch)) {
    set_error("transe_presort: needs 1 <= batch <= %d, 1 <= n_rel <= %d, 1 <= n_nodes < 2^31 (batch=%lld n_rel=%d n_nodes=%lld)",
              kTrSmallSort / 3, kTrMaxRel, (long long)batch, n_rel, (long long)n_nodes);
    return KGAT_E_UNSUPPORTED;
  }
  if (n_batches == 0) return KGAT_OK;
  KGAT_CHECK_ARG(h && r && pos_t && neg_t && sorted, "transe_presort: null pointer");
  KGAT_CHECK_ARG(aligned16(sorted), "transe_presort: the output must be 16-byte aligned");
  if (sorted_bytes < (size_t)n_batches * transr_sorted_layout(batch, n_rel).bytes) {
    set_error("transe_presort: output buffer too small");
    return KGAT_E_WORKSPACE;
  }
  // the TransR presort's block is the one this file reads
  return kgat_transr_presort_f32(n_nodes, n_rel, n_batches, batch, h, r, pos_t, neg_t, sorted, sorted_bytes, stream);
}

int kgat_transe_forward_f32(int64_t n_nodes, int n_rel, int d, int64_t batch, const int32_t* h, const int32_t* r,
                            const int32_t* pos_t, const int32_t* neg_t, const float* ent, const float* rel,
                            float reg_lambda, float* loss, void* scratch, size_t scratch_bytes, kgat_stream_t stream) {
  KGAT_RETURN_IF(transe_check("transe_forward", n_nodes, n_rel, d, batch, h, r, pos_t, neg_t, scratch, scratch_bytes));
  KGAT_CHECK_ARG(ent && rel && loss, "transe_forward: null pointer");
  KGAT_CHECK_ARG(aligned16(ent) && aligned16(rel), "transe_forward: ent and rel must be 16-byte aligned");
  const TeScratch w = transe_scratch(scratch, batch, d, n_rel);
  const size_t block = transr_sorted_layout(batch, n_rel).bytes;
  const int rc = kgat_transr_presort_f32(n_nodes, n_rel, 1, batch, h, r, pos_t, neg_t, w.sorted, block, stream);
  if (rc != KGAT_OK) return rc;
  return transe_launch_forward("transe_forward", n_nodes, n_rel, d, batch, h, r, pos_t, neg_t, ent, rel, reg_lambda, loss,
                               kg_sorted(w.sorted, batch, n_rel), w, nullptr, 0ull, as_stream(stream));
}

int kgat_transe_backward_f32(int64_t n_nodes, int n_rel, int d, int64_t batch, const int32_t* h, const int32_t* r,
                             const int32_t* pos_t, const int32_t* neg_t, const float* grad_scale, float* grad_ent,
                             float* grad_rel, void* scratch, size_t scratch_bytes, kgat_stream_t stream) {
  KGAT_RETURN_IF(transe_check("transe_backward", n_nodes, n_rel, d, batch, h, r, pos_t, neg_t, scratch, scratch_bytes));
  KGAT_CHECK_ARG(grad_ent && grad_rel, "transe_backward: null gradient pointer");
  KGAT_CHECK_ARG(aligned16(grad_ent) && aligned16(grad_rel), "transe_backward: the gradients must be 16-byte aligned");
  const TeScratch w = transe_scratch(scratch, batch, d, n_rel);
  return transe_launch_backward("transe_backward", n_nodes, n_rel, d, batch, kg_sorted(w.sorted, batch, n_rel), w, grad_scale,
                                grad_ent, grad_rel, as_stream(stream));
}

int kgat_transe_loss_grad_f32(int64_t n_nodes, int n_rel, int d, int64_t batch, const int32_t* h, const int32_t* r,
                              const int32_t* pos_t, const int32_t* neg_t, const float* ent, const float* rel,
                              float reg_lambda, float* loss, float* grad_ent, float* grad_rel, void* scratch,
                              size_t scratch_bytes, kgat_stream_t stream) {
  KGAT_RETURN_IF(transe_check("transe_loss_grad", n_nodes, n_rel, d, batch, h, r, pos_t, neg_t, scratch, scratch_bytes));
  KGAT_CHECK_ARG(ent && rel && loss && grad_ent && grad_rel, "transe_loss_grad: null pointer");
  KGAT_CHECK_ARG(aligned16(ent) && aligned16(rel) && aligned16(grad_ent) && aligned16(grad_rel),
                 "transe_loss_grad: the tables and the gradients must be 16-byte aligned");
  const TeScratch w = transe_scratch(scratch, batch, d, n_rel);
  const size_t block = transr_sorted_layout(batch, n_rel).bytes;
  int rc = kgat_transr_presort_f32(n_nodes, n_rel, 1, batch, h, r, pos_t, neg_t, w.sorted, block, stream);
  if (rc != KGAT_OK) return rc;
  const KgSorted so = kg_sorted(w.sorted, batch, n_rel);
  rc = transe_launch_forward("transe_loss_grad", n_nodes, n_rel, d, batch, h, r, pos_t, neg_t, ent, rel, reg_lambda, loss, so, w,
                             nullptr, 0ull, as_stream(stream));
  if (rc != KGAT_OK) return rc;
  return transe_launch_backward("transe_loss_grad", n_nodes, n_rel, d, batch, so, w, nullptr, grad_ent, grad_rel,
                                as_stream(stream));
}

int kgat_transe_adam_step_f32(int64_t n_nodes, int n_rel, int d, int64_t batch, const int32_t* h, const int32_t* r,
                              const int32_t* pos_t, const int32_t* neg_t, const void* sorted, float* ent, float* rel,
                              float* const* exp_avg_host, float* const* exp_avg_sq_host, const int64_t* steps_host,
                              double lr, double beta1, double beta2, double eps, float reg_lambda, float* loss,
                              uint64_t* row_slot, uint64_t tag, void* scratch, size_t scratch_bytes, kgat_stream_t stream) {
  KGAT_RETURN_IF(transe_check("transe_adam_step", n_nodes, n_rel, d, batch, h, r, pos_t, neg_t, scratch, scratch_bytes));
  KGAT_CHECK_ARG(sorted && ent && rel && exp_avg_host && exp_avg_sq_host && steps_host && loss && row_slot,
                 "transe_adam_step: null pointer");
  KGAT_RETURN_IF(row_tag_check<kTrSlotBits>("transe_adam_step", tag));
  KGAT_CHECK_ARG(aligned16(sorted), "transe_adam_step: the sorted block must be 16-byte aligned");
  TeAdamArgs a;
  float* const ps[2] = {ent, rel};
  const int64_t sizes[2] = {(int64_t)n_nodes * d, (int64_t)n_rel * d};
  KGAT_RETURN_IF(adam_fill("transe_adam_step", a.t, 2, sizes, ps, exp_avg_host, exp_avg_sq_host, steps_host, lr, beta1, beta2,
                           eps, true));
  hipStream_t st = as_stream(stream);
  const TeScratch w = transe_scratch(scratch, batch, d, n_rel);
  const KgSorted so = kg_sorted(sorted, batch, n_rel);
  const int rc = transe_launch_forward("transe_adam_step", n_nodes, n_rel, d, batch, h, r, pos_t, neg_t, ent, rel, reg_lambda,
                                       loss, so, w, reinterpret_cast<unsigned long long*>(row_slot), (unsigned long long)tag, st);
  if (rc != KGAT_OK) return rc;
  a.d = d; a.n_part = w.n_part; a.total = (int32_t)(3 * batch);
  a.row_slot = reinterpret_cast<const unsigned long long*>(row_slot);
  a.tag = (unsigned long long)tag;
  a.DX = w.DX; a.part = w.part; a.run_len = so.run_len; a.chunk_ptr = so.chunk_ptr;
  hipLaunchKernelGGL(transe_adam_kernel, dim3((unsigned)a.t.first_block[2]), dim3(256), 0, st, a, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)eps);
  KGAT_CHECK_LAUNCH("transe_adam");
  return KGAT_OK;
}

}  // extern "C"
