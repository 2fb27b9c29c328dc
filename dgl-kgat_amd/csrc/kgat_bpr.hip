// BPR loss of the CF phase (reference models.py:170-178, get_loss; _L2_loss_mean :9-11) and its gradient with
// respect to the readout, for gfx950.  The reference's expression is ~30 torch operators forward and ~45 backward
// (gathers, batched dot products, logsigmoid, three regularisers, an index_put with a device sort): 75 launches of
// a few microseconds each, 0.7 ms of the 1.6 ms CF step, all of it launch latency.  Here:
//   forward   bpr_sample_kernel (one wavefront per sample: the three rows, five dot products) + bpr_reduce_kernel
//   backward  four launches of bounded work: bpr_sort_zero_kernel (slices of 4,096 row ids sorted in LDS beside
//             three quarters of the zero fill of the N x F gradient) + bpr_merge_kernel (every id's place among all
//             ids: a stable merge by binary searches advanced together, beside the rest of the fill; up to 65,536 ids -
//             beyond: the device radix sort of kgat_graph.hip + a memset) +
//             bpr_window_kernel (a wavefront per 32 sorted positions adds their contributions in order; rows inside
//             the window are written, pieces of rows that cross its edges left as partials) + bpr_carry_kernel (the
//             crossing rows' pieces in window order): fixed order of additions, no float atomics, bitwise
//             reproducible; scaled by the incoming gradient read from device memory (no host synchronisation, no
//             separate multiply pass)
//   loss = -mean_b logsigmoid(<s,p> - <s,n>) + lambda (mean_b |s|^2/2 + mean_b |p|^2/2 + mean_b |n|^2/2)
// Below them, BPR-MF pretraining (the same loss with the embedding table as the readout) as three-launch iterations
// without a dense gradient: kgat_mf_presort_f32 + kgat_mf_adam_step_f32, on the kernels' shared bodies.
#include <math.h>

#include "kgat_step_common.h"
#include "kgat_lds_sort.h"

namespace kgat {

// per sample b: out[b] = logsigmoid(x), out[B + b] = (|s|^2 + 0)/2 ..., coef[b] = sigmoid(-x)
__global__ __launch_bounds__(256) void bpr_sample_kernel(int64_t batch, int64_t n_nodes, int F,
                                                         const float* __restrict__ emb, int64_t stride, const int32_t* __restrict__ u,
                                                         const int32_t* __restrict__ p, const int32_t* __restrict__ n,
                                                         float* __restrict__ part, float* __restrict__ coef) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= batch) return;
  if ((uint64_t)u[b] >= (uint64_t)n_nodes || (uint64_t)p[b] >= (uint64_t)n_nodes || (uint64_t)n[b] >= (uint64_t)n_nodes) {
    // an id outside [0, n_nodes) (torch would fail a device-side assertion): NaN in the loss, no access
    if (lane == 0) {
      part[b] = __builtin_nanf(""); part[batch + b] = 0.f; part[2 * batch + b] = 0.f; part[3 * batch + b] = 0.f;
      coef[b] = 0.f;
    }
    return;
  }
  const float* rs = emb + (size_t)u[b] * stride;
  const float* rp = emb + (size_t)p[b] * stride;
  const float* rn = emb + (size_t)n[b] * stride;
  float sp = 0.f, sn = 0.f, ss = 0.f, pp = 0.f, nn = 0.f;
  for (int c = lane * 4; c < F; c += 256) {
    const float4 a = *reinterpret_cast<const float4*>(rs + c);
    const float4 x = *reinterpret_cast<const float4*>(rp + c);
    const float4 y = *reinterpret_cast<const float4*>(rn + c);
    sp += a.x * x.x + a.y * x.y + a.z * x.z + a.w * x.w;
    sn += a.x * y.x + a.y * y.y + a.z * y.z + a.w * y.w;
    ss += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
    pp += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
    nn += y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w;
  }
  sp = wave_sum(sp); sn = wave_sum(sn); ss = wave_sum(ss); pp = wave_sum(pp); nn = wave_sum(nn);
  if (lane == 0) {
    const float x = sp - sn;
    // logsigmoid(x) = min(x, 0) - log1p(exp(-|x|)); sigmoid(-x) = 1 / (1 + exp(x))
    part[b] = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
    part[batch + b] = 0.5f * ss;
    part[2 * batch + b] = 0.5f * pp;
    part[3 * batch + b] = 0.5f * nn;
    coef[b] = x >= 0.f ? expf(-x) / (1.f + expf(-x)) : 1.f / (1.f + expf(x));
  }
}

// loss = -mean(part[0:B]) + lambda (mean(part[B:2B]) + mean(part[2B:3B]) + mean(part[3B:4B])), fixed order: the sums
// of 1,024 threads in sixteen wavefronts.  A block of THREADS < 1,024 threads (the fused MF iteration's, where the
// reduction rides in a launch of 256-thread blocks) plays the sixteen wavefronts in turn: the same additions.
template <int THREADS>
__device__ __forceinline__ void bpr_reduce_body(int64_t batch, const float* __restrict__ part, float reg_lambda,
                                                float* __restrict__ loss) {
  __shared__ float s_red[4][16];
  const int lane = threadIdx.x & 63;
  for (int w = threadIdx.x >> 6; w < 16; w += THREADS / 64) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = w * 64 + lane; i < batch; i += 1024)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += part[k * batch + i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc[k] = wave_sum(acc[k]);
      if (lane == 0) s_red[k][w] = acc[k];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float x = 0.f;
      for (int j = 0; j < 16; ++j) x += s_red[k][j];
      t[k] = x / (float)batch;
    }
    loss[0] = -t[0] + reg_lambda * (t[1] + t[2] + t[3]);
  }
}

__global__ __launch_bounds__(1024) void bpr_reduce_kernel(int64_t batch, const float* __restrict__ part,
                                                          float reg_lambda, float* __restrict__ loss) {
  bpr_reduce_body<1024>(batch, part, reg_lambda, loss);
}

__global__ __launch_bounds__(256) void bpr_keys_kernel(int64_t batch, const int32_t* __restrict__ u,
                                                       const int32_t* __restrict__ p, const int32_t* __restrict__ n,
                                                       int32_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * batch) return;
  const int64_t b = i % batch;
  const int role = (int)(i / batch);
  keys[i] = role == 0 ? u[b] : (role == 1 ? p[b] : n[b]);
}

// The dense gradient from the sorted ids, in two launches of bounded work (the scheme of the aggregation's merge
// tiles and finish launch).  Launch one: a wavefront per WINDOW of 32 sorted positions fetches the 32 samples' indices
// and coefficients side by side (lanes 0-31: two dependent round trips for the window), then walks the positions in
// order, the partner rows of eight positions in flight at a time; a row id whose contributions begin and end inside
// the window is written at once, a first / last piece of a run that crosses the window's edge goes to the window's
// partial slot 0 / 1.  Launch two: the wavefront of the window in which a crossing run BEGINS adds the run's partials
// in window order and writes the row.  Every sum has a fixed order (a run inside one window: sample order, as ever;
// a crossing run: its pieces in sample order, then the pieces in window order): bitwise reproducible, no atomics.
// (The first form - one wavefront per run, one sample after the other, three dependent round trips each - is fine
// for uniformly drawn ids; the reference's samplers draw interactions uniformly over EDGES, so a popular item is the
// positive of hundreds of samples of a batch: ~1 us per sample on one wavefront, +0.9 ms on a 1.0-ms step.)
constexpr int kBprWin = 32;

struct BprSample {   // what the window's lane l knows about sorted position base + l
  int32_t key, role, r1, r2;
  float cv;
  bool ok;
};

// COMPACT (the fused MF iteration, below): a row completed inside the window goes to row `sorted position of the run's
// head` of a 3 B x F buffer instead of row `id` of the dense gradient; the pieces of crossing runs as ever.
template <bool COMPACT>
__device__ __forceinline__ void bpr_window_body(int64_t w, int64_t batch, int64_t n_nodes, int F,
                                                const float* __restrict__ emb, int64_t stride,
                                                const int32_t* __restrict__ u, const int32_t* __restrict__ p,
                                                const int32_t* __restrict__ n, const float* __restrict__ coef,
                                                float reg_lambda, const float* __restrict__ grad_scale,
                                                const int32_t* __restrict__ sorted,
                                                const int32_t* __restrict__ order, float* __restrict__ grad,
                                                float* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int64_t total = 3 * batch;
  const int64_t base = w * kBprWin;
  if (base >= total) return;
  const int m = (int)(total - base < kBprWin ? total - base : kBprWin);
  const float scale = (grad_scale ? grad_scale[0] : 1.f) / (float)batch;
  const float lam = reg_lambda * scale;
  BprSample me;
  {
    const int64_t pos = base + (lane < m ? lane : m - 1);
    me.key = sorted[pos];
    const int64_t idx = order[pos];
    const int64_t b = idx % batch;
    me.role = (int32_t)(idx / batch);
    const int32_t ub = u[b], pb = p[b], nb = n[b];
    me.ok = (uint64_t)ub < (uint64_t)n_nodes && (uint64_t)pb < (uint64_t)n_nodes && (uint64_t)nb < (uint64_t)n_nodes &&
            (uint64_t)me.key < (uint64_t)n_nodes;
    const float cs = coef[b] * scale;   // -dL/dx
    // the partner rows: p and n for the source row (dL/ds = dL/dx (p - n)), the source row for p / n (dL/dp = dL/dx s,
    // dL/dn = -dL/dx s)
    me.r1 = me.ok ? (me.role == 0 ? pb : ub) : 0;
    me.r2 = me.ok ? (me.role == 0 ? nb : ub) : 0;
    me.cv = me.role == 0 ? cs : (me.role == 1 ? -cs : cs);
    if (!me.ok) me.key = me.key < 0 || (uint64_t)me.key >= (uint64_t)n_nodes ? (int32_t)n_nodes : me.key;
  }
  const int32_t prev_key = base > 0 ? sorted[base - 1] : -1;
  const int32_t next_key = base + m < total ? sorted[base + m] : -2;
  for (int c0 = 0; c0 < F; c0 += 256) {   // (every lane stays in the loop: the samples live in lanes 0-31)
    const bool live = c0 + lane * 4 < F;
    const int c = live ? c0 + lane * 4 : 0;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int32_t cur = __shfl(me.key, 0, 64);
    int64_t head = base;   // the sorted position at which the current run enters the window
    bool first_piece = true;
    auto flush = [&](bool last_piece) {
      if ((uint64_t)cur >= (uint64_t)n_nodes) return;              // ids outside the table carry nothing
      const bool starts = !(first_piece && prev_key == cur), ends = !(last_piece && next_key == cur);
      if (!live) return;
      if (starts && ends) *reinterpret_cast<float4*>(grad + (size_t)(COMPACT ? head : (int64_t)cur) * F + c) = acc;
      else *reinterpret_cast<float4*>(partials + ((size_t)w * 2 + (starts ? 1 : 0)) * F + c) = acc;
    };
    constexpr int RB = 8;   // positions whose rows are in flight together
    for (int t0 = 0; t0 < m; t0 += RB) {
      float4 x[RB], y[RB], o[RB];
      int32_t kt[RB], rl[RB];
      float cv[RB];
      bool okt[RB];
#pragma unroll
      for (int t = 0; t < RB; ++t) {
        const int tt = t0 + t < m ? t0 + t : m - 1;
        kt[t] = __shfl(me.key, tt, 64);
        rl[t] = __shfl(me.role, tt, 64);
        okt[t] = __shfl((int)me.ok, tt, 64) != 0;
        cv[t] = __shfl(me.cv, tt, 64);
        const int32_t a1 = __shfl(me.r1, tt, 64), a2 = __shfl(me.r2, tt, 64);
        x[t] = *reinterpret_cast<const float4*>(emb + (size_t)a1 * stride + c);
        y[t] = *reinterpret_cast<const float4*>(emb + (size_t)a2 * stride + c);
        o[t] = *reinterpret_cast<const float4*>(emb + (size_t)(okt[t] ? kt[t] : 0) * stride + c);
      }
#pragma unroll
      for (int t = 0; t < RB; ++t) {
        if (t0 + t >= m) continue;
        if (kt[t] != cur) {   // (wave-uniform)
          flush(false);
          acc = make_float4(0.f, 0.f, 0.f, 0.f);
          cur = kt[t];
          head = base + t0 + t;
          first_piece = false;
        }
        if (!okt[t]) continue;   // (a sample with an id outside the table: the forward made the loss NaN)
        float4 d;
        if (rl[t] == 0) d = make_float4(-cv[t] * (x[t].x - y[t].x), -cv[t] * (x[t].y - y[t].y), -cv[t] * (x[t].z - y[t].z),
                                        -cv[t] * (x[t].w - y[t].w));
        else d = make_float4(cv[t] * x[t].x, cv[t] * x[t].y, cv[t] * x[t].z, cv[t] * x[t].w);
        acc.x += d.x + lam * o[t].x; acc.y += d.y + lam * o[t].y; acc.z += d.z + lam * o[t].z; acc.w += d.w + lam * o[t].w;
      }
    }
    flush(true);
  }
}

__global__ __launch_bounds__(256) void bpr_window_kernel(int64_t batch, int64_t n_nodes, int F,
                                                         const float* __restrict__ emb, int64_t stride,
                                                         const int32_t* __restrict__ u, const int32_t* __restrict__ p,
                                                         const int32_t* __restrict__ n, const float* __restrict__ coef,
                                                         float reg_lambda, const float* __restrict__ grad_scale,
                                                         const int32_t* __restrict__ sorted,
                                                         const int32_t* __restrict__ order, float* __restrict__ grad,
                                                         float* __restrict__ partials) {
  bpr_window_body<false>((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), batch, n_nodes, F, emb, stride, u, p, n, coef,
                         reg_lambda, grad_scale, sorted, order, grad, partials);
}

// the runs that cross window edges: the wavefront of the window in which such a run begins (its last piece, slot 1)
// adds the following windows' first pieces (slot 0) in window order
__global__ __launch_bounds__(256) void bpr_carry_kernel(int64_t batch, int64_t n_nodes, int F,
                                                        const int32_t* __restrict__ sorted,
                                                        const float* __restrict__ partials, float* __restrict__ grad) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t total = 3 * batch;
  const int64_t base = w * kBprWin;
  if (base >= total) return;
  const int m = (int)(total - base < kBprWin ? total - base : kBprWin);
  if (base + m >= total) return;                      // the last window: nothing continues
  const int32_t key = sorted[base + m - 1];
  if (sorted[base + m] != key) return;                // its last run ends with the window
  if ((uint64_t)key >= (uint64_t)n_nodes) return;
  // does that run begin in this window?  (its first position is inside it, or it fills the window from its start on
  // with another id before it)
  if (sorted[base] == key && base > 0 && sorted[base - 1] == key) return;   // a middle window of the run
  // the windows behind it that the run reaches: window w + j continues it iff its first id is the key; it is the last
  // one iff the run ends inside it (or at its end)
  int64_t n_follow = 0;
  while (true) {   // 64 windows per look
    const int64_t wj = w + 1 + n_follow + lane;
    const bool cont = wj * kBprWin < total && sorted[wj * kBprWin] == key;
    const unsigned long long mk = __ballot(cont);
    if (mk == ~0ull) { n_follow += 64; continue; }
    n_follow += __builtin_ctzll(~mk);
    break;
  }
  for (int c0 = 0; c0 < F; c0 += 256) {
    const int c = c0 + lane * 4;
    if (c >= F) continue;
    float4 acc = *reinterpret_cast<const float4*>(partials + ((size_t)w * 2 + 1) * F + c);
    for (int64_t j0 = 0; j0 < n_follow; j0 += 8) {
      float4 v[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int64_t wj = w + 1 + (j0 + t < n_follow ? j0 + t : n_follow - 1);
        v[t] = *reinterpret_cast<const float4*>(partials + ((size_t)wj * 2 + 0) * F + c);
      }
#pragma unroll
      for (int t = 0; t < 8; ++t)
        if (j0 + t < n_follow) { acc.x += v[t].x; acc.y += v[t].y; acc.z += v[t].z; acc.w += v[t].w; }
    }
    *reinterpret_cast<float4*>(grad + (size_t)key * F + c) = acc;
  }
}

// ---- stable sort of the 3B row ids, role-major (i = role * B + b), beside the zero fill of the dense gradient.
// The general device sort (kgat_graph.hip) takes four launches per digit - twelve dependent launches for 30,720
// eighteen-bit keys, 0.10 of the CF step's 0.99 ms, all of it launch latency.  Here, up to 65,536 ids: launch one -
// workgroup L sorts slice L (4,096 consecutive ids) in LDS (LdsSort, kgat_lds_sort.h), packed values
// key << 17 | index; the workgroups behind the slices clear `zero` (the N x F gradient) meanwhile.  Launch two - one
// thread per id finds its place among ALL ids: its rank in its own slice + what the earlier slices hold up to its
// key + what the later slices hold below it (binary searches over <= 15 sorted slices): a stable merge without a
// merge tree.  Ids outside [0, N) sort as N, behind every real row.  (One workgroup sorting all 30,720 ids from
// registers was measured first: 180 us - 1,440 wavefront-iterations of ~100 instructions on one CU.)
constexpr int kSliceSort = 4096;
constexpr int kSliceSortMaxLists = 16;
constexpr int kSlicePosBits = 17;    // index among the 3B <= 65,536 ids
constexpr int kSliceDigitBits = 9;   // 18-bit ids (the CKGs of the reference's datasets) in TWO passes; eight bits took three

// slice `slice` of one batch's role-major id list, sorted into lists[slice * kSliceSort ...)
__device__ __forceinline__ void bpr_slice_sort_body(int32_t slice, int32_t batch, int64_t n_nodes, int key_bits,
                                                    const int32_t* __restrict__ u, const int32_t* __restrict__ p,
                                                    const int32_t* __restrict__ n, uint64_t* __restrict__ lists) {
  __shared__ LdsSort<uint64_t, kSliceSort, kSliceDigitBits, kSlicePosBits> s_sort;
  const int tid = threadIdx.x;
  const int32_t total = 3 * batch;
  const int32_t g0 = slice * kSliceSort;
  const int32_t cnt = total - g0 < kSliceSort ? total - g0 : kSliceSort;
  for (int32_t i = tid; i < cnt; i += kLdsSortThreads) {
    const int32_t gi = g0 + i;
    const int32_t role = gi / batch, b = gi - role * batch;
    const int32_t id = role == 0 ? u[b] : (role == 1 ? p[b] : n[b]);
    const uint64_t key = (uint64_t)(uint32_t)id >= (uint64_t)n_nodes ? (uint64_t)n_nodes : (uint64_t)id;
    s_sort.buf[0][i] = (key << kSlicePosBits) | (uint64_t)gi;
  }
  const uint64_t* s = s_sort.sort(cnt, key_bits);
  for (int32_t i = tid; i < cnt; i += kLdsSortThreads) lists[g0 + i] = s[i];
}

__global__ __launch_bounds__(kLdsSortThreads) void bpr_sort_zero_kernel(
    int32_t batch, int32_t n_lists, int64_t n_nodes, int key_bits, const int32_t* __restrict__ u,
    const int32_t* __restrict__ p, const int32_t* __restrict__ n, uint64_t* __restrict__ lists, float* __restrict__ zero,
    int64_t n_zero) {
  if ((int32_t)blockIdx.x >= n_lists) {
    zero_fill_behind(zero, n_zero, (unsigned)n_lists, kLdsSortThreads);
    return;
  }
  bpr_slice_sort_body((int32_t)blockIdx.x, batch, n_nodes, key_bits, u, p, n, lists);
}

// the place of every id among all ids (see above); thread t = position t of the concatenated sorted slices
// (NL: the slices the search is unrolled over - 8 at the CF step's batch, 30,720 ids in eight slices)
template <int NL>
__device__ __forceinline__ void bpr_merge_body(int32_t t, int32_t total, int32_t n_lists, const uint64_t* __restrict__ lists,
                                               int32_t* __restrict__ order, int32_t* __restrict__ sorted) {
  if (t >= total) return;
  const uint64_t v = lists[t];
  const uint64_t key = v >> kSlicePosBits;
  const int32_t mine = t / kSliceSort;
  int32_t pos = t - mine * kSliceSort;
  // One binary search per other slice - earlier slices: ids <= key come first (upper bound); later slices: ids < key
  // (lower bound) - all of them advanced TOGETHER, one probe of every slice per round: the probes of a round are
  // independent loads (round 6: slice after slice it was a chain of up to 15 x 12 dependent L2 round trips, 19.7 us
  // for the CF step's 30,720 ids).  Same positions.
  int32_t lo[NL], hi[NL];
#pragma unroll
  for (int L = 0; L < NL; ++L) {
    const int32_t g0 = L * kSliceSort;
    lo[L] = 0;
    hi[L] = (L < n_lists && L != mine) ? (total - g0 < kSliceSort ? total - g0 : kSliceSort) : 0;
  }
  for (int step = 0; step < 13; ++step) {   // 2^12 = kSliceSort entries: 13 halvings empty every range
    uint64_t probe[NL];
#pragma unroll
    for (int L = 0; L < NL; ++L) {
      // (unconditional: a load under a lane mask is waited for on the spot - sixteen round trips per round again; an
      //  empty range probes entry 0 of its slice, or of slice 0 if the slice does not exist, and ignores it)
      const int32_t mid = lo[L] < hi[L] ? (lo[L] + hi[L]) >> 1 : 0;
      probe[L] = lists[(L < n_lists ? L * kSliceSort : 0) + mid] >> kSlicePosBits;
    }
#pragma unroll
    for (int L = 0; L < NL; ++L) {
      const int32_t mid = (lo[L] + hi[L]) >> 1;
      const uint64_t bound = L < mine ? key + 1 : key;
      if (lo[L] < hi[L]) {
        if (probe[L] < bound) lo[L] = mid + 1; else hi[L] = mid;
      }
    }
  }
#pragma unroll
  for (int L = 0; L < NL; ++L) pos += lo[L];
  order[pos] = (int32_t)(v & ((1ull << kSlicePosBits) - 1ull));
  sorted[pos] = (int32_t)key;
}

template <int NL>
__global__ __launch_bounds__(256) void bpr_merge_kernel(int32_t total, int32_t n_lists, const uint64_t* __restrict__ lists,
                                                        int32_t* __restrict__ order, int32_t* __restrict__ sorted,
                                                        float* __restrict__ zero, int64_t n_zero) {
  // the blocks behind the merge's own: the second part of the gradient's zero fill (see kgat_bpr_grad_f32)
  const int32_t merge_blocks = (total + 255) / 256;
  if ((int32_t)blockIdx.x >= merge_blocks) {
    zero_fill_behind(zero, n_zero, (unsigned)merge_blocks, 256);
    return;
  }
  bpr_merge_body<NL>((int32_t)blockIdx.x * 256 + threadIdx.x, total, n_lists, lists, order, sorted);
}

// The workspace of both entries: per-sample partials (4 B floats) | keys, order (3 B int32 each) | the window partials
// of the gradient (two rows of F floats per 32 sorted positions) | sort scratch: the slice sort's packed lists + its
// sorted keys (up to kSliceSort * kSliceSortMaxLists ids), or the device radix sort's, whichever is larger.  Carved
// from `base`; over a null base `bytes` is all that is used.
struct BprWorkspace {
  float* part;
  int32_t *keys, *order;
  float* win_part;
  size_t sort_off;   // the sort scratch begins here
  uint64_t* lists = nullptr;
  int32_t* sorted = nullptr;
  size_t bytes;
};
static BprWorkspace bpr_workspace(void* base, int64_t batch, int F) {
  if (batch < 1) batch = 1;
  if (F < 4) F = 4;
  BprWorkspace w;
  Carver cv(base);
  w.part = cv.take<float>((size_t)batch * 4);
  w.keys = cv.take<int32_t>((size_t)batch * 3);
  w.order = cv.take<int32_t>((size_t)batch * 3);
  w.win_part = cv.take<float>((size_t)((3 * batch + kBprWin - 1) / kBprWin) * 2 * (size_t)F);
  w.sort_off = cv.off;
  Carver cs(cv.base + cv.off);
  if (3 * batch <= kSliceSort * kSliceSortMaxLists) {
    w.lists = cs.take<uint64_t>((size_t)batch * 3);
    w.sorted = cs.take<int32_t>((size_t)batch * 3);
  }
  const size_t radix = radix_sort_workspace_bytes(3 * batch);
  w.bytes = cv.off + (cs.off > radix ? cs.off : radix) + 256;
  return w;
}

// ---------------------------------------------------------------------------------------------
// BPR-MF pretraining as a sequence of three-launch iterations (reference kgat.py:150-168 with the embedding table itself
// as the readout: get_loss -> backward -> optimizer.step -> zero_grad; ~640 iterations per epoch at the amazon-book
// shape and the authors' MF batch of 1,024).  The treatment the KG phase got in kgat_transr.hip (transr_adam_step):
//  * the sort of a batch's 3 B row ids depends on nothing but the ids, and a phase's batches are drawn up front: ONE
//    launch sorts them all (mf_presort_kernel: a workgroup per batch, the shared LdsSort), role-major and stable - the
//    order the slice sort + rank merge above produce - and leaves sorted ids, order and run lengths per batch; beyond
//    8,192 ids per batch (up to 65,536: the reference's CF batch of 10,240) the slice sort + rank merge themselves, over
//    all batches at once, and a third launch for the run lengths;
//  * no dense gradient.  At most 3 B of the N rows have one, and torch's dense Adam moves every row all the same: the
//    window kernel (bpr_window_body<true>: the additions of bpr_window_kernel) writes a row completed inside its window
//    at the sorted position of the run's head in a 3 B x F buffer, pieces of crossing runs into the window's two partial
//    slots as ever; workgroups behind the windows tag the batch's rows in `row_slot` (one 64-bit word per node: call
//    tag << 17 | head position + 1; a stale word carries an older tag, so nothing is ever cleared), and the last
//    workgroup reduces the loss (bpr_reduce_body).  The Adam launch streams p, m, v of every row and takes g = 0 unless
//    the row's word carries this call's tag - then the row's compact sum, or for a crossing run its pieces in window
//    order (bpr_carry_kernel's order).  Gone: the N x F zero fill, the N x F gradient read, the sort and the merge in
//    front of every iteration, the carry launch.  Same arithmetic on the same values: the bits of kgat_bpr_loss_f32 +
//    kgat_bpr_grad_f32 + kgat_adam_step_f32.
// Every gradient row is a function of the OLD table, so the window launch must end before a parameter moves: the Adam
// launch cannot merge into it.
constexpr int kMfSmallSort = 8192;   // 3 B ids in one workgroup's LDS
constexpr int kMfPosBits = 13;       // a position among kMfSmallSort
constexpr int kMfMaxIds = kSliceSort * kSliceSortMaxLists;   // 3 B ids by slice sort + rank merge
constexpr int kMfSlotBits = 17;      // row_slot word = call tag << 17 | (sorted position of the run's head + 1 <= 65,536)
constexpr int kMfMaxF = 256;

// per-batch block of the presort's output (offsets in bytes, 256-byte aligned)
// (+ beyond kMfSmallSort ids: the slice sort's packed lists, scratch of the presort)
struct MfSortedLayout {
  size_t sorted_ids, order, run_len, lists, bytes;
};
static MfSortedLayout mf_sorted_layout(int64_t batch) {
  const size_t ids = 3 * (size_t)(batch > 0 ? batch : 1);
  const size_t piece = align_up(ids * 4, 256);
  return MfSortedLayout{0, piece, 2 * piece, 3 * piece, 3 * piece + (ids > (size_t)kMfSmallSort ? align_up(ids * 8, 256) : 0)};
}

struct MfPresortArgs {
  int32_t batch;
  int key_bits;
  int64_t n_nodes;
  const int32_t *u, *p, *n;   // n_batches x batch each
  unsigned char* sorted;
  MfSortedLayout lay;
};

// PT: uint32_t while every key (ids, and n_nodes for an id outside the table) is below 2^19, else uint64_t
template <typename PT>
__global__ __launch_bounds__(kLdsSortThreads) void mf_presort_kernel(MfPresortArgs a) {
  __shared__ LdsSort<PT, kMfSmallSort, sizeof(PT) == 4 ? 9 : 8, kMfPosBits> s_sort;
  const int tid = threadIdx.x;
  const int32_t total = 3 * a.batch;
  const size_t o = (size_t)blockIdx.x * a.batch;
  unsigned char* blk = a.sorted + (size_t)blockIdx.x * a.lay.bytes;
  int32_t* __restrict__ sorted_ids = reinterpret_cast<int32_t*>(blk + a.lay.sorted_ids);
  int32_t* __restrict__ order = reinterpret_cast<int32_t*>(blk + a.lay.order);
  int32_t* __restrict__ run_len = reinterpret_cast<int32_t*>(blk + a.lay.run_len);
  for (int32_t i = tid; i < total; i += kLdsSortThreads) {
    const int32_t role = i / a.batch, b = i - role * a.batch;
    const int32_t id = role == 0 ? a.u[o + b] : (role == 1 ? a.p[o + b] : a.n[o + b]);
    // (ids outside [0, N) sort as N, behind every real row: bpr_sort_zero_kernel's key)
    const PT key = (uint64_t)(uint32_t)id >= (uint64_t)a.n_nodes ? (PT)a.n_nodes : (PT)id;
    s_sort.buf[0][i] = (key << kMfPosBits) | (PT)i;
  }
  const PT* s = s_sort.sort(total, a.key_bits);
  for (int32_t q = tid; q < total; q += kLdsSortThreads) {
    const PT key = s[q] >> kMfPosBits;
    sorted_ids[q] = (int32_t)key;
    order[q] = (int32_t)(s[q] & (PT)(kMfSmallSort - 1));
    int32_t len = 0;   // the length of the run that STARTS at q, 0 elsewhere
    if (q == 0 || (s[q - 1] >> kMfPosBits) != key) {
      len = 1;
      while (q + len < total && (s[q + len] >> kMfPosBits) == key) ++len;
    }
    run_len[q] = len;
  }
}

// The same block for 8,192 < 3 B <= 65,536 ids in three launches over all batches (blockIdx.y = the batch): the slice
// sort, the rank merge (kgat_bpr_grad_f32's two, without the zero fill), and the run lengths - the head of a run finds
// the run's end by a binary search of the sorted ids.
__global__ __launch_bounds__(kLdsSortThreads) void mf_slice_sort_kernel(MfPresortArgs a) {
  const size_t o = (size_t)blockIdx.y * a.batch;
  unsigned char* blk = a.sorted + (size_t)blockIdx.y * a.lay.bytes;
  bpr_slice_sort_body((int32_t)blockIdx.x, a.batch, a.n_nodes, a.key_bits, a.u + o, a.p + o, a.n + o,
                      reinterpret_cast<uint64_t*>(blk + a.lay.lists));
}

template <int NL>
__global__ __launch_bounds__(256) void mf_merge_kernel(MfPresortArgs a, int32_t n_lists) {
  unsigned char* blk = a.sorted + (size_t)blockIdx.y * a.lay.bytes;
  bpr_merge_body<NL>((int32_t)blockIdx.x * 256 + threadIdx.x, 3 * a.batch, n_lists,
                     reinterpret_cast<const uint64_t*>(blk + a.lay.lists), reinterpret_cast<int32_t*>(blk + a.lay.order),
                     reinterpret_cast<int32_t*>(blk + a.lay.sorted_ids));
}

__global__ __launch_bounds__(256) void mf_run_len_kernel(MfPresortArgs a) {
  unsigned char* blk = a.sorted + (size_t)blockIdx.y * a.lay.bytes;
  const int32_t* __restrict__ sorted_ids = reinterpret_cast<const int32_t*>(blk + a.lay.sorted_ids);
  int32_t* __restrict__ run_len = reinterpret_cast<int32_t*>(blk + a.lay.run_len);
  const int32_t total = 3 * a.batch;
  const int32_t q = (int32_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= total) return;
  const int32_t key = sorted_ids[q];
  int32_t len = 0;
  if (q == 0 || sorted_ids[q - 1] != key) {
    int32_t lo = q + 1, hi = total;   // the first position behind q whose id is larger
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (sorted_ids[mid] <= key) lo = mid + 1; else hi = mid;
    }
    len = lo - q;
  }
  run_len[q] = len;
}

struct MfStepArgs {
  int64_t batch, n_nodes;
  int F;
  const float* emb;
  const int32_t *u, *p, *n;
  const float *coef, *part;
  float reg_lambda;
  const int32_t *sorted_ids, *order, *run_len;
  float *compact, *partials, *loss;
  unsigned long long* row_slot;
  unsigned long long tag;
  int win_blocks, tag_blocks;
};

// second launch of an iteration: blocks [0, win_blocks) the windows, the next tag_blocks the row tags (one thread per
// sorted position: the head of a run of a real row writes the row's word), the last block the loss
__global__ __launch_bounds__(256) void mf_window_kernel(MfStepArgs a) {
  const int bx = (int)blockIdx.x;
  if (bx < a.win_blocks) {
    bpr_window_body<true>((int64_t)bx * 4 + (threadIdx.x >> 6), a.batch, a.n_nodes, a.F, a.emb, a.F, a.u, a.p, a.n, a.coef,
                          a.reg_lambda, nullptr, a.sorted_ids, a.order, a.compact, a.partials);
  } else if (bx < a.win_blocks + a.tag_blocks) {
    row_tag_write<kMfSlotBits>(a.row_slot, a.tag, (int64_t)(bx - a.win_blocks) * 256 + threadIdx.x, 3 * a.batch, a.run_len,
                               a.sorted_ids, a.n_nodes);
  } else {
    bpr_reduce_body<256>(a.batch, a.part, a.reg_lambda, a.loss);
  }
}

// third launch: dense Adam over the table, the gradient through row_slot: adam_chunk_walk.
struct MfAdamArgs {
  AdamTensors<1> t;
  int F;
  int32_t total;   // 3 B
  const unsigned long long* row_slot;
  unsigned long long tag;
  const float *compact, *partials;
  const int32_t* run_len;
};

__global__ __launch_bounds__(256) void mf_adam_kernel(MfAdamArgs a, float w1, float beta2, float w2, float eps) {
  adam_chunk_walk(a.t, 0, w1, beta2, w2, eps, [&](int64_t i) {
    const int64_t row = i / a.F;
    const int c = (int)(i - row * a.F);
    const int32_t q = row_tag_position<kMfSlotBits>(a.row_slot, row, a.tag, a.total);
    if (q < 0) return zero4();
    const int32_t w = q / kBprWin, last = (q + run_length(a.run_len, q, a.total) - 1) / kBprWin;
    if (last == w) return *reinterpret_cast<const float4*>(a.compact + (size_t)q * a.F + c);
    // bpr_carry_kernel's order: the piece in the window where the run begins, then the following windows' first pieces
    // (every second row of the partials) in window order
    return ordered_row_sum<8>(a.partials, 2 * (size_t)a.F, w + 1, last - w, c,
                              *reinterpret_cast<const float4*>(a.partials + ((size_t)w * 2 + 1) * a.F + c));
  });
}

// the iteration's workspace: per-sample partials (4 B floats) | coef (B) | the compact gradient rows (3 B x F) | the
// windows' partial rows (two of F floats per 32 sorted positions)
struct MfStepWorkspace {
  float *part, *coef, *compact, *win_part;
  size_t bytes;
};
static MfStepWorkspace mf_step_workspace(void* base, int64_t batch, int F) {
  if (batch < 1) batch = 1;
  if (F < 4) F = 4;
  MfStepWorkspace w;
  Carver cv(base);
  w.part = cv.take<float>((size_t)batch * 4);
  w.coef = cv.take<float>((size_t)batch);
  w.compact = cv.take<float>((size_t)batch * 3 * (size_t)F);
  w.win_part = cv.take<float>((size_t)((3 * batch + kBprWin - 1) / kBprWin) * 2 * (size_t)F);
  w.bytes = cv.off;
  return w;
}

}  // namespace kgat

using namespace kgat;

extern "C" {

size_t kgat_bpr_workspace_bytes(int64_t batch, int F) { return bpr_workspace(nullptr, batch, F).bytes; }

int kgat_bpr_loss_f32(int64_t n_nodes, int F, const float* emb, int64_t emb_stride, int64_t batch, const int32_t* u,
                      const int32_t* p, const int32_t* n, float reg_lambda, float* loss, float* coef, void* workspace,
                      size_t workspace_bytes, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_nodes >= 0 && batch >= 1 && F >= 4 && F % 4 == 0 && emb_stride >= F && emb_stride % 4 == 0,
                 "bpr_loss: bad sizes (F and the row stride must be multiples of 4, batch >= 1)");
  KGAT_CHECK_ARG(batch < ((int64_t)1 << 29), "bpr_loss: batch too large");
  KGAT_CHECK_ARG(emb && u && p && n && loss && coef && workspace, "bpr_loss: null pointer");
  KGAT_CHECK_ARG((reinterpret_cast<uintptr_t>(emb) & 15) == 0, "bpr_loss: emb must be 16-byte aligned");
  const BprWorkspace w = bpr_workspace(workspace, batch, F);
  if (workspace_bytes < w.bytes) {
    set_error("bpr_loss: workspace too small");
    return KGAT_E_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(bpr_sample_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, batch, n_nodes, F, emb,
                     emb_stride, u, p, n, w.part, coef);
  KGAT_CHECK_LAUNCH("bpr_sample");
  hipLaunchKernelGGL(bpr_reduce_kernel, dim3(1), dim3(1024), 0, st, batch, (const float*)w.part, reg_lambda, loss);
  KGAT_CHECK_LAUNCH("bpr_reduce");
  return KGAT_OK;
}

int kgat_bpr_grad_f32(int64_t n_nodes, int F, const float* emb, int64_t emb_stride, int64_t batch, const int32_t* u,
                      const int32_t* p, const int32_t* n, const float* coef, float reg_lambda, const float* grad_scale,
                      float* grad, void* workspace, size_t workspace_bytes, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_nodes >= 1 && batch >= 1 && F >= 4 && F % 4 == 0 && emb_stride >= F && emb_stride % 4 == 0,
                 "bpr_grad: bad sizes (F and the row stride must be multiples of 4, batch >= 1)");
  KGAT_CHECK_ARG(batch < ((int64_t)1 << 29), "bpr_grad: batch too large");
  KGAT_CHECK_ARG(emb && u && p && n && coef && grad && workspace, "bpr_grad: null pointer");
  KGAT_CHECK_ARG(((reinterpret_cast<uintptr_t>(emb) | reinterpret_cast<uintptr_t>(grad)) & 15) == 0,
                 "bpr_grad: emb and grad must be 16-byte aligned");
  const BprWorkspace w = bpr_workspace(workspace, batch, F);
  if (workspace_bytes < w.bytes) {
    set_error("bpr_grad: workspace too small");
    return KGAT_E_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int32_t* sorted = nullptr;
  if (w.lists != nullptr && n_nodes < ((int64_t)1 << 30)) {
    const int32_t total = (int32_t)(3 * batch), n_lists = (total + kSliceSort - 1) / kSliceSort;
    // The zero fill of the N x F gradient (112 MB at the amazon-book size: 25 us of stores) rides beside the two
    // launches in front of the scatter, both of them chains of round trips on a few workgroups: the sort's launch
    // (~17 us with two radix passes) takes the first 75 %, the merge's (12 us) the rest.  F is a multiple of 4, so both
    // parts are whole float4s.
    const unsigned zero_blocks = 2u * (unsigned)device_cu_count();
    const int64_t n_all = (int64_t)n_nodes * F;
    const int64_t n_first = (n_all * 75 / 100) / 4 * 4;
    hipLaunchKernelGGL(bpr_sort_zero_kernel, dim3((unsigned)n_lists + zero_blocks), dim3(kLdsSortThreads), 0, st,
                       (int32_t)batch, n_lists, n_nodes, bits_for(n_nodes), u, p, n, w.lists, grad, n_first);
    KGAT_CHECK_LAUNCH("bpr_sort_zero");
    const unsigned merge_blocks = (unsigned)((total + 255) / 256), zero_blocks2 = 8u * (unsigned)device_cu_count();
    if (n_lists <= 8)
      hipLaunchKernelGGL(bpr_merge_kernel<8>, dim3(merge_blocks + zero_blocks2), dim3(256), 0, st, total, n_lists,
                         (const uint64_t*)w.lists, w.order, w.sorted, grad + n_first, n_all - n_first);
    else
      hipLaunchKernelGGL(bpr_merge_kernel<kSliceSortMaxLists>, dim3(merge_blocks + zero_blocks2), dim3(256), 0, st, total,
                         n_lists, (const uint64_t*)w.lists, w.order, w.sorted, grad + n_first, n_all - n_first);
    KGAT_CHECK_LAUNCH("bpr_merge");
    sorted = w.sorted;
  } else {
    hipLaunchKernelGGL(bpr_keys_kernel, dim3((unsigned)((3 * batch + 255) / 256)), dim3(256), 0, st, batch, u, p, n, w.keys);
    KGAT_CHECK_LAUNCH("bpr_keys");
    const int rc = radix_sort_index(w.keys, 3 * batch, bits_for(n_nodes - 1), w.order, &sorted,
                                    static_cast<char*>(workspace) + w.sort_off, workspace_bytes - w.sort_off, st);
    if (rc != KGAT_OK) return rc;
    if (hipMemsetAsync(grad, 0, (size_t)n_nodes * F * sizeof(float), st) != hipSuccess) {
      set_error("bpr_grad: memset failed");
      return KGAT_E_HIP;
    }
  }
  {
    const int64_t n_win = (3 * batch + kBprWin - 1) / kBprWin;
    hipLaunchKernelGGL(bpr_window_kernel, dim3((unsigned)((n_win + 3) / 4)), dim3(256), 0, st, batch, n_nodes, F, emb,
                       emb_stride, u, p, n, coef, reg_lambda, grad_scale, sorted, (const int32_t*)w.order, grad, w.win_part);
    KGAT_CHECK_LAUNCH("bpr_window");
    hipLaunchKernelGGL(bpr_carry_kernel, dim3((unsigned)((n_win + 3) / 4)), dim3(256), 0, st, batch, n_nodes, F, sorted,
                       (const float*)w.win_part, grad);
  }
  KGAT_CHECK_LAUNCH("bpr_carry");
  return KGAT_OK;
}

int kgat_mf_supported(int64_t n_nodes, int F, int64_t batch) {
  return F >= 4 && F % 4 == 0 && F <= kMfMaxF && batch > 0 && 3 * batch <= kMfMaxIds && n_nodes > 0 && n_nodes < INT32_MAX;
}

size_t kgat_mf_sorted_bytes(int64_t batch) { return mf_sorted_layout(batch).bytes; }

int kgat_mf_presort_f32(int64_t n_nodes, int64_t n_batches, int64_t batch, const int32_t* u, const int32_t* p,
                        const int32_t* n, void* sorted, size_t sorted_bytes, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_batches >= 0 && n_batches < (1 << 30), "mf_presort: bad batch count");
  if (!kgat_mf_supported(n_nodes, 4, batch)) {
    set_error("mf_presort: needs 1 <= batch <= %d, 1 <= n_nodes < 2^31 (batch=%lld n_nodes=%lld)", kMfMaxIds / 3,
              (long long)batch, (long long)n_nodes);
    return KGAT_E_UNSUPPORTED;
  }
  if (n_batches == 0) return KGAT_OK;
  KGAT_CHECK_ARG(u && p && n && sorted, "mf_presort: null pointer");
  const MfSortedLayout lay = mf_sorted_layout(batch);
  if (sorted_bytes < (size_t)n_batches * lay.bytes) {
    set_error("mf_presort: output buffer too small");
    return KGAT_E_WORKSPACE;
  }
  const int key_bits = bits_for(n_nodes);   // (the key of an id outside the table is n_nodes itself)
  const MfPresortArgs a = {(int32_t)batch, key_bits, n_nodes, u, p, n, static_cast<unsigned char*>(sorted), lay};
  if (3 * batch > kMfSmallSort) {
    const int32_t total = (int32_t)(3 * batch), n_lists = (total + kSliceSort - 1) / kSliceSort;
    const unsigned nb = (unsigned)n_batches;   // (gridDim.y <= 65,535)
    KGAT_CHECK_ARG(n_batches <= 65535, "mf_presort: at most 65,535 batches of more than %d ids per call", kMfSmallSort);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mf_slice_sort_kernel, dim3((unsigned)n_lists, nb), dim3(kLdsSortThreads), 0, st, a);
    KGAT_CHECK_LAUNCH("mf_slice_sort");
    const unsigned merge_blocks = (unsigned)((total + 255) / 256);
    if (n_lists <= 8) hipLaunchKernelGGL(mf_merge_kernel<8>, dim3(merge_blocks, nb), dim3(256), 0, st, a, n_lists);
    else hipLaunchKernelGGL(mf_merge_kernel<kSliceSortMaxLists>, dim3(merge_blocks, nb), dim3(256), 0, st, a, n_lists);
    KGAT_CHECK_LAUNCH("mf_merge");
    hipLaunchKernelGGL(mf_run_len_kernel, dim3(merge_blocks, nb), dim3(256), 0, st, a);
    KGAT_CHECK_LAUNCH("mf_run_len");
    return KGAT_OK;
  }
  if (key_bits > 32 - kMfPosBits)
    hipLaunchKernelGGL(mf_presort_kernel<uint64_t>, dim3((unsigned)n_batches), dim3(kLdsSortThreads), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(mf_presort_kernel<uint32_t>, dim3((unsigned)n_batches), dim3(kLdsSortThreads), 0, as_stream(stream), a);
  KGAT_CHECK_LAUNCH("mf_presort");
  return KGAT_OK;
}

size_t kgat_mf_step_workspace_bytes(int64_t batch, int F) { return mf_step_workspace(nullptr, batch, F).bytes; }

int kgat_mf_adam_step_f32(int64_t n_nodes, int F, int64_t batch, const int32_t* u, const int32_t* p, const int32_t* n,
                          const void* sorted, float* emb, float* exp_avg, float* exp_avg_sq, int64_t step, double lr,
                          double beta1, double beta2, double eps, float reg_lambda, float* loss, uint64_t* row_slot,
                          uint64_t tag, void* workspace, size_t workspace_bytes, kgat_stream_t stream) {
  if (!kgat_mf_supported(n_nodes, F, batch)) {
    set_error("mf_adam_step: needs F a multiple of 4 and <= %d, 1 <= batch <= %d, 1 <= n_nodes < 2^31 (F=%d batch=%lld n_nodes=%lld)",
              kMfMaxF, kMfMaxIds / 3, F, (long long)batch, (long long)n_nodes);
    return KGAT_E_UNSUPPORTED;
  }
  KGAT_CHECK_ARG(u && p && n && sorted && emb && exp_avg && exp_avg_sq && loss && row_slot && workspace,
                 "mf_adam_step: null pointer");
  KGAT_RETURN_IF(row_tag_check<kMfSlotBits>("mf_adam_step", tag));
  MfAdamArgs ad;
  const int64_t n_elem = n_nodes * F;
  KGAT_RETURN_IF(adam_fill("mf_adam_step", ad.t, 1, &n_elem, &emb, &exp_avg, &exp_avg_sq, &step, lr, beta1, beta2, eps, true));
  KGAT_CHECK_ARG(aligned16(sorted) && aligned16(workspace),
                 "mf_adam_step: the sorted block and the workspace must be 16-byte aligned");
  const MfStepWorkspace w = mf_step_workspace(workspace, batch, F);
  if (workspace_bytes < w.bytes) {
    set_error("mf_adam_step: workspace too small");
    return KGAT_E_WORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const MfSortedLayout lay = mf_sorted_layout(batch);
  const unsigned char* blk = static_cast<const unsigned char*>(sorted);
  const int32_t* sorted_ids = reinterpret_cast<const int32_t*>(blk + lay.sorted_ids);
  const int32_t* order = reinterpret_cast<const int32_t*>(blk + lay.order);
  const int32_t* run_len = reinterpret_cast<const int32_t*>(blk + lay.run_len);
  hipLaunchKernelGGL(bpr_sample_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, st, batch, n_nodes, F,
                     (const float*)emb, (int64_t)F, u, p, n, w.part, w.coef);
  KGAT_CHECK_LAUNCH("mf_sample");
  const int64_t n_win = (3 * batch + kBprWin - 1) / kBprWin;
  MfStepArgs a;
  a.batch = batch; a.n_nodes = n_nodes; a.F = F; a.emb = emb; a.u = u; a.p = p; a.n = n;
  a.coef = w.coef; a.part = w.part; a.reg_lambda = reg_lambda;
  a.sorted_ids = sorted_ids; a.order = order; a.run_len = run_len;
  a.compact = w.compact; a.partials = w.win_part; a.loss = loss;
  a.row_slot = reinterpret_cast<unsigned long long*>(row_slot);
  a.tag = (unsigned long long)tag;
  a.win_blocks = (int)((n_win + 3) / 4);
  a.tag_blocks = (int)((3 * batch + 255) / 256);
  hipLaunchKernelGGL(mf_window_kernel, dim3((unsigned)(a.win_blocks + a.tag_blocks + 1)), dim3(256), 0, st, a);
  KGAT_CHECK_LAUNCH("mf_window");
  ad.F = F; ad.total = (int32_t)(3 * batch);
  ad.row_slot = a.row_slot; ad.tag = a.tag; ad.compact = w.compact; ad.partials = w.win_part; ad.run_len = run_len;
  hipLaunchKernelGGL(mf_adam_kernel, dim3((unsigned)ad.t.first_block[1]), dim3(256), 0, st, ad, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), (float)eps);
  KGAT_CHECK_LAUNCH("mf_adam");
  return KGAT_OK;
}

}  // extern "C"
