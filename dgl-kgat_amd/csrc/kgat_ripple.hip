// Ripple-set attention for gfx950: the inner operator of RippleNet (Wang et al., CIKM 2018), the KGAT paper's
// path-based baseline.  A user's ripple set of hop k is M triples (h_i, r_i, t_i), sorted ascending by (r, h, t); for
// sample b with user u_b and the query table U (n_samples x n_rel x d, U[b, r] = v_b R_r, one matmul of the caller)
//     s_i = <U[b, r_i], ent[h_i]>      p = softmax_i(s)      o[b] = sum_i p_i ent[t_i]
// and, given g_o,
//     gp_i = <ent[t_i], g_o[b]>        gl_i = p_i (gp_i - sum_j p_j gp_j)
//     grad_U[b, r] = sum_{i : r_i = r} gl_i ent[h_i]          (a zero row for a relation the set lacks)
// In torch operators this gathers three (n_samples, M, d) blocks; here nothing of that size exists.  Both kernels: one
// wavefront per sample (four per workgroup), d / 4 lanes per row (16 bytes per lane), G = 256 / d lane groups.
//   forward   slot i goes to group i mod G, four slots of a group in flight per look.  A logit: per lane
//             fma(x.w, q.w, fma(x.z, q.z, fma(x.y, q.y, x.x * q.x))) over its four columns, then the butterfly over the
//             d / 4 lanes of the group (strides d / 8, ..., 1).  The logits sit in LDS (at most 128 per sample).  The first
//             look of tail rows is requested BEFORE the softmax's reductions.  Softmax: lane j holds slots j and j + 64;
//             the maximum over the wavefront (exact in any order), e = expf(s - max), the lane's e_j + e_{j + 64}, the
//             butterfly over the 64 lanes (strides 32, ..., 1), p = e / sum.  o: a group adds p_i * ent[t_i] (one fma per
//             column) in ascending i from 0; the G partials are combined by the butterfly over the groups (g with
//             g ^ G/2, ..., g ^ 1).
//   backward  gp as the logits above (tail rows against g_o[b]); lane j forms fma(p_{j+64}, gp_{j+64}, p_j * gp_j), the
//             64-lane butterfly gives sum_j p_j gp_j; gl = p * (gp - sum).  grad_U: relation r goes to group r mod G,
//             which finds r's run in the sorted set (two binary searches over the relations in LDS) and adds
//             gl_i * ent[h_i] (one fma per column) in ascending i from the run's first slot - no combination across
//             groups - and writes the row once, zeros where the run is empty.  No memset.
// No float atomics, every order fixed: bitwise reproducible.  All arithmetic fp32 on the vector ALU.
// A sample whose user id lies outside [0, n_users), or whose set holds an id outside its table, reads nothing there
// and gets NaN outputs (torch would fail a device-side assertion).
// What bounds them: the forward two 16-byte gathers per lane and slot plus one read of U[b]'s touched rows; the backward
// the same two gathers plus the dense write of grad_U[b] (n_rel x d per sample).
#include "kgat_common.h"

namespace kgat {

constexpr int kRpMaxMemory = 128;   // slots of a set: the logits of a sample in LDS, two per lane
constexpr int kRpMaxRel = 4096;
constexpr int kRpLook = 4;          // rows a lane group requests per look
using RpWidths = WidthList<16, 32, 64, 128>;

struct RpArgs {
  int64_t n_samples;
  int32_t n_memory, n_rel, n_hop, hop, n_nodes, n_users;
  const float *ent, *U;
  const int32_t *mem_h, *mem_r, *mem_t, *users;
  float *o, *p;                  // forward
  const float *p_in, *g_o;       // backward
  float *grad_U, *gl;
};

// what one lane's LDS write shows to the other lanes of its wavefront
__device__ __forceinline__ void rp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float rp_dot4(const float4& x, const float4& q) {
  return fmaf(x.w, q.w, fmaf(x.z, q.z, fmaf(x.y, q.y, x.x * q.x)));
}
// the butterfly over the L lanes of a group: strides L / 2, ..., 1
template <int L>
__device__ __forceinline__ float rp_lanes_sum(float v) {
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
// the butterfly over the lane groups of a wavefront (L lanes each): strides 32, 16, ..., L
template <int L>
__device__ __forceinline__ float rp_groups_sum(float v) {
#pragma unroll
  for (int off = kWave / 2; off >= L; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
__device__ __forceinline__ float rp_wave_max(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}

// The set of sample b: its first slot in mem_h / mem_r / mem_t, or -1 for a user id outside [0, n_users).
__device__ __forceinline__ int64_t rp_set_of(const RpArgs& a, int64_t b) {
  const int32_t u = a.users[b];
  if ((uint32_t)u >= (uint32_t)a.n_users) return -1;
  return ((int64_t)u * a.n_hop + a.hop) * a.n_memory;
}

// The dots <row(ids[i]), q_i> of every slot into s_out[0 .. M): slot i to group i mod G, kRpLook slots per look.  `q_of`
// gives the lane's four columns of slot i's query (called for in-range slots only).  Returns whether an id was bad.
template <int D, typename QOf>
__device__ __forceinline__ bool rp_slot_dots(const float* __restrict__ table, int32_t n_rows, const int32_t* __restrict__ ids,
                                             int M, float* s_out, QOf q_of) {
  constexpr int L = D / 4, G = kWave / L;
  const int lane = threadIdx.x & (kWave - 1), sl = lane % L, g = lane / L, c = 4 * sl;
  bool bad = false;
  for (int i0 = 0; i0 < M; i0 += G * kRpLook) {
    float4 x[kRpLook], q[kRpLook];
#pragma unroll
    for (int u = 0; u < kRpLook; ++u) {
      const int i = i0 + u * G + g;
      x[u] = q[u] = zero4();
      if (i < M) {
        const int32_t id = ids[i];
        if ((uint32_t)id < (uint32_t)n_rows) {
          x[u] = *reinterpret_cast<const float4*>(table + (size_t)id * D + c);
          bad |= !q_of(i, q[u]);
        } else {
          bad = true;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kRpLook; ++u) {
      const int i = i0 + u * G + g;
      const float s = rp_lanes_sum<L>(rp_dot4(x[u], q[u]));
      if (sl == 0 && i < M) s_out[i] = s;
    }
  }
  return bad;
}

// ---- forward: wavefront w of the grid takes sample w.
template <int D>
__global__ __launch_bounds__(256) void ripple_fwd_kernel(RpArgs a) {
  constexpr int L = D / 4, G = kWave / L;
  __shared__ float s_p[4][kRpMaxMemory];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1), sl = lane % L, g = lane / L, c = 4 * sl;
  const int64_t b = (int64_t)blockIdx.x * 4 + wv;
  if (b >= a.n_samples) return;   // (whole wavefronts leave)
  const int M = a.n_memory;
  const int64_t set = rp_set_of(a, b);
  bool bad = set < 0;
  const int32_t* __restrict__ mh = a.mem_h + (bad ? 0 : set);
  const int32_t* __restrict__ mr = a.mem_r + (bad ? 0 : set);
  const int32_t* __restrict__ mt = a.mem_t + (bad ? 0 : set);
  const float* __restrict__ Ub = a.U + (size_t)b * a.n_rel * D;
  float* sp = s_p[wv];
  const int n_slots = bad ? 0 : M;   // (a bad user's set is never read)
  bad |= rp_slot_dots<D>(a.ent, a.n_nodes, mh, n_slots, sp, [&](int i, float4& q) {
    const int32_t r = mr[i];
    if ((uint32_t)r >= (uint32_t)a.n_rel) return false;
    q = *reinterpret_cast<const float4*>(Ub + (size_t)r * D + c);
    return true;
  });
  auto load_tails = [&](int i0, float4* x) {
#pragma unroll
    for (int u = 0; u < kRpLook; ++u) {
      const int i = i0 + u * G + g;
      x[u] = zero4();
      if (i < n_slots) {
        const int32_t t = mt[i];
        if ((uint32_t)t < (uint32_t)a.n_nodes) x[u] = *reinterpret_cast<const float4*>(a.ent + (size_t)t * D + c);
        else bad = true;
      }
    }
  };
  float4 x[kRpLook];
  load_tails(0, x);   // in flight across the softmax
  rp_wave_sync();
  const int j0 = lane, j1 = lane + kWave;
  const float s0 = j0 < n_slots ? sp[j0] : -INFINITY, s1 = j1 < n_slots ? sp[j1] : -INFINITY;
  const float mx = rp_wave_max(fmaxf(s0, s1));
  const float e0 = j0 < n_slots ? expf(s0 - mx) : 0.f, e1 = j1 < n_slots ? expf(s1 - mx) : 0.f;
  const float sum = wave_sum(e0 + e1);
  float p0 = e0 / sum, p1 = e1 / sum;
  rp_wave_sync();   // (every lane has read its logits)
  if (j0 < n_slots) sp[j0] = p0;
  if (j1 < n_slots) sp[j1] = p1;
  rp_wave_sync();
  float4 acc = zero4();
  for (int i0 = 0; i0 < n_slots; i0 += G * kRpLook) {
    if (i0 > 0) load_tails(i0, x);
#pragma unroll
    for (int u = 0; u < kRpLook; ++u) {   // (a slot past the end adds +0 * 0: no bit changes)
      const int i = i0 + u * G + g;
      acc = fma4(i < n_slots ? sp[i] : 0.f, x[u], acc);
    }
  }
  acc = make_float4(rp_groups_sum<L>(acc.x), rp_groups_sum<L>(acc.y), rp_groups_sum<L>(acc.z), rp_groups_sum<L>(acc.w));
  if (__ballot(bad) != 0ull) {
    const float nan = __builtin_nanf("");
    acc = make_float4(nan, nan, nan, nan);
    p0 = p1 = nan;
  }
  if (g == 0) *reinterpret_cast<float4*>(a.o + (size_t)b * D + c) = acc;
  if (j0 < M) a.p[(size_t)b * M + j0] = p0;
  if (j1 < M) a.p[(size_t)b * M + j1] = p1;
}

// ---- backward: wavefront w of the grid writes gl[w] and every row of grad_U[w].
template <int D>
__global__ __launch_bounds__(256) void ripple_bwd_kernel(RpArgs a) {
  constexpr int L = D / 4, G = kWave / L;
  __shared__ float s_g[4][kRpMaxMemory];
  __shared__ int32_t s_r[4][kRpMaxMemory];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1), sl = lane % L, g = lane / L, c = 4 * sl;
  const int64_t b = (int64_t)blockIdx.x * 4 + wv;
  if (b >= a.n_samples) return;   // (whole wavefronts leave)
  const int M = a.n_memory;
  const int64_t set = rp_set_of(a, b);
  bool bad = set < 0;
  const int32_t* __restrict__ mh = a.mem_h + (bad ? 0 : set);
  const int32_t* __restrict__ mr = a.mem_r + (bad ? 0 : set);
  const int32_t* __restrict__ mt = a.mem_t + (bad ? 0 : set);
  float* sg = s_g[wv];
  int32_t* sr = s_r[wv];
  const int n_slots = bad ? 0 : M;
  const float4 go = *reinterpret_cast<const float4*>(a.g_o + (size_t)b * D + c);
  bad |= rp_slot_dots<D>(a.ent, a.n_nodes, mt, n_slots, sg, [&](int, float4& q) {
    q = go;
    return true;
  });
  const int j0 = lane, j1 = lane + kWave;
  if (j0 < n_slots) sr[j0] = mr[j0];
  if (j1 < n_slots) sr[j1] = mr[j1];
  rp_wave_sync();
  const float p0 = j0 < n_slots ? a.p_in[(size_t)b * M + j0] : 0.f, p1 = j1 < n_slots ? a.p_in[(size_t)b * M + j1] : 0.f;
  const float gp0 = j0 < n_slots ? sg[j0] : 0.f, gp1 = j1 < n_slots ? sg[j1] : 0.f;
  const float dot = wave_sum(fmaf(p1, gp1, p0 * gp0));
  float gl0 = p0 * (gp0 - dot), gl1 = p1 * (gp1 - dot);
  rp_wave_sync();   // (every lane has read its gp)
  if (j0 < n_slots) sg[j0] = gl0;
  if (j1 < n_slots) sg[j1] = gl1;
  rp_wave_sync();
  // a bad id anywhere in the set is known before the first row is written
  for (int i = lane; i < n_slots; i += kWave) bad |= (uint32_t)mh[i] >= (uint32_t)a.n_nodes;
  const bool poison = __ballot(bad) != 0ull;
  const float nan = __builtin_nanf("");
  float* __restrict__ gU = a.grad_U + (size_t)b * a.n_rel * D;
  for (int r0 = 0; r0 < a.n_rel; r0 += G) {
    const int r = r0 + g;
    if (r >= a.n_rel) continue;
    int lo = 0, hi = 0;
    if (!poison) {
      // r's run [lo, hi): the first slot whose relation is >= r, the first whose relation is > r
      int e = n_slots;
      while (lo < e) {
        const int mid = (lo + e) >> 1;
        if (sr[mid] < r) lo = mid + 1; else e = mid;
      }
      hi = lo;
      e = n_slots;
      while (hi < e) {
        const int mid = (hi + e) >> 1;
        if (sr[mid] <= r) hi = mid + 1; else e = mid;
      }
    }
    float4 acc = poison ? make_float4(nan, nan, nan, nan) : zero4();
    for (int i0 = lo; i0 < hi; i0 += kRpLook) {
      float4 x[kRpLook];
      float w[kRpLook];
#pragma unroll
      for (int u = 0; u < kRpLook; ++u) {
        const int i = i0 + u;
        x[u] = zero4();
        w[u] = 0.f;
        if (i < hi) {
          x[u] = *reinterpret_cast<const float4*>(a.ent + (size_t)mh[i] * D + c);   // (in range: checked above)
          w[u] = sg[i];
        }
      }
#pragma unroll
      for (int u = 0; u < kRpLook; ++u)
        if (i0 + u < hi) acc = fma4(w[u], x[u], acc);
    }
    *reinterpret_cast<float4*>(gU + (size_t)r * D + c) = acc;
  }
  if (j0 < M) a.gl[(size_t)b * M + j0] = poison ? nan : gl0;
  if (j1 < M) a.gl[(size_t)b * M + j1] = poison ? nan : gl1;
}

// the checks both entries share
static int ripple_check(const char* who, int64_t n_samples, int d, int n_memory, int n_rel, int n_hop, int hop,
                        int64_t n_nodes, int64_t n_users) {
  KGAT_CHECK_ARG(n_samples >= 0 && d >= 0 && n_memory >= 0 && n_rel >= 0 && n_hop >= 1 && n_nodes > 0 && n_nodes < INT32_MAX &&
                 n_users > 0 && n_users < INT32_MAX, "%s: needs n_samples, d, n_memory, n_rel >= 0, n_hop >= 1 and 1 <= n_nodes, "
                 "n_users < 2^31 (n_samples=%lld d=%d n_memory=%d n_rel=%d n_hop=%d n_nodes=%lld n_users=%lld)", who,
                 (long long)n_samples, d, n_memory, n_rel, n_hop, (long long)n_nodes, (long long)n_users);
  KGAT_CHECK_ARG(hop >= 0 && hop < n_hop, "%s: hop %d outside [0, %d)", who, hop, n_hop);
  if (!kgat_ripple_supported(d, n_memory, n_rel, n_samples)) {
    set_error("%s: needs d in {16, 32, 64, 128}, 1 <= n_memory <= %d, 1 <= n_rel <= %d and 1 <= n_samples <= 4 (2^31 - 1) (d=%d "
              "n_memory=%d n_rel=%d n_samples=%lld)", who, kRpMaxMemory, kRpMaxRel, d, n_memory, n_rel, (long long)n_samples);
    return KGAT_E_UNSUPPORTED;
  }
  return KGAT_OK;
}

}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_ripple_supported(int d, int n_memory, int n_rel, int64_t n_samples) {
  return has_width(RpWidths{}, d) && n_memory >= 1 && n_memory <= kRpMaxMemory && n_rel >= 1 && n_rel <= kRpMaxRel &&
         n_samples >= 1 && (n_samples + 3) / 4 <= (int64_t)INT32_MAX;
}

int kgat_ripple_hop_fwd_f32(int64_t n_samples, int d, int n_memory, int n_rel, int n_hop, int hop, int64_t n_nodes,
                            int64_t n_users, const float* ent, const float* U, const int32_t* mem_h, const int32_t* mem_r,
                            const int32_t* mem_t, const int32_t* users, float* o, float* p, kgat_stream_t stream) {
  KGAT_RETURN_IF(ripple_check("ripple_hop_fwd", n_samples, d, n_memory, n_rel, n_hop, hop, n_nodes, n_users));
  KGAT_CHECK_ARG(ent && U && mem_h && mem_r && mem_t && users && o && p, "ripple_hop_fwd: null pointer");
  KGAT_CHECK_ARG(aligned16(ent) && aligned16(U) && aligned16(o), "ripple_hop_fwd: ent, U and o must be 16-byte aligned");
  RpArgs a = {};
  a.n_samples = n_samples; a.n_memory = n_memory; a.n_rel = n_rel; a.n_hop = n_hop; a.hop = hop;
  a.n_nodes = (int32_t)n_nodes; a.n_users = (int32_t)n_users;
  a.ent = ent; a.U = U; a.mem_h = mem_h; a.mem_r = mem_r; a.mem_t = mem_t; a.users = users; a.o = o; a.p = p;
  const unsigned blocks = (unsigned)((n_samples + 3) / 4);
  hipStream_t st = as_stream(stream);
  return dispatch_width(RpWidths{}, d, [&](auto w) -> int {
    hipLaunchKernelGGL(ripple_fwd_kernel<decltype(w)::value>, dim3(blocks), dim3(256), 0, st, a);
    KGAT_CHECK_LAUNCH("ripple_hop_fwd");
    return (int)KGAT_OK;
  });
}

int kgat_ripple_hop_bwd_f32(int64_t n_samples, int d, int n_memory, int n_rel, int n_hop, int hop, int64_t n_nodes,
                            int64_t n_users, const float* ent, const float* U, const int32_t* mem_h, const int32_t* mem_r,
                            const int32_t* mem_t, const int32_t* users, const float* p, const float* g_o, float* grad_U,
                            float* gl, kgat_stream_t stream) {
  KGAT_RETURN_IF(ripple_check("ripple_hop_bwd", n_samples, d, n_memory, n_rel, n_hop, hop, n_nodes, n_users));
  KGAT_CHECK_ARG(ent && U && mem_h && mem_r && mem_t && users && p && g_o && grad_U && gl, "ripple_hop_bwd: null pointer");
  KGAT_CHECK_ARG(aligned16(ent) && aligned16(U) && aligned16(g_o) && aligned16(grad_U),
                 "ripple_hop_bwd: ent, U, g_o and grad_U must be 16-byte aligned");
  RpArgs a = {};
  a.n_samples = n_samples; a.n_memory = n_memory; a.n_rel = n_rel; a.n_hop = n_hop; a.hop = hop;
  a.n_nodes = (int32_t)n_nodes; a.n_users = (int32_t)n_users;
  a.ent = ent; a.U = U; a.mem_h = mem_h; a.mem_r = mem_r; a.mem_t = mem_t; a.users = users;
  a.p_in = p; a.g_o = g_o; a.grad_U = grad_U; a.gl = gl;
  const unsigned blocks = (unsigned)((n_samples + 3) / 4);
  hipStream_t st = as_stream(stream);
  return dispatch_width(RpWidths{}, d, [&](auto w) -> int {
    hipLaunchKernelGGL(ripple_bwd_kernel<decltype(w)::value>, dim3(blocks), dim3(256), 0, st, a);
    KGAT_CHECK_LAUNCH("ripple_hop_bwd");
    return (int)KGAT_OK;
  });
}

}  // extern "C"
