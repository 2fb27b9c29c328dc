// Shared pieces of the attention-logit kernels (internal; see kgat_att.hip for the design).
#pragma once
#include <math.h>

#include "kgat_common.h"

namespace kgat {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kAttThreads = 256;
constexpr int kAttChunk = 1024;  // edges of one relation per workgroup

// Locate (relation, chunk) for a block: blocks are laid out relation by relation,
// ceil(E_r / kAttChunk) blocks each.  Returns false past the end.
__device__ __forceinline__ bool att_locate(const int32_t* __restrict__ rel_ptr, int n_rel,
                                           int block, int& r_out, int32_t& beg, int32_t& end) {
  int acc = 0;
  for (int r = 0; r < n_rel; ++r) {
    const int32_t b = rel_ptr[r], e = rel_ptr[r + 1];
    const int nb = (e - b + kAttChunk - 1) / kAttChunk;
    if (block < acc + nb) {
      r_out = r;
      beg = b + (block - acc) * kAttChunk;
      end = (beg + kAttChunk < e) ? beg + kAttChunk : e;
      return true;
    }
    acc += nb;
  }
  return false;
}

// tanh for the epilogue.  ACCURATE = 0: 1 - 2/(exp(2x)+1) with the hardware exp2/rcp
// (absolute error ~1e-7, which is what the logit sum_j t_j*tanh(.) is sensitive to; the
// relative error near 0 is not preserved).  ACCURATE = 1: the device library's tanhf.
template <int ACCURATE>
__device__ __forceinline__ float att_tanh(float x) {
  if (ACCURATE) return tanhf(x);
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);  // exp(2x) = 2^(2x*log2 e)
  return fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}

// tanh(x) given y = x * 2*log2(e) (the scale is folded into the caller's fma)
__device__ __forceinline__ float att_tanh_scaled(float y) {
  return fmaf(-2.0f, __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(y) + 1.0f), 1.0f);
}
constexpr float kTwoLog2e = 2.8853900817779268f;

// Sum over aligned groups of LANES lanes inside a DPP row; every lane gets its group's total.  log2(LANES)
// v_add_f32 with DPP operands, no LDS round trip.  lanes_sum<16> is the sum over one slot q of the MFMA layout.
template <int LANES>
__device__ __forceinline__ float lanes_sum(float v) {
  static_assert(LANES == 2 || LANES == 4 || LANES == 8 || LANES == 16, "a power-of-two part of a 16-lane row");
  v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));                   // quad_perm [1,0,3,2]
  if (LANES >= 4) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
  if (LANES >= 8) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true));  // row_half_mirror
  if (LANES >= 16) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, true)); // row_mirror
  return v;
}

// One node row as an MFMA fragment: lane group q takes floats 16m + 4q .. + 3 of row `row`, m = 0 .. D_/16 - 1, into
// a[4m .. 4m + 3].  32-bit byte offsets from the table base (the launchers guarantee N * d * 4 < 4 GiB): one scalar
// base + one VGPR offset per row instead of 64-bit address arithmetic per load.
template <int D_>
__device__ __forceinline__ void att_load_row_frag(float (&a)[D_ / 4], const float* __restrict__ ent, int32_t row, int q) {
  const char* base = reinterpret_cast<const char*>(ent);
  const uint32_t o = (uint32_t)row * (uint32_t)(D_ * 4) + (uint32_t)(q * 16);
#pragma unroll
  for (int m = 0; m < D_ / 16; ++m) {
    const float4 v = *reinterpret_cast<const float4*>(base + o + m * 64);
    a[4 * m + 0] = v.x; a[4 * m + 1] = v.y; a[4 * m + 2] = v.z; a[4 * m + 3] = v.w;
  }
}

template <int D_, int TILES>
struct AFrag {
  float t[TILES][D_ / 4], h[TILES][D_ / 4];
};

// Gather the A fragments (tail and head embedding rows) of TILES 16-edge tiles.
template <int D_, int TILES>
__device__ __forceinline__ void att_load_a(AFrag<D_, TILES>& f, const float* __restrict__ ent,
                                           const int32_t (&rs)[TILES], const int32_t (&rd)[TILES],
                                           int q) {
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const float4* ps = reinterpret_cast<const float4*>(ent + (size_t)rs[t] * D_) + q;
    const float4* pd = reinterpret_cast<const float4*>(ent + (size_t)rd[t] * D_) + q;
#pragma unroll
    for (int m = 0; m < D_ / 16; ++m) {
      const float4 a = ps[m * 4];
      const float4 b = pd[m * 4];
      f.t[t][4 * m + 0] = a.x; f.t[t][4 * m + 1] = a.y; f.t[t][4 * m + 2] = a.z; f.t[t][4 * m + 3] = a.w;
      f.h[t][4 * m + 0] = b.x; f.h[t][4 * m + 1] = b.y; f.h[t][4 * m + 2] = b.z; f.h[t][4 * m + 3] = b.w;
    }
  }
}


// What a launcher gets from an entry of kgat_att.hip: the arrays every form reads, then each form's own.
struct AttArgs {
  const char* entry;  // names the entry in its messages
  hipStream_t st;
  int n_rel;
  int64_t n_edges;
  const int32_t *rel_ptr, *perm, *src_g, *pos_g;
  const float *ent, *W_R, *rel;
  float *logits, *logits_csr;
  // one-kernel form: the grouped head nodes; workgroups of the chunk and generic kernels
  const int32_t* dst_g = nullptr;
  unsigned n_blocks = 0;
  // group forms: gid per grouped position, gptr per relation, g_node per group, the per-group scratch table
  // (split: G, n_groups x k; folded: V, n_groups x d)
  const int32_t *gid = nullptr, *gptr = nullptr, *g_node = nullptr;
  float* G_tab = nullptr;
  bool f32_products = false;           // fused / folded forms: fp32 MFMA products instead of the bf16-piece products
  // fused form
  const int32_t* rec_g = nullptr;      // packed (source node | group slot << 28) per grouped position
  const int32_t *tiles = nullptr, *rel_tptr = nullptr;  // work tiles (kgat_fold_tiles) and their range per relation
  const int32_t* part_tptr = nullptr;  // tile range per workgroup, n_parts of them (null: one workgroup per CU)
  unsigned n_parts = 0;
  float* logits_g = nullptr;           // logits in grouped order
  long long* part_clocks = nullptr;    // measurement aid: s_memrealtime at every workgroup's start and end
};

// The widths with W_r in a wavefront's registers (persistent, split, fold-head, fused kernels) and with the d = 128
// kernels that keep it in LDS beside them.
using AttWidths = WidthList<16, 32, 64>;
using AttWidths128 = WidthList<16, 32, 64, 128>;
constexpr int kAttMaxRelLds = 4096;

// The support rule of every MFMA form: one square width of the form's list, a per-relation tile prefix that fits the kernels'
// LDS table, node rows addressed with 32-bit byte offsets.
template <typename Widths>
inline bool att_shape_ok(int64_t n_nodes, int d, int k, int n_rel, Widths widths) {
  return d == k && has_width(widths, d) && n_rel > 0 && n_rel <= kAttMaxRelLds &&
         (unsigned long long)n_nodes * (unsigned long long)d * 4ull < (1ull << 32);
}

// kgat_att_persistent.hip (compiled with -amdgpu-mfma-vgpr-form: its epilogue reads the MFMA
// results from VGPRs directly); each returns KGAT_E_UNSUPPORTED for widths it does not cover.
int launch_att_persistent_any(int d, const AttArgs& a);
int launch_att_split_any(int d, const AttArgs& a);
int launch_att_fold_head_any(int d, const AttArgs& a);  // writes V (n_groups x d) into a.G_tab
int launch_att_fold_fused_any(int d, const AttArgs& a);

// Lanes that share one edge in the per-edge dot product of the folded forms (a lane holds
// d / (4 * lanes) float4 pieces of the tail row and of the group's V row).  Fewer lanes per edge
// mean fewer instructions per edge (measured at d = 64, fused form: 16 lanes 0.251 ms, 8 lanes
// 0.229, 4 lanes 0.215, 2 lanes 0.217); the stand-alone per-edge launch, which lives on loads in
// flight rather than on issue slots, is fastest with 8 (0.281 ms against 0.308 with 4).  The two
// therefore sum a dot product in different orders and agree to fp32 rounding, not bit for bit.
template <int D_>
constexpr int kFusedLanesPerEdge() { return D_ / 4 < 4 ? D_ / 4 : 4; }
template <int D_>
constexpr int kTailLanesPerEdge() { return D_ / 4 < 8 ? D_ / 4 : 8; }

}  // namespace kgat
