// All-pairs evaluation of RippleNet (ripple_models.RippleNet) for gfx950: per user the K best unseen items and their
// scores, nothing of size users x items written.  DESIGN.md 32.
//
// A ripple set depends on the user only, so scoring one user against every item is attention with the ITEMS as the
// queries and the M memories of a hop as keys (key_i = R_{r_i} ent[h_i]) and values (ent[t_i]).
//
//  1. ripple_eval_keys_kernel: the key table [user of the call][hop][slot][d], one fmaf chain per element.
//  2. ripple_eval_sweep_kernel: ONE USER per workgroup.  Its operands - keys and tail rows of every hop and W - are laid
//     out in LDS once as MFMA A fragments; the four wavefronts then split the item tiles of the segment.  Every product
//     of a tile has the item as the accumulator's column (= the lane):
//         logits  S = Key (M x d)   . v (d x 32 items)        softmax over the slots: in-lane + one half-wave exchange
//         answer  o = Tail^T (d x M) . p (M x 32 items)
//         update  v' = W (d x d)    . (v + o)                 (the *_transform modes)
//     and each product takes the previous accumulator REGISTERS as its B operand: the k pair (2 s, 2 s + 1) of a
//     v_mfma_f32_32x32x2_f32 is (lower half-wave, upper half-wave), so the accumulator's rows are numbered such that
//     register s of half m holds row 2 s + m (rip_row) - which is also how kgat_eval_items_kmajor_f32 hands out the item
//     rows.  No LDS round trip and no lane movement between the products.  The 32 scores of a tile lie across the lanes
//     and go through the candidate buffer of kgat_topk_wave.h.
//  3. nfm_eval_merge_kernel (kgat_topk_wave.h): one wavefront per user merges the lists of the segments' wavefronts.
#include "kgat_topk_wave.h"

namespace kgat {

constexpr int kRipMaxM = 64, kRipMaxHop = 2, kRipMaxSeg = 16;   // (kRipMaxSeg x kNfmNW lists per user)

typedef float floatx4r __attribute__((ext_vector_type(4)));

// Row r of a 32-row block (the MFMA's A-operand row = the accumulator's row) holds index rip_index(r) of the block:
// accumulator register s (s < 16) of half-wave m is row (s & 3) + 8 (s >> 2) + 4 m and is to hold index 2 s + m.
__host__ __device__ constexpr int rip_row(int index) { return ((index >> 1) & 3) + 8 * (index >> 3) + 4 * (index & 1); }

struct RipArgs {
  int64_t n_users, n_nodes, n_items, n_tiles;
  int FQ, M, H, mode, all_hops, K;
  const int32_t* user_ids;
  const float* itemT;
  const float* keys;
  const float* ent;
  const int32_t* mem_t;
  const float* W;
  const int32_t* train_ptr;
  const int32_t* train_items;
  float* list_s;
  int32_t* list_i;
};

// key[uc, k, i, a] = sum_c R_{r_i}[a, c] ent[h_i][c]: thread (pair, a) walks the slots of its (user, hop) pair and keeps
// row a of the current relation's matrix in registers across a run of equal relations.
template <int D>
__global__ __launch_bounds__(256) void ripple_eval_keys_kernel(int64_t n_pairs, const int32_t* __restrict__ user_ids,
                                                               int H, int M, int n_rel, int64_t n_nodes, int64_t n_users,
                                                               const float* __restrict__ ent,
                                                               const float* __restrict__ rel,
                                                               const int32_t* __restrict__ mem_h,
                                                               const int32_t* __restrict__ mem_r,
                                                               float* __restrict__ keys) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t pair = g / D;
  const int a = (int)(g % D);
  if (pair >= n_pairs) return;
  const int64_t uid = user_ids[pair / H];
  const int k = (int)(pair % H);
  float* out = keys + (size_t)pair * M * D + a;
  if (uid < 0 || uid >= n_users) {             // nothing is read for such a user; the sweep lists nothing for it
    for (int i = 0; i < M; ++i) out[(size_t)i * D] = 0.f;
    return;
  }
  const int32_t* mh = mem_h + ((size_t)uid * H + k) * M;
  const int32_t* mr = mem_r + ((size_t)uid * H + k) * M;
  floatx4r R[D / 4];
  int cur = -1;
  for (int i = 0; i < M; ++i) {
    const int r = mr[i], h = mh[i];
    if (r < 0 || r >= n_rel || h < 0 || h >= n_nodes) {
      out[(size_t)i * D] = __builtin_nanf("");
      continue;
    }
    if (r != cur) {
      const floatx4r* row = reinterpret_cast<const floatx4r*>(rel + ((size_t)r * D + a) * D);
#pragma unroll
      for (int c = 0; c < D / 4; ++c) R[c] = row[c];
      cur = r;
    }
    const floatx4r* hr = reinterpret_cast<const floatx4r*>(ent + (size_t)h * D);
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < D / 4; ++c) {
      const floatx4r x = hr[c];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = fmaf(R[c][e], x[e], acc);
    }
    out[(size_t)i * D] = acc;
  }
}

// acc[b] += A_b . x for NB blocks of 32 output rows: the A fragments [block][NQ][64 lanes][4 k pairs] in LDS (`a`
// points at this lane's float4 of block 0, quad 0), x the B operand in accumulator registers: k pair s is register
// s & 15 of x[s >> 4].
template <int NB, int NQ, int NX>
__device__ __forceinline__ void rip_mma(floatx16 (&acc)[NB], const floatx4r* __restrict__ a, const floatx16 (&x)[NX]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    floatx4r a4[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) a4[b] = a[(b * NQ + q) * 64];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int b = 0; b < NB; ++b)
        acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[b][c], x[(4 * q + c) >> 4][(4 * q + c) & 15], acc[b], 0, 0, 0);
  }
}

// D: the embedding width, MB: blocks of 32 slots.  LDS (dynamic): keys [H][MB][D / 8][64][4], tails [H][DB][4 MB][64][4],
// W [DB][D / 8][64][4] (the transform modes only), then the four wavefronts' candidate buffers.
template <int D, int MB>
__global__ __launch_bounds__(kNfmNW * 64) void ripple_eval_sweep_kernel(const RipArgs a) {
  constexpr int S = D / 2, SQ = S / 4;           // k pairs over the columns, quads of them
  constexpr int DB = (D + 31) / 32;              // blocks of 32 columns as accumulator rows
  constexpr int MP = 32 * MB, MS = MP / 2, MQ = MS / 4;
  constexpr int RD = D < 32 ? D / 2 : 16;        // accumulator registers of a column block that hold columns
  extern __shared__ __attribute__((aligned(16))) float rip_lds[];
  const int H = a.H, M = a.M, K = a.K;
  float* keyF = rip_lds;
  float* tailF = keyF + H * MB * S * 64;
  float* wF = tailF + H * DB * MS * 64;
  float* cand_s = wF + (a.mode >= 2 ? DB * S * 64 : 0);
  int32_t* cand_i = reinterpret_cast<int32_t*>(cand_s + kNfmNW * kNfmCap);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ul = lane & 31, half = lane >> 5;
  const int64_t u = blockIdx.x;                  // position in user_ids
  const int seg = blockIdx.y, n_seg = gridDim.y;
  const size_t list = ((size_t)u * n_seg * kNfmNW + (size_t)seg * kNfmNW + w) * K;
  const int64_t uid = a.user_ids[u];
  if (uid < 0 || uid >= a.n_users) {             // (the whole workgroup leaves: before the barrier)
    for (int x = lane; x < K; x += 64) { a.list_s[list + x] = kNegInf; a.list_i[list + x] = kIdxPad; }
    return;
  }
  // the user's operands, read in source order, scattered to where the MFMAs read them: element (row index j, k index
  // c) of a block goes to quad (c >> 1) >> 2, lane rip_row(j) + 32 (c & 1), slot (c >> 1) & 3
  for (int x = tid; x < H * MP * D; x += kNfmNW * 64) {
    const int c = x % D, slot = x / D % MP, k = x / (D * MP);
    const float val = slot < M ? a.keys[(((size_t)u * H + k) * M + slot) * D + c] : 0.f;
    const int s = c >> 1;
    keyF[(((k * MB + (slot >> 5)) * SQ + (s >> 2)) * 64 + rip_row(slot & 31) + 32 * (c & 1)) * 4 + (s & 3)] = val;
  }
  for (int x = tid; x < H * MP * DB * 32; x += kNfmNW * 64) {
    const int f = x % (DB * 32), slot = x / (DB * 32) % MP, k = x / (DB * 32 * MP);
    float val = 0.f;
    if (slot < M && f < D) {
      const int t = a.mem_t[((size_t)uid * H + k) * M + slot];
      val = t >= 0 && t < a.n_nodes ? a.ent[(size_t)t * D + f] : __builtin_nanf("");
    }
    const int s = slot >> 1;
    tailF[(((k * DB + (f >> 5)) * MQ + (s >> 2)) * 64 + rip_row(f & 31) + 32 * (slot & 1)) * 4 + (s & 3)] = val;
  }
  if (a.mode >= 2)
    for (int x = tid; x < DB * 32 * D; x += kNfmNW * 64) {
      const int c = x % D, j = x / D;
      const int s = c >> 1;
      wF[((((j >> 5)) * SQ + (s >> 2)) * 64 + rip_row(j & 31) + 32 * (c & 1)) * 4 + (s & 3)] =
          j < D ? a.W[(size_t)j * D + c] : 0.f;
    }
  __syncthreads();                               // (the only workgroup barrier)

  const int64_t t_lo = a.n_tiles * seg / n_seg, t_hi = a.n_tiles * (seg + 1) / n_seg;
  float* cs = cand_s + w * kNfmCap;
  int32_t* ci = cand_i + w * kNfmCap;
  const int32_t tr_lo = a.train_ptr[u], tr_hi = a.train_ptr[u + 1];
  const floatx4r* frag = reinterpret_cast<const floatx4r*>(a.itemT) + lane;   // + (tile FQ + quad) 64
  const floatx4r* kf = reinterpret_cast<const floatx4r*>(keyF) + lane;
  const floatx4r* tf = reinterpret_cast<const floatx4r*>(tailF) + lane;
  const floatx4r* wf = reinterpret_cast<const floatx4r*>(wF) + lane;

  int cnt = 0, kept = 0;
  float tau = kNegInf;   // the K-th best key of this wavefront's tiles so far: -inf while fewer than K are held
  int64_t t = t_lo + w;
  floatx4r nxt[SQ];
  if (t < t_hi) {
#pragma unroll
    for (int q = 0; q < SQ; ++q) nxt[q] = frag[((size_t)t * a.FQ + q) * 64];
  }
  for (; t < t_hi; t += kNfmNW) {
    // v_0: register s of half m is column 2 s + m of the item - the fragment as it is
    floatx16 v[DB], osum[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        v[db][r] = r < RD ? nxt[(16 * db + r) >> 2][r & 3] : 0.f;
        osum[db][r] = 0.f;
      }
    {
      const int64_t tn = t + kNfmNW < t_hi ? t + kNfmNW : t;   // (past the end this tile again, unused)
#pragma unroll
      for (int q = 0; q < SQ; ++q) nxt[q] = frag[((size_t)tn * a.FQ + q) * 64];
    }
#pragma unroll 1
    for (int k = 0; k < H; ++k) {
      floatx16 p[MB];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) p[mb][r] = 0.f;
      rip_mma<MB, SQ, DB>(p, kf + (size_t)k * MB * SQ * 64, v);
      // softmax over the slots of the lane's item: register r of block mb is slot 32 mb + 2 r + half
      float mx = kNegInf;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (32 * mb + 2 * r + half < M) mx = fmaxf(mx, p[mb][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      float part = 0.f;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float e = 32 * mb + 2 * r + half < M ? __expf(p[mb][r] - mx) : 0.f;   // a padded slot: exactly 0
          p[mb][r] = e;
          part += e;
        }
      const float other = __shfl_xor(part, 32, 64);
      const float inv = 1.0f / (half ? other + part : part + other);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) p[mb][r] *= inv;
      floatx16 o[DB];
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
      rip_mma<DB, MQ, MB>(o, tf + (size_t)k * DB * MQ * 64, p);
      if (a.all_hops || k == H - 1) {
#pragma unroll
        for (int db = 0; db < DB; ++db) osum[db] += o[db];
      }
      if (a.mode == 0) {
#pragma unroll
        for (int db = 0; db < DB; ++db) v[db] = o[db];
      } else if (a.mode == 1) {
#pragma unroll
        for (int db = 0; db < DB; ++db) v[db] += o[db];
      } else {
        if (a.mode == 3) {
#pragma unroll
          for (int db = 0; db < DB; ++db) o[db] = v[db] + o[db];
        }
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) v[db][r] = 0.f;
        rip_mma<DB, SQ, DB>(v, wf, o);
      }
    }
    // y = <v_H, sum of the answers>: a lane adds its columns in ascending (block, register) order from 0, one fma each;
    // the two half-waves' sums are added (lower half + upper half: the same bits on both lanes)
    float part = 0.f;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int r = 0; r < RD; ++r) part = fmaf(v[db][r], osum[db][r], part);
    const float other = __shfl_xor(part, 32, 64);
    const float key = half ? other + part : part + other;
    const int64_t it = t * kEvalTile + ul;
    // (the padded end of the last tile and the upper half-wave's copies are never candidates)
    const bool pass = half == 0 && it < a.n_items && key >= tau;
    nfm_append(cs, ci, lane, K, pass, key, (int32_t)it, a.train_items, tr_lo, tr_hi, cnt, kept, tau);
  }
  // this wavefront's list: at most K entries, in no order, padded with (-inf, pad)
  nfm_prune(cs, ci, lane, K, a.train_items, tr_lo, tr_hi, cnt, kept, tau);
  for (int x = lane; x < K; x += 64) {
    a.list_s[list + x] = x < cnt ? cs[x] : kNegInf;
    a.list_i[list + x] = x < cnt ? ci[x] : kIdxPad;
  }
}

using RipWidths = WidthList<16, 32, 64>;

// item segments of a launch: about two rounds of two resident workgroups per CU, at least eight tiles per wavefront (a
// workgroup first lays the user's operands out in LDS, about the work of a tile or two)
static int rip_segments(int64_t n_users, int64_t n_tiles) {
  const int64_t want = (int64_t)device_cu_count() * 4;
  int64_t seg = (want + n_users - 1) / (n_users > 0 ? n_users : 1);
  const int64_t most = n_tiles / (8 * kNfmNW) > 0 ? n_tiles / (8 * kNfmNW) : 1;
  if (seg > most) seg = most;
  if (seg > kRipMaxSeg) seg = kRipMaxSeg;
  return seg < 1 ? 1 : (int)seg;
}

static size_t rip_lds_bytes(int d, int M, int H, int mode) {
  const int MP = (M + 31) / 32 * 32, DP = (d + 31) / 32 * 32;
  return ((size_t)H * MP * d + (size_t)H * MP * DP + (mode >= 2 ? (size_t)DP * d : 0) + 2 * kNfmNW * kNfmCap) * 4;
}

struct RipScratch { float* list_s; int32_t* list_i; size_t bytes; };
static RipScratch rip_carve(void* scratch, int64_t n_users, int64_t n_items, int K) {
  const int64_t n_tiles = (n_items + kEvalTile - 1) / kEvalTile;
  const size_t lists = (size_t)n_users * rip_segments(n_users, n_tiles) * kNfmNW * K;
  Carver cv(scratch);
  RipScratch s;
  s.list_s = cv.take<float>(lists);
  s.list_i = cv.take<int32_t>(lists);
  s.bytes = cv.off;
  return s;
}

template <int D, int MB>
static int rip_launch_sweep(dim3 grid, size_t lds, hipStream_t st, const RipArgs& args) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(ripple_eval_sweep_kernel<D, MB>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    set_error("eval_ripple_topk: cannot reserve %zu bytes of LDS", lds);
    return KGAT_E_HIP;
  }
  hipLaunchKernelGGL((ripple_eval_sweep_kernel<D, MB>), grid, dim3(kNfmNW * 64), lds, st, args);
  return KGAT_OK;
}

}  // namespace kgat

using namespace kgat;

extern "C" {

int kgat_eval_ripple_supported(int d, int n_memory, int n_hop, int mode, int K) {
  return has_width(RipWidths{}, d) && n_memory >= 1 && n_memory <= kRipMaxM && n_hop >= 1 && n_hop <= kRipMaxHop &&
         mode >= 0 && mode <= 3 && K >= 1 && K <= kNfmMaxK;
}

int kgat_eval_ripple_keys_f32(int64_t n_call, const int32_t* user_ids, int d, int n_memory, int n_hop, int n_rel,
                              int64_t n_nodes, int64_t n_users, const float* ent, const float* relation_emb,
                              const int32_t* mem_h, const int32_t* mem_r, float* keys, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_call >= 0 && n_rel >= 1 && n_nodes >= 1 && n_nodes < ((int64_t)1 << 31) && n_users >= 1 &&
                     n_users < ((int64_t)1 << 31),
                 "eval_ripple_keys: bad sizes (n_call = %lld, n_rel = %d, n_nodes = %lld, n_users = %lld)",
                 (long long)n_call, n_rel, (long long)n_nodes, (long long)n_users);
  if (!kgat_eval_ripple_supported(d, n_memory, n_hop, 0, 1)) {
    set_error("eval_ripple_keys: d = %d (16, 32, 64), n_memory = %d (1..%d) or n_hop = %d (1..%d) not supported", d,
              n_memory, kRipMaxM, n_hop, kRipMaxHop);
    return KGAT_E_UNSUPPORTED;
  }
  KGAT_CHECK_ARG(n_call * n_hop * d < ((int64_t)1 << 31) * 256, "eval_ripple_keys: too many users in one call (%lld)",
                 (long long)n_call);
  KGAT_CHECK_ARG(user_ids && ent && relation_emb && mem_h && mem_r && keys, "eval_ripple_keys: null pointer");
  KGAT_CHECK_ARG(aligned16(ent) && aligned16(relation_emb) && aligned16(keys),
                 "eval_ripple_keys: ent, relation_emb and keys must be 16-byte aligned");
  if (n_call == 0) return KGAT_OK;
  const int64_t n_pairs = n_call * n_hop;
  const unsigned grid = (unsigned)((n_pairs * d + 255) / 256);
  const int rc = dispatch_width(RipWidths{}, d, [&](auto D) {
    hipLaunchKernelGGL((ripple_eval_keys_kernel<D()>), dim3(grid), dim3(256), 0, as_stream(stream), n_pairs, user_ids,
                       n_hop, n_memory, n_rel, n_nodes, n_users, ent, relation_emb, mem_h, mem_r, keys);
    return KGAT_OK;
  });
  if (rc != KGAT_OK) return rc;
  KGAT_CHECK_LAUNCH("eval_ripple_keys");
  return KGAT_OK;
}

size_t kgat_eval_ripple_scratch_bytes(int64_t n_call, int64_t n_items, int d, int n_memory, int n_hop, int K) {
  if (n_call <= 0 || n_items <= 0 || !kgat_eval_ripple_supported(d, n_memory, n_hop, 0, K)) return 256;
  return rip_carve(nullptr, n_call, n_items, K).bytes;
}

int kgat_eval_ripple_topk_f32(int64_t n_call, const int32_t* user_ids, int64_t n_items, int d, int n_memory, int n_hop,
                              int mode, int all_hops, int64_t n_nodes, int64_t n_users, const float* itemT,
                              const float* keys, const float* ent, const int32_t* mem_t, const float* W,
                              const int32_t* train_ptr, const int32_t* train_items, int K, void* scratch,
                              size_t scratch_bytes, int32_t* topk_items, float* topk_scores, kgat_stream_t stream) {
  KGAT_CHECK_ARG(n_call >= 0 && n_call < ((int64_t)1 << 31) && n_items >= 1 &&
                     n_items < ((int64_t)1 << 31) - kEvalTile && n_nodes >= 1 && n_nodes < ((int64_t)1 << 31) &&
                     n_users >= 1 && n_users < ((int64_t)1 << 31),
                 "eval_ripple_topk: bad sizes (n_call = %lld, n_items = %lld, n_nodes = %lld, n_users = %lld)",
                 (long long)n_call, (long long)n_items, (long long)n_nodes, (long long)n_users);
  if (!kgat_eval_ripple_supported(d, n_memory, n_hop, mode, K)) {
    set_error("eval_ripple_topk: d = %d (16, 32, 64), n_memory = %d (1..%d), n_hop = %d (1..%d), mode = %d (0..3) or "
              "K = %d (1..%d) not supported", d, n_memory, kRipMaxM, n_hop, kRipMaxHop, mode, K, kNfmMaxK);
    return KGAT_E_UNSUPPORTED;
  }
  KGAT_CHECK_ARG(user_ids && itemT && keys && ent && mem_t && train_ptr && scratch && topk_items && (W || mode < 2),
                 "eval_ripple_topk: null pointer");
  KGAT_CHECK_ARG(aligned16(itemT) && aligned16(keys) && aligned16(ent) && aligned16(scratch),
                 "eval_ripple_topk: itemT, keys, ent and scratch must be 16-byte aligned");
  if (scratch_bytes < kgat_eval_ripple_scratch_bytes(n_call, n_items, d, n_memory, n_hop, K)) {
    set_error("eval_ripple_topk: scratch too small (%zu bytes, %zu needed)", scratch_bytes,
              kgat_eval_ripple_scratch_bytes(n_call, n_items, d, n_memory, n_hop, K));
    return KGAT_E_WORKSPACE;
  }
  if (n_call == 0) return KGAT_OK;
  const int64_t n_tiles = (n_items + kEvalTile - 1) / kEvalTile;
  const int n_seg = rip_segments(n_call, n_tiles);
  const RipScratch ws = rip_carve(scratch, n_call, n_items, K);
  hipStream_t st = as_stream(stream);
  RipArgs args;
  args.n_users = n_users;
  args.n_nodes = n_nodes;
  args.n_items = n_items;
  args.n_tiles = n_tiles;
  args.FQ = eval_fp2(d) / 4;
  args.M = n_memory;
  args.H = n_hop;
  args.mode = mode;
  args.all_hops = all_hops != 0;
  args.K = K;
  args.user_ids = user_ids;
  args.itemT = itemT;
  args.keys = keys;
  args.ent = ent;
  args.mem_t = mem_t;
  args.W = W;
  args.train_ptr = train_ptr;
  args.train_items = train_items;
  args.list_s = ws.list_s;
  args.list_i = ws.list_i;
  const dim3 grid((unsigned)n_call, (unsigned)n_seg);
  const size_t lds = rip_lds_bytes(d, n_memory, n_hop, mode);
  const int rc = dispatch_width(RipWidths{}, d, [&](auto D) {
    return n_memory <= 32 ? rip_launch_sweep<D(), 1>(grid, lds, st, args) : rip_launch_sweep<D(), 2>(grid, lds, st, args);
  });
  if (rc != KGAT_OK) return rc;
  KGAT_CHECK_LAUNCH("eval_ripple_sweep");
  hipLaunchKernelGGL(nfm_eval_merge_kernel, dim3((unsigned)((n_call + kNfmNW - 1) / kNfmNW)), dim3(kNfmNW * 64), 0, st,
                     n_call, n_seg * kNfmNW, K, (const float*)ws.list_s, (const int32_t*)ws.list_i,
                     (const float*)nullptr, topk_items, topk_scores);
  KGAT_CHECK_LAUNCH("eval_ripple_merge");
  return KGAT_OK;
}

}  // extern "C"
