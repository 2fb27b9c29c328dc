// Shared by the three evaluation translation units (kgat_eval.hip: K <= 32, recall / ndcg in the merge;
// kgat_eval_topk.hip: K <= 128, ranked lists and metrics at several cut-offs; kgat_eval_rank.hip: exact ranks at any
// depth): constants, the total order, the LDS layout and the launch plan, each a function of the candidate buffer's
// size `cap`, and the host side of a sweep's launch.  The sweep's device text is kgat_eval_walk.h.  Not part of the ABI.
#pragma once
#include <functional>
#include <queue>
#include <type_traits>
#include <vector>
#include "kgat_common.h"

namespace kgat {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kEvalCap = 64;      // candidate entries per user (one per lane of the pruning wavefront)
constexpr int kEvalMaxK = 32;
// the wide sweep (kgat_eval_topk.hip): ceil(CAP / 64) entries per lane of the pruning wavefront.  156 entries are
// what four wavefronts' buffers may take of a CU's 160 KB (4 x (32 x 156 x 8 + 256) = 160,768 bytes): one per SIMD.
constexpr int kEvalTopkMaxK = 128;
constexpr int kEvalCapWide = 128, kEvalCapWidest = 156;
__host__ __device__ constexpr int eval_cap(int K) {
  return K <= kEvalMaxK ? kEvalCap : (K <= 64 ? kEvalCapWide : kEvalCapWidest);
}
constexpr int kEvalTile = 32;     // items per MFMA tile
// (item tiles in flight per wavefront: two, one in the widest register form - NT in the kernel)
constexpr float kNegInf = -__builtin_inff();
constexpr int kIdxPad = 0x7fffffff;

// A float as an unsigned integer with the same order (for atomicMax on a shared threshold) and back.
__device__ __forceinline__ unsigned ordered_bits(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// "a ranks before b": score descending, position ascending
__device__ __forceinline__ bool ranks_before(float sa, int ia, float sb, int ib) {
  return sa > sb || (sa == sb && ia < ib);
}

// Descending bitonic sort of one (score, position) entry per lane over the wavefront.
__device__ __forceinline__ void wave_sort_desc(float& s, int& i, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const float so = __shfl_xor(s, j, 64);
      const int io = __shfl_xor(i, j, 64);
      const bool lower = (lane & j) == 0;          // this lane is the lower index of its pair
      const bool desc = (lane & k) == 0;           // this block sorts descending (final k = 64: every lane)
      const bool mine_first = ranks_before(s, i, so, io);
      // the lower lane of a descending pair keeps the entry that ranks first
      const bool keep = (lower == desc) ? mine_first : !mine_first;
      s = keep ? s : so;
      i = keep ? i : io;
    }
  }
}

// position `it` in the ascending list a[lo, hi)?
__device__ __forceinline__ bool in_sorted(const int32_t* __restrict__ a, int32_t lo, int32_t hi, int32_t it) {
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    const int32_t v = a[mid];
    if (v == it) return true;
    if (v < it) lo = mid + 1; else hi = mid;
  }
  return false;
}

// tile boundaries of the grid's segments (a kernel argument): segment y sweeps tiles [b[y], b[y + 1])
constexpr int kEvalMaxLists = 66;
struct EvalBounds { int32_t b[kEvalMaxLists + 1]; };

struct EvalLds {
  // per wavefront: cand_s / cand_i [32 users][cap], kept [32]; then (LDS form only) the users' rows [FP2][64]
  static __host__ __device__ size_t per_wave_bytes(int FP2, bool rows_in_registers = false, int cap = kEvalCap) {
    return (size_t)32 * cap * 8 + 32 * 4 * 2 + (rows_in_registers ? (size_t)0 : (size_t)FP2 * 64 * 4);
  }
};

// KG > 0 (round 6): the users' rows - the B operand of every MFMA of the sweep - live in REGISTERS (KG groups of 8
// k pairs = 8 KG values per lane: 88 at the reference readout's 176 columns) instead of LDS.  The LDS form spends
// 22.5 KB per wavefront on them, so a CU holds ONE workgroup = one wavefront per SIMD, and that wavefront's candidate
// handling (vector ALU) leaves the matrix pipe idle: the sweep ran at 0.57 of the fp32-MFMA peak, the launch at 0.30.
// With the rows in registers a wavefront needs 16.6 KB, two workgroups of four fit a CU, and a second wavefront per
// SIMD issues MFMAs while the first one filters; no ds_read per MFMA either.  The arithmetic is the same fmaf chain
// in the same k order: same score bits.  KG = 0: the LDS form (any width).
// Instantiated for KG = 11 (the 64 + 64 + 32 + 16 = 176-column readout of the reference's default model), 6 and 16: a
// width in (40, 96] / (96, 176] / (176, 256] is padded with zero columns to 96 / 176 / 256 and takes the register form
// of that size (70,679 x 24,915, K = 20: 160 columns 9.1 ms in the LDS form, 5.7 padded to 176; 88 columns 6.4 vs 3.1;
// 192 columns 17.1 ms in the LDS form).  Narrower rows are cheaper in the LDS form (16 columns: 2.2 ms), wider ones do
// not fit the registers.
// KG = 22 (352 columns: the 128 + 128 + 64 + 32 readout of the d = 128 model) keeps 176 row values per lane and ONE item
// tile in flight instead of two (a single accumulator chain per wavefront; the second wavefront of the SIMD fills in).
__host__ __device__ constexpr int eval_reg_kg(int F) {
  return F <= 40 ? 0 : (F <= 96 ? 6 : (F <= 176 ? 11 : (F <= 256 ? 16 : (F <= 352 ? 22 : 0))));
}

// k pairs of a row, padded with zeros: to the register form's size where there is one, else to the unroll of the MFMA loop
static int eval_fp2(int F) { return eval_reg_kg(F) > 0 ? eval_reg_kg(F) * 8 : ((F + 1) / 2 + 7) / 8 * 8; }

constexpr size_t kEvalLdsPerCu = (size_t)160 * 1024;

// wavefronts of workgroups of nw that a CU holds with a wide buffer: what the LDS fits, one per SIMD at most (the wide
// kernels are built for that)
static int eval_wide_resident(int F, int cap, int nw) {
  const size_t wg = EvalLds::per_wave_bytes(eval_fp2(F), eval_reg_kg(F) > 0, cap) * nw;
  const int waves = (int)(kEvalLdsPerCu / wg) * nw;
  return waves > 4 ? 4 : waves;
}

static int eval_waves_per_block(int F, int cap = kEvalCap) {
  const int FP2 = eval_fp2(F);
  if (cap == kEvalCap) {
    if (eval_reg_kg(F) > 0) return 4;
    // the largest workgroup whose wavefronts' LDS (candidates + the users' rows) fits a CU
    for (int nw = 4; nw >= 1; nw >>= 1)
      if (EvalLds::per_wave_bytes(FP2) * nw <= kEvalLdsPerCu) return nw;
    return 0;
  }
  // the wide buffers: workgroups of two in the register forms (two of them fit a CU: one wavefront per SIMD), in the
  // LDS form the size that keeps most wavefronts on a CU
  if (eval_reg_kg(F) > 0) return 2;
  int best = 0, most = 0;
  for (int nw = 4; nw >= 1; nw >>= 1)
    if (eval_wide_resident(F, cap, nw) > most) { most = eval_wide_resident(F, cap, nw); best = nw; }
  return best;
}

// workgroups a CU holds at a time (the LDS is the bound in every form)
static int eval_slots_per_cu(int F, int cap = kEvalCap) {
  if (cap == kEvalCap) return eval_reg_kg(F) > 0 ? 2 : 1;
  const int nw = eval_waves_per_block(F, cap);
  return nw > 0 && eval_wide_resident(F, cap, nw) >= nw ? eval_wide_resident(F, cap, nw) / nw : 1;
}

// Launch plan.  One grid: the item tiles are split into segments so that the grid has a few workgroups per CU.
//
// Segment sizes (round 6).  A CU holds `slots` workgroups at a time and the hardware hands the grid out in order, one
// segment row (all user blocks) after the other: with equal segments the reference's shape is 2,212 workgroups on
// 512 slots - 4.3 rounds, the fifth a third full.  The plan therefore also considers rows whose LAST segments are
// shorter (the stragglers of the last round are short ones) and one or two more rows than the minimum, simulates the
// in-order hand-out of each candidate (a workgroup costs its tiles plus a fixed share for its prologue, closing prunes
// and list) and keeps the shortest.  (Worth 2 % on the chip, not the 11 % of the simulation: a CU left with one
// workgroup runs it faster.)
constexpr double kEvalFixedCost = 0.02;   // a workgroup's fixed work, in units of one user block's whole sweep
struct EvalPlanH { int nw, seg, n_lists; EvalBounds bounds; };

static double eval_makespan(int64_t blocks, int64_t slots, const double* frac, int n) {
  // in-order list scheduling on `slots` identical slots: a min-heap of the slots' finishing times
  std::priority_queue<double, std::vector<double>, std::greater<double>> h;
  for (int64_t i = 0; i < slots; ++i) h.push(0.0);
  double last = 0.0;
  for (int r = 0; r < n; ++r) {
    const double cost = frac[r] + kEvalFixedCost;
    for (int64_t x = 0; x < blocks; ++x) {
      const double t = h.top() + cost;
      h.pop();
      h.push(t);
      if (t > last) last = t;
    }
  }
  return last;
}

static EvalPlanH eval_plan(int64_t n_users, int64_t n_items, int F, int cap = kEvalCap) {
  EvalPlanH p;
  p.nw = eval_waves_per_block(F, cap);
  const int64_t n_tiles = (n_items + kEvalTile - 1) / kEvalTile;
  const int64_t rest = n_tiles;
  const int nw = p.nw > 0 ? p.nw : 1;
  const int64_t blocks = (n_users + 32 * nw - 1) / (32 * nw);
  const int64_t slots = (int64_t)device_cu_count() * eval_slots_per_cu(F, cap);   // resident workgroups (LDS bound)
  // about two rounds of resident workgroups (measured against one and four at the shapes of the reference's three
  // datasets and at 8,000 users: profiles/r06_eval_scan.txt - every row more is another prologue, warm-up and list
  // per user, one round leaves the last workgroups of an uneven grid alone on the chip)
  const int64_t want = slots * 2;
  int64_t seg = (want + blocks - 1) / (blocks > 0 ? blocks : 1);
  const int64_t max_seg = rest / 16 > 0 ? rest / 16 : 1;     // at least 16 tiles (512 items) per segment
  if (seg > max_seg) seg = max_seg;
  if (seg > 64) seg = 64;
  if (seg < 1) seg = 1;
  // candidates: seg .. seg + 2 rows, equal or with a short tail (weights 1, .., 1, 1/2, 1/4)
  double best = -1.0, best_frac[kEvalMaxLists];
  int best_n = (int)seg;
  for (int i = 0; i < best_n; ++i) best_frac[i] = 1.0 / best_n;
  if (seg > 1 && blocks <= 16 * slots) {   // (one row, or a grid of many rounds: nothing to gain)
    for (int n = (int)seg; n <= (int)seg + 2 && n <= max_seg && n <= 64; ++n)
      for (int tail = 0; tail <= 1; ++tail) {
        if (tail && n < 3) continue;
        double w[kEvalMaxLists], sum = 0.0;
        for (int i = 0; i < n; ++i) { w[i] = !tail || i < n - 2 ? 1.0 : (i == n - 2 ? 0.5 : 0.25); sum += w[i]; }
        bool ok = true;
        for (int i = 0; i < n; ++i) { w[i] /= sum; ok = ok && w[i] * rest >= 8.0; }
        if (!ok) continue;
        const double mk = eval_makespan(blocks, slots, w, n);
        if (best < 0.0 || mk < best) { best = mk; best_n = n; for (int i = 0; i < n; ++i) best_frac[i] = w[i]; }
      }
  }
  p.seg = best_n;
  p.n_lists = p.seg;
  int y = 0;
  p.bounds.b[0] = 0;
  double acc = 0.0;
  for (int i = 0; i < p.seg; ++i) {
    acc += best_frac[i];
    int64_t e = i == p.seg - 1 ? n_tiles : (int64_t)(acc * (double)rest + 0.5);
    if (e <= p.bounds.b[y]) e = p.bounds.b[y] + 1;                      // (never empty; rest >= seg)
    if (e > n_tiles - (p.seg - 1 - i)) e = n_tiles - (p.seg - 1 - i);
    p.bounds.b[++y] = (int32_t)e;
  }
  for (int i = y + 1; i <= kEvalMaxLists; ++i) p.bounds.b[i] = (int32_t)n_tiles;
  return p;
}

// ---------------------------------------------------------------------------------- launching a sweep (host)
// (the kernels address a segment's fragments with 32-bit offsets)
static int eval_check_segments(const char* who, const EvalPlanH& pl, int FP2) {
  for (int y = 0; y < pl.n_lists; ++y)
    KGAT_CHECK_ARG((int64_t)(pl.bounds.b[y + 1] - pl.bounds.b[y]) * FP2 * 256 < ((int64_t)1 << 32),
                   "%s: a segment of %d tiles is beyond 4 GB of fragments", who, pl.bounds.b[y + 1] - pl.bounds.b[y]);
  return KGAT_OK;
}

// The form of a width (kg = eval_reg_kg(F)) and a plan (nw = pl.nw) as compile-time values: returns fn(NW, KG), both
// std::integral_constants.  A register form runs workgroups of REG_NW wavefronts - what eval_waves_per_block plans: 4
// with the K <= 32 buffer and in the rank sweep, 2 with the wide buffers - the LDS form workgroups of nw.  fn is
// instantiated for these seven forms and no other, so this ladder IS the set of kernels a family builds.
template <int V> using EvalInt = std::integral_constant<int, V>;
template <int REG_NW, typename Fn>
static auto eval_with_form(int kg, int nw, Fn&& fn) {
  if (kg == 6) return fn(EvalInt<REG_NW>{}, EvalInt<6>{});
  if (kg == 11) return fn(EvalInt<REG_NW>{}, EvalInt<11>{});
  if (kg == 16) return fn(EvalInt<REG_NW>{}, EvalInt<16>{});
  if (kg == 22) return fn(EvalInt<REG_NW>{}, EvalInt<22>{});
  if (nw == 4) return fn(EvalInt<4>{}, EvalInt<0>{});
  if (nw == 2) return fn(EvalInt<2>{}, EvalInt<0>{});
  return fn(EvalInt<1>{}, EvalInt<0>{});
}

// ONE launch of a sweep kernel over (blocks of 32 pl.nw columns) x (item segments), its LDS reserved first.
template <typename Kernel, typename... Args>
static int eval_launch_sweep(const char* who, Kernel kernel, int64_t n_cols, const EvalPlanH& pl, size_t lds_per_wave,
                             hipStream_t st, Args... args) {
  const size_t lds = lds_per_wave * pl.nw;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess) {
    set_error("%s: cannot reserve %zu bytes of LDS", who, lds);
    return KGAT_E_HIP;
  }
  const unsigned gx = (unsigned)((n_cols + 32 * pl.nw - 1) / (32 * pl.nw));
  hipLaunchKernelGGL(kernel, dim3(gx, (unsigned)pl.n_lists), dim3(pl.nw * 64), lds, st, args...);
  return KGAT_OK;
}

// The workspace of the sweeps that keep lists: the segments' partial lists of every user, part_s / part_i
// [n_users][pl.n_lists][K], and the shared K-th best per user (order-preserving bits), tau_shared [n_users].
struct EvalListsWs { float* part_s; int32_t* part_i; unsigned* tau_shared; };
static size_t eval_lists_workspace_bytes(int64_t n_users, const EvalPlanH& pl, int K) {
  return 2 * align_up((size_t)n_users * pl.n_lists * K * 4, 256) + align_up((size_t)n_users * 4, 256) + 256;
}
static EvalListsWs eval_lists_carve(void* workspace, int64_t n_users, const EvalPlanH& pl, int K) {
  Carver cv(workspace);
  EvalListsWs ws;
  ws.part_s = cv.take<float>((size_t)n_users * pl.n_lists * K);
  ws.part_i = cv.take<int32_t>((size_t)n_users * pl.n_lists * K);
  ws.tau_shared = cv.take<unsigned>((size_t)n_users);
  return ws;
}

// The sweep of a family that keeps lists - `kernel`: eval_topk_kernel or eval_topk_wide_kernel at the plan's form, over
// buffers of `cap` entries - into ws.
template <typename Kernel>
static int eval_lists_sweep(const char* who, Kernel kernel, int cap, int64_t n_users, const int32_t* user_ids,
                            int64_t n_items, int F, const float* emb, int64_t emb_stride, const float* itemT,
                            const int32_t* train_ptr, const int32_t* train_items, int K, const EvalPlanH& pl,
                            const EvalListsWs& ws, hipStream_t st) {
  const int FP2 = eval_fp2(F);
  KGAT_RETURN_IF(eval_check_segments(who, pl, FP2));
  if (pl.n_lists > 1 && hipMemsetAsync(ws.tau_shared, 0, (size_t)n_users * 4, st) != hipSuccess) {
    set_error("%s: cannot clear the shared thresholds", who);
    return KGAT_E_HIP;
  }
  return eval_launch_sweep(who, kernel, n_users, pl, EvalLds::per_wave_bytes(FP2, eval_reg_kg(F) > 0, cap), st, n_users,
                           user_ids, n_items, FP2, F, pl.bounds, emb, emb_stride, itemT, train_ptr, train_items, K,
                           ws.part_s, ws.part_i, pl.n_lists > 1 ? ws.tau_shared : nullptr);
}

// kgat_eval.hip: the K <= 32 sweep over a plan made with the default buffer (kgat_eval_topk_f32 launches it too; the
// lists as three pointers: the library exports this name as it is)
int eval_sweep_launch(const char* who, int64_t n_users, const int32_t* user_ids, int64_t n_items, int F, const float* emb,
                      int64_t emb_stride, const float* itemT, const int32_t* train_ptr, const int32_t* train_items, int K,
                      const EvalPlanH& pl, float* part_s, int32_t* part_i, unsigned* tau_shared, hipStream_t st);

}  // namespace kgat
