  // The walk of the evaluation sweeps over a segment's item tiles: 32 columns (users, or rank slots) per wavefront
  // against item tiles of 32, one v_mfma_f32_32x32x2_f32 chain per tile in k order.  Included inside a kernel, in
  // parts (KGAT_EVAL_WALK_PART, undefined again here), by the candidate sweep of kgat_eval_sweep_body.h and by
  // eval_rank_sweep_kernel of kgat_eval_rank.hip: this ONE text is why their scores agree bit for bit.  Shared as
  // text, not as a function template and not through a callable over acc / the ring buffers: a generic lambda per step
  // sent the captured arrays to scratch, a template parameter changed the K <= 32 kernels' registers.
  //  1, the rows: REG, NT, U and breg[] / ub[] filled (the kernel fences before part 3).  The kernel has its template
  //     parameter KG (k groups of the register form; 0: the LDS form), the arguments F and FP2, lane / half,
  //     `const float* row` (the column's row of emb), `bool u_ok` (the column exists) and `float* ub` (the wavefront's
  //     [FP2][64] floats of LDS in the LDS form).
  //  2, the accumulators: acc[NT] and nan_padded_tail; the kernel has n_items.  Three parts, not two, because the
  //     ORDER of the kernel's local arrays steers the register allocation: the rank kernel declares its counters
  //     between the rows and acc, as it did when it carried its own copy of this text.
  //  3, the loop.  The kernel has itemT, the segment's tiles [t_lo, t_hi) and a callable check(int64_t t0): what to do
  //     with the finished scores acc[t] of the tiles t0 + t < t_hi (it may overwrite them).
#if KGAT_EVAL_WALK_PART == 1
  constexpr bool REG = KG > 0;
  constexpr int NT = KG > 16 ? 1 : 2;   // item tiles in flight: one where the columns' rows leave no registers for two
  constexpr int U = 8;
  typedef float floatx4 __attribute__((ext_vector_type(4)));
  // B fragments: lane (column ul, half) holds the row's elements k = 2s + half
  float breg[REG ? KG * 8 : 1];
  if constexpr (REG) {
#pragma unroll
    for (int s = 0; s < KG * 8; ++s) {
      const int k = 2 * s + half;
      breg[s] = (u_ok && k < F) ? row[k < F ? k : 0] : 0.f;
    }
  } else {
    for (int s = 0; s < FP2; ++s) {
      const int k = 2 * s + half;
      ub[s * 64 + lane] = (u_ok && k < F) ? row[k] : 0.f;
    }
  }
#elif KGAT_EVAL_WALK_PART == 2
  floatx16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  // acc[t][r]: column ul, item position 32 (t0 + t) + (r & 3) + 8 (r >> 2) + 4 half
  // The padded end of the last tile (a wave-uniform branch) becomes NaN, which compares false with everything: both
  // checks open with it.  ib: the lane's first item position of `tile`, the tile of acc[t].
  auto nan_padded_tail = [&](int t, int64_t tile, int ib) {
    if ((tile + 1) * kEvalTile > n_items) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (ib + (r & 3) + 8 * (r >> 2) >= n_items) acc[t][r] = __builtin_nanf("");
    }
  };
#elif KGAT_EVAL_WALK_PART == 3
  // A fragments: one coalesced 16-byte load per lane per FOUR MFMAs (itemT's layout, eval_items_kmajor_kernel).  The
  // sweep is a flat sequence of steps (tile group, group of U k pairs); a step's loads are issued while the previous
  // step's MFMAs run.
  if constexpr (REG) {
    // Two tile groups per loop iteration = 4 KG half steps (tile group, k group, half of the k group; 44 at KG = 11) with
    // compile-time k groups - the register index of the B operand.  A half step is two 16-byte loads per lane (four k
    // pairs of both tiles) and eight MFMAs; its loads are issued THREE half steps ahead into a ring of four buffers (the
    // registers of two whole-step buffers: one step ahead was 1,024 MFMA cycles, about the L2's latency under this
    // load; three half steps are 1,536).  4 KG is a multiple of 4: the ring position of a half step is a compile-time
    // constant.  A group past the end re-reads the clamped last tile and is skipped.
    // (written out, not a loop: `#pragma unroll` over the steps was declined by the optimiser, and a generic lambda
    //  per step - the index as an integral_constant - sent every captured array to scratch)
    static_assert(KG <= 22 && U == 8, "the step list below is written out for up to 2 x 22 steps of 2 halves");
    const floatx16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float h0[4][NT], h1[4][NT], h2[4][NT], h3[4][NT];
    const size_t seg_bytes = (size_t)(t_hi - t_lo) * KG * 2048;
    const __amdgpu_buffer_rsrc_t seg_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(itemT) + (size_t)t_lo * KG * 512, 0, (int)(unsigned)seg_bytes, 0x00020000);
    auto issue_half = [&](float (&a)[4][NT], int64_t tg, int g, int q) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int64_t tt = tg + t < t_hi ? tg + t : t_hi - 1;   // (a clamped duplicate tile is ignored below)
        // (a buffer load: the segment's fragments as a resource, the wave-uniform offset in a scalar register, the lane's
        //  16 bytes the only vector operand - as a global load every address was two 64-bit vector adds, six vector
        //  instructions per half step; the host checks that a segment's fragments stay below 4 GB: eval_check_segments)
        const unsigned soff = (unsigned)(((tt - t_lo) * KG + g) * 2 + q) * 1024u;
        const floatx4 v = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(seg_rsrc, lane * 16, (int)soff, 0));
#pragma unroll
        for (int c = 0; c < 4; ++c) a[c][t] = v[c];
      }
    };
    issue_half(h0, t_lo, 0, 0);
    issue_half(h1, t_lo, 0, 1);
    issue_half(h2, t_lo, 1, 0);
#define KGAT_EVAL_HALF(J, CUR, NXT)                                                                       \
    if constexpr (J < 4 * KG) {                                                                           \
      constexpr int j = J, g = (j / 2) % KG, q = j % 2, jn = j + 3, gn = (jn / 2) % KG, qn = jn % 2;      \
      const int64_t tt = t0 + (j / 2 / KG) * NT, tn = t0 + (jn / 2 / KG) * NT;                            \
      issue_half(NXT, tn, gn, qn);                                                                        \
      /* the loads go out HERE, ahead of this half step's MFMAs: left to itself the scheduler sinks them between */ \
      /* the MFMAs and waits for each a few instructions after issuing it                                         */ \
      __builtin_amdgcn_sched_barrier(0);                                                                  \
      if (tt < t_hi) { /* wave-uniform */                                                                 \
        _Pragma("unroll") for (int c = 0; c < 4; ++c)                                                     \
          _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                  \
            /* (a tile group's first MFMA adds to the constant 0: no clearing of 32 registers per group) */ \
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(CUR[c][t], breg[g * U + 4 * q + c],             \
                                                          (g == 0 && q == 0 && c == 0) ? zero16 : acc[t], 0, 0, 0); \
        __builtin_amdgcn_sched_barrier(0);                                                                \
        if (g == KG - 1 && q == 1) check(tt);                                                             \
      }                                                                                                   \
    }
#define KGAT_EVAL_HALF4(J) KGAT_EVAL_HALF(J, h0, h3) KGAT_EVAL_HALF(J + 1, h1, h0) KGAT_EVAL_HALF(J + 2, h2, h1) KGAT_EVAL_HALF(J + 3, h3, h2)
    for (int64_t t0 = t_lo; t0 < t_hi; t0 += 2 * NT) {
      KGAT_EVAL_HALF4(0) KGAT_EVAL_HALF4(4) KGAT_EVAL_HALF4(8) KGAT_EVAL_HALF4(12) KGAT_EVAL_HALF4(16) KGAT_EVAL_HALF4(20)
      KGAT_EVAL_HALF4(24) KGAT_EVAL_HALF4(28) KGAT_EVAL_HALF4(32) KGAT_EVAL_HALF4(36) KGAT_EVAL_HALF4(40) KGAT_EVAL_HALF4(44)
      KGAT_EVAL_HALF4(48) KGAT_EVAL_HALF4(52) KGAT_EVAL_HALF4(56) KGAT_EVAL_HALF4(60) KGAT_EVAL_HALF4(64) KGAT_EVAL_HALF4(68)
      KGAT_EVAL_HALF4(72) KGAT_EVAL_HALF4(76) KGAT_EVAL_HALF4(80) KGAT_EVAL_HALF4(84)   // (beyond 4 KG: compiled out)
    }
#undef KGAT_EVAL_HALF4
#undef KGAT_EVAL_HALF
  } else {
    // (two register buffers, the loop unrolled by two so that no buffer is copied)
    const floatx4* a_base = reinterpret_cast<const floatx4*>(itemT) + lane;
    const int KGR = FP2 / U;                                     // k groups per tile group (FP2 is a multiple of U)
    struct Pos { int64_t t0; int g; };
    auto advance = [&](Pos& p) { if (++p.g == KGR) { p.g = 0; p.t0 += NT; } };
    auto issue = [&](float (&a)[U][NT], const Pos& p) {
      // (unconditional: a load under a branch makes the compiler's counted vmcnt waits conservative - it then waited
      // for the NEXT step's loads before this step's MFMAs; past the end the clamped tile is loaded again, unused)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int64_t tt = p.t0 + t < t_hi ? p.t0 + t : t_hi - 1;   // (a clamped duplicate tile is ignored below)
        const floatx4* ap = a_base + ((size_t)tt * KGR + p.g) * (U / 4) * 64;
#pragma unroll
        for (int q = 0; q < U / 4; ++q) {
          const floatx4 v = ap[q * 64];
#pragma unroll
          for (int c = 0; c < 4; ++c) a[4 * q + c][t] = v[c];
        }
      }
    };
    auto compute = [&](const float (&a)[U][NT], const Pos& p) {
      if (p.t0 >= t_hi) return;
      float b[U];
#pragma unroll
      for (int u = 0; u < U; ++u) b[u] = ub[(p.g * U + u) * 64 + lane];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][t], b[u], acc[t], 0, 0, 0);
      if (p.g == KGR - 1) {
        check(p.t0);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;   // (here, behind the check's branch: not a select per step)
      }
    };
    float a0[U][NT], a1[U][NT];
    Pos p0{t_lo, 0}, p1{t_lo, 0};
    advance(p1);
    issue(a0, p0);
    while (p0.t0 < t_hi) {
      issue(a1, p1);
      compute(a0, p0);
      advance(p0); advance(p0);
      issue(a0, p0);
      compute(a1, p1);
      advance(p1); advance(p1);
    }
  }
#else
#error "KGAT_EVAL_WALK_PART must be 1 (the rows), 2 (the accumulators) or 3 (the loop)"
#endif
#undef KGAT_EVAL_WALK_PART
