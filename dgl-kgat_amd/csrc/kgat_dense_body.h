// The body of the dense forward kernels of kgat_dense.hip - included INSIDE each of its two entry points,
// bi_interaction_kernel (one weight: the product, the sum, the concatenation) and bi2_kernel (the two-term
// Bi-Interaction: two weights and the sign record), so that both compile the same statements while the one-weight
// kernels keep their signature and their code.  Expects in scope: the template parameters DI, DO, MODE, VEC_NORM, DEFER,
// COMB and the arguments n_rows, P, HN, W1, W2, slope, drop_threshold, keep_scale, seed, index0, h_out, signs, norm_out,
// norm_stride, ego, df (W1 and signs are read by the two-term form only).  No include guard: included twice.
  constexpr bool TRAIN = MODE == 2;
  constexpr bool BI2 = COMB == kCombBi2;
  static_assert(!DEFER || MODE == 1, "the deferred rows go with the no-grad form");
  static_assert(COMB == kCombMul || MODE >= 1, "the sum and the concatenation need H and HN apart");
  constexpr int KS = DI / 4, KT = DO / 16;
  constexpr int DIW = COMB == kCombCat ? 2 * DI : DI, KSW = (BI2 ? 2 * DI : DIW) / 4;  // W's columns, the staged k-steps
  // W2 is staged once per workgroup through LDS (coalesced 16-byte reads of the whole matrix),
  // laid out in B-fragment order so that every wave then pulls its fragments with
  // conflict-free ds_read_b32: s_w[(s*KT + c)*64 + q*16 + i] = W2[16c + i][16*(s>>2) + 4q + (s&3)]
  __shared__ float s_w[KSW * KT * kWave];
  for (int idx = threadIdx.x * 4; idx < DO * DIW; idx += 256 * 4) {
    const float4 v = *reinterpret_cast<const float4*>((BI2 ? W1 : W2) + idx);
    const int j = idx / DIW, k0 = idx % DIW;  // four consecutive k of output column j
    const int c = j >> 4, i = j & 15;
    const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = k0 + t;
      const int s = (k >> 4) * 4 + (k & 3), q = (k >> 2) & 3;
      s_w[(s * KT + c) * kWave + q * 16 + i] = vv[t];
    }
  }
  if constexpr (BI2) {  // the product's weight behind the sum's: k-steps KS .. 2 KS - 1
    for (int idx = threadIdx.x * 4; idx < DO * DI; idx += 256 * 4) {
      const float4 v = *reinterpret_cast<const float4*>(W2 + idx);
      const int j = idx / DI, k0 = idx % DI;
      const int c = j >> 4, i = j & 15;
      const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = k0 + t;
        const int s = KS + (k >> 4) * 4 + (k & 3), q = (k >> 2) & 3;
        s_w[(s * KT + c) * kWave + q * 16 + i] = vv[t];
      }
    }
  }
  __syncthreads();

  const int lane = threadIdx.x % kWave;
  const int i = lane & 15, q = lane >> 4;
  const int64_t n_waves = (int64_t)gridDim.x * (256 / kWave);
  // (the wavefront's index through readfirstlane: its tile range is then held in SGPRs and the tile loop's branches
  // are scalar - as a per-lane value the loop was compiled as divergent control flow, exec-masked block by block)
  const int64_t wv = (int64_t)blockIdx.x * (256 / kWave) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int32_t n_tiles = (n_rows + 15) >> 4;
  const int32_t t_begin = (int32_t)((int64_t)n_tiles * wv / n_waves);
  const int32_t t_end = (int32_t)((int64_t)n_tiles * (wv + 1) / n_waves);
  if (t_begin >= t_end) return;

  // W2's fragments live in registers for the whole launch - except at 128 x 128, where they would
  // need 256 VGPRs: there every MFMA takes its fragment from the LDS copy (one conflict-free
  // ds_read_b32 each)
constexpr int kBiWLdsAbove = 128;  // (A/B builds: 0 = fragments always from LDS, fewer registers, more wavefronts per SIMD)
  // (the concatenation's W is twice as large: its fragments always come from LDS - held in registers they cost it
  // occupancy against the product at every width, and spill at 128 -> 128; kernel-resource-usage)
  // (the two-term form's pair of weights is that size too: from LDS as well)
  constexpr bool W_IN_LDS = COMB == kCombCat || BI2 || KS * KT > kBiWLdsAbove;
  float wreg[W_IN_LDS ? 1 : KSW][W_IN_LDS ? 1 : KT];
  if (!W_IN_LDS) {
#pragma unroll
    for (int s = 0; s < KSW; ++s)
#pragma unroll
      for (int c = 0; c < KT; ++c) wreg[W_IN_LDS ? 0 : s][W_IN_LDS ? 0 : c] = s_w[(s * KT + c) * kWave + lane];
  }

  // MODE >= 1: the rows of H and of HN are REQUESTED here and multiplied when the tile is computed (round 4, second
  // form).  The first form multiplied here, which put the waits for both row sets - one after the other, the ego
  // copy in between - into the load step: two exposed memory round trips per tile with nothing else of the
  // wavefront in flight, and no overlap with the previous tile's matrix work whatever kBiPrefetch said (round 4's
  // A/B, NOTEBOOK.md; non-temporal loads of the rows lost theirs as well).
  constexpr bool LATE_MUL = MODE >= 1;
constexpr int kBiPrefetch = 2;
  constexpr int PF = KS * kBiPrefetch <= 64 ? kBiPrefetch : (64 / KS >= 2 ? 64 / KS : 2);  // <= 64 VGPRs of rows in flight (x 2 with HN)
  // DEFER: per stage, the offsets of the row this lane loads NEXT (requested one load step ahead), and what the load
  // step found out for the tile step: nf = followers of the row's chain of tile partials (-1: a row without in-edges,
  // 0: an ordinary row or a one-partial chain), bh = the chain's head tile
  constexpr int LPR = DI / 4;
  struct Defer { int32_t rb, re, nf, bh, slot; };
  auto row_offsets = [&](int32_t t, Defer& d) {
    int32_t ra = (t << 4) + i;
    ra = ra < n_rows ? ra : n_rows - 1;
    d.rb = df.indptr[ra];
    d.re = df.indptr[ra + 1];
  };
  auto load_a = [&](int32_t t, float (&a)[KS], float (&b)[LATE_MUL ? KS : 1], Defer& d) {
    int32_t ra = (t << 4) + i;
    ra = ra < n_rows ? ra : n_rows - 1;
    const float4* pa = reinterpret_cast<const float4*>(P + (size_t)ra * DI) + q;
#pragma unroll
    for (int m = 0; m < DI / 16; ++m) {
      const float4 v = pa[m * 4];
      a[4 * m + 0] = v.x; a[4 * m + 1] = v.y; a[4 * m + 2] = v.z; a[4 * m + 3] = v.w;
    }
    if constexpr (LATE_MUL) {
      const float4* pb = reinterpret_cast<const float4*>(HN + (size_t)ra * DI) + q;
      if constexpr (DEFER) {
        // a row the aggregation's tiles left as partials: the head partial has an HN row's layout - it is requested
        // in the row's place, the followers when the tile is computed
        const int32_t rb = d.rb - df.e0, re = d.re - df.e0;
        const int32_t te_mask = (1 << df.te_shift) - 1;
        const int32_t bh = rb >> df.te_shift, bl = (re - 1) >> df.te_shift;
        const bool empty = rb == re;
        const bool lo_al = (rb & te_mask) == 0;
        const bool partial = !empty && (bh != bl || lo_al || (re & te_mask) == 0 || d.re == df.e1);
        if (partial) pb = df.bpart + ((size_t)bh * 2 + (lo_al ? 0 : 1)) * LPR + q;
        d.nf = empty ? -1 : (partial ? bl - bh : 0);
        d.bh = bh;
        d.slot = lo_al ? 0 : 1;
      }
#pragma unroll
      for (int m = 0; m < DI / 16; ++m) {
        const float4 v = pb[m * 4];
        b[4 * m + 0] = v.x; b[4 * m + 1] = v.y; b[4 * m + 2] = v.z; b[4 * m + 3] = v.w;
      }
      if constexpr (DEFER) row_offsets(t + PF, d);  // (clamped to the last row past the end)
    }
  };
  auto tile = [&](int32_t t, float (&a)[KS], float (&b)[LATE_MUL ? KS : 1], const int32_t nf, const int32_t bh, const int32_t slot) {
    const int32_t row0 = t << 4;
    if constexpr (DEFER) {
      if (__builtin_amdgcn_ballot_w64(nf != 0) != 0ull) {  // (uniform: about a third of the 16-row tiles)
        const bool is_long = nf >= kDeferLongChain;
        if (nf < 0) {
#pragma unroll
          for (int s = 0; s < KS; ++s) b[s] = 0.f;
        } else if (nf > 0 && !is_long) {
          // acc = head partial; acc += the followers' first-row partials, in tile order (spmm_finish_kernel)
          const float4* pf = df.bpart + ((size_t)(bh + 1) * 2) * LPR + q;
          for (int32_t k = 0; k < nf; ++k, pf += 2 * LPR) {
#pragma unroll
            for (int m = 0; m < DI / 16; ++m) {
              const float4 v = pf[m * 4];
              b[4 * m + 0] += v.x; b[4 * m + 1] += v.y; b[4 * m + 2] += v.z; b[4 * m + 3] += v.w;
            }
          }
        }
        // hub rows (a chain of more than kDeferLongChain tiles): the whole wavefront sums one row, as the finish
        // launch does - lane group g = lane / LPR takes the tiles head + g, head + g + SPW, ..., a fixed shuffle
        // tree adds the groups' sums - and hands the row to its four lanes
        unsigned long long todo = __builtin_amdgcn_ballot_w64(is_long && q == 0);
        if (todo) {
          constexpr int SPW = kWave / LPR;
          const int g = lane / LPR, sl = lane % LPR;
          while (todo) {
            const int src = __ffsll((long long)todo) - 1;  // (q == 0: the lane index is the row's i)
            todo &= todo - 1;
            const int32_t bo = __shfl(bh, src, kWave);
            const int32_t bl = bo + __shfl(nf, src, kWave);
            const int so = __shfl(slot, src, kWave);
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            int32_t bb = bo + g;
            constexpr int U = 8;
            for (; bb + (U - 1) * SPW <= bl; bb += U * SPW) {
              float4 v[U];
#pragma unroll
              for (int u = 0; u < U; ++u) {
                const int32_t tt = bb + u * SPW;
                v[u] = df.bpart[((size_t)tt * 2 + ((tt == bo) ? so : 0)) * LPR + sl];
              }
#pragma unroll
              for (int u = 0; u < U; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
            }
            for (; bb <= bl; bb += SPW) {
              const float4 v = df.bpart[((size_t)bb * 2 + ((bb == bo) ? so : 0)) * LPR + sl];
              acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
#pragma unroll
            for (int off = LPR; off < kWave; off <<= 1) {
              acc.x += __shfl_xor(acc.x, off, kWave); acc.y += __shfl_xor(acc.y, off, kWave);
              acc.z += __shfl_xor(acc.z, off, kWave); acc.w += __shfl_xor(acc.w, off, kWave);
            }
            // every lane group now holds the row (lane sl: columns 4 sl .. 4 sl + 3); lane (i, q) takes 4 (4m + q)..
#pragma unroll
            for (int m = 0; m < DI / 16; ++m) {
              const float x = __shfl(acc.x, 4 * m + q, kWave), y = __shfl(acc.y, 4 * m + q, kWave);
              const float z = __shfl(acc.z, 4 * m + q, kWave), w = __shfl(acc.w, 4 * m + q, kWave);
              if (i == src) { b[4 * m + 0] = x; b[4 * m + 1] = y; b[4 * m + 2] = z; b[4 * m + 3] = w; }
            }
          }
        }
      }
    }
    if constexpr (LATE_MUL) {
      if (MODE >= 1 && ego.out != nullptr && row0 + i < n_rows) {
        float4* pe = reinterpret_cast<float4*>(ego.out + (size_t)(row0 + i) * ego.stride) + q;
#pragma unroll
        for (int m = 0; m < DI / 16; ++m) st_final4(pe + m * 4, make_float4(a[4 * m + 0], a[4 * m + 1], a[4 * m + 2], a[4 * m + 3]));
      }
      if constexpr (COMB == kCombMul) {
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] *= b[s];
      } else if constexpr (COMB == kCombSum) {
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] += b[s];
      } else if constexpr (BI2) {  // a = h + h_N, b = h * h_N: in the registers the rows came in
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const float pr = a[s] * b[s];
          a[s] += b[s];
          b[s] = pr;
        }
      }
    }
    floatx4_d acc[KT];
#pragma unroll
    for (int c = 0; c < KT; ++c) acc[c] = (floatx4_d){0.f, 0.f, 0.f, 0.f};
    floatx4_d acc2[BI2 ? KT : 1];  // the product term's pre-activations (two-term form)
    uint32_t sbits[BI2 && TRAIN ? KT : 1];
    // (the concatenation's fragments from LDS through an index the compiler cannot prove loop-invariant, so they are
    // read per tile - left to itself it hoists the reads out of the tile loop into registers, up to 512 values per lane
    // at 128 -> 128, and spills)
    int wl = lane;
    if constexpr ((COMB == kCombCat || BI2) && W_IN_LDS) asm volatile("" : "+v"(wl));
    // operands swapped (A = W2 fragment, B = the tile's rows): the accumulators hold Z^T, i.e.
    // acc[c][j] = Z[row0 + i][16c + 4q + j] - four consecutive columns per lane, so the results
    // leave as 16-byte stores (a quarter of the store instructions of the row-major result)
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int c = 0; c < KT; ++c)
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            W_IN_LDS ? s_w[(s * KT + c) * kWave + wl] : wreg[W_IN_LDS ? 0 : s][W_IN_LDS ? 0 : c], a[s], acc[c], 0, 0, 0);
    if constexpr (COMB == kCombCat) {  // the h_N half of K: W's k-steps KS .. 2 KS - 1 on the rows of HN
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int c = 0; c < KT; ++c)
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              W_IN_LDS ? s_w[((KS + s) * KT + c) * kWave + wl] : wreg[W_IN_LDS ? 0 : KS + s][W_IN_LDS ? 0 : c], b[s],
              acc[c], 0, 0, 0);
    }
    if constexpr (BI2) {  // z2 = (h * h_N) W2^T into its own accumulators
#pragma unroll
      for (int c = 0; c < KT; ++c) acc2[c] = (floatx4_d){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int c = 0; c < KT; ++c)
          acc2[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w[((KS + s) * KT + c) * kWave + wl], b[s], acc2[c], 0, 0, 0);
    }
    const int32_t row = row0 + i;
    // row norm: per 16-column tile the sum of squares over the row's four lanes (i, q = 0..3), then the tiles'
    // partials in tile order - the order of the fused aggregation + dense launch (kgat_spmm_impl.h: tile_ssq),
    // whose wavefronts each own one column tile, so the two paths give the same bits
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < KT; ++c) {
      float part = 0.f;
      uint32_t sb = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float z = acc[c][j];
        if constexpr (BI2 && TRAIN) sb |= (z > 0.f ? 1u : 0u) << (8 * j);
        z = z >= 0.f ? z : z * slope;
        if constexpr (BI2) {  // LeakyReLU per term, then the sum
          const float z2 = acc2[c][j];
          if constexpr (TRAIN) sb |= (z2 > 0.f ? 2u : 0u) << (8 * j);
          z += z2 >= 0.f ? z2 : z2 * slope;
        }
        if (TRAIN)
          z = drop_keep(seed, index0 + (uint32_t)row * (uint32_t)DO + (uint32_t)(16 * c + 4 * q + j), drop_threshold)
                  ? z * keep_scale : 0.f;
        acc[c][j] = z;
        part = j == 0 ? z * z : fmaf(z, z, part);
      }
      part += __shfl_xor(part, 16, kWave);
      part += __shfl_xor(part, 32, kWave);
      ss = c == 0 ? part : ss + part;
      if constexpr (BI2 && TRAIN) sbits[c] = sb;
    }
    const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);  // one division per row; the 4 x KT values are scaled by it
    if (row < n_rows) {
#pragma unroll
      for (int c = 0; c < KT; ++c) {
        const float z0 = acc[c][0], z1 = acc[c][1], z2 = acc[c][2], z3 = acc[c][3];
        // (the lane's four columns are four consecutive bytes of the row's sign record)
        if constexpr (BI2 && TRAIN) *reinterpret_cast<uint32_t*>(signs + (size_t)row * DO + 16 * c + 4 * q) = sbits[c];
        if (h_out) *reinterpret_cast<float4*>(h_out + (size_t)row * DO + 16 * c + 4 * q) = make_float4(z0, z1, z2, z3);
        if (norm_out) {
          float* dst = norm_out + (size_t)row * norm_stride + 16 * c + 4 * q;
          if (VEC_NORM) {
            st_final4(reinterpret_cast<float4*>(dst), make_float4(z0 * inv, z1 * inv, z2 * inv, z3 * inv));
          } else {
            dst[0] = z0 * inv; dst[1] = z1 * inv; dst[2] = z2 * inv; dst[3] = z3 * inv;
          }
        }
      }
    }
  };

  // Ring of PF stages: the rows of tile t + PF are requested once tile t is computed.  (Round 4 measured an explicit
  // two-buffer loop, load t + 1 / compute t, with unconditional load steps against it: stand-alone faster at 64 -> 64
  // (37.2 vs 38.9 us), slower at 32 -> 16 (14.8 vs 14.0); inside the step the ring wins, 0.4374 vs 0.4395 ms:
  // profiles/r04_bi_late_mul_ab.txt; that form is in the history, commit c6eba96 and before.  Round 4 had
  // also tried PF = 4, W2's fragments from LDS with 4 and 8 workgroups per CU and a 1,024-block grid:
  // profiles/r04_bi_probe.txt - the launch runs at the rate of a device copy of its bytes.)
  float a[PF][KS], b[PF][LATE_MUL ? KS : 1];
  Defer d[PF];
#pragma unroll
  for (int p = 0; p < PF; ++p) {
    d[p] = Defer{0, 0, 0, 0, 0};
    if (DEFER) row_offsets(t_begin + p, d[p]);
  }
#pragma unroll
  for (int p = 0; p < PF; ++p)
    if (t_begin + p < t_end) load_a(t_begin + p, a[p], b[p], d[p]);
  for (int32_t t = t_begin; t < t_end; t += PF) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      if (t + p < t_end) {
        // (nf / bh by value: the load step below overwrites the stage's record)
        tile(t + p, a[p], b[p], d[p].nf, d[p].bh, d[p].slot);
        if (t + p + PF < t_end) load_a(t + p + PF, a[p], b[p], d[p]);
      }
    }
  }
