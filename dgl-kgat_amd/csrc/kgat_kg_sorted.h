// The per-batch block that kgat_transr_presort_f32 leaves for an iteration of a KG phase, and the limits that go with
// it: shared by the TransR iteration (kgat_transr.hip) and the TransE one (kgat_transe.hip), which reads the same block.
// Not part of the ABI.
#pragma once
#include "kgat_common.h"

namespace kgat {

constexpr int kTrChunk = 64;      // samples per partial W-gradient block / per partial relation-gradient row
constexpr int kTrSmallSort = 8192;
constexpr int kTrMaxRel = 4096;   // relations (chunk table built by one workgroup, 4 keys per thread)
constexpr int kTrSlotBits = 14;   // row_slot word = call tag << 14 | (first sorted position of the row's run + 1); 3 * batch <= 8192 < 2^14

// the most chunks a batch's chunk table can hold: one per started kTrChunk samples of every relation
inline size_t transr_max_chunks(int64_t batch, int n_rel) {
  return (size_t)(batch > 0 ? batch : 1) / kTrChunk + (size_t)(n_rel > 0 ? n_rel : 0) + 1;
}

// per-batch block of the presort's output (offsets in bytes, 256-byte aligned)
struct TrSortedLayout {
  size_t order, seg, chunk_ptr, chunks, sorted_ids, row_order, inv_pos, run_len, bytes;
};
inline TrSortedLayout transr_sorted_layout(int64_t batch, int n_rel) {
  const size_t b = (size_t)(batch > 0 ? batch : 1);
  const size_t n_part = transr_max_chunks(batch, n_rel);
  TrSortedLayout l;
  size_t w = 0;
  l.order = w; w += align_up(b * 4, 256);
  l.seg = w; w += align_up(((size_t)n_rel + 2) * 4, 256);
  l.chunk_ptr = w; w += align_up(((size_t)n_rel + 2) * 4, 256);
  l.chunks = w; w += align_up(n_part * 8, 256);
  l.sorted_ids = w; w += align_up(3 * b * 4, 256);
  l.row_order = w; w += align_up(3 * b * 4, 256);
  l.inv_pos = w; w += align_up(3 * b * 4, 256);
  l.run_len = w; w += align_up(3 * b * 4, 256);
  l.bytes = w;
  return l;
}

// the pieces of one block as typed pointers: const for the iterations that read it, writable for the presort
template <typename I, typename I2>
struct KgSortedT {
  I *order, *seg, *chunk_ptr;
  I2* chunks;
  I *sorted_ids, *row_order, *inv_pos, *run_len;
};
using KgSorted = KgSortedT<const int32_t, const int2>;
using KgSortedOut = KgSortedT<int32_t, int2>;

template <typename I, typename I2, typename Byte>
__host__ __device__ inline KgSortedT<I, I2> kg_sorted_at(Byte* blk, const TrSortedLayout& lay) {
  KgSortedT<I, I2> s;
  s.order = reinterpret_cast<I*>(blk + lay.order);
  s.seg = reinterpret_cast<I*>(blk + lay.seg);
  s.chunk_ptr = reinterpret_cast<I*>(blk + lay.chunk_ptr);
  s.chunks = reinterpret_cast<I2*>(blk + lay.chunks);
  s.sorted_ids = reinterpret_cast<I*>(blk + lay.sorted_ids);
  s.row_order = reinterpret_cast<I*>(blk + lay.row_order);
  s.inv_pos = reinterpret_cast<I*>(blk + lay.inv_pos);
  s.run_len = reinterpret_cast<I*>(blk + lay.run_len);
  return s;
}
inline KgSorted kg_sorted(const void* block, int64_t batch, int n_rel) {
  return kg_sorted_at<const int32_t, const int2>(static_cast<const unsigned char*>(block), transr_sorted_layout(batch, n_rel));
}

}  // namespace kgat
