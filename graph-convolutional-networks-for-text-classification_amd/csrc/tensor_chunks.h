// Up to MAXT contiguous fp32 tensors cut into chunks of CHUNK elements, one workgroup per
// chunk (adam.hip, keep.hip); a prefix table in the kernel's arguments maps a workgroup to
// (tensor, chunk).  A tensor whose buffers all sit at the same offset from a 16-B boundary
// has a scalar head of up to 3 elements in its chunk 0 (lanes 0..2) and 16-B pieces from
// there on, each chunk's ragged tail scalar again (lanes 32..34, another wave than the
// head's); a tensor whose buffers disagree is all scalar (head -1).  A tensor of `head`
// elements or fewer still has its one chunk; an empty one has none.
// Plain C++17 for a host compiler (tensor_chunks_check.cpp), Span also device code.
#pragma once

#include <stdint.h>
#include <initializer_list>

#ifdef __HIPCC__
#define GCNK_CHUNKS_FN __host__ __device__ __forceinline__
#else
#define GCNK_CHUNKS_FN inline
#endif

namespace gcnk {
namespace chunks {

template <int MAXT>
struct Table {
  int32_t first[MAXT + 1];   // first[i]: the first workgroup of tensor i; first[nt ..] = all chunks
  int32_t head[MAXT];        // scalar elements in front of the 16-B aligned body; -1: all scalar
};

// head of a tensor: its buffers all at the same offset from 16 B, that offset a multiple of 4
inline int32_t head_of(std::initializer_list<const void*> bufs) {
  const uintptr_t off = reinterpret_cast<uintptr_t>(*bufs.begin()) & 15u;
  for (const void* b : bufs)
    if ((reinterpret_cast<uintptr_t>(b) & 15u) != off) return -1;
  return off % 4 == 0 ? (int32_t)(((16 - off) & 15u) / 4) : -1;
}

// tensor i (numel >= 0; tensors in order) behind the `chunks` counted so far, and the closing
// fill first[i + 1 ..] = all chunks, which stands behind the last tensor; false past 2^31 chunks
template <int CHUNK, int MAXT>
inline bool append(Table<MAXT>& tab, int i, int64_t numel, int32_t head, int64_t& chunks) {
  tab.first[i] = (int32_t)chunks;
  tab.head[i] = head;
  const int64_t body = head < 0 ? numel : (numel > head ? numel - head : 0);
  chunks += numel > 0 ? (body + CHUNK - 1) / CHUNK + (body == 0 ? 1 : 0) : 0;
  if (chunks > INT32_MAX) return false;
  for (int j = i + 1; j <= MAXT; ++j) tab.first[j] = (int32_t)chunks;
  return true;
}

// The span of chunk `chunk` = blk - first[i] of the tensor i that workgroup blk works on, the
// last with first[i] <= blk; work = blk < first[MAXT].  Each kernel selects i's entries and
// its own pointers in one unrolled loop, before its barrier: a helper picking the pointers
// copied the whole argument block to scratch, and one selecting first and head apart from
// them was sunk behind keep_kernel's decision, onto the path in front of its loads.
template <int CHUNK>
struct Span {
  int64_t numel, e0, e1;          // elements [e0, e1), e0 16-B aligned in every buffer unless head < 0
  int32_t chunk, head, len, n4;   // len = e1 - e0 (0 without work), n4 16-B pieces of it
  bool work;                      // false: the one workgroup of a launch of empty tensors only

  GCNK_CHUNKS_FN Span(int32_t chunk_, int32_t head_, bool work_, int64_t numel_)
      : numel(numel_), chunk(chunk_), head(head_), work(work_) {
    e0 = (int64_t)(head < 0 ? 0 : head) + (int64_t)chunk * CHUNK;
    e1 = e0 + (int64_t)CHUNK < numel ? e0 + (int64_t)CHUNK : numel;
    len = work && e1 > e0 ? (int32_t)(e1 - e0) : 0;
    n4 = head < 0 ? 0 : len / 4;
  }

  // the element lane tid moves beside the 16-B pieces (head >= 0): the scalar head in front of
  // chunk 0's aligned body, or the chunk's ragged tail; -1: none
  GCNK_CHUNKS_FN int64_t edge(int tid) const {
    if (chunk == 0 && tid < head && tid < numel) return tid;
    if (tid >= 32 && tid - 32 < len - 4 * n4) return e0 + 4 * (int64_t)n4 + (tid - 32);
    return -1;
  }
};

}  // namespace chunks
}  // namespace gcnk
