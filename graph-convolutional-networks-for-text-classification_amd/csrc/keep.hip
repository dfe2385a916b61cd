// "Keep the parameters of the best epoch" in one launch behind the epoch tail
// (utils.py:216-262 EarlyStopping.save_checkpoint, which the reference calls -- commented
// out -- at utils.py:244 and utils.py:254, the two places where the validation loss
// improved): up to 8 contiguous fp32 tensors are copied src -> dst when the tail that just
// ran recorded an improving epoch, and not a byte of dst is written otherwise.  Nothing is
// decided on the host.  The contract -- the decision, the state words -- is in
// include/gcnk.h.
//
// The decision is read from three words that earlier launches on the stream wrote (the
// tail's `epoch` and `counter`, this kernel's own `seen`), so it is uniform over the
// launch: one lane reads them and they reach the workgroup through LDS (adam_kernel's step
// word).  The last workgroup to arrive at `arrivals` knows every other has read the three
// words and only then stores the new state.
//
// Work is cut like the Adam step's: chunks of GCNK_KEEP_CHUNK elements found through a
// prefix table in the kernel's arguments; a tensor whose src and dst sit at the same offset
// from a 16-B boundary has a scalar head of up to 3 elements in its chunk 0 and 16-B
// accesses from there on (a chunk's ragged tail is scalar again); one whose buffers disagree
// is all scalar.  The copy moves 32-bit words, never floats: NaN payloads, -0.0 and
// denormals arrive as they left.
//
// What differs from the Adam step's layout was measured (settled choices): the
// arrivals are one returning atomic per workgroup on one word, about 12 ns each in a row,
// so R8's 730 chunks of 2,048 cost 10.7 us a launch whether it copied or not.  A chunk is
// 8,192 elements here and a workgroup 1,024 threads (two 16-B pieces per thread, as there):
// 183 arrivals.  A chunk's loads are issued only once the decision is known, so a launch
// that does not copy costs its three words per workgroup and no other traffic; dst is
// stored nontemporally (it is not read again before a restore).
#include "gcnk_common.h"

namespace gcnk {
namespace {

constexpr int kChunk = GCNK_KEEP_CHUNK;
constexpr int kThreads = 1024;
constexpr int kPieces = kChunk / (4 * kThreads);   // 16-B pieces per thread
constexpr int kMaxTensors = GCNK_KEEP_MAX_TENSORS;

struct KeepArgs {
  gcnk_keep_tensor t[kMaxTensors];
  int32_t first[kMaxTensors + 1];   // first[i]: the first workgroup of tensor i; first[nt ..] = all chunks
  int32_t head[kMaxTensors];        // scalar elements in front of the 16-B aligned body; -1: all scalar
  int32_t hold;                     // GCNK_KEEP_HOLD_STATE
};

typedef uint32_t u4a __attribute__((ext_vector_type(4), aligned(16)));

__device__ __forceinline__ void store16(u4a* p, const u4a& v) { __builtin_nontemporal_store(v, p); }

static_assert(kChunk == kPieces * 4 * kThreads && kPieces >= 1, "a workgroup holds a chunk as whole 16-B pieces per thread");

__global__ void __launch_bounds__(kThreads) keep_kernel(const KeepArgs a, const gcnk_epoch_state* __restrict__ es,
                                                   gcnk_keep_state* state) {
  __shared__ int32_t s_word[3];   // epoch, counter, seen
  const int tid = threadIdx.x;
  const int32_t blk = blockIdx.x;
  int32_t epoch = 0, counter = 0, seen = 0;
  if (tid == 0) {
    epoch = __hip_atomic_load(&es->epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    counter = __hip_atomic_load(&es->counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    seen = __hip_atomic_load(&state->seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }

  // (tensor, chunk) of this workgroup: selected without indexing the argument block dynamically
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.t[0].src);
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.t[0].dst);
  int64_t numel = a.t[0].numel;
  int32_t first = 0, head = a.head[0];
#pragma unroll
  for (int i = 1; i < kMaxTensors; ++i)
    if (blk >= a.first[i]) {
      src = reinterpret_cast<const uint32_t*>(a.t[i].src);
      dst = reinterpret_cast<uint32_t*>(a.t[i].dst);
      numel = a.t[i].numel;
      first = a.first[i];
      head = a.head[i];
    }
  const bool work = blk < a.first[kMaxTensors];   // (a launch of empty tensors only updates the state)
  const int32_t chunk = blk - first;

  const int64_t e0 = (int64_t)(head < 0 ? 0 : head) + (int64_t)chunk * kChunk;   // 16-B aligned in both buffers
  const int64_t e1 = min(e0 + (int64_t)kChunk, numel);
  const int32_t len = work && e1 > e0 ? (int32_t)(e1 - e0) : 0;
  const int32_t n4 = head < 0 ? 0 : len / 4;
  const u4a* s4 = reinterpret_cast<const u4a*>(src + e0);
  u4a* d4 = reinterpret_cast<u4a*>(dst + e0);

  if (tid == 0) { s_word[0] = epoch; s_word[1] = counter; s_word[2] = seen; }
  __syncthreads();
  epoch = s_word[0];
  const bool copy = epoch > s_word[2] && s_word[1] == 0;   // fresh, and the tail's two "checkpoint" branches
  if (tid == 0 && !a.hold) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the three words have been read before this workgroup is counted in
    const int32_t arrived = __hip_atomic_fetch_add(&state->arrivals, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived == (int32_t)gridDim.x - 1) {
      if (copy) {
        state->best = epoch;
        state->copies += 1;
      }
      __hip_atomic_store(&state->arrivals, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&state->seen, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (!copy || !work) return;

  if (head < 0) {   // buffers at different offsets from a 16-B boundary: scalar
    for (int64_t e = e0 + tid; e < e1; e += kThreads) dst[e] = src[e];
    return;
  }
  u4a v[kPieces];   // every load of the chunk in flight before its first store
#pragma unroll
  for (int it = 0; it < kPieces; ++it)
    if (tid + kThreads * it < n4) v[it] = s4[tid + kThreads * it];
#pragma unroll
  for (int it = 0; it < kPieces; ++it)
    if (tid + kThreads * it < n4) store16(d4 + tid + kThreads * it, v[it]);
  // the scalar head in front of chunk 0's aligned body, and the chunk's ragged tail
  int64_t e = -1;
  if (chunk == 0 && tid < head && tid < numel) e = tid;
  else if (tid >= 32 && tid - 32 < len - 4 * n4) e = e0 + 4 * (int64_t)n4 + (tid - 32);
  if (e >= 0) dst[e] = src[e];
}

}  // namespace
}  // namespace gcnk

using namespace gcnk;

extern "C" int gcnk_keep_best_f32(const gcnk_keep_tensor* t, int32_t ntensors, const gcnk_epoch_state* epoch_state,
                                  gcnk_keep_state* state, int32_t flags, void* stream) {
  const char* who = "gcnk_keep_best_f32";
  if (ntensors < 0 || ntensors > kMaxTensors || (flags & ~GCNK_KEEP_HOLD_STATE)) {
    set_error("%s: bad argument (ntensors=%d, at most %d per call; flags=%d)", who, ntensors, kMaxTensors, flags);
    return GCNK_EARG;
  }
  if (ntensors == 0) return GCNK_OK;
  if (!t || !epoch_state || !state) {
    set_error("%s: null tensor table, epoch state or state", who);
    return GCNK_EARG;
  }
  if ((reinterpret_cast<uintptr_t>(state) & 3u) || (reinterpret_cast<uintptr_t>(epoch_state) & 3u)) {
    set_error("%s: state and epoch state must be 4-byte aligned", who);
    return GCNK_EARG;
  }
  KeepArgs a = {};
  int64_t chunks = 0;
  for (int i = 0; i < ntensors; ++i) {
    const gcnk_keep_tensor& x = t[i];
    if (x.numel < 0 || (x.numel > 0 && (!x.src || !x.dst))) {
      set_error("%s: tensor %d: null buffer or numel < 0 (numel=%lld)", who, i, (long long)x.numel);
      return GCNK_EARG;
    }
    if (x.numel > (int64_t)(INT64_MAX / 8)) {
      set_error("%s: tensor %d: numel=%lld is out of range", who, i, (long long)x.numel);
      return GCNK_EARG;
    }
    // a src that a dst of this launch overlaps would be read while, or after, it is written
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(x.src), s1 = s0 + 4 * (uintptr_t)x.numel;
    for (int j = 0; j < ntensors; ++j) {
      const uintptr_t d0 = reinterpret_cast<uintptr_t>(t[j].dst);
      const uintptr_t d1 = d0 + 4 * (uintptr_t)(t[j].numel > 0 ? t[j].numel : 0);
      if (x.numel > 0 && t[j].numel > 0 && s0 < d1 && d0 < s1) {
        set_error("%s: tensor %d's src overlaps tensor %d's dst", who, i, j);
        return GCNK_EARG;
      }
    }
    const uintptr_t off = reinterpret_cast<uintptr_t>(x.src) & 15u;
    const bool same = (reinterpret_cast<uintptr_t>(x.dst) & 15u) == off && off % 4 == 0;
    a.t[i] = x;
    a.first[i] = (int32_t)chunks;
    a.head[i] = same ? (int32_t)(((16 - off) & 15u) / 4) : -1;
    const int64_t body = same ? (x.numel > a.head[i] ? x.numel - a.head[i] : 0) : x.numel;
    chunks += x.numel > 0 ? (body + kChunk - 1) / kChunk + (body == 0 ? 1 : 0) : 0;
    if (chunks > INT32_MAX) {
      set_error("%s: more than 2^31 chunks in one call", who);
      return GCNK_EARG;
    }
  }
  for (int i = ntensors; i <= kMaxTensors; ++i) a.first[i] = (int32_t)chunks;
  a.hold = (flags & GCNK_KEEP_HOLD_STATE) ? 1 : 0;
  if (chunks == 0 && a.hold) return GCNK_OK;
  hipLaunchKernelGGL(keep_kernel, dim3((unsigned)(chunks > 0 ? chunks : 1)), dim3(kThreads), 0, (hipStream_t)stream, a,
                     epoch_state, state);
  return launch_check("keep_kernel");
}
