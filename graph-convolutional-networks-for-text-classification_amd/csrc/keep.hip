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
// word).  The last workgroup to arrive at `arrivals` stores the new state (arrive_last,
// gcnk_common.h).
//
// Work is cut into chunks of GCNK_KEEP_CHUNK elements by tensor_chunks.h's table.  The copy
// moves 32-bit words, never floats: NaN payloads, -0.0 and denormals arrive as they left.
//
// What differs from the Adam step's layout was measured (settled choices): the
// arrivals are one returning atomic per workgroup on one word, about 12 ns each in a row,
// so R8's 730 chunks of 2,048 cost 10.7 us a launch whether it copied or not.  A chunk is
// 8,192 elements here and a workgroup 1,024 threads (two 16-B pieces per thread, as there):
// 183 arrivals.  A chunk's loads are issued only once the decision is known, so a launch
// that does not copy costs its three words per workgroup and no other traffic; dst is
// stored nontemporally (it is not read again before a restore).
#include "gcnk_common.h"
#include "tensor_chunks.h"

namespace gcnk {
namespace {

constexpr int kChunk = GCNK_KEEP_CHUNK;
constexpr int kThreads = 1024;
constexpr int kPieces = kChunk / (4 * kThreads);   // 16-B pieces per thread
constexpr int kMaxTensors = GCNK_KEEP_MAX_TENSORS;

struct KeepArgs {
  gcnk_keep_tensor t[kMaxTensors];
  chunks::Table<kMaxTensors> tab;
  int32_t hold;                     // GCNK_KEEP_HOLD_STATE
};

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

  // this workgroup's tensor, selected here (tensor_chunks.h: a shared helper doing it cost scratch, or this launch time)
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.t[0].src);
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.t[0].dst);
  int64_t numel = a.t[0].numel;
  int32_t first = 0, head = a.tab.head[0];
#pragma unroll
  for (int i = 1; i < kMaxTensors; ++i)
    if (blk >= a.tab.first[i]) {
      src = reinterpret_cast<const uint32_t*>(a.t[i].src);
      dst = reinterpret_cast<uint32_t*>(a.t[i].dst);
      numel = a.t[i].numel;
      first = a.tab.first[i];
      head = a.tab.head[i];
    }
  // (without work, a launch of empty tensors only, the state is still updated)
  const chunks::Span<kChunk> s(blk - first, head, blk < a.tab.first[kMaxTensors], numel);
  const u32x4a* s4 = reinterpret_cast<const u32x4a*>(src + s.e0);
  u32x4a* d4 = reinterpret_cast<u32x4a*>(dst + s.e0);

  if (tid == 0) { s_word[0] = epoch; s_word[1] = counter; s_word[2] = seen; }
  __syncthreads();
  epoch = s_word[0];
  const bool copy = epoch > s_word[2] && s_word[1] == 0;   // fresh, and the tail's two "checkpoint" branches
  if (tid == 0 && !a.hold && arrive_last(&state->arrivals)) {
    if (copy) {
      state->best = epoch;
      state->copies += 1;
    }
    __hip_atomic_store(&state->arrivals, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&state->seen, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!copy || !s.work) return;

  if (s.head < 0) {   // buffers at different offsets from a 16-B boundary: scalar
    for (int64_t e = s.e0 + tid; e < s.e1; e += kThreads) dst[e] = src[e];
    return;
  }
  u32x4a v[kPieces];   // every load of the chunk in flight before its first store
#pragma unroll
  for (int it = 0; it < kPieces; ++it)
    if (tid + kThreads * it < s.n4) v[it] = s4[tid + kThreads * it];
#pragma unroll
  for (int it = 0; it < kPieces; ++it)
    if (tid + kThreads * it < s.n4) store16_nt(d4 + tid + kThreads * it, v[it]);
  const int64_t e = s.edge(tid);
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
  int64_t nchunks = 0;
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
    a.t[i] = x;
    if (!chunks::append<kChunk>(a.tab, i, x.numel, chunks::head_of({x.src, x.dst}), nchunks)) {
      set_error("%s: more than 2^31 chunks in one call", who);
      return GCNK_EARG;
    }
  }
  a.hold = (flags & GCNK_KEEP_HOLD_STATE) ? 1 : 0;
  if (nchunks == 0 && a.hold) return GCNK_OK;
  hipLaunchKernelGGL(keep_kernel, dim3((unsigned)(nchunks > 0 ? nchunks : 1)), dim3(kThreads), 0, (hipStream_t)stream, a,
                     epoch_state, state);
  return launch_check("keep_kernel");
}
