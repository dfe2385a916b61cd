// The tail of a training epoch in one launch (trainer.py:378-398 TopicGCNTrainer.val on
// the validation set, trainer.py:372-376 the history row and the early-stopping decision,
// utils.py:216-255 EarlyStopping), with nothing decided on the host.
//
// Written with the library's separate kernels an epoch ends in a memset, class_stats_kernel,
// ce_forward_kernel and ce_reduce_kernel, a device->host copy of their 3 P + 2 numbers and
// a Python EarlyStopping object: one stream drain per epoch.  Here one dense pass over the
// M rows computes, per scored row, the loss terms exactly as ce_forward_kernel does (the
// arithmetic is ce_row.h's, shared with loss.hip) and the predicted class exactly as
// class_stats_kernel does; the class counts go into the epoch's history row with integer
// atomics (exact), the float64 loss partials to the workspace.  The last workgroup to
// arrive sums the partials in ce_reduce_kernel's order, runs the early-stopping state
// machine in float64 and writes the row's two losses and the state.  Once `stopped` is
// set, a launch writes nothing: epochs queued past the stop are no-ops, and `stopped` is
// the gate gcnk_adam_gated_f32 reads.
//
// Between workgroups there is one hand-off and no wait (arrive_last, gcnk_common.h): a
// workgroup's partial is stored agent-coherently by the lane that then counts it in; the
// last to arrive reads the partials with agent-coherent loads behind a workgroup barrier
// that lane has joined.  The state's epoch and stopped words are read by every workgroup at
// entry, by that same lane, and written only by the last arriver.
#include "ce_row.h"

namespace gcnk {
namespace {

using namespace ce;

// "first maximum; a NaN wins and stays" (class_stats_kernel's scan) as an order on
// (value, column): a NaN before any number, the larger number first, the smaller column
// among equals -- the scan's result is this order's first element
__device__ __forceinline__ bool pred_before(float av, int32_t ai, float bv, int32_t bi) {
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return an && (!bn || ai < bi);
  return av > bv || (av == bv && ai < bi);
}

template <int LPR, bool VEC>
__global__ void __launch_bounds__(256)
epoch_tail_kernel(const float* __restrict__ logits, int64_t ld, int32_t M, int32_t P,
                  const int64_t* __restrict__ target, const int32_t* __restrict__ counts, int64_t n,
                  const float* __restrict__ train_loss, gcnk_epoch_state* state,
                  int32_t* __restrict__ history, int32_t max_epoch, int32_t patience, double delta,
                  double* part) {
  constexpr int RPB = 256 / LPR;   // rows per workgroup
  constexpr int STEP = 4 * LPR;    // columns per pass
  __shared__ double s_w[256];      // the rows' weighted losses; in the last arriver, then the 256 runs
  __shared__ int32_t s_cnt[3 * kMaxClasses + 1];   // tp | fp | fn | correct of this workgroup's rows
  __shared__ int32_t s_word[3];    // epoch, stopped, "this workgroup arrived last"
  const int tid = threadIdx.x;
  const int g = tid / LPR, lg = tid % LPR;
  int32_t e = 0, stopped = 0;
  if (tid == 0) {   // in flight while the rows are read
    e = __hip_atomic_load(&state->epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    stopped = __hip_atomic_load(&state->stopped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  for (int i = tid; i < 3 * P + 1; i += 256) s_cnt[i] = 0;

  const int64_t r = (int64_t)blockIdx.x * RPB + g;
  int32_t cnt = 0;
  if (r < M) cnt = counts ? counts[r] : 1;
  const bool scored = cnt > 0;          // uniform over the lane group
  const float* z = logits + (scored ? r : 0) * ld;
  float v[4], mx, s;
  row_max_sum<LPR, VEC>(z, lg, P, scored, v, mx, s);

  // the predicted class: each lane's columns in ascending order, then the lane group
  float bv = v[0];
  int32_t bi = 4 * lg;
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (pred_before(v[j], 4 * lg + j, bv, bi)) { bv = v[j]; bi = 4 * lg + j; }
  if (LPR == 64 && scored)
    for (int32_t c = 4 * lg + STEP; c < P; c += STEP) {
      float u[4];
      load4<VEC>(z, c, P, -INFINITY, u);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (pred_before(u[j], c + j, bv, bi)) { bv = u[j]; bi = c + j; }
    }
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int32_t oi = __shfl_xor(bi, off, 64);
    if (pred_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }

  int64_t t = -1;
  if (lg == 0) {
    double w = 0.0;
    if (scored) {
      t = target[r];
      w = row_weighted_loss(z, P, t, cnt, row_lse(mx, s));
    }
    s_w[g] = w;
  }
  if (tid == 0) { s_word[0] = e; s_word[1] = stopped; }
  block_tree<RPB>(s_w);   // (its first barrier also publishes s_word and the zeroed s_cnt)
  e = s_word[0];
  // stopped: nothing at all is written.  (A state whose epoch is outside [0, max_epoch) names no history row.)
  if (s_word[1] != 0 || e < 0 || e >= max_epoch) return;

  if (lg == 0 && scored) {
    if (bi == t) {
      atomicAdd(&s_cnt[bi], cnt);                    // tp
      atomicAdd(&s_cnt[3 * P], cnt);                 // correct
    } else {
      atomicAdd(&s_cnt[P + bi], cnt);                // fp of the predicted class
      if (t >= 0 && t < P) atomicAdd(&s_cnt[2 * P + (int32_t)t], cnt);   // fn of the true class
    }
  }
  if (tid == 0) {
    __hip_atomic_store(part + blockIdx.x, s_w[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_word[2] = arrive_last(&state->arrivals);
  }
  __syncthreads();
  int32_t* row = history + (int64_t)e * (3 * (int64_t)P + 3);
  for (int j = tid; j < 3 * P + 1; j += 256)
    if (s_cnt[j]) atomicAdd(&row[2 + j], s_cnt[j]);
  if (!s_word[2]) return;

  // the last arriver: the partials in ce_reduce_kernel's order
  const double run = partial_run((int32_t)gridDim.x, [&](int32_t b) {
    return __hip_atomic_load(part + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  });
  s_w[tid] = run;   // (s_w[0] was read before the barrier above)
  __syncthreads();
  if (tid != 0) return;
  const float val_loss = mean_of_runs(s_w, n);

  // utils.py:238-255 in float64, with its comparisons
  const double score = -(double)val_loss;
  double best = state->best;
  int32_t counter = state->counter, reason = 0;
  if (e == 0) {
    best = score;
  } else if (score < best + delta) {
    counter += 1;
    if (counter >= patience) reason = GCNK_EPOCH_STOP_PATIENCE;
  } else {
    best = score;
    counter = 0;
  }
  if (!reason && e + 1 == max_epoch) reason = GCNK_EPOCH_STOP_MAX_EPOCH;

  reinterpret_cast<float*>(row)[0] = train_loss ? *train_loss : NAN;
  reinterpret_cast<float*>(row)[1] = val_loss;
  state->best = best;
  state->counter = counter;
  if (reason) state->stop_epoch = e;
  __hip_atomic_store(&state->arrivals, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&state->stopped, reason, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&state->epoch, e + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

inline int32_t tail_blocks(int32_t M, int32_t P) {
  const int32_t b = blocks(M, P);
  return b > 0 ? b : 1;   // M == 0 still runs the state machine (on the NaN loss of an empty set)
}

template <bool VEC, typename... A>
void launch_tail(int lpr, dim3 grid, hipStream_t s, A... a) {
#define GCNK_TAIL(L)                                                                         \
  case L:                                                                                    \
    hipLaunchKernelGGL((epoch_tail_kernel<L, VEC>), grid, dim3(256), 0, s, a...);            \
    break;
  switch (lpr) {
    GCNK_TAIL(1) GCNK_TAIL(2) GCNK_TAIL(4) GCNK_TAIL(8) GCNK_TAIL(16) GCNK_TAIL(32) GCNK_TAIL(64)
  }
#undef GCNK_TAIL
}

}  // namespace
}  // namespace gcnk

using namespace gcnk;

extern "C" int64_t gcnk_epoch_tail_workspace_bytes(int32_t M, int32_t P) {
  if (M < 0 || P < 1 || P > kMaxClasses) {
    set_error("gcnk_epoch_tail_workspace_bytes: bad argument (M=%d P=%d)", M, P);
    return GCNK_EARG;
  }
  return (int64_t)tail_blocks(M, P) * 8;
}

extern "C" int gcnk_epoch_tail_f32(const float* logits, int64_t ld, int32_t M, int32_t P, const int64_t* target,
                                   const int32_t* counts, int64_t n, const float* train_loss,
                                   gcnk_epoch_state* state, void* history, int32_t max_epoch, int32_t patience,
                                   double delta, void* workspace, int64_t workspace_bytes, void* stream) {
  if (M < 0 || P < 1 || P > kMaxClasses || ld < P || n < 0 || max_epoch < 1 || patience < 0 || !(delta == delta)) {
    set_error("gcnk_epoch_tail_f32: bad argument (M=%d P=%d ld=%lld n=%lld max_epoch=%d patience=%d delta=%g; "
              "1 <= P <= %d, ld >= P, max_epoch >= 1, patience >= 0)", M, P, (long long)ld, (long long)n, max_epoch,
              patience, delta, kMaxClasses);
    return GCNK_EARG;
  }
  if (!state || !history || (M > 0 && (!logits || !target))) {
    set_error("gcnk_epoch_tail_f32: null state, history, logits or target");
    return GCNK_EARG;
  }
  if ((reinterpret_cast<uintptr_t>(state) & 7u) || (reinterpret_cast<uintptr_t>(history) & 3u)) {
    set_error("gcnk_epoch_tail_f32: state must be 8-byte aligned, history 4-byte aligned");
    return GCNK_EARG;
  }
  const int32_t nblk = tail_blocks(M, P);
  if (!workspace || workspace_bytes < (int64_t)nblk * 8 || (reinterpret_cast<uintptr_t>(workspace) & 7u)) {
    set_error("gcnk_epoch_tail_f32: workspace of %lld bytes at an 8-byte aligned address needed (got %lld)",
              (long long)nblk * 8, (long long)workspace_bytes);
    return GCNK_EARG;
  }
  hipStream_t s = (hipStream_t)stream;
  int32_t* hist = static_cast<int32_t*>(history);
  double* part = static_cast<double*>(workspace);
  const int lpr = lanes_per_row(P);
  if (aligned16(logits) && ld % 4 == 0 && P % 4 == 0)
    launch_tail<true>(lpr, dim3((unsigned)nblk), s, logits, ld, M, P, target, counts, n, train_loss, state, hist,
                      max_epoch, patience, delta, part);
  else
    launch_tail<false>(lpr, dim3((unsigned)nblk), s, logits, ld, M, P, target, counts, n, train_loss, state, hist,
                       max_epoch, patience, delta, part);
  return launch_check("epoch_tail_kernel");
}
