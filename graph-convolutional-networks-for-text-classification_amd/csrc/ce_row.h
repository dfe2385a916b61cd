// The row arithmetic of the mean cross-entropy, shared by its own kernels (loss.hip) and
// by the epoch tail that fuses the validation loss (epoch.hip): one statement of how a row
// is laid over its lane group, how lse_r and counts[r] * l_r are formed, how a workgroup's
// rows meet and how the workgroups' partials are summed, so the two agree bit for bit.
//
// A row is owned by one lane group of LPR lanes (the smallest power of two covering
// ceil(P / 4) four-column pieces, at most 64); wider rows (P > 256) loop in passes of 256
// columns.  Row sums meet in a shuffle tree of fixed shape; the loss is summed in float64:
// a fixed tree over a workgroup's rows, then the workgroups' partials in index order.
#pragma once
#include "gcnk_common.h"

#include <cmath>

namespace gcnk {
namespace ce {

constexpr int kMaxClasses = 1024;   // gcnk_class_stats's limit

// four consecutive columns c .. c + 3 of row z; columns >= P read as `fill`
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ z, int32_t c, int32_t P, float fill, float (&v)[4]) {
  if constexpr (VEC) {   // P % 4 == 0, 16-B aligned rows
    if (c < P) {
      const float4 t = *reinterpret_cast<const float4*>(z + c);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
      v[0] = v[1] = v[2] = v[3] = fill;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = c + j < P ? z[c + j] : fill;
  }
}

template <int LPR>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The row's maximum and sum of exp(z - max) over its lane group: lane lg holds columns
// 4 lg .. 4 lg + 3 of every pass (its first piece is left in v, padded with -inf past P).
// Every lane takes part in the shuffles; an unscored group computes on zeros and is dropped
// by the caller.
template <int LPR, bool VEC>
__device__ __forceinline__ void row_max_sum(const float* __restrict__ z, int lg, int32_t P, bool scored, float (&v)[4],
                                            float& mx, float& s) {
  constexpr int STEP = 4 * LPR;    // columns per pass
  const float ninf = -INFINITY;
  if (scored) load4<VEC>(z, 4 * lg, P, ninf, v); else v[0] = v[1] = v[2] = v[3] = 0.f;
  mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
  if (LPR == 64 && scored)
    for (int32_t c = 4 * lg + STEP; c < P; c += STEP) {
      float u[4];
      load4<VEC>(z, c, P, ninf, u);
      mx = fmaxf(mx, fmaxf(fmaxf(u[0], u[1]), fmaxf(u[2], u[3])));
    }
  mx = group_max<LPR>(mx);
  s = (expf(v[0] - mx) + expf(v[1] - mx)) + (expf(v[2] - mx) + expf(v[3] - mx));
  if (LPR == 64 && scored)
    for (int32_t c = 4 * lg + STEP; c < P; c += STEP) {
      float u[4];
      load4<VEC>(z, c, P, ninf, u);
      s += (expf(u[0] - mx) + expf(u[1] - mx)) + (expf(u[2] - mx) + expf(u[3] - mx));
    }
  s = group_sum<LPR>(s);
}

__device__ __forceinline__ float row_lse(float mx, float s) { return mx + logf(s); }

// counts[r] * l_r in float64; a target outside [0, P): NaN loss, nothing read
__device__ __forceinline__ double row_weighted_loss(const float* __restrict__ z, int32_t P, int64_t t, int32_t cnt,
                                                    float lse) {
  const float zt = t >= 0 && t < P ? z[t] : NAN;
  return (double)cnt * ((double)lse - (double)zt);
}

// the fixed tree over a workgroup's RPB rows (s_w[g] written by row g's first lane, before a
// barrier here); the sum is left in s_w[0], read by thread 0
template <int RPB>
__device__ __forceinline__ void block_tree(double* s_w) {
  __syncthreads();
#pragma unroll
  for (int st = RPB / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) s_w[threadIdx.x] += s_w[threadIdx.x + st];
    __syncthreads();
  }
}

// thread i's run of consecutive partials, summed in index order (256 threads, `load(b)`
// reads partial b)
template <typename Load>
__device__ __forceinline__ double partial_run(int32_t nblk, Load load) {
  const int32_t run = (nblk + 255) / 256;
  const int32_t b0 = threadIdx.x * run, b1 = min(b0 + run, nblk);
  double acc = 0.0;
  for (int32_t b = b0; b < b1; ++b) acc += load(b);
  return acc;
}

// fp32( (the 256 runs, in index order) / n ): thread 0 only
__device__ __forceinline__ float mean_of_runs(const double* s, int64_t n) {
  double t = s[0];
  for (int i = 1; i < 256; ++i) t += s[i];
  return (float)(t / (double)n);
}

// lanes per row: the smallest power of two covering ceil(P / 4) float4 pieces, at most 64
inline int lanes_per_row(int32_t P) {
  const int pieces = (P + 3) / 4;
  int l = 1;
  while (l < pieces && l < 64) l <<= 1;
  return l;
}
inline int32_t blocks(int32_t M, int32_t P) {
  const int rpb = 256 / lanes_per_row(P);
  return (int32_t)(((int64_t)M + rpb - 1) / rpb);
}

}  // namespace ce
}  // namespace gcnk
