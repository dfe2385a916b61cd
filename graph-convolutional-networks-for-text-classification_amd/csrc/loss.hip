// Mean cross-entropy of logits[M x P] over a node set (trainer.py:307 nn.CrossEntropyLoss
// applied to logits[train_lst], trainer.py:358-361 its forward and backward, trainer.py:383
// the validation loss), without materialising logits[idx] and without a scatter.
//
// ATen runs `crit(logits[idx], target[idx])` as an index gather, a log-softmax, an nll
// reduce and, in the backward, a radix sort + merge passes + float accumulation to scatter
// the gathered rows' gradients back.  Here the index set is turned ONCE into per-row
// multiplicities (ce_row_counts_kernel, integer atomics: exact), after which the forward and
// the backward are dense passes over the M rows: a row's loss / gradient is weighted by how
// often the set names it, so duplicates are exact and nothing is sorted or scattered.
//
// A row is owned by one lane group of LPR lanes (the smallest power of two covering
// ceil(P / 4) four-column pieces, at most 64); wider rows (P > 256) loop in passes of 256
// columns.  Row sums meet in a shuffle tree of fixed shape; the loss is summed in float64:
// a fixed tree over a workgroup's rows, the workgroups' partials in index order by a second
// launch, one rounding to fp32.  No float atomics: bitwise reproducible.
#include "ce_row.h"

namespace gcnk {
namespace {

using namespace ce;   // the row arithmetic, shared with epoch.hip

__global__ void __launch_bounds__(256)
ce_row_counts_kernel(const int64_t* __restrict__ idx, int64_t n, int32_t M, int32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t r = idx[i];
  atomicAdd(counts + (r >= 0 && r < M ? r : (int64_t)M), 1);   // out of range: counted in counts[M], never a row
}

template <int LPR, bool VEC>
__global__ void __launch_bounds__(256)
ce_forward_kernel(const float* __restrict__ logits, int64_t ld, int32_t M, int32_t P,
                  const int64_t* __restrict__ target, const int32_t* __restrict__ counts,
                  float* __restrict__ lse_out, double* __restrict__ part) {
  constexpr int RPB = 256 / LPR;   // rows per workgroup
  __shared__ double s_w[RPB];
  const int g = threadIdx.x / LPR, lg = threadIdx.x % LPR;
  const int64_t r = (int64_t)blockIdx.x * RPB + g;
  int32_t cnt = 0;
  if (r < M) cnt = counts ? counts[r] : 1;
  const bool scored = cnt > 0;          // uniform over the lane group
  const float* z = logits + (scored ? r : 0) * ld;
  float v[4], mx, s;
  row_max_sum<LPR, VEC>(z, lg, P, scored, v, mx, s);

  if (lg == 0) {
    double w = 0.0;
    if (scored) {
      const float lse = row_lse(mx, s);
      w = row_weighted_loss(z, P, target[r], cnt, lse);
      if (lse_out) lse_out[r] = lse;
    }
    s_w[g] = w;
  }
  block_tree<RPB>(s_w);
  if (threadIdx.x == 0) part[blockIdx.x] = s_w[0];
}

// loss = fp32( (sum of the partials, in index order) / n ): thread i sums its run of
// consecutive partials, thread 0 the 256 runs, both in index order
__global__ void __launch_bounds__(256)
ce_reduce_kernel(const double* __restrict__ part, int32_t nblk, int64_t n, float* __restrict__ loss) {
  __shared__ double s[256];
  s[threadIdx.x] = partial_run(nblk, [&](int32_t b) { return part[b]; });
  __syncthreads();
  if (threadIdx.x != 0) return;
  *loss = mean_of_runs(s, n);
}

template <int LPR, bool VEC>
__global__ void __launch_bounds__(256)
ce_backward_kernel(const float* __restrict__ logits, int64_t ld, int32_t M, int32_t P,
                   const int64_t* __restrict__ target, const int32_t* __restrict__ counts, int64_t n,
                   const float* __restrict__ lse_in, const float* __restrict__ grad_out,
                   float* __restrict__ dlogits, int64_t ldd) {
  constexpr int RPB = 256 / LPR;
  constexpr int STEP = 4 * LPR;
  const int g = threadIdx.x / LPR, lg = threadIdx.x % LPR;
  const int64_t r = (int64_t)blockIdx.x * RPB + g;
  if (r >= M) return;
  const int32_t cnt = counts ? counts[r] : 1;
  float* d = dlogits + r * ldd;
  float coef = 0.f, lse = 0.f;
  int64_t t = -1;
  if (cnt > 0) {
    // g * (counts / n): a power-of-two g scales every element exactly
    coef = (grad_out ? *grad_out : 1.0f) * (float)((double)cnt / (double)n);
    lse = lse_in[r];
    t = target[r];
  }
  const float* z = logits + r * ld;
  for (int32_t c = 4 * lg; c < P; c += STEP) {
    float o[4] = {0.f, 0.f, 0.f, 0.f};   // rows the set does not name: +0.0
    if (cnt > 0) {
      float v[4];
      load4<VEC>(z, c, P, 0.f, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = coef * (expf(v[j] - lse) - (c + j == t ? 1.0f : 0.0f));
    }
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(d + c) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c + j < P) d[c + j] = o[j];   // columns P .. ldd - 1 are never written
    }
  }
}

inline int32_t ce_blocks(int32_t M, int32_t P) { return blocks(M, P); }

template <bool VEC>
void launch_forward(int lpr, dim3 grid, hipStream_t s, const float* logits, int64_t ld, int32_t M, int32_t P,
                    const int64_t* target, const int32_t* counts, float* lse, double* part) {
#define GCNK_CE_FWD(L)                                                                                              \
  case L:                                                                                                           \
    hipLaunchKernelGGL((ce_forward_kernel<L, VEC>), grid, dim3(256), 0, s, logits, ld, M, P, target, counts, lse,   \
                       part);                                                                                       \
    break;
  switch (lpr) {
    GCNK_CE_FWD(1) GCNK_CE_FWD(2) GCNK_CE_FWD(4) GCNK_CE_FWD(8) GCNK_CE_FWD(16) GCNK_CE_FWD(32) GCNK_CE_FWD(64)
  }
#undef GCNK_CE_FWD
}

template <bool VEC>
void launch_backward(int lpr, dim3 grid, hipStream_t s, const float* logits, int64_t ld, int32_t M, int32_t P,
                     const int64_t* target, const int32_t* counts, int64_t n, const float* lse, const float* grad_out,
                     float* dlogits, int64_t ldd) {
#define GCNK_CE_BWD(L)                                                                                              \
  case L:                                                                                                           \
    hipLaunchKernelGGL((ce_backward_kernel<L, VEC>), grid, dim3(256), 0, s, logits, ld, M, P, target, counts, n,    \
                       lse, grad_out, dlogits, ldd);                                                                \
    break;
  switch (lpr) {
    GCNK_CE_BWD(1) GCNK_CE_BWD(2) GCNK_CE_BWD(4) GCNK_CE_BWD(8) GCNK_CE_BWD(16) GCNK_CE_BWD(32) GCNK_CE_BWD(64)
  }
#undef GCNK_CE_BWD
}

}  // namespace
}  // namespace gcnk

using namespace gcnk;

extern "C" int gcnk_ce_row_counts(const int64_t* idx, int64_t n, int32_t M, int32_t* counts, void* stream) {
  if (n < 0 || M < 0 || !counts || (n > 0 && !idx)) {
    set_error("gcnk_ce_row_counts: bad argument (n=%lld M=%d)", (long long)n, M);
    return GCNK_EARG;
  }
  hipStream_t s = (hipStream_t)stream;
  int rc = hip_check(hipMemsetAsync(counts, 0, ((size_t)M + 1) * 4, s), "ce_row_counts memset");
  if (rc || n == 0) return rc;
  hipLaunchKernelGGL(ce_row_counts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, idx, n, M, counts);
  return launch_check("ce_row_counts_kernel");
}

extern "C" int64_t gcnk_ce_workspace_bytes(int32_t M, int32_t P) {
  if (M < 0 || P < 1 || P > kMaxClasses) {
    set_error("gcnk_ce_workspace_bytes: bad argument (M=%d P=%d)", M, P);
    return GCNK_EARG;
  }
  return (int64_t)ce_blocks(M, P) * 8;
}

extern "C" int gcnk_ce_forward_f32(const float* logits, int64_t ld, int32_t M, int32_t P, const int64_t* target,
                                   const int32_t* counts, int64_t n, float* loss, float* lse, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  if (M < 0 || P < 1 || P > kMaxClasses || ld < P || n < 0) {
    set_error("gcnk_ce_forward_f32: bad argument (M=%d P=%d ld=%lld n=%lld; 1 <= P <= %d, ld >= P)", M, P,
              (long long)ld, (long long)n, kMaxClasses);
    return GCNK_EARG;
  }
  if (M == 0) return GCNK_OK;
  if (!logits || !target || !loss) {
    set_error("gcnk_ce_forward_f32: null logits, target or loss");
    return GCNK_EARG;
  }
  const int32_t nblk = ce_blocks(M, P);
  if (!workspace || workspace_bytes < (int64_t)nblk * 8 || (reinterpret_cast<uintptr_t>(workspace) & 7u)) {
    set_error("gcnk_ce_forward_f32: workspace of %lld bytes at an 8-byte aligned address needed (got %lld)",
              (long long)nblk * 8, (long long)workspace_bytes);
    return GCNK_EARG;
  }
  hipStream_t s = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  const int lpr = lanes_per_row(P);
  if (aligned16(logits) && ld % 4 == 0 && P % 4 == 0)
    launch_forward<true>(lpr, dim3((unsigned)nblk), s, logits, ld, M, P, target, counts, lse, part);
  else
    launch_forward<false>(lpr, dim3((unsigned)nblk), s, logits, ld, M, P, target, counts, lse, part);
  int rc = launch_check("ce_forward_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(ce_reduce_kernel, dim3(1), dim3(256), 0, s, part, nblk, n, loss);
  return launch_check("ce_reduce_kernel");
}

extern "C" int gcnk_ce_backward_f32(const float* logits, int64_t ld, int32_t M, int32_t P, const int64_t* target,
                                    const int32_t* counts, int64_t n, const float* lse, const float* grad_out,
                                    float* dlogits, int64_t ldd, void* stream) {
  if (M < 0 || P < 1 || P > kMaxClasses || ld < P || ldd < P || n < 0) {
    set_error("gcnk_ce_backward_f32: bad argument (M=%d P=%d ld=%lld ldd=%lld n=%lld; 1 <= P <= %d, ld, ldd >= P)", M,
              P, (long long)ld, (long long)ldd, (long long)n, kMaxClasses);
    return GCNK_EARG;
  }
  if (M == 0) return GCNK_OK;
  if (!logits || !target || !lse || !dlogits) {
    set_error("gcnk_ce_backward_f32: null logits, target, lse or dlogits");
    return GCNK_EARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const int32_t nblk = ce_blocks(M, P);
  const int lpr = lanes_per_row(P);
  if (aligned16(logits) && ld % 4 == 0 && aligned16(dlogits) && ldd % 4 == 0 && P % 4 == 0)
    launch_backward<true>(lpr, dim3((unsigned)nblk), s, logits, ld, M, P, target, counts, n, lse, grad_out, dlogits,
                          ldd);
  else
    launch_backward<false>(lpr, dim3((unsigned)nblk), s, logits, ld, M, P, target, counts, n, lse, grad_out, dlogits,
                           ldd);
  return launch_check("ce_backward_kernel");
}
