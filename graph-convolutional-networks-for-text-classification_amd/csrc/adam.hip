// Adam step of up to 8 parameter tensors in one launch (trainer.py:308 th.optim.Adam,
// trainer.py:362 optimizer.step(); with GCNK_ADAM_ZERO_GRAD also trainer.py:359
// optimizer.zero_grad()).
//
// torch.optim.Adam runs a step as a dozen multi_tensor_apply launches (lerp, mul,
// addcmul, sqrt, div, addcdiv, ...), each a pass over the parameters' bytes.  Here a step
// is one pass: read p, g, m, v, write p, m, v (28 B per element, the compulsory traffic).
// The contract -- the arithmetic, its roundings, the step word -- is in include/gcnk.h.
//
// Work is cut into chunks of GCNK_ADAM_CHUNK elements by tensor_chunks.h's table.
#include "gcnk_common.h"
#include "tensor_chunks.h"

#include <cmath>

namespace gcnk {
namespace {

constexpr int kChunk = GCNK_ADAM_CHUNK;
constexpr int kMaxTensors = GCNK_ADAM_MAX_TENSORS;

struct AdamArgs {
  gcnk_adam_tensor t[kMaxTensors];
  chunks::Table<kMaxTensors> tab;
  double lr, beta1, beta2;
  float omb1, b2, omb2, eps, wd;   // fp32( beta2 ), fp32( 1 - beta ) formed in float64
  int32_t zero_grad, advance;
};

struct Coef {
  float omb1, b2, omb2, eps, wd, step_size, sqrt_bc2;
};

__device__ __forceinline__ void adam_elem(const Coef& k, float& p, float g, float& m, float& v) {
  // the operations in the order torch's own step takes them (lerp_, mul_ + addcmul_, sqrt / div / add_,
  // addcdiv_), so the roundings fall where the reference trainer's fall, up to the fused multiply-adds
  g = fmaf(k.wd, p, g);
  m = fmaf(k.omb1, g - m, m);
  v = fmaf(k.b2, v, (k.omb2 * g) * g);
  const float denom = sqrtf(v) / k.sqrt_bc2 + k.eps;
  p = p - (k.step_size * m) / denom;
}

static_assert(kChunk == 2 * 4 * 256, "a workgroup of 256 threads holds a chunk as two float4 pieces per thread");

__global__ void __launch_bounds__(256) adam_kernel(const AdamArgs a, int32_t* __restrict__ state,
                                                   const int32_t* __restrict__ gate) {
  __shared__ float s_step[3];   // the two step factors; the gate word
  const int tid = threadIdx.x;
  const int32_t blk = blockIdx.x;
  // The step word: read at entry by one lane (the load is in flight while the chunk's own loads are
  // issued).  After the barrier below that lane counts this workgroup in, and the last to arrive stores
  // t + 1 (arrive_last, gcnk_common.h).  Nothing else passes between workgroups.
  // The gate (gcnk_adam_gated_f32): a word an earlier launch on the stream wrote, so every workgroup of
  // this launch reads the same value; read by the same lane and broadcast with the step factors.  Closed,
  // the workgroup returns behind the barrier having stored nothing and counted itself in nowhere.
  int32_t t = 0, closed = 0;
  if (tid == 0) {
    t = __hip_atomic_load(state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gate) closed = __hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }

  // this workgroup's tensor, selected here (tensor_chunks.h: a shared helper doing it cost scratch, or keep's time)
  float *p = a.t[0].p, *g = a.t[0].g, *m = a.t[0].m, *v = a.t[0].v;
  int64_t numel = a.t[0].numel;
  int32_t first = 0, head = a.tab.head[0];
#pragma unroll
  for (int i = 1; i < kMaxTensors; ++i)
    if (blk >= a.tab.first[i]) {
      p = a.t[i].p; g = a.t[i].g; m = a.t[i].m; v = a.t[i].v;
      numel = a.t[i].numel;
      first = a.tab.first[i];
      head = a.tab.head[i];
    }
  // (without work, a launch of empty tensors only, the step still advances)
  const chunks::Span<kChunk> s(blk - first, head, blk < a.tab.first[kMaxTensors], numel);

  // the 16-B aligned body of the chunk, loaded before the step factors are known
  float4* p4 = reinterpret_cast<float4*>(p + s.e0);
  float4* g4 = reinterpret_cast<float4*>(g + s.e0);
  float4* m4 = reinterpret_cast<float4*>(m + s.e0);
  float4* v4 = reinterpret_cast<float4*>(v + s.e0);
  float4 pe[2], ge[2], me[2], ve[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int32_t i = tid + 256 * it;
    if (i < s.n4) {
      pe[it] = p4[i]; ge[it] = g4[i]; me[it] = m4[i]; ve[it] = v4[i];
    }
  }

  if (tid == 0) {
    // the two bias corrections, in float64 from t + 1, each rounded once
    const double tn = (double)(t + 1);
    s_step[0] = (float)(a.lr / (1.0 - pow(a.beta1, tn)));
    s_step[1] = (float)sqrt(1.0 - pow(a.beta2, tn));
    s_step[2] = __int_as_float(closed);
  }
  __syncthreads();
  if (__float_as_int(s_step[2]) != 0) return;
  if (tid == 0 && a.advance && arrive_last(state + 1)) {
    __hip_atomic_store(state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(state, t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!s.work) return;
  const Coef k = {a.omb1, a.b2, a.omb2, a.eps, a.wd, s_step[0], s_step[1]};

  auto scalar = [&](int64_t e) {
    float ps = p[e], ms = m[e], vs = v[e];
    const float gs = g[e];
    adam_elem(k, ps, gs, ms, vs);
    p[e] = ps; m[e] = ms; v[e] = vs;
    if (a.zero_grad) g[e] = 0.f;
  };
  if (s.head < 0) {   // buffers at different offsets from a 16-B boundary: scalar
    for (int64_t e = s.e0 + tid; e < s.e1; e += 256) scalar(e);
    return;
  }
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int32_t i = tid + 256 * it;
    if (i < s.n4) {
      adam_elem(k, pe[it].x, ge[it].x, me[it].x, ve[it].x);
      adam_elem(k, pe[it].y, ge[it].y, me[it].y, ve[it].y);
      adam_elem(k, pe[it].z, ge[it].z, me[it].z, ve[it].z);
      adam_elem(k, pe[it].w, ge[it].w, me[it].w, ve[it].w);
      p4[i] = pe[it]; m4[i] = me[it]; v4[i] = ve[it];
      if (a.zero_grad) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  const int64_t e = s.edge(tid);
  if (e >= 0) scalar(e);
}

}  // namespace
}  // namespace gcnk

using namespace gcnk;

static int adam_launch(const char* who, const gcnk_adam_tensor* t, int32_t ntensors, double lr, double beta1,
                       double beta2, double eps, double weight_decay, int32_t* state, int32_t flags,
                       const int32_t* gate, void* stream) {
  if (ntensors < 0 || ntensors > kMaxTensors) {
    set_error("%s: bad argument (ntensors=%d, at most %d per call)", who, ntensors, kMaxTensors);
    return GCNK_EARG;
  }
  if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) ||
      !(weight_decay >= 0.0) || (flags & ~(GCNK_ADAM_ZERO_GRAD | GCNK_ADAM_HOLD_STEP))) {
    set_error("%s: bad argument (lr=%g beta1=%g beta2=%g eps=%g weight_decay=%g flags=%d; lr, eps, weight_decay >= 0, "
              "0 <= beta < 1)", who, lr, beta1, beta2, eps, weight_decay, flags);
    return GCNK_EARG;
  }
  if (ntensors == 0) return GCNK_OK;
  if (!t || !state) {
    set_error("%s: null tensor table or state", who);
    return GCNK_EARG;
  }
  AdamArgs a = {};
  int64_t nchunks = 0;
  for (int i = 0; i < ntensors; ++i) {
    const gcnk_adam_tensor& x = t[i];
    if (x.numel < 0 || (x.numel > 0 && (!x.p || !x.g || !x.m || !x.v))) {
      set_error("%s: tensor %d: null buffer or numel < 0 (numel=%lld)", who, i, (long long)x.numel);
      return GCNK_EARG;
    }
    a.t[i] = x;
    if (!chunks::append<kChunk>(a.tab, i, x.numel, chunks::head_of({x.p, x.g, x.m, x.v}), nchunks)) {
      set_error("%s: more than 2^31 chunks in one call", who);
      return GCNK_EARG;
    }
  }
  a.lr = lr;
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.omb1 = (float)(1.0 - beta1);
  a.b2 = (float)beta2;
  a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  a.wd = (float)weight_decay;
  a.zero_grad = (flags & GCNK_ADAM_ZERO_GRAD) ? 1 : 0;
  a.advance = (flags & GCNK_ADAM_HOLD_STEP) ? 0 : 1;
  if (nchunks == 0 && !a.advance) return GCNK_OK;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)(nchunks > 0 ? nchunks : 1)), dim3(256), 0, (hipStream_t)stream, a,
                     state, gate);
  return launch_check("adam_kernel");
}

extern "C" int gcnk_adam_f32(const gcnk_adam_tensor* t, int32_t ntensors, double lr, double beta1, double beta2,
                             double eps, double weight_decay, int32_t* state, int32_t flags, void* stream) {
  return adam_launch("gcnk_adam_f32", t, ntensors, lr, beta1, beta2, eps, weight_decay, state, flags, nullptr, stream);
}

extern "C" int gcnk_adam_gated_f32(const gcnk_adam_tensor* t, int32_t ntensors, double lr, double beta1, double beta2,
                                   double eps, double weight_decay, int32_t* state, int32_t flags,
                                   const int32_t* gate, void* stream) {
  return adam_launch("gcnk_adam_gated_f32", t, ntensors, lr, beta1, beta2, eps, weight_decay, state, flags, gate,
                     stream);
}
