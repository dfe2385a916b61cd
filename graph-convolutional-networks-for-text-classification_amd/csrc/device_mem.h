// Device memory idioms of libgcnk's kernels (gfx950), each stated once: the 4-float register vector, raw
// buffer resources with their typed accesses, the 16-byte / nontemporal stores.  Included by gcnk_common.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gcnk {

// Four floats in four consecutive VGPRs: the MFMA 16x16x4 C/D fragment and the payload of one 16-byte access.
// A pointer is cast to an aligned form so that the access is ONE 16-byte instruction: through a float4* the
// backend may split a store it has sunk out of a branch into dword + dwordx3.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4a __attribute__((ext_vector_type(4), aligned(16)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(16)));

// ----------------------------------------------------------------------------
// Raw buffer resources (stride 0).  `bytes` is the resource's num_records: a lane whose byte offset (vector +
// scalar offset, both 32-bit) is at or past it reads 0 and stores nothing, with no compare, select or branch
// in the kernel.  Below it the access goes to base + offset unchecked, so the HOST must have checked that the
// operand spans at least `bytes` and that every offset the kernel forms for a live lane fits 32 bits.  A kernel
// turns a lane off with the offset kBufOob (or by OR-ing it in): the host's span checks keep it past every resource.
constexpr uint32_t kBufOob = 0x7ff00000u;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* base, uint32_t bytes) {
  // word 3: DATA_FORMAT = 32 (bits 18:15), all else 0 -- what gfx9 raw (untyped) buffer accesses take
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
// The same, or (`on` false) the zero-byte resource: every lane reads 0 and stores
// nothing whatever its offset, and base is never dereferenced.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc_if(bool on, const void* base, uint32_t bytes) {
  return buffer_rsrc(base, on ? bytes : 0u);
}

// Cache policy of a buffer access (the builtin's aux operand).  kBufSc1 is the agent-coherent form (past the per-XCD
// L2, what relaxed agent-scope atomics get): a hand-off through memory needs it on EVERY access to the bytes.
constexpr int kBufPlain = 0;
constexpr int kBufSc1 = 16;

// Typed accesses: voff the lane's byte offset, soff a wave-uniform one added to it.
template <int POLICY = kBufPlain>
__device__ __forceinline__ uint32_t buf_load_u32(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff = 0) {
  return __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, POLICY);
}
template <int POLICY = kBufPlain>
__device__ __forceinline__ float buf_load_f32(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff = 0) {
  return __uint_as_float(buf_load_u32<POLICY>(r, voff, soff));
}
template <int POLICY = kBufPlain>
__device__ __forceinline__ u32x3 buf_load_u32x3(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff = 0) {
  return __builtin_amdgcn_raw_buffer_load_b96(r, (int)voff, (int)soff, POLICY);
}
template <int POLICY = kBufPlain>
__device__ __forceinline__ f32x4 buf_load_f32x4(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff = 0) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, POLICY));
}
// (two doubles: the 16-byte access of a float64 row)
typedef double f64x2 __attribute__((ext_vector_type(2)));
template <int POLICY = kBufPlain>
__device__ __forceinline__ f64x2 buf_load_f64x2(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff = 0) {
  return __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, POLICY));
}
// (one double)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
template <int POLICY = kBufPlain>
__device__ __forceinline__ double buf_load_f64(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff = 0) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, POLICY));
}
template <int POLICY = kBufPlain>
__device__ __forceinline__ void buf_store_f64(double v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff = 0) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, (int)voff, (int)soff, POLICY);
}
template <int POLICY = kBufPlain>
__device__ __forceinline__ void buf_store_f32(float v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff = 0) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, (int)voff, (int)soff, POLICY);
}
template <int POLICY = kBufPlain>
__device__ __forceinline__ void buf_store_f32x4(const f32x4& v, __amdgpu_buffer_rsrc_t r, uint32_t voff,
                                                uint32_t soff = 0) {
  __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)voff, (int)soff, POLICY);
}

// ----------------------------------------------------------------------------
// Stores through a pointer (p 16-byte aligned for the 16-byte forms).
// One 16-byte store instruction whatever the surrounding control flow.
__device__ __forceinline__ void store16(float* p, const float4& v) {
  *reinterpret_cast<f32x4a*>(__builtin_assume_aligned(p, 16)) = f32x4a{v.x, v.y, v.z, v.w};
}
// Nontemporal (streaming) stores: output that this kernel does not read again
// leaves no dirty lines in the XCD L2s for the end-of-kernel write-back.
__device__ __forceinline__ void store16_nt(float* p, const f32x4& v) {
  __builtin_nontemporal_store(f32x4a{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4a*>(p));
}
__device__ __forceinline__ void store16_nt(float* p, const float4& v) { store16_nt(p, f32x4{v.x, v.y, v.z, v.w}); }
// (four 32-bit words: every bit pattern survives)
__device__ __forceinline__ void store16_nt(u32x4a* p, const u32x4a& v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void store4_nt(float* p, float v) { __builtin_nontemporal_store(v, p); }

}  // namespace gcnk
