// gc2's aggregation out = A-hat S2 + b2 (reference layer.py:106,110) from the
// hub factor (factor.py): one launch, two kinds of workgroup.
//
// The generic row kernel walks row unit -> item range -> items -> B rows: three
// serial waits before the first gather.  On a factored (A-hat, X) pair a light
// row's nonzeros are its own diagonal plus hub columns, so its sum needs its
// own S2 row, the H hub rows of S2 and its A_H items -- the items gc1's block
// records already hold.  A hub row is a plain long CSR row.
//
//   hub-row workgroups (blockIdx.x < H, first in the grid: the longest): the
//     row's item range and id come from the kernel arguments; round 1 loads
//     kHubU items per lane group, round 2 gathers their S2 rows (16-B loads,
//     all in flight); each lane sums its items in ascending order, the lane
//     groups meet through LDS in a fixed order (16 collectors, then one sum).
//     Rows longer than one pass (G * kHubU items) loop in passes.
//   document workgroups (one per 32-row block record): the opening round
//     issues the record by LDS-DMA, diag, the precede counts, the row ids, the
//     hub ids (from the kernel arguments) and b2; the second round the H hub
//     rows of S2 by LDS-DMA and each row's own S2 row (their addresses need
//     the ids: the one dependent round of this path); after the barrier a
//     row's items and their hub rows are read from LDS: one fma chain from +0
//     in CSR column order -- the diagonal at its sorted position -- and the
//     bias.  That is the order of
//     spmm_row_kernel's one-unit rows (gather_rows: one chain from zero in item
//     order, finish_row: + bias), so those rows are bit for bit the row kernel's.
//
// Out-of-range lanes go through buffer resources sized to the operands (loads
// return 0, stores are dropped); no global partials, counters or atomics.
// The output rows are stored write-through (sc1): nothing in this launch reads
// them, and plain stores left them as dirty lines in the XCD L2s for the
// end-of-kernel write-back (2.94-2.97 against 2.99-3.01 us replayed; nontemporal
// stores 3.33-3.35: DESIGN section 5, "What each launch leaves at its seam").
#include "hub_block.h"

#include <algorithm>

namespace gcnk {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxHubs = 128;
constexpr int kHubU = 16;                  // items (and gathers) in flight per lane of a hub-row workgroup
constexpr int kDocU = 8;                   // items of a document row read from LDS per batch
constexpr int kCollect = 16;               // collector groups of the hub rows' fixed-order combine
constexpr int kPartSlots = 384;            // combine slots: 16 * ceil(G / 16) * P4 <= 336, zero past the real ones

struct Gc2Args {
  int32_t M, H, P, rec_words;
  const int32_t* rec;
  const float* diag;
  const int32_t* pre;
  const int32_t* hub_ci;
  const float* hub_val;
  const float* S2;
  const float* b2;
  float* out;
  uint32_t ld4, ldo4;                      // leading dimensions in bytes
  uint32_t s2_bytes, out_bytes, pos_bytes, b2_bytes;
  unsigned long long* stamps;              // debug timeline (-DGCNK_STAMPS), normally null
  // in the argument block: a hub row's id and item range arrive with the other
  // arguments, and the document blocks read the ids with one vector load
  int32_t hub_id[kMaxHubs];
  int32_t hub_rp[kMaxHubs + 1];
};

__device__ __forceinline__ void fma4(f32x4& acc, float a, const f32x4& b) {
  acc.x = fmaf(a, b.x, acc.x);
  acc.y = fmaf(a, b.y, acc.y);
  acc.z = fmaf(a, b.z, acc.z);
  acc.w = fmaf(a, b.w, acc.w);
}

// 4 x s_memrealtime per workgroup (entry, operands landed, sums done, exit), thread 0
__device__ __forceinline__ void stamp2(const Gc2Args& a, int k) {
#ifndef GCNK_STAMPS
  (void)a;
  (void)k;
#else
  if (a.stamps && threadIdx.x == 0) a.stamps[4 * (unsigned long long)blockIdx.x + k] = __builtin_amdgcn_s_memrealtime();
#endif
}

// acc += items [jb, je) of a document row, in order, kDocU at a time from LDS:
// the item words, then their hub rows of S2, then the fmas.  A slot past the
// row's end reads the zeroed row behind s_hub with its value masked to 0:
// fma(0, 0, acc) is acc exactly.  (One select per term on the LDS offset and one
// AND on the value: a select per product element made the chain ~36 instructions
// a term, 1.4 us of a lone wave's issue.)
template <int P4>
__device__ __forceinline__ void doc_chain(f32x4& acc, const HubItem* s_items, const float* s_hub, int zero_off, int c,
                                          int jb, int je) {
  constexpr int P = 4 * P4;
  for (int j0 = jb; j0 < je; j0 += kDocU) {
    HubItem it[kDocU];
    f32x4 hv[kDocU];
#pragma unroll
    for (int u = 0; u < kDocU; ++u) it[u] = s_items[min(j0 + u, je - 1)];
#pragma unroll
    for (int u = 0; u < kDocU; ++u)
      hv[u] = *reinterpret_cast<const f32x4*>(s_hub + (j0 + u < je ? it[u].x * P : zero_off) + 4 * c);
#pragma unroll
    for (int u = 0; u < kDocU; ++u) fma4(acc, __int_as_float(it[u].y & (j0 + u < je ? -1 : 0)), hv[u]);
  }
}

// P4 = P / 4: lanes per row (each a 16-B column vector)
template <int P4>
__global__ void __launch_bounds__(kThreads) factored_spmm_row_kernel(Gc2Args a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int P = 4 * P4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = tid % P4;
  stamp2(a, 0);
  const __amdgpu_buffer_rsrc_t r_s2 = buffer_rsrc(a.S2, a.s2_bytes);
  const __amdgpu_buffer_rsrc_t r_out = buffer_rsrc(a.out, a.out_bytes);
  // a hub row's range and id, read with the other arguments in the entry block
  // (behind the branch they were a scalar round trip of their own; a document
  // workgroup reads hub 127's words and drops them)
  const int hsel = min((int)blockIdx.x, kMaxHubs - 1);
  const int32_t hub_b = a.hub_rp[hsel], hub_e = a.hub_rp[hsel + 1], hub_row = a.hub_id[hsel];
  const f32x4 bv = buf_load_f32x4(buffer_rsrc(a.b2, a.b2_bytes), 16u * c);   // (no b2: an empty resource, reads 0)
  asm volatile("" ::"s"(hub_b), "s"(hub_e), "s"(hub_row));   // (pinned here: the compiler sank them behind the branch)

  if ((int)blockIdx.x < a.H) {
    // ---- hub row h: items [b, b + n) of the hub CSR, G lane groups take items g, g + G, ...
    constexpr int G = kThreads / P4;
    const int32_t b = hub_b, n = hub_e - hub_b;
    const int32_t row = hub_row;
    const int g = tid / P4;
    const bool live = g < G;                // (P = 12, 20, 28: the last threads hold no group)
    const __amdgpu_buffer_rsrc_t r_ci = buffer_rsrc(a.hub_ci + b, 4u * (uint32_t)n);
    const __amdgpu_buffer_rsrc_t r_v = buffer_rsrc(a.hub_val + b, 4u * (uint32_t)n);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int32_t k0 = 0; k0 < n; k0 += G * kHubU) {
      uint32_t col[kHubU];
      float val[kHubU];
      f32x4 s[kHubU];
#pragma unroll
      for (int j = 0; j < kHubU; ++j) {     // round 1: past the row's end (or a dead thread) reads 0
        const uint32_t off = live ? 4u * (uint32_t)(k0 + g + G * j) : kBufOob;
        col[j] = buf_load_u32(r_ci, off);
        val[j] = buf_load_f32(r_v, off);
      }
      stamp2(a, 1);
#pragma unroll
      for (int j = 0; j < kHubU; ++j) {     // round 2: their S2 rows; no item, no load (0)
        // (a mask OR-ed in, not a select of the offset: the select became a branch around each load)
        const uint32_t dead = live && k0 + g + G * j < n ? 0u : kBufOob;
        s[j] = buf_load_f32x4(r_s2, (col[j] * a.ld4 + 16u * c) | dead);
      }
      // (every gather issued before the first fma: the scheduler otherwise pulled
      // the fmas up between them to save registers, a wait for all but one load
      // after the third gather)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < kHubU; ++j) fma4(acc, val[j], s[j]);   // ascending items (0 * 0 past the end)
    }
    // the lane groups meet: slot = thread; collector q sums groups q, q + 16, ...
    // in order, then lane c of group 0 sums the collectors in order
    f32x4* s_part = reinterpret_cast<f32x4*>(smem);
    f32x4* s_coll = s_part + kPartSlots;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    s_part[tid] = live ? acc : zero;
    if (tid < kPartSlots - kThreads) s_part[kThreads + tid] = zero;
    __syncthreads();
    constexpr int NJ = (G + kCollect - 1) / kCollect;
    if (tid < kCollect * P4) {
      f32x4 p[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) p[j] = s_part[(g + kCollect * j) * P4 + c];
      f32x4 t = p[0];
#pragma unroll
      for (int j = 1; j < NJ; ++j) t += p[j];
      s_coll[tid] = t;
    }
    __syncthreads();
    stamp2(a, 2);
    if (tid < P4) {
      f32x4 p[kCollect];
#pragma unroll
      for (int q = 0; q < kCollect; ++q) p[q] = s_coll[q * P4 + c];
      f32x4 t = p[0];
#pragma unroll
      for (int q = 1; q < kCollect; ++q) t += p[q];
      t += bv;
      buf_store_f32x4<kBufSc1>(t, r_out, (uint32_t)row * a.ldo4 + 16u * c);
    }
    stamp2(a, 3);
    return;
  }

  // ---- document block: positions 32 blk .. 32 blk + 31 of the block order
  const int blk = (int)blockIdx.x - a.H;
  int32_t* s_rec = reinterpret_cast<int32_t*>(smem);
  float* s_hub = smem + a.rec_words;                       // [H][P], then a zero row
  const int i = tid / P4;                                  // row of the block (threads past 32 rows: none)
  const bool rowt = i < kHubRows;
  // round 1 (b2 above): the record by LDS-DMA; per row thread its diag, precede
  // count and row id; per thread the hub id of each 16-B piece of S2[hubs] it
  // stages (a vector load from the argument block: scalar loads of the ids cost
  // the workgroup three serial round trips, ~1 us cold)
  const int32_t* rec = a.rec + (int64_t)blk * a.rec_words;
  {
    const int rw4 = a.rec_words / 4;
    for (int e0 = wv * 64; e0 < rw4; e0 += kThreads)
      if (e0 + lane < rw4) lds_dma16(rec + 4 * (e0 + lane), s_rec + 4 * e0);
  }
  const uint32_t pos4 = rowt ? 4u * (uint32_t)(blk * kHubRows + i) : kBufOob;
  const float dg = buf_load_f32(buffer_rsrc(a.diag, a.pos_bytes), pos4);
  const int32_t pre = (int32_t)buf_load_u32(buffer_rsrc(a.pre, a.pos_bytes), pos4);
  const int32_t rid =
      (int32_t)buf_load_u32(buffer_rsrc(rec, 4u * (uint32_t)a.rec_words), rowt ? 4u * (uint32_t)(kHubRecRow + i) : kBufOob);
  constexpr int NQ = (kMaxHubs * P4 + kThreads - 1) / kThreads;   // pieces of S2[hubs] per thread
  const int nh4 = a.H * P4;
  int32_t hid[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) hid[q] = a.hub_id[min((tid + kThreads * q) / P4, kMaxHubs - 1)];
#pragma unroll
  for (int q = 0; q < NQ; ++q) asm volatile("" : "+v"(hid[q]));   // (loaded in this round: not sunk to its use)
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  // round 2: S2[hubs] by LDS-DMA (piece t -> float4 t of s_hub) and the row's own
  // S2 row (the diagonal's term; no diagonal: no load, 0) -- its address needs
  // the row id, the hub rows' their ids: the one dependent round of this path
  const bool doc = rowt && rid >= 0 && pre >= 0;           // not a position past M, nor a hub row's (its own workgroup)
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (tid + kThreads * q < nh4)
      lds_dma16(a.S2 + (int64_t)hid[q] * (a.ld4 / 4) + 4 * ((tid + kThreads * q) % P4),
                s_hub + 4 * (kThreads * q + 64 * wv));
  if (tid < P4) *reinterpret_cast<f32x4*>(s_hub + a.H * P + 4 * tid) = f32x4{0.f, 0.f, 0.f, 0.f};   // the zero row
  const f32x4 own = buf_load_f32x4(r_s2, ((uint32_t)rid * a.ld4 + 16u * c) | (doc && dg != 0.f ? 0u : kBufOob));
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's DMA and loads have landed
  __syncthreads();
  stamp2(a, 1);
  if (!rowt) return;                     // (whole waves at P <= 16; the rest of a wave's lanes otherwise)
  // CSR column order: the `pre` hub items below the diagonal, the diagonal (no
  // diagonal: diag and the unloaded own row are both 0, and fma(0, 0, acc) is acc),
  // the other items
  const int32_t off0 = s_rec[i], off1 = s_rec[i + 1];
  const HubItem* s_items = reinterpret_cast<const HubItem*>(s_rec + kHubRecHead);
  const int jb = doc ? off0 : 0, je = doc ? off1 : 0, jm = doc ? min(off0 + pre, off1) : 0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  doc_chain<P4>(acc, s_items, s_hub, a.H * P, c, jb, jm);
  fma4(acc, dg, own);
  doc_chain<P4>(acc, s_items, s_hub, a.H * P, c, jm, je);
  stamp2(a, 2);
  acc += bv;
  buf_store_f32x4<kBufSc1>(acc, r_out, doc ? (uint32_t)rid * a.ldo4 + 16u * c : kBufOob);
  stamp2(a, 3);
}

template <int P4>
int launch_gc2(const Gc2Args& a, unsigned grid, size_t lds_b, void* stream) {
  hipLaunchKernelGGL((factored_spmm_row_kernel<P4>), dim3(grid), dim3(kThreads), lds_b,
                     reinterpret_cast<hipStream_t>(stream), a);
  return launch_check("factored_spmm_row_kernel");
}

}  // namespace
}  // namespace gcnk

using namespace gcnk;

extern "C" int gcnk_hubfactor_gc2_f32(int32_t M, int32_t H, int32_t P, const int32_t* rec, int32_t rec_words,
                                      const float* diag, const int32_t* pre, const int32_t* hub_ids,
                                      const int32_t* hub_rp, const int32_t* hub_ci, const float* hub_val,
                                      const float* S2, int64_t lds2, const float* b2, float* out, int64_t ldo,
                                      void* stream) {
  if (M <= 0 || H <= 0 || P <= 0 || !rec || !diag || !pre || !hub_ids || !hub_rp || !hub_ci || !hub_val || !S2 ||
      !out || !hub_rec_words_ok(rec_words) || lds2 < P || ldo < P) {
    set_error("gcnk_hubfactor_gc2_f32: bad sizes or null operand (M=%d hubs=%d P=%d rec_words=%d)", M, H, P,
              rec_words);
    return GCNK_EARG;
  }
  const int64_t nblk = hub_blocks(M);
  const int64_t s2_bytes = 4 * ((int64_t)(M - 1) * lds2 + P), out_bytes = 4 * ((int64_t)(M - 1) * ldo + P);
  const int64_t lds_doc = 4 * ((int64_t)rec_words + ((int64_t)H + 1) * P);   // record | S2[hubs] | a zero row
  const int64_t lds_hub = 16 * (int64_t)(kPartSlots + kCollect * 8);
  if (P % 4 || P > 32 || H > kMaxHubs || lds2 % 4 || ldo % 4 || !aligned16(S2) || !aligned16(out) ||
      !aligned16(rec) || (b2 && !aligned16(b2)) || s2_bytes > (int64_t)kBufOob || out_bytes > (int64_t)kBufOob ||
      nblk * rec_words * 4 > (int64_t)kBufOob || lds_doc > 64 * 1024) {
    set_error("gcnk_hubfactor_gc2_f32: unsupported shape (P=%d %% 4, P <= 32, hubs=%d <= 128, 16-B rows, "
              "operands below 2 GiB, %lld B of LDS <= 64 KiB)", P, H, (long long)lds_doc);
    return GCNK_EUNSUP;
  }
  Gc2Args a;
  a.M = M; a.H = H; a.P = P; a.rec_words = rec_words;
  a.rec = rec; a.diag = diag; a.pre = pre; a.hub_ci = hub_ci; a.hub_val = hub_val;
  a.S2 = S2; a.b2 = b2; a.out = out;
  a.ld4 = (uint32_t)(4 * lds2); a.ldo4 = (uint32_t)(4 * ldo);
  a.s2_bytes = (uint32_t)s2_bytes; a.out_bytes = (uint32_t)out_bytes;
  a.pos_bytes = (uint32_t)(nblk * kHubRows * 4); a.b2_bytes = b2 ? 4u * (uint32_t)P : 0u;
  a.stamps = debug_stamps();
  for (int j = 0; j < kMaxHubs; ++j) a.hub_id[j] = j < H ? hub_ids[j] : 0;
  for (int j = 0; j <= kMaxHubs; ++j) a.hub_rp[j] = hub_rp[j <= H ? j : H];
  for (int j = 0; j < H; ++j)
    if (a.hub_id[j] < 0 || a.hub_id[j] >= M || a.hub_rp[j + 1] < a.hub_rp[j] || a.hub_rp[0] < 0) {
      set_error("gcnk_hubfactor_gc2_f32: hub %d has a bad row id or item range", j);
      return GCNK_EARG;
    }
  const unsigned grid = (unsigned)(H + nblk);
  const size_t lds_b = (size_t)std::max(lds_doc, lds_hub);
  switch (P / 4) {
    case 1: return launch_gc2<1>(a, grid, lds_b, stream);
    case 2: return launch_gc2<2>(a, grid, lds_b, stream);
    case 3: return launch_gc2<3>(a, grid, lds_b, stream);
    case 4: return launch_gc2<4>(a, grid, lds_b, stream);
    case 5: return launch_gc2<5>(a, grid, lds_b, stream);
    case 6: return launch_gc2<6>(a, grid, lds_b, stream);
    case 7: return launch_gc2<7>(a, grid, lds_b, stream);
    default: return launch_gc2<8>(a, grid, lds_b, stream);
  }
}
