// Hub-factored first GCN layer for gfx950: gc1 of the reference's doc-topic
// graph without the topic rows' gather-and-combine.
//
// Reference (layer.py:102,106,110,182,185 inside GCN.forward, layer.py:164-190):
//   H1 = dropout(relu(A-hat (X W1) + b1)),   S2 = H1 W2   (gc2's support, layer.py:102)
//
// Structure used (checked on the host, factor.py): the rows of A-hat split into
// a few hub rows (R8: the 50 topics) and light rows (the 7,674 documents) whose
// nonzeros are hub columns plus their own diagonal, and X's light rows are
// supported on a small contiguous column range Kc (R8: the 50 topic-weight
// columns).  Then, with S_T = X_hubs W1 (the hub rows of X W1, computed by the
// tile GEMM beforehand),
//   light row d:  (A X W1)[d] = (A_dd X[d, Kc]) W1[Kc] + sum_t A[d, t] S_T[t]
//   hub row t:    (A X W1)[t] = (sum_d A[t, d] X[d, Kc]) W1[Kc] + sum_t' A[t, t'] S_T[t']
// i.e. Z = U W1[Kc] + A_H S_T with U [M x Kc] dense and A_H [M x hubs] sparse,
// both fixed by (A-hat, X) and built once (factor.py).  The topic rows' sums over
// ~600 document rows each -- the north-star SpMM's long pole -- move into U's
// hub rows (the (A X) W association; fp32 rounding differs from A (X W) by
// ~1e-6 relative), and the document rows never read or write their S1 rows.
//
// One workgroup = one block of hub_block.h (32 rows, 8 waves: 2 row strips x 4
// quarters of the F columns):
//   0. every operand of the block in one round of loads: W1[Kc] and S_T into LDS,
//      the block's U rows into LDS (16-B DMA; or its U fragments into registers),
//      its A_H record into LDS, the wave's W2 fragments into registers;
//   1. Z_strip = U_strip W1[Kc] on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains);
//   2. Z through LDS to row-major; + A_H S_T, + b1, ReLU, dropout (mask or hash,
//      the row kernel's epilogue); H1 stored only when a backward needs it;
//   3. S2 = H1 W2 on MFMA from the same LDS tile (K split over the two halves,
//      summed in a fixed order).
// No atomics, no hand-off between workgroups: bitwise reproducible.
#include "hub_block.h"

#include <type_traits>

namespace gcnk {
namespace {

constexpr int kMaxKsteps = 32;  // Kc <= 128
// compile-time shapes (every MFMA unconditional, operands in fixed registers):
// KS k-steps of U W1[Kc] (Kc <= 4 KS; U columns past Kc read as zero, W1 rows
// past Kc staged as zero) beside the block's NTQ and NP (only tiles holding a
// column of F are computed; the last one's columns past F come from zeroed or
// W1 LDS words and are never used)
// (18: the 20ng-shaped X's 70 topic-weight columns, whose W1 rows at 25 k-steps
// would take the block's LDS past 160 KiB)
__host__ __device__ constexpr int pick_ks(int kc) { return kc <= 52 ? 13 : kc <= 72 ? 18 : kc <= 100 ? 25 : 32; }

struct FactorArgs {
  int32_t M, F, Kc, nhub, P;
  const float* U; int64_t ldu;          // [M x >= Kc], rows in block order
  const float* W; int64_t ldw; int32_t k0;  // W1 rows k0 .. k0 + Kc - 1 (ldw == F: staged flat)
  const float* S; int64_t lds;          // S_T [nhub x F]
  const int32_t* rec; int32_t rec_words;  // the blocks' records
  const float* W2; int64_t ldw2;        // [F x P]
  int32_t u_lds;                        // 1: the block's U rows staged in LDS by 16-B DMA (ldu % 4 == 0, aligned)
  float* H; int64_t ldh;                // nullable
  float* C2; int64_t ldc2;              // [M x P]
  uint32_t c2_bytes;                    // C2's span (below kBufOob: stored through a buffer resource)
  Epi epi;
};

template <int KS, int NTQ, int NP>
__global__ void __launch_bounds__(kHubThreads)
hubfactor_gc1_kernel(FactorArgs a) {
  resolve_rng(a.epi);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int strip = wv & 1, quarter = wv >> 1;
  const int F = a.F, Q = F / 4;
  constexpr int Fp = 64 * NTQ, Fz = hub_z_stride(NTQ);
  constexpr int Kr = 4 * KS;
  const int blk = (int)blockIdx.x;
  const int64_t m0 = (int64_t)blk * kHubRows;  // position in the block order (U's rows)
  // LDS: region1 = s_B [Kr][F] + hub_bpad zeros (phase 1), then s_Z [kHubRows][Fz]
  //      | s_S [nhub][F] | s_bias [F] | s_rec | s_red [NP][3][2][64][4]
  // Every global operand is staged here in the one round of loads that opens the
  // kernel: a global load behind an LDS-read index costs a full memory round trip
  // under load (~1-2 us each, measured), so nothing after the first wait touches
  // global memory except the stores.
  const int r1 = hub_region1_floats(Kr, F, NTQ);
  float* s_B = smem;
  float* s_Z = smem;
  float* s_S = smem + r1;
  float* s_bias = s_S + a.nhub * F;
  int32_t* s_rec = reinterpret_cast<int32_t*>(s_bias + F);
  float* s_red = reinterpret_cast<float*>(s_rec + a.rec_words);
  // u_lds: U's 32 rows [kHubRows][KPU] after s_red; row stride = 4 (mod 64), so lane
  // (row c, quadrant q) reading k = 4 s + q hits bank 4 c + q (conflict-free)
  constexpr int KPU = 64 * ((4 * KS - 4 + 63) / 64) + 4;
  float* s_U = s_red + hub_red_floats(NP);

  // ---- 0. loads, all issued before the first wait: zeros first (no LDS-DMA in
  //      flight yet), then LDS-DMA of W1[Kc] (flat), U's rows (u_lds; else the
  //      U fragments straight into registers below), the block's record, S_T
  //      and b1; phase 3's W2 fragments straight into registers
  for (int e = a.Kc * F + tid; e < Kr * F + hub_bpad(F, NTQ); e += kHubThreads) s_B[e] = 0.f;
  if (!a.epi.bias)
    for (int e = tid; e < F; e += kHubThreads) s_bias[e] = 0.f;
  // (splitting these loads by wave role -- waves 0-3 phase 1's operands, the
  // first barrier waiting only for those -- measured 9.28 against 9.35 us:
  // profiles/r05_factor_ulds_ab.log; not kept)
  {
    const int n4 = a.Kc * Q;  // float4 pieces of W1[k0 .. k0 + Kc) (rows of F floats, ldw == F)
    const float* wsrc = a.W + (int64_t)a.k0 * a.ldw;
    for (int e0 = wv * 64; e0 < n4; e0 += kHubThreads)
      if (e0 + lane < n4) lds_dma16(wsrc + 4 * (e0 + lane), s_B + 4 * e0);
    // U's rows by 16-B DMA (the per-lane fragment loads -- 16 rows x 16 B per
    // instruction -- cost ~1.1 us of the block: profiles/r05_factor_ulds_ab.log);
    // one instruction per row, pieces covering Kc (inside the row: ldu % 4 == 0)
    if (a.u_lds)
      for (int r = wv; r < kHubRows; r += kHubThreads / 64)
        if (m0 + r < a.M && 4 * lane < a.Kc) lds_dma16(a.U + (m0 + r) * a.ldu + 4 * lane, s_U + r * KPU);
    const int32_t* rec = a.rec + (int64_t)blk * a.rec_words;
    for (int e0 = wv * 64; e0 < a.rec_words / 4; e0 += kHubThreads)
      if (e0 + lane < a.rec_words / 4) lds_dma16(rec + 4 * (e0 + lane), s_rec + 4 * e0);
    const int s4 = a.nhub * Q;  // S_T [nhub x F] flat (lds == F)
    for (int e0 = wv * 64; e0 < s4; e0 += kHubThreads)
      if (e0 + lane < s4) lds_dma16(a.S + 4 * (e0 + lane), s_S + 4 * e0);
    if (a.epi.bias)
      for (int e0 = wv * 64; e0 < Q; e0 += kHubThreads)
        if (e0 + lane < Q) lds_dma16(a.epi.bias + 4 * (e0 + lane), s_bias + 4 * e0);
  }
  // Phase 3's B fragments, W2[k][16 t + n] for this wave's quarter of the K = F
  // sum (ldw2 == P; rows past F and columns past P read 0).  W2 depends on
  // nothing the kernel computes: read from LDS after the phase-2 barrier, each
  // fragment sat behind its own compare, exec mask and 32-bit multiply (~150
  // instructions a wave on the block's serial path).
  constexpr int kq = Fp / 16;  // k-steps per quarter
  float bw[NP][kq];
  {
    const __amdgpu_buffer_rsrc_t rw = buffer_rsrc(a.W2, F * a.P * 4);
#pragma unroll
    for (int t = 0; t < NP; ++t)
      hub_proj_frags(bw[t], rw, 4 * quarter * kq + (lane >> 4), a.P, 16 * t + (lane & 15), a.P);
  }
  float af[KS];
  const int64_t urow = m0 + 16 * strip + (lane & 15);
  if (!a.u_lds) {
    const float* up = a.U + urow * a.ldu + (lane >> 4);
#pragma unroll
    for (int s = 0; s < KS; ++s)
      af[s] = (urow < a.M && 4 * s + (lane >> 4) < a.Kc) ? up[4 * s] : 0.f;
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's DMA and fragment loads have landed
  __syncthreads();
  if (a.u_lds) {   // (cells past Kc or past M were not written: selected away)
    const float* su = s_U + (16 * strip + (lane & 15)) * KPU + (lane >> 4);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      // bit mask, not a select: a select let the compiler sink each read into a
      // branch with its own LDS wait (13 round trips)
      const bool ok = urow < a.M && 4 * s + (lane >> 4) < a.Kc;
      af[s] = __int_as_float(__float_as_int(su[4 * s]) & (ok ? -1 : 0));
    }
  }
  stamp(a.epi, 0);

  // ---- 1. Z = U W1[Kc] for this wave's strip and column quarter
  f32x4 acc[NTQ];
#pragma unroll
  for (int i = 0; i < NTQ; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // The phase is bound by MFMA issue (the fragment reads hide behind the other
  // wave of the SIMD: reading them ahead of the MFMAs changed nothing or lost,
  // DESIGN section 5), so only the real tiles of F are computed, as hub_deal
  // deals them.  A slot without a real tile stores its zero accumulator: those
  // columns of s_Z feed phase 3 against zero W2 rows and must be finite.
  const HubDeal deal = hub_deal(strip, quarter, lane, F, NTQ);
  const int c0 = deal.c0;
  {
    const int nt = deal.nt;
    auto run = [&](auto ntc) __attribute__((always_inline)) {
      constexpr int NT = decltype(ntc)::value;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float* br = s_B + (4 * s + (lane >> 4)) * F + c0;
        float bf[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) bf[i] = br[i * kHubTileStep];
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s], bf[i], acc[i], 0, 0, 0);
      }
    };
    if (nt == NTQ) {
      run(std::integral_constant<int, NTQ>{});
    } else if (nt == NTQ - 1) {
      run(std::integral_constant<int, NTQ - 1>{});
    } else {   // narrow F: fewer real tiles, uniform tests
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float* br = s_B + (4 * s + (lane >> 4)) * F + c0;
#pragma unroll
        for (int i = 0; i < NTQ - 2; ++i)
          if (i < nt) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s], br[i * kHubTileStep], acc[i], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // s_B is overwritten by s_Z below
  stamp(a.epi, 1);
  // C/D map of the 16x16 f32 MFMA: reg r -> row (lane >> 4) * 4 + r, col lane & 15
#pragma unroll
  for (int i = 0; i < NTQ; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      s_Z[(16 * strip + (lane >> 4) * 4 + r) * Fz + c0 + i * kHubTileStep] = acc[i][r];
  __syncthreads();

  // ---- 2. row-major epilogue, 16 threads per row, NTQ float4 columns each
  //      (q = c16 + 16 u; slots past F computed from finite LDS words and
  //      dropped): + A_H S_T, + b1, ReLU, dropout; H1 stored when a backward
  //      needs it.  No bounds test inside the item loop, so each item's NTQ
  //      LDS reads issue together.
  {
    const int r = tid >> 4, c16 = tid & 15;
    const int64_t row = s_rec[kHubRecRow + r];  // output row (-1 past M)
    float4 z[NTQ];
#pragma unroll
    for (int u = 0; u < NTQ; ++u) z[u] = *reinterpret_cast<const float4*>(s_Z + r * Fz + 4 * (c16 + 16 * u));
    const HubItem* it = reinterpret_cast<const HubItem*>(s_rec + kHubRecHead);
    const int k1 = s_rec[r + 1];
    // b1's slots with the z reads, one wait for all of them (slots past F read
    // the words after s_bias -- inside the block's LDS -- and are dropped)
    float4 bv[NTQ];
#pragma unroll
    for (int u = 0; u < NTQ; ++u) bv[u] = *reinterpret_cast<const float4*>(s_bias + 4 * (c16 + 16 * u));
    // One item at a time, the next item's word read ahead of this item's S_T
    // rows (index clamped to the row's last item; the word read past the end is
    // never used): an item costs one LDS round trip, not two, which shortens the
    // blocks holding a hub row's long list.  Across the eight waves the loop is
    // bound by LDS throughput, not by the item chain: every form that reads S_T
    // rows it does not need lost (groups of 2-4 items with masked values past the
    // row's end, a rotating prefetch of the next item's rows).
    {
      int k = s_rec[r];
      const int kl = k1 - 1;
      HubItem p = it[max(min(k, kl), 0)];
#pragma unroll 2
      for (; k < k1; ++k) {
        const HubItem pn = it[min(k + 1, kl)];
        const float v = __int_as_float(p.y);
        const float* srow = s_S + p.x * F + 4 * c16;
        float4 sv[NTQ];
#pragma unroll
        for (int u = 0; u < NTQ; ++u) {
          // the last column slot only where it lies inside F (R8: 2 of 16 lanes):
          // inactive lanes move no LDS bytes
          if (u == NTQ - 1 && c16 + 16 * u >= Q) { sv[u] = make_float4(0.f, 0.f, 0.f, 0.f); continue; }
          sv[u] = *reinterpret_cast<const float4*>(srow + 64 * u);
        }
#pragma unroll
        for (int u = 0; u < NTQ; ++u) Vec<4>::fma(z[u], v, sv[u]);
        p = pn;
      }
    }
    if (row >= 0) {
      auto put = [&](int q, const float4& h) __attribute__((always_inline)) {
        if (a.H) store16_nt(a.H + row * a.ldh + 4 * q, h);  // H1 for the backward
        *reinterpret_cast<float4*>(s_Z + r * Fz + 4 * q) = h;
      };
      // eval / no-dropout: one uniform branch around all the elements (tested
      // per element, the dropout path's code sat on the plain path: ~50
      // instructions and several branches per float4)
      if (a.epi.code == GCNK_EPI_BIAS_RELU) {
#pragma unroll
        for (int u = 0; u < NTQ; ++u) {
          const int q = c16 + 16 * u;
          if (q < Q) {
            put(q, make_float4(fmaxf(z[u].x + bv[u].x, 0.f), fmaxf(z[u].y + bv[u].y, 0.f),
                               fmaxf(z[u].z + bv[u].z, 0.f), fmaxf(z[u].w + bv[u].w, 0.f)));
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < NTQ; ++u) {
          const int q = c16 + 16 * u;
          if (q < Q) put(q, Vec<4>::epi(a.epi, z[u], bv[u], row, 4 * (int64_t)q));
        }
      }
    }
  }
  __syncthreads();
  stamp(a.epi, 2);

  // ---- 3. S2 = H1 W2 on MFMA: strip x quarter of the K = F sum each (W2's rows
  //      past F and columns past P as zero), NP 16-column n-tiles of P, quarters
  //      added in order
  f32x4 pc[NP];
  {
    float av[kq];
#pragma unroll
    for (int j = 0; j < kq; ++j) av[j] = s_Z[(16 * strip + (lane & 15)) * Fz + 4 * (quarter * kq + j) + (lane >> 4)];
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      f32x4 p0 = f32x4{0.f, 0.f, 0.f, 0.f}, p1 = p0;
#pragma unroll
      for (int j = 0; j < kq; j += 2) {
        p0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bw[t][j], p0, 0, 0, 0);
        p1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j + 1], bw[t][j + 1], p1, 0, 0, 0);
      }
      pc[t] = p0 + p1;
    }
  }
  if (quarter > 0)
#pragma unroll
    for (int t = 0; t < NP; ++t)
      *reinterpret_cast<f32x4*>(s_red + (((t * 3 + quarter - 1) * 2 + strip) * 64 + lane) * 4) = pc[t];
  // the lane's four output row ids: one 16-B read ahead of the barrier (a read
  // per store, each behind its own wait, was four round trips after it)
  const int4 orow = *reinterpret_cast<const int4*>(s_rec + kHubRecRow + 16 * strip + (lane >> 4) * 4);
  __syncthreads();
  if (quarter == 0) {
    // through a buffer resource over C2: a row id of -1 (past M) and a column past P are sent past it, so the
    // four stores sit behind no branch or 64-bit multiply.  Plain stores: gc2 gathers S2 right away, and
    // write-through or nontemporal ones made this kernel slower ("What each launch leaves
    // at its seam")
    const __amdgpu_buffer_rsrc_t rc2 = buffer_rsrc(a.C2, a.c2_bytes);
    const int rid[4] = {orow.x, orow.y, orow.z, orow.w};
    uint32_t roff[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) roff[r] = rid[r] >= 0 ? (uint32_t)rid[r] * (4u * (uint32_t)a.ldc2) : kBufOob;
#pragma unroll
    for (int t = 0; t < NP; ++t) {
#pragma unroll
      for (int qq = 0; qq < 3; ++qq)
        pc[t] += *reinterpret_cast<const f32x4*>(s_red + (((t * 3 + qq) * 2 + strip) * 64 + lane) * 4);
      const int p = 16 * t + (lane & 15);
      const uint32_t poff = p < a.P ? 4u * (uint32_t)p : kBufOob;
#pragma unroll
      for (int r = 0; r < 4; ++r) buf_store_f32(pc[t][r], rc2, roff[r] + poff);
    }
  }
  stamp(a.epi, 3);
}


// Debug/test aid: every workgroup fills the whole 160 KiB of LDS with `word`.
// LDS is not cleared between workgroups, so a kernel launched next on the same
// CUs starts from these words wherever it reads LDS it has not written (the
// tests poison it with NaN bits before the factored kernel).
__global__ void __launch_bounds__(1024) lds_poison_kernel(uint32_t word) {
  extern __shared__ uint32_t s_all[];
  for (int i = threadIdx.x; i < 160 * 1024 / 4; i += 1024) s_all[i] = word;
  __syncthreads();
  if (s_all[(threadIdx.x * 37) % (160 * 1024 / 4)] != word) s_all[0] = 0;  // keep the stores
}

}  // namespace
}  // namespace gcnk

using namespace gcnk;

extern "C" int gcnk_debug_poison_lds(uint32_t word, void* stream) {
  return launch_big_lds<lds_poison_kernel>("lds_poison_kernel", dim3(1024), dim3(1024), 160 * 1024, stream, word);
}

static int64_t hubfactor_lds_bytes(int32_t F, int32_t Kc, int32_t nhub, int32_t rec_words, int32_t P) {
  const int64_t r1 = hub_region1_floats(4 * pick_ks(Kc), F, hub_pick_ntq(F));
  return 4 * (r1 + (int64_t)nhub * F + F + rec_words + hub_red_floats(hub_pick_np(P)));
}

// U's staged rows (u_lds): kHubRows rows of 4 KS floats at a stride of 4 (mod 64)
static int64_t hubfactor_u_bytes(int32_t Kc) {
  const int64_t ks = pick_ks(Kc);
  return 4 * (int64_t)kHubRows * (64 * ((4 * ks - 4 + 63) / 64) + 4);
}

extern "C" int64_t gcnk_hubfactor_lds_bytes(int32_t F, int32_t Kc, int32_t nhub, int32_t rec_words, int32_t P) {
  if (F <= 0 || Kc <= 0 || nhub <= 0 || rec_words < kHubRecHead || P <= 0 || P > kHubProjMax) return GCNK_EARG;
  return hubfactor_lds_bytes(F, Kc, nhub, rec_words, P);
}

// What gcnk_hubfactor_gc1_f32 launches for a shape, and whether it launches at
// all: the one place these rules live.  The entry point launches from this and
// gcnk_hubfactor_gc1_route reports it.  Returns the first check that fails, in
// the entry point's order (its own checks on the other operands sit between
// them): 0 none, 1 sizes, 2 leading dimensions, 3 unsupported shape, 5 LDS.
struct FactorRoute {
  int ks, ntq, np, u_lds;
  int64_t lds_b;       // the operands' LDS bytes (hubfactor_lds_bytes)
  int64_t lds_launch;  // dynamic LDS of the launch: lds_b, plus U's staged rows when u_lds
};

static int hubfactor_route(int32_t F, int32_t Kc, int32_t nhub, int32_t rec_words, int32_t P, int64_t ldu,
                           bool u_aligned16, FactorRoute& rt) {
  rt = FactorRoute{};
  if (F <= 0 || Kc <= 0 || nhub <= 0 || P <= 0) return 1;
  if (ldu < Kc || !hub_rec_words_ok(rec_words)) return 2;
  if (F % 4 || F > 256 || Kc > 4 * kMaxKsteps || P > kHubProjMax) return 3;
  rt.ks = pick_ks(Kc); rt.ntq = hub_pick_ntq(F); rt.np = hub_pick_np(P);
  rt.lds_b = hubfactor_lds_bytes(F, Kc, nhub, rec_words, P);
  if (rt.lds_b > 160 * 1024) return 5;
  // U's rows through LDS where they fit (R8: 95 + 8.7 KB; the 20ng-shaped 70
  // topic-weight columns at 152 KB take the direct loads)
  rt.u_lds = ldu % 4 == 0 && u_aligned16 && rt.lds_b + hubfactor_u_bytes(Kc) <= 160 * 1024;
  rt.lds_launch = rt.lds_b + (rt.u_lds ? hubfactor_u_bytes(Kc) : 0);
  return 0;
}

extern "C" int gcnk_hubfactor_gc1_route(int32_t F, int32_t Kc, int32_t nhub, int32_t rec_words, int32_t P,
                                        int64_t ldu, int32_t u_aligned16, int64_t* out6) {
  FactorRoute rt;
  const int bad = out6 ? hubfactor_route(F, Kc, nhub, rec_words, P, ldu, u_aligned16 != 0, rt) : 1;
  if (bad == 1 || bad == 2) {
    set_error("gcnk_hubfactor_gc1_route: null out6, bad sizes or leading dimension (F=%d Kc=%d hubs=%d P=%d)", F, Kc,
              nhub, P);
    return GCNK_EARG;
  }
  if (bad) {
    set_error("gcnk_hubfactor_gc1_route: unsupported (F=%d %% 4, F <= 256, Kc=%d <= 128, P=%d <= 32, %lld B of LDS "
              "<= 160 KiB)", F, Kc, P, (long long)rt.lds_b);
    return GCNK_EUNSUP;
  }
  out6[0] = rt.ks; out6[1] = rt.ntq; out6[2] = rt.np; out6[3] = rt.u_lds; out6[4] = rt.lds_launch;
  out6[5] = 1;  // workgroups per 32 rows
  return GCNK_OK;
}

template <int KS, int NTQ, int NP>
static int launch_factor(const FactorArgs& a, int64_t nblk, int64_t lds_b, void* stream) {
  return launch_big_lds<hubfactor_gc1_kernel<KS, NTQ, NP>>("hubfactor_gc1_kernel", dim3((unsigned)nblk),
                                                           dim3(kHubThreads), (size_t)lds_b, stream, a);
}

extern "C" int gcnk_hubfactor_gc1_f32(int32_t M, int32_t F, int32_t Kc, int32_t nhub, int32_t P, const float* U,
                                      int64_t ldu, const float* W, int64_t ldw, int32_t k0, const float* S,
                                      int64_t lds, const int32_t* rec, int32_t rec_words, const float* bias,
                                      int32_t epilogue, const uint8_t* drop_mask, int64_t ldm, float drop_scale,
                                      float keep_prob, uint64_t seed, uint64_t offset, const uint64_t* rng_base,
                                      const float* W2, int64_t ldw2, float* H, int64_t ldh, float* C2,
                                      int64_t ldc2, void* stream) {
  FactorRoute rt;
  const int bad = hubfactor_route(F, Kc, nhub, rec_words, P, ldu, aligned16(U), rt);
  if (bad == 1 || M <= 0 || !U || !W || !S || !rec || !W2 || !C2 || k0 < 0) {
    set_error("gcnk_hubfactor_gc1_f32: bad sizes or null operand (M=%d F=%d Kc=%d hubs=%d P=%d)", M, F, Kc, nhub, P);
    return GCNK_EARG;
  }
  if (bad == 2 || ldw < F || lds < F || ldw2 < P || ldc2 < P || (H && ldh < F)) {
    set_error("gcnk_hubfactor_gc1_f32: leading dimension too small");
    return GCNK_EARG;
  }
  const int64_t c2_bytes = 4 * ((int64_t)(M - 1) * ldc2 + P);
  if (bad == 3 || ldw != F || lds != F || ldw2 != P || !aligned16(W) || !aligned16(S) || (H && !aligned16(H)) ||
      (H && ldh % 4) || (bias && !aligned16(bias)) || c2_bytes >= (int64_t)kBufOob) {
    set_error("gcnk_hubfactor_gc1_f32: unsupported shape (F=%d %% 4, F <= 256, Kc <= 128, P <= 32, 16-B rows, "
              "S2 below 2 GiB)", F);
    return GCNK_EUNSUP;
  }
  FactorArgs a;
  const int rc = make_epi("gcnk_hubfactor_gc1_f32", bias, epilogue, drop_mask, ldm, drop_scale, keep_prob, seed, offset,
                          rng_base, F, kEpiAllCodes, &a.epi);
  if (rc) return rc;
  if (bad == 5) {
    set_error("gcnk_hubfactor_gc1_f32: %lld B of LDS per workgroup > 160 KiB (F=%d Kc=%d hubs=%d)",
              (long long)rt.lds_b, F, Kc, nhub);
    return GCNK_EUNSUP;
  }
  a.M = M; a.F = F; a.Kc = Kc; a.nhub = nhub; a.P = P;
  a.u_lds = rt.u_lds;
  a.U = U; a.ldu = ldu; a.W = W; a.ldw = ldw; a.k0 = k0;
  a.S = S; a.lds = lds; a.rec = rec; a.rec_words = rec_words;
  a.W2 = W2; a.ldw2 = ldw2; a.H = H; a.ldh = ldh; a.C2 = C2; a.ldc2 = ldc2;
  a.c2_bytes = (uint32_t)c2_bytes;
  const int64_t nblk = hub_blocks(M);
  const int ks = rt.ks, ntq = rt.ntq, np = rt.np;
  const int64_t lds_l = rt.lds_launch;
#define GCNK_FACTOR_CASE(KS_, NTQ_)                                                   \
  if (ks == KS_ && ntq == NTQ_)                                                       \
    return np == 1 ? launch_factor<KS_, NTQ_, 1>(a, nblk, lds_l, stream)              \
                   : launch_factor<KS_, NTQ_, 2>(a, nblk, lds_l, stream);
  GCNK_FACTOR_CASE(13, 2) GCNK_FACTOR_CASE(13, 3) GCNK_FACTOR_CASE(13, 4)
  GCNK_FACTOR_CASE(18, 2) GCNK_FACTOR_CASE(18, 3) GCNK_FACTOR_CASE(18, 4)
  GCNK_FACTOR_CASE(25, 2) GCNK_FACTOR_CASE(25, 3) GCNK_FACTOR_CASE(25, 4)
  GCNK_FACTOR_CASE(32, 2) GCNK_FACTOR_CASE(32, 3) GCNK_FACTOR_CASE(32, 4)
#undef GCNK_FACTOR_CASE
  set_error("gcnk_hubfactor_gc1_f32: no kernel for Kc=%d F=%d", Kc, F);
  return GCNK_EUNSUP;
}
